"""-m gpu: beam search (include/a3vlm_hip.h, "Beam search").  a3v_beam_select and a3v_beam_advance are compared bit for bit with
their restatement (tests/beam_ref.py), a3v_kv_permute_tails with torch indexing on a pre-call copy of the caches, and
MetaModel.beam_search (fp32 stream) with the oracle decoder run under the restatement's whole-search driver."""
import os

import numpy as np
import pytest
import torch

import beam_ref
from a3vlm_amd import ops
from a3vlm_amd.model import beam
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY, synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ 1. select
def _select_inputs(G, K, V, mode, seed):
    R = G * K
    rng = np.random.default_rng(seed)
    if mode == "ties":          # values on a coarse grid: exact ties across beams and across the strides of a thread
        z = (rng.integers(-8, 9, size=(R, V)) * 0.5).astype(np.float32)
        lse = rng.integers(2, 4, size=R).astype(np.float32)
        cum = (-rng.integers(0, 3, size=R) * 0.5).astype(np.float32)
    else:
        z = rng.standard_normal((R, V)).astype(np.float32) * 3
        lse = beam_ref.lse_rows(z)
        cum = (-rng.random(R) * 5).astype(np.float32)
    z[rng.random((R, V)) < 0.05] = -np.inf
    alive = np.ones(R, np.uint8)
    for r in range(R):
        if r % 5 == 1:
            alive[r] = 0                                   # a dead beam
        if r % 7 == 2:
            z[r] = np.nan                                  # a row of NaN
        if r % 7 == 5:
            z[r] = -np.inf                                 # a row of -inf
    trans = np.full((3, V), -1, np.int16)
    trans[0] = 0                                           # every token
    trans[1, :max(min(V, 2 * K) - 1, 1)] = 1               # fewer than 2K tokens
    trans[2, ::3] = 2
    state = np.array([[0, 1, 2, 7, -1][r % 5] for r in range(R)], np.int32)       # 7 and -1: outside [0, n_states)
    return z, lse, cum, alive, trans, state


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "constrained"])
@pytest.mark.parametrize("mode", ["ties", "random"])
@pytest.mark.parametrize("pad", [1, 0], ids=["stride-V+1", "stride-V"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [37, 1027, 4099, 32000])
def test_beam_select_is_bit_equal_to_the_restatement(V, K, G, pad, mode, constrained):
    z, lse, cum, alive, trans, state = _select_inputs(G, K, V, mode, seed=V + 10 * K + G)
    R = G * K
    store = torch.full((R, V + pad), 7.0, dtype=torch.float32, device=DEV)
    zd = store[:, :V]
    zd.copy_(dev(z))
    # (V + 1 is a multiple of 4 for V = 1027 and 4099: there the rows of stride V are the ones off the 16-byte grid)
    cs = torch.full((G, 2 * K), 5.0, dtype=torch.float32, device=DEV)
    cb = torch.full((G, 2 * K), 99, dtype=torch.int32, device=DEV)
    ct = torch.full((G, 2 * K), 99, dtype=torch.int32, device=DEV)
    kw = dict(trans=dev(trans), state=dev(state)) if constrained else {}
    ops.beam_select(zd, dev(lse), dev(cum), dev(alive), K, cs, cb, ct, **kw)
    ws, wb, wt, _ = beam_ref.select(z, lse, cum, alive, K, trans if constrained else None, state if constrained else None)
    assert np.array_equal(cb.cpu().numpy(), wb) and np.array_equal(ct.cpu().numpy(), wt), (cb.cpu(), wb, ct.cpu(), wt)
    assert np.array_equal(bits(cs.cpu().numpy()), bits(ws))
    if mode == "ties" and V >= 1027 and K > 1:
        s0 = ws[0][ws[0] > -np.inf]
        assert len(s0) > len(np.unique(s0)), "the case holds exact ties among the taken candidates"
    assert float(store[:, V:].sum()) == 7.0 * R * pad, "the padding column was not written"


# ------------------------------------------------------------------ 2. advance
def _ref_to_dev(st):
    d = beam.BeamState(st.G, st.K, st.ld_tok, DEV)
    for name in ("cum", "alive", "state", "parent", "next_tok", "pos", "glen", "done", "base", "limit", "pool_n", "pool_added", "pool_score",
                 "pool_cum", "pool_len", "pool_seq", "pool_ids"):
        getattr(d, name).copy_(dev(getattr(st, name)))
    return d


def _same_state(d, st, what):
    for name in ("alive", "state", "parent", "next_tok", "pos", "glen", "done", "pool_n", "pool_added", "pool_len", "pool_seq", "pool_ids"):
        assert np.array_equal(getattr(d, name).cpu().numpy(), getattr(st, name)), (what, name, getattr(d, name).cpu().numpy(), getattr(st, name))
    for name in ("cum",):
        assert np.array_equal(bits(getattr(d, name).cpu().numpy()), bits(getattr(st, name))), (what, name)
    n = st.pool_n
    for g in range(st.G):                                  # the score and sum of a filled slot, bit for bit
        for name in ("pool_score", "pool_cum"):
            assert np.array_equal(bits(getattr(d, name)[g, :n[g]].cpu().numpy()), bits(getattr(st, name)[g, :n[g]])), (what, name, g)


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "constrained"])
@pytest.mark.parametrize("early", [True, False], ids=["early", "no-early"])
@pytest.mark.parametrize("penalty", [1.0, 0.6, 2.0])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_beam_advance_is_bit_equal_to_the_restatement(K, penalty, early, constrained):
    """Random candidate lists over 7 steps of 4 groups, with EOS at any rank, unfilled slots, NaN scores and indices out of range;
    the limit, a step without a taker and the cache position cap end three of the groups (asserted).  Whole state, token buffers
    and pool after every step.  The pool's branches are scripted one by one in the test below."""
    G, V, eos, ld, steps = 4, 11, 2, 6, 7
    rng = np.random.default_rng(100 * K + int(10 * penalty) + early)
    st = beam_ref.State(G, K, ld)
    limits, bases = [1, 3, 9, 5], [5, 40, 0, 60]           # group 2: limit > ld_tok; group 3: pos_cap - base = 4 < limit
    for g in range(G):
        st.start(g, bases[g], limits[g], 0 if constrained else -1)
    trans = None
    if constrained:
        trans = rng.integers(-1, 3, size=(3, V)).astype(np.int16)
        st.state[::2] = 9                                  # outside [0, n_states): unconstrained rows among constrained ones
    d = _ref_to_dev(st)
    len_div = beam_ref.len_div_table(ld + 2, penalty)
    tin, tout = np.full((G * K, ld), -7, np.int64), np.full((G * K, ld), -9, np.int64)
    d.tokens[0].copy_(dev(tin))
    d.tokens[1].copy_(dev(tout))
    for step in range(steps):
        sc = np.sort(rng.integers(-12, 0, size=(G, 2 * K)) * 0.25, axis=1)[:, ::-1].astype(np.float32)      # descending, with ties
        be = rng.integers(-1, K + 1, size=(G, 2 * K)).astype(np.int32)                                     # -1 and K: out of range
        be[rng.random((G, 2 * K)) < 0.6] = 0
        to = rng.integers(-1, V + 1, size=(G, 2 * K)).astype(np.int32)                                     # -1 and V: out of range
        to[rng.random((G, 2 * K)) < 0.3] = eos
        sc[rng.random((G, 2 * K)) < 0.05] = np.nan
        empty = rng.random((G, 2 * K)) < 0.15
        sc[empty], be[empty], to[empty] = -np.inf, -1, -1
        if step == 2:
            sc[1], be[1], to[1] = -np.inf, -1, -1          # no taker at all
        beam_ref.advance(sc, be, to, st, tin, tout, V, eos, early, len_div, 64, trans)
        ops.beam_advance(dev(sc), dev(be), dev(to), d, d.tokens[0], d.tokens[1], V, eos, early, dev(len_div), 64,
                         trans=dev(trans) if constrained else None)
        _same_state(d, st, step)
        assert np.array_equal(d.tokens[1].cpu().numpy(), tout) and np.array_equal(d.tokens[0].cpu().numpy(), tin), step
        tin, tout = tout, tin
        d.tokens.reverse()
    assert st.done[0] and st.done[1] and st.done[3], "the limit, no taker, and the position cap end a group"
    assert st.glen[3] <= 4 and st.glen[2] <= ld
    assert {"limit", "none"} & set(st.events), st.events       # group 0 (limit 1) ends at step 0 by one of the two


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_beam_advance_scripted_pool_branches(K):
    """One group, no early stopping, length_penalty 0 (score = sum).  Step 1 fills the pool from ranks 0 .. K-1 (pool_n == K) and
    goes on; step 2 offers a tie with the worst entry (dropped: the earlier entry stays); step 3 a better one (the worst is
    replaced); step 4 a worse one (dropped) and a single taker (fewer than K); step 5 nothing at all (no taker: done).  Every
    branch is asserted to have been taken by the restatement, and the device equals it after every step."""
    V, eos, ld = 11, 2, 8
    st = beam_ref.State(1, K, ld)
    st.start(0, 20, 7)
    d = _ref_to_dev(st)
    len_div = beam_ref.len_div_table(ld + 2, 0.0)
    tin, tout = np.full((K, ld), -7, np.int64), np.full((K, ld), -9, np.int64)
    d.tokens[0].copy_(dev(tin))
    d.tokens[1].copy_(dev(tout))
    worst = -1.0 - 0.125 * (K - 1)
    live = lambda s, n: [(s - 0.01 * j, j % K if n > 1 else 0, 3 + j % 8) for j in range(n)]
    script = [[(-1.0 - 0.125 * j, 0, eos) for j in range(K)] + live(-0.5, K),
              [(worst, 0, eos)] + live(-0.4, 2 * K - 1),
              [(-0.9, 0, eos)] + live(-0.3, 2 * K - 1),
              [(-5.0, 0, eos)] + live(-0.2, 1),
              []]
    want = [{"full", "goes_on"}, {"tie_rejected", "goes_on"}, {"replaced", "goes_on"}, {"rejected"} | ({"fewer"} if K > 1 else set()), {"none"}]
    for step, (items, ev) in enumerate(zip(script, want)):
        sc = np.full((1, 2 * K), -np.inf, np.float32)
        be = np.full((1, 2 * K), -1, np.int32)
        to = np.full((1, 2 * K), -1, np.int32)
        for j, (s_, b_, t_) in enumerate(items):
            sc[0, j], be[0, j], to[0, j] = s_, b_, t_
        st.events.clear()
        beam_ref.advance(sc, be, to, st, tin, tout, V, eos, False, len_div, 64)
        assert ev <= set(st.events), (step, st.events)
        ops.beam_advance(dev(sc), dev(be), dev(to), d, d.tokens[0], d.tokens[1], V, eos, False, dev(len_div), 64)
        _same_state(d, st, step)
        assert np.array_equal(d.tokens[1].cpu().numpy(), tout), step
        tin, tout = tout, tin
        d.tokens.reverse()
        assert st.pool_n[0] == K
    assert st.done[0] and st.pool_score[0].min() == np.float32(-0.9 if K == 1 else min(-0.9, worst + 0.125))


# ------------------------------------------------------------------ 3. permute
MAPS = {2: [[0, 1], [1, 0], [1, 1]],
        3: [[0, 1, 2], [1, 2, 0], [2, 2, 2], [0, 0, 2]],
        8: [[0, 1, 2, 3, 4, 5, 6, 7], [1, 0, 3, 2, 5, 4, 7, 6], [5, 5, 5, 5, 5, 5, 5, 5], [1, 2, 0, 0, 4, 4, 7, 3]]}
SPANS = [(8, 64), (5, 67), (64, 128), (63, 65), (17, 17), (3, 12), (0, 128), (60, 121)]


@pytest.mark.parametrize("slack", [0, 50], ids=["tail_max-exact", "tail_max-larger"])
@pytest.mark.parametrize("lo,hi", SPANS)
@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_kv_permute_tails_moves_exactly_the_spans(dtype, hd, K, lo, hi, slack):
    Hkv, Smax, layers, G = 2, 128, 2, 2
    B = G * K
    itype = torch.int16 if dtype == BF else torch.int32
    maps = MAPS[K]
    for mi in range(len(maps)):
        pm = [maps[mi], maps[(mi + 1) % len(maps)]]       # two groups, two maps
        parent = [g * K + p for g in range(G) for p in pm[g]]
        tail_lo, pos = [lo] * B, [hi] * B
        dead = B - 1                                       # a dead row: its own parent, pos -1, and nobody's child here or not
        parent[dead], pos[dead] = dead, -1
        if K == 3:                                         # a row with a shorter span of its own
            tail_lo[0] = min(lo + 1, hi)
        ks, vs = [], []
        for i in range(layers):
            k = torch.randn(B, Hkv, Smax, hd, generator=torch.Generator().manual_seed(10 + i)).to(dtype)
            v = torch.randn(B, Hkv, hd, Smax, generator=torch.Generator().manual_seed(20 + i)).to(dtype)
            k[:, :, :lo], k[:, :, hi:], v[..., :lo], v[..., hi:] = float("nan"), float("nan"), float("nan"), float("nan")   # canaries
            ks.append(k.to(DEV))
            vs.append(v.to(DEV))
        wk, wv = [k.clone() for k in ks], [v.clone() for v in vs]
        for k0, v0, k1, v1 in zip(ks, vs, wk, wv):
            for r in range(B):
                if parent[r] != r and pos[r] > tail_lo[r]:
                    k1[r, :, tail_lo[r]:pos[r]] = k0[parent[r], :, tail_lo[r]:pos[r]]
                    v1[r, :, :, tail_lo[r]:pos[r]] = v0[parent[r], :, :, tail_lo[r]:pos[r]]
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
        ops.kv_permute_tails(ks, vs, i32(parent), i32(tail_lo), i32(pos), hi - lo + slack, K)
        torch.cuda.synchronize()
        for i in range(layers):
            assert torch.equal(ks[i].view(itype), wk[i].view(itype)), (mi, i, "K")
            assert torch.equal(vs[i].view(itype), wv[i].view(itype)), (mi, i, "V^T")


# ------------------------------------------------------------------ 4. model level, fp32 stream
LONG = "Where is the drawer handle of the cabinet, and which way does it open? " * 2       # 85 tokens: a shared prefix of 64
PROMPTS = ["Detect the lid", LONG, "Open", "Find the door of the microwave", "Close the drawer"]
GEN = [4, 6, 1, 5, 3]
MARGIN = 1e-3
STD = 0.3                              # of the decoder weights: wide enough logits for gaps above the margin
SEED_TEXT, SEED_IMAGE = 0, 1           # weight seeds chosen on the CPU (the replay below) for a margin >= MARGIN in every case


def _replay(dec, eos, V, tokens, K, limit, itok=None, **kw):
    def logits_fn(seqs):
        t = torch.tensor([tokens + s for s in seqs], dtype=torch.long)
        return dec.forward_inference(t, 0, None if itok is None else itok.expand(len(seqs), -1, -1)).numpy()
    return beam_ref.search(logits_fn, K, limit, eos, V, **kw)


def _tiny_meta(max_seq_len=192, seed=SEED_TEXT):
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False,
                   max_seq_len=max_seq_len)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=seed, std=STD)
    mm.llma.load_state_dict(sd)
    mm.to(torch.float32).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": max_seq_len}), sd)
    return mm, dec


def _count_prefills(mm):
    calls = []
    orig = mm.llma.prefill_row

    def counted(row, *a, **k):
        calls.append(row)
        return orig(row, *a, **k)
    mm.llma.prefill_row = counted
    return calls


@pytest.fixture(scope="module")
def text_model():
    return _tiny_meta()


def _check_against_replay(mm, dec, prompts, gens, img, itok, K, rows, penalty=1.0, early=True):
    V, eos = mm.llma.args.vocab_size, mm.tokenizer.eos_id
    calls = _count_prefills(mm)
    try:
        texts, ids, sc = mm.beam_search(prompts, img, num_beams=K, batch_rows=rows, max_gen_len=gens, num_return_sequences=K, return_ids=True,
                                        return_scores=True, length_penalty=penalty, early_stopping=early)
    finally:
        del mm.llma.prefill_row
    assert len(calls) == len(prompts), "one prefill per prompt"
    for i, (p, g) in enumerate(zip(prompts, gens)):
        t = mm.tokenizer.encode(p, bos=True, eos=False)
        pool, margin = _replay(dec, eos, V, t, K, g, None if itok is None else itok[i:i + 1], length_penalty=penalty, early_stopping=early)
        assert margin >= MARGIN, (i, K, margin)
        # the margin guards what is taken, not the order of two hypotheses with near-equal scores: compare them by their ids
        want = {tuple(h[2]): h for h in pool}
        assert sorted(map(tuple, ids[i])) == sorted(want), (i, K, rows, ids[i], pool)
        for s, t, x in zip(sc[i], ids[i], texts[i]):
            h = want[tuple(t)]
            assert abs(s["sum"] - h[1]) < MARGIN / 2 and abs(s["score"] - h[0]) < MARGIN / 2, (i, s, h)
            assert x == mm.tokenizer.decode(t)
        assert [s["score"] for s in sc[i]] == sorted((s["score"] for s in sc[i]), reverse=True), "best first"


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("K", [2, 4])
def test_beam_search_equals_the_oracle_replay(text_model, K, rows):
    mm, dec = text_model
    _check_against_replay(mm, dec, PROMPTS, GEN, None, None, K, rows)


def test_beam_search_without_early_stopping_and_with_a_length_penalty(text_model):
    """the stop rule of early_stopping=False and a full pool's admissions are guarded by the replay's margin too (beam_ref.search)"""
    mm, dec = text_model
    _check_against_replay(mm, dec, PROMPTS, GEN, None, None, 3, 7, penalty=0.5, early=False)


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("K", [2, 4])
def test_beam_search_with_image_equals_the_oracle_replay(K, rows):
    TK = dict(dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=256)
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
    m = plugin.Transformer(plugin.ModelArgs(**TK, vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1), with_visual=True)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(**TK), seed=SEED_IMAGE, std=STD)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    m.load_state_dict({**sd, **vsd})
    mm.llma = m.to(DEV)
    prompts, gens = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open"], [5, 3, 4]
    img = synth_image(3, size=112, seed=3)
    itok = ref_cpu.assemble_image_tokens(ref_cpu.encode_image(img, vsd, vit_layers=2, vit_heads=4, n_views=1), vsd["start_img"], vsd["end_img"])
    assert itok.shape[1] >= 64, "the image words alone reach past the first 64 boundary: every sibling reads a shared prefix"
    _check_against_replay(mm, ref_cpu.OracleDecoder(ref_cpu.OracleArgs(**TK), sd), prompts, gens, img, itok, K, rows)


# ------------------------------------------------------------------ 5. model level, bf16, the fused step
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}
BF_PROMPTS, BF_GEN, BF_ROWS, BF_K = [LONG, "Detect the lid", "Find the door of the microwave"], 8, 8, 4
# Per-token |log-prob of the ragged decode step - log-prob of a teacher-forced prefill_row|, maximum over the greedy answers of
# generate_many(return_logprobs=True) for the same models and prompts (profiles/beam_search.md): the loop without beam search.
PARENT_DIFF = {64: 0.016272, 128: 0.052339}


def _bf16_meta(hd):
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
    V = mm.tokenizer.n_words
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=V, max_seq_len=256, max_batch_size=BF_ROWS, **GEOM[hd]))
    m.load_state_dict(ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=256, **GEOM[hd]), seed=0, std=0.05))
    mm.llma = m.to(BF).to(DEV)
    return mm


def _teacher_forced(mm, prompt_ids, ids):
    """raw log-prob of every id of the answer (and, last, of EOS behind it) from prefill_row of prompt + answer prefix, row 0"""
    out = []
    for t in range(len(ids) + 1):
        z = mm.llma.prefill_row(0, torch.tensor([prompt_ids + ids[:t]], dtype=torch.long, device=DEV))[0].double()
        lp = z - torch.logsumexp(z, -1)
        out.append(float(lp[ids[t] if t < len(ids) else mm.tokenizer.eos_id]))
    return out


def bf16_parent_difference(hd):
    mm = _bf16_meta(hd)
    _, ids, sc = mm.generate_many(BF_PROMPTS, None, batch_rows=BF_ROWS, max_gen_len=BF_GEN, return_ids=True, return_logprobs=True)
    worst = 0.0
    for p, i, s in zip(BF_PROMPTS, ids, sc):
        tf = _teacher_forced(mm, mm.tokenizer.encode(p, bos=True, eos=False), i)
        worst = max([worst] + [abs(a - b) for a, b in zip(s["logprobs"], tf)])
    return worst


def bf16_beam_difference(hd):
    """max over every token of every returned hypothesis of |the search's increment of cum - the teacher-forced log-prob|.  The
    increments are read off snapshots of (token rows, cum) after every step: a hypothesis' prefix of t ids is the token row of one
    live beam after step t."""
    mm = _bf16_meta(hd)
    m = mm.llma
    from a3vlm_amd import lib
    assert lib.load().a3v_llama_decode_step_rows_form(BF_ROWS, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, 0) == 2, "the fused C step"
    assert not getattr(m, "_per_kernel_decode", False)
    snaps, moved = [], []
    orig = beam.BeamState.step

    def step(self, *a, **k):
        orig(self, *a, **k)
        snaps.append((self.glen.tolist(), self.tokens[0].tolist(), self.cum.tolist(), self.alive.tolist(), self.done.tolist(), self.base.tolist()))
        par = self.parent.tolist()
        moved.append(sum(p != r for r, p in enumerate(par)))
    beam.BeamState.step = step
    try:
        _, ids, sc = mm.beam_search(BF_PROMPTS, None, num_beams=BF_K, batch_rows=BF_ROWS, max_gen_len=BF_GEN, num_return_sequences=BF_K,
                                    return_ids=True, return_scores=True, poll_every=1)
    finally:
        beam.BeamState.step = orig
    assert sum(moved) > 0, "some beam was re-parented: tails were permuted"
    worst, n_tok = 0.0, 0
    for p, per_ids, per_sc in zip(BF_PROMPTS, ids, sc):
        pt = mm.tokenizer.encode(p, bos=True, eos=False)
        assert len(per_ids) == BF_K
        for h, s in zip(per_ids, per_sc):
            tf = _teacher_forced(mm, pt, h)
            cums = [0.0]
            for t in range(1, len(h) + 1):       # the live row of this prompt's group whose first t ids are h[:t], after its step t
                hit = [c for glen, toks, cum, alive, done, base in snaps for g in range(len(glen)) if glen[g] == t and base[g] == len(pt)
                       for r, c in enumerate(cum) if r // BF_K == g and toks[r][:t] == h[:t] and (alive[r] or done[g]) and c > float("-inf")]
                assert hit, (p, h, t)
                cums.append(hit[0])
            if len(h) < BF_GEN:                  # ended by EOS: its last increment is the EOS log-prob
                cums.append(s["sum"])
            inc = [b - a for a, b in zip(cums, cums[1:])]
            worst = max([worst] + [abs(a - b) for a, b in zip(inc, tf)])
            n_tok += len(inc)
            assert abs(s["sum"] - cums[-1]) < 1e-5 * max(len(h), 1)
    assert n_tok > 0
    return worst


@pytest.mark.parametrize("hd", [64, 128])
def test_bf16_fused_step_increments_equal_teacher_forced_logprobs(hd):
    """bf16, the fused decode step with shared prompt keys behind a3v_kv_permute_tails: every returned hypothesis is teacher-forced
    through prefill_row and its per-token raw log-probs are compared with the search's increments (a mis-permuted tail shows
    here).  Bound: twice the same difference of the plain ragged loop (generate_many greedy, no beam code), measured for the same
    model and prompts: PARENT_DIFF; the same kernels run in both.  Both numbers are in profiles/beam_search.md."""
    got = bf16_beam_difference(hd)
    print(f"hd {hd}: beam {got:.6f}  plain ragged loop {PARENT_DIFF[hd]:.6f}  bound {2 * PARENT_DIFF[hd]:.6f}")
    assert got <= 2 * PARENT_DIFF[hd], (hd, got, PARENT_DIFF[hd])


def test_one_beam_is_the_greedy_answer_of_generate_many(text_model):
    mm, dec = text_model
    V, eos = mm.llma.args.vocab_size, mm.tokenizer.eos_id
    for p, g in zip(PROMPTS, GEN):                           # the margin condition on the top-2 gap: the replay at K = 1
        _, margin = _replay(dec, eos, V, mm.tokenizer.encode(p, bos=True, eos=False), 1, g)
        assert margin >= MARGIN, (p, margin)
    _, want, lp = mm.generate_many(PROMPTS, None, batch_rows=3, max_gen_len=GEN, return_ids=True, return_logprobs=True)
    _, ids, sc = mm.beam_search(PROMPTS, None, num_beams=1, batch_rows=3, max_gen_len=GEN, return_ids=True, return_scores=True)
    assert ids == want
    for s, l in zip(sc, lp):
        assert abs(s["sum"] - l["sum"]) < 1e-4 * max(len(l["logprobs"]), 1), (s, l)


def test_every_hypothesis_matches_the_constraint(text_model):
    mm, _ = text_model
    pattern = r"\[[0-9]{1,3}(, [0-9]{1,3}){1,3}\]"
    a = mm.constraint_automaton(pattern)
    texts, ids = mm.beam_search(PROMPTS[:3], None, num_beams=3, batch_rows=6, max_gen_len=24, num_return_sequences=3, constraint=a,
                                return_ids=True)
    n = 0
    for per_t, per_i in zip(texts, ids):
        for t, i in zip(per_t, per_i):
            n += 1
            if len(i) < 24:                                  # ended by EOS: a whole match; at the limit: a viable prefix
                assert a.accepts(t), t
            else:
                assert a.viable_prefix(t), t
    assert n > 0


# ------------------------------------------------------------------ 6. the eval entry
def test_eval_entry_num_beams(tmp_path):
    import json
    import subprocess
    import sys
    import types
    from a3vlm_amd import checkpoint as ck
    vit = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({**{k: v for k, v in TINY.items() if k != "max_seq_len"}, **vit}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, **TINY), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    ckdir = ck.save_checkpoint(str(tmp_path / "ck"), types.SimpleNamespace(precision="tf32", only_save_trainable=False), mm, None, None, None, epoch=0)
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_v2", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2", "--num_workers", "0",
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "8", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32",
           "--continuous_rows", "2"]
    for flag, extra in (("plain", []), ("zero", ["--num_beams", "0"]), ("beams", ["--num_beams", "2", "--length_penalty", "0.8"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = open(tmp_path / "logs" / "plain" / "demo.json", "rb").read()
    assert a == open(tmp_path / "logs" / "zero" / "demo.json", "rb").read(), "without the flag: the bytes the entry wrote before"
    plain = json.loads(a)
    for rec in plain:
        assert sorted(rec) == sorted(["answer", "format_answer", "annotation", "question", "image", "fail"])
    recs = json.loads(open(tmp_path / "logs" / "beams" / "demo.json").read())
    assert len(recs) == len(plain) == 3
    for rec in recs:
        assert sorted(rec) == sorted(["answer", "format_answer", "annotation", "question", "image", "fail", "beam_score", "logprob_sum"])
        assert rec["logprob_sum"] < 0 and rec["beam_score"] >= rec["logprob_sum"]
    r = subprocess.run(cmd + ["--addition_flag", "bad", "--num_beams", "3"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--continuous_rows" in r.stderr


def test_refusals_raise_with_nothing_allocated():
    mm, _ = _tiny_meta()
    for kw, match in ((dict(num_beams=9, batch_rows=16), "num_beams"), (dict(num_beams=4, batch_rows=3), "batch_rows"),
                      (dict(num_beams=2, batch_rows=2, num_return_sequences=3), "num_return_sequences"),
                      (dict(num_beams=2, batch_rows=2, temperature=0.5), "temperature"),
                      (dict(num_beams=2, batch_rows=2, repetition_penalty=1.2), "repetition_penalty"),
                      (dict(num_beams=2, batch_rows=2, lookup=3), "lookup"),
                      (dict(num_beams=2, batch_rows=2, additional_stop_symbols=["###"]), "additional_stop_symbols")):
        with pytest.raises(ValueError, match=match):
            mm.beam_search(["Lid?"], None, max_gen_len=2, **kw)
    assert mm.llma._cache_shape is None and not mm.llma._k_cache, "nothing was allocated"
