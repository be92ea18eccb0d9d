"""-m gpu: a3v_sample_top_k_p (top-k and min-p beside top-p on the device) against tests/sampler_ref.py, and the three generate
methods with ``top_k`` / ``min_p`` against an oracle replay that samples with sampler_ref at the same uniforms.

Shapes: V = 1003 (no multiple of 4), 32000, 32768 (the largest row whose e_i is kept in LDS), 50000 (the recomputing form); B = 8
and 1; one case with ld > V and one with rows off a 16-byte boundary; uniforms include 0 and the largest float below 1.

What is exact and what is not.  The top-k edge is a comparison of the logits' own bits and min_p is placed between two neighbouring
e values of the row, so a drawn id must lie in the kept set without any tolerance.  The position of a draw inside the kept set is
compared with the oracle's inverse CDF by the boundary rule of tests/test_gpu_sampling.py (same eps: the device sums fp32 masses in
histogram order, the oracle in rank order)."""
import functools
import json
import os

import pytest
import torch

import genctl_ref as G
import sampler_ref as S
from a3vlm_amd import lib, ops
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
VS = [1003, 32000, 32768, 50000]
U_EDGE = [0.0, 0.99999994, 0.5]


def _boundary_ok(ps, idx, p, u, got, want, eps):
    """tests/test_gpu_sampling.py's rule on the oracle's FINAL distribution (ps, idx: one row of sampler_ref.nucleus): got == want,
    or u lies within eps (in probability mass) of the CDF interval of ``got``."""
    if got == want:
        return True
    ids = idx.tolist()
    a = ids.index(got)
    if float(ps[a]) <= 0:
        # top_p >= 1: the reference's fp32 cumsum drifts past 1.0 somewhere in the tail and cuts what is behind (an artefact of its
        # summation order, < 1e-3 of the mass); a token of that tail is a legitimate draw of "keep all" at a uniform that close to
        # 1 -- whether it passed top-k and min-p the caller checks exactly
        return p >= 1.0 and u >= 1.0 - 1e-3
    cdf = torch.cumsum(ps.double(), -1)
    lo = float(cdf[a - 1]) if a > 0 else 0.0
    return lo - eps <= u <= float(cdf[a]) + eps


def _uniforms(seed, n=64):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(U_EDGE + torch.rand(n - len(U_EDGE), generator=g).tolist(), dtype=torch.float32)


def _draws(row, T, k, p, m, u):
    """One row, len(u) draws in one launch (the row repeated: one block per uniform)."""
    rows = row.to(DEV).expand(len(u), -1).contiguous()
    out = torch.empty(len(u), dtype=torch.long, device=DEV)
    return ops.sample_top_k_p(rows, T, k, p, m, u.to(DEV), out).cpu().tolist()


@functools.lru_cache(maxsize=None)
def _rows(V):
    """8 rows of bf16-rounded logits (thousands of exactly equal values).  Row 0 and 4: the 50th largest value also given to five
    tokens that ranked lower (the k-th value is tied at k = 50); row 1: one token holds all the mass; row 2: all tied; row 3: every
    7th logit is -inf."""
    g = torch.Generator().manual_seed(100 + V)
    z = (torch.randn(8, V, generator=g) * 2.5).bfloat16().float()
    for r in (0, 4):
        order = torch.argsort(z[r], descending=True, stable=True)
        z[r, order[torch.tensor([60, 200, 333, 700, 1000])]] = float(z[r, order[49]])
    z[1, 777] = 60.0
    z[2] = 0.25
    z[3, ::7] = float("-inf")
    return z


def _min_p_between(e_sorted, a):
    """The geometric mean of two neighbouring sorted e values at rank >= a that are at least 1e-4 apart (relative): no e_i of the row,
    on the device or in the oracle (expf implementations differ by an ulp), sits on the threshold."""
    e = e_sorted.double()
    n = len(e)
    while a + 1 < n and not (e[a + 1] > 0 and e[a] / e[a + 1] > 1 + 1e-4):
        a += 1
    if a + 1 >= n:                     # no such pair below rank a (an all-tied row, a one-token row): the top of the row decides
        return 1.0 if float(e[0]) == float(e[-1]) else 0.5 if float(e[1]) < 0.25 else float(torch.sqrt(e[0] * e[1]))
    return float(torch.sqrt(e[a] * e[a + 1]))


# ---------------------------------------------------------------- 1. off means old
def test_filters_off_returns_the_ids_of_sample_top_p(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "sampling.json")))["cases"]
    sets = [((torch.randn(c["rows"], c["vocab"], generator=torch.Generator().manual_seed(c["seed"])) * 3), c["temperature"], c["p"]) for c in cases]
    g = torch.Generator().manual_seed(11)
    sets += [((torch.randn(8, 32000, generator=g) * 2.5).bfloat16().float(), T, p) for T, p in ((0.1, 0.75), (1.0, 0.95), (0.7, 1.0))]
    sets += [(_rows(V), 0.7, 0.9) for V in (1003, 32768, 50000)]
    for cache in ("1", "0"):
        with lib.env(A3V_SAMPLER_CACHE=cache):
            for z, T, p in sets:
                B, V = z.shape
                zd = z.to(DEV)
                a, b = torch.empty(B, dtype=torch.long, device=DEV), torch.empty(B, dtype=torch.long, device=DEV)
                for uval in U_EDGE + torch.rand(5, generator=g).tolist():
                    u = torch.full((B,), uval, device=DEV) if uval in U_EDGE else torch.rand(B, generator=g).to(DEV)
                    ops.sample_top_p(zd, T, p, u, a)
                    for k in (0, V, V + 5):
                        assert torch.equal(ops.sample_top_k_p(zd, T, k, p, 0.0, u, b), a), (cache, V, T, p, k, uval)


# ---------------------------------------------------------------- 2. top_k = 1 is the arg-max
@pytest.mark.parametrize("B", [8, 1])
@pytest.mark.parametrize("V", VS)
def test_top_k_one_is_argmax(V, B):
    g = torch.Generator().manual_seed(V + B)
    z = torch.randn(B, V, generator=g) * 3
    assert all(int((r == r.max()).sum()) == 1 for r in z), "distinct maxima"
    zd = z.to(DEV)
    want = ops.argmax(zd, torch.empty(B, dtype=torch.long, device=DEV))
    assert want.cpu().tolist() == z.argmax(-1).tolist()
    out = torch.empty(B, dtype=torch.long, device=DEV)
    for uval in U_EDGE + [0.123, 0.9]:
        for T, p, m in ((0.7, 0.9, 0.0), (1.0, 1.0, 0.3)):
            assert torch.equal(ops.sample_top_k_p(zd, T, 1, p, m, torch.full((B,), uval, device=DEV), out), want), (uval, T, p, m)


def test_row_stride_and_unaligned_rows():
    """ld > V, and rows that start off a 16-byte boundary (a view one float into a wider buffer): the ids of the dense copy."""
    g = torch.Generator().manual_seed(5)
    B, V = 8, 1003
    z = (torch.randn(B, V, generator=g) * 2.5).bfloat16().float().to(DEV)
    u = torch.rand(B, generator=g).to(DEV)
    want = ops.sample_top_k_p(z, 0.7, 20, 0.9, 0.05, u, torch.empty(B, dtype=torch.long, device=DEV)).clone()
    wide = torch.full((B, V + 9), 99.0, device=DEV)               # a read past the row's end would meet the largest logit there is
    wide[:, :V] = z
    assert torch.equal(ops.sample_top_k_p(wide[:, :V], 0.7, 20, 0.9, 0.05, u, torch.empty(B, dtype=torch.long, device=DEV)), want)
    off = torch.full((B * (V + 4) + 1,), 99.0, device=DEV)[1:].view(B, V + 4)     # V + 4 = 1007 floats per row, first row at +4 bytes
    off[:, :V] = z
    assert off.data_ptr() % 16 == 4 and off.stride(0) == V + 4
    assert torch.equal(ops.sample_top_k_p(off[:, :V], 0.7, 20, 0.9, 0.05, u, torch.empty(B, dtype=torch.long, device=DEV)), want)


# ---------------------------------------------------------------- 3, 4, 6. kept set (exact), draw position (boundary rule), reproducible
@pytest.mark.parametrize("V", VS)
def test_kept_set_is_exact_and_draws_follow_the_oracles_cdf(V):
    z = _rows(V)
    T = 0.7
    u = _uniforms(V)
    esort = torch.sort(S.e_values(z, T), dim=-1, descending=True).values
    bad = []
    for r in range(z.shape[0]):
        row = z[r:r + 1]
        cfgs = [(2, 1.0, 0.0), (50, 1.0, 0.0), (V - 1, 1.0, 0.0), (0, 1.0, _min_p_between(esort[r], 5)), (0, 1.0, _min_p_between(esort[r], 200))]
        if r != 2:     # the all-tied row under top-p < 1: 0.9 V equal masses, the cut itself moves by a few tokens with the summation order
            cfgs.append((50, 0.9, _min_p_between(esort[r], 12)))
        for k, p, m in cfgs:
            got = _draws(row[0], T, k, p, m, u)
            ps, idx = S.nucleus(row, T, k, p, m)
            want = S.draw(ps, idx, u).tolist()
            if p >= 1.0:      # exact: K and the min-p cut, no tolerance
                kept = S.top_k_mask(row, k)[0] & (S.e_values(row, T)[0] >= m)
                out = [t for t in got if not bool(kept[t])]
                assert not out, (V, r, k, m, out[:5], int(kept.sum()))
            eps = 4e-5 if p < 1.0 else 1e-3
            bad += [(r, k, p, m, float(uu), a, b) for uu, a, b in zip(u, got, want) if not _boundary_ok(ps[0], idx[0], p, float(uu), a, b, eps)]
        if r == 1:
            assert set(_draws(row[0], T, 50, 0.9, 0.05, u)) == {777}
    assert not bad, (len(bad), bad[:5])
    # reproducible: the same inputs three times
    zd, ud = z.to(DEV), torch.rand(8, generator=torch.Generator().manual_seed(1)).to(DEV)
    a = ops.sample_top_k_p(zd, T, 50, 0.9, 0.05, ud, torch.empty(8, dtype=torch.long, device=DEV)).clone()
    for _ in range(3):
        assert torch.equal(ops.sample_top_k_p(zd, T, 50, 0.9, 0.05, ud, torch.empty(8, dtype=torch.long, device=DEV)), a)


@pytest.mark.parametrize("V", VS)
def test_every_token_tied_at_the_kth_value_is_reachable(V):
    """Rows 0 and 4: the 50th value is shared by tokens a cut at exactly 50 tokens would drop.  A uniform in the middle of each tied
    token's interval of the oracle's CDF (the tie group is the bottom of the kept set: the top of the CDF) draws that token."""
    z = _rows(V)
    T = 1.0
    for r in (0, 4):
        row = z[r:r + 1]
        K = S.top_k_mask(row, 50)[0]
        t = float(torch.topk(row[0], 50).values[-1])
        tied = torch.nonzero(row[0] == t).flatten().tolist()
        assert int(K.sum()) > 50 and len(tied) >= 6 and all(bool(K[i]) for i in tied)
        ps, idx = S.nucleus(row, T, 50, 1.0, 0.0)
        cdf = torch.cumsum(ps[0].double(), -1)
        ids = idx[0].tolist()
        pos = [ids.index(i) for i in tied]
        assert max(pos) == int(K.sum()) - 1 and pos == sorted(pos), "the tie group closes the ranking, in index order"
        u = torch.tensor([float(cdf[a] - ps[0, a].double() / 2) for a in pos], dtype=torch.float32)
        assert _draws(row[0], T, 50, 1.0, 0.0, u) == tied, (V, r)


# ---------------------------------------------------------------- 5. distribution
def test_draws_follow_the_final_distribution():
    """4000 draws of one row at top_k 20, top_p 0.9, min_p 0.05 (tests/test_gpu_sampling.py's row and its 0.02)."""
    g = torch.Generator().manual_seed(3)
    V = 1000
    logits = torch.randn(1, V, generator=g)
    logits[0, :50] += 4.0
    ps, idx = S.nucleus(logits, 1.0, 20, 0.9, 0.05)
    want = torch.zeros(V).scatter_(0, idx[0], ps[0])
    assert 1 < int((want > 0).sum()) < 20, "top-p or min-p cuts inside the 20"
    N = 4000
    got = _draws(logits[0], 1.0, 20, 0.9, 0.05, torch.rand(N, generator=g))
    freq = torch.bincount(torch.tensor(got), minlength=V).float() / N
    print(f"kept {int((want > 0).sum())} tokens, max |freq - p| = {float((freq - want).abs().max()):.4f}")
    assert float(freq[want == 0].sum()) == 0.0
    assert float((freq - want).abs().max()) < 0.02


# ---------------------------------------------------------------- 7. errors
def test_argument_errors_launch_nothing():
    z = torch.randn(2, 64, device=DEV)
    u = torch.rand(2, device=DEV)
    out = torch.full((2,), -7, dtype=torch.long, device=DEV)
    for k, m in ((-1, 0.0), (0, 1.5), (3, -0.5)):
        with pytest.raises(lib.A3VError, match="A3V_ERR_ARG"):
            ops.sample_top_k_p(z, 1.0, k, 0.9, m, u, out)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7]


# ---------------------------------------------------------------- 8. model level
PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
GEN = 8
TOPK, MINP, TOPP = 5, 0.1, 0.9


def _replay(dec, prompt_tokens, eos, T, penalty, uniform):
    """ref_cpu.generate_greedy with the sampled branch drawing by sampler_ref from the (penalised) row at uniform(step) [B]."""
    V = dec.args.vocab_size
    start = min(len(t) for t in prompt_tokens)
    seen = [set(t) for t in prompt_tokens]

    def sampler(step, logits):
        z = logits.float()
        if penalty != 1.0:
            mask = torch.zeros_like(z, dtype=torch.bool)
            for b, s in enumerate(seen):
                mask[b, [t for t in s if 0 <= t < V]] = True
            z = G.penalise(z, mask, penalty)
        nxt = S.sample_at(z, T, TOPK, TOPP, MINP, uniform(step))
        for b in range(z.shape[0]):
            if start + step - len(prompt_tokens[b]) >= 0:
                seen[b].add(int(nxt[b]))
        return nxt
    return ref_cpu.generate_greedy(dec, prompt_tokens, max_gen_len=GEN, eos_id=eos, sampler=sampler)[1]


@pytest.fixture(scope="module")
def model_case():
    from a3vlm_amd.model.meta import MetaModel
    from oracle.gen_golden import TINY
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=96)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(torch.float32).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": 96}), sd)
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in PROMPTS]
    return mm, dec, pt


@pytest.mark.parametrize("penalty", [1.0, 1.2], ids=["plain", "penalty"])
@pytest.mark.parametrize("T", [0.7, 0.1])
def test_generate_equals_the_oracle_replay(model_case, T, penalty):
    mm, dec, pt = model_case
    sel = [0, 2, 4]                                          # prompts of different lengths: two rows are teacher-forced at first
    ids = [pt[i] for i in sel]
    U = torch.rand(GEN + max(map(len, ids)) - min(map(len, ids)) + 1, len(sel), generator=torch.Generator().manual_seed(17))
    want = _replay(dec, ids, mm.tokenizer.eos_id, T, penalty, lambda step: U[step])
    _, got = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, temperature=T, top_p=TOPP, top_k=TOPK, min_p=MINP,
                         repetition_penalty=penalty, return_ids=True, sample_uniforms=U)
    assert got == want, (got, want)
    if T == 0.7 and penalty == 1.0:       # the filters matter: not what top-p alone draws from the same uniforms
        _, plain = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, temperature=T, top_p=TOPP, return_ids=True, sample_uniforms=U)
        assert plain != got


@pytest.mark.parametrize("penalty", [1.0, 1.2], ids=["plain", "penalty"])
@pytest.mark.parametrize("T", [0.7, 0.1])
def test_generate_many_equals_the_oracle_per_prompt_for_any_batch_rows(model_case, T, penalty):
    mm, dec, pt = model_case
    U = torch.rand(len(PROMPTS), GEN + 3, generator=torch.Generator().manual_seed(23))
    want = [_replay(dec, [t], mm.tokenizer.eos_id, T, penalty, lambda step, i=i: U[i, step:step + 1])[0] for i, t in enumerate(pt)]
    for rows in (1, 2, 4):
        got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, temperature=T, top_p=TOPP, top_k=TOPK, min_p=MINP,
                               repetition_penalty=penalty, return_ids=True, sample_uniforms=U)[1]
        assert got == want, (rows, got, want)


def test_stream_generate_takes_the_filters(model_case):
    mm, dec, pt = model_case
    # top_k = 1 makes the stream's own uniforms irrelevant: the greedy answer
    want = ref_cpu.generate_greedy(dec, [pt[0]], max_gen_len=GEN, eos_id=mm.tokenizer.eos_id)[1][0]
    last = list(mm.stream_generate(PROMPTS[0], None, max_gen_len=GEN, temperature=0.7, top_k=1))[-1]
    assert last["end_of_content"] and last["text"] == mm.tokenizer.decode(want)


def test_defaults_never_reach_the_new_entry(model_case, monkeypatch):
    mm, _, _ = model_case
    P3 = [PROMPTS[i] for i in (0, 2, 4)]
    U = torch.rand(GEN + 40, 3, generator=torch.Generator().manual_seed(5))
    UM = torch.rand(len(PROMPTS), GEN + 3, generator=torch.Generator().manual_seed(6))

    def boom(*a, **k):
        raise AssertionError("ops.sample_top_k_p called with the default top_k / min_p")
    monkeypatch.setattr(ops, "sample_top_k_p", boom)
    a = mm.generate(P3, None, max_gen_len=GEN, temperature=0.7, top_p=0.75, sample_uniforms=U, return_ids=True)
    b = mm.generate(P3, None, max_gen_len=GEN, temperature=0.7, top_p=0.75, sample_uniforms=U, return_ids=True, top_k=0, min_p=0.0)
    assert a == b
    a = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, temperature=0.7, top_p=0.75, sample_uniforms=UM, return_ids=True)
    b = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, temperature=0.7, top_p=0.75, sample_uniforms=UM, return_ids=True, top_k=0, min_p=0.0)
    assert a == b
    # temperature 0 stays the arg-max and ignores all three filters
    assert mm.generate(P3, None, max_gen_len=GEN, top_k=3, min_p=0.5, top_p=0.1) == mm.generate(P3, None, max_gen_len=GEN)
    with pytest.raises(AssertionError, match="sample_top_k_p called"):
        mm.generate(P3, None, max_gen_len=GEN, temperature=0.7, top_k=5, sample_uniforms=U)
    for kw in (dict(top_k=-1), dict(min_p=1.5)):
        with pytest.raises(ValueError):
            mm.generate(P3, None, max_gen_len=GEN, temperature=0.7, **kw)
