"""-m gpu: parallel sampling over shared prompt keys (include/a3vlm_hip.h, "Shared prompt keys").  Every device check is an equality:
the shared forms read a row's leading keys from another cache row and must give, bit for bit, what the plain ragged entries give on
caches into which that prefix was physically copied -- while the sibling's own copy of those positions holds NaN."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY, synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _strides(H, Hkv, hd, Smax):
    return (H * hd, H * hd, hd, Hkv * Smax * hd, Smax * hd, hd, Hkv * hd * Smax, hd * Smax, Smax, H * hd, H * hd, hd)


def _effective(src, shared, sk, sk_max, B):
    """the header's rule: own row -> 0, else min(shared, keys of the row) rounded down to 64"""
    out = []
    for b in range(B):
        own = not 0 <= src[b] < B or src[b] == b
        out.append(0 if own else max(min(shared[b], min(sk[b], sk_max)), 0) & ~63)
    return out


def _copied_and_poisoned(k, vt, src, eff):
    """(caches with the prefix physically copied from the source row, caches whose sibling prefixes hold NaN instead)"""
    kc, vc, kp, vp = k.clone(), vt.clone(), k.clone(), vt.clone()
    for b, e in enumerate(eff):
        if e > 0:
            kc[b, :, :e] = k[src[b], :, :e]
            vc[b, :, :, :e] = vt[src[b], :, :, :e]
            kp[b, :, :e] = float("nan")
            vp[b, :, :, :e] = float("nan")
    return kc, vc, kp, vp


# ------------------------------------------------------------------ 1. attention
# (src_row, shared, sk) per row; row 0 is the source
CASES = {
    "boundaries": [(0, 0, 200), (0, 64, 65), (0, 128, 200), (0, 128, 100)],       # first own key right behind the boundary; shared > sk
    "unrounded-and-out-of-range": [(0, 0, 200), (0, 100, 200), (-1, 128, 150), (7, 128, 150)],
    "idle-and-one-level": [(0, 0, 200), (0, 128, 0), (2, 0, 200), (2, 192, 90)],  # row 3 reads row 2's own cache, clamped to 64
}


def _attn_case(case, hd, H, Hkv, sk_max, dtype):
    B, Smax = 4, 384
    src, shared, sk = (list(x) for x in zip(*CASES[case]))
    eff = _effective(src, shared, sk, sk_max, B)
    if case == "boundaries" and sk_max >= 200:
        assert eff == [0, 64, 128, 64]
    if case == "unrounded-and-out-of-range" and sk_max >= 200:
        assert eff == [0, 64, 0, 0]
    q = gen(B, H * hd, seed=hd + H).to(dtype).to(DEV)
    k = gen(B, Hkv, Smax, hd, seed=1).to(dtype).to(DEV)
    vt = gen(B, Hkv, hd, Smax, seed=2).to(dtype).to(DEV)
    for b, n in enumerate(sk):                         # the cache tail may hold anything
        k[b, :, max(n, 0):] = float("nan")
        vt[b, :, :, max(n, 0):] = float("nan")
    kc, vc, kp, vp = _copied_and_poisoned(k, vt, src, eff)
    st = _strides(H, Hkv, hd, Smax)
    want = torch.full((B, H * hd), float("nan"), dtype=dtype, device=DEV)
    got = want.clone()
    scratch = ctr = None
    if dtype == BF and hd in (64, 128):
        scratch = torch.full((ops.attention_scratch_floats(B, H, hd, sk_max),), float("nan"), dtype=torch.float32, device=DEV)
        ctr = torch.zeros(B * H, dtype=torch.int32, device=DEV)
    ops.attention_decode_rows(q, kc, vc, want, i32(sk), sk_max, B, H, Hkv, hd, st, scratch, ctr)
    ops.attention_decode_rows_shared(q, kp, vp, got, i32(sk), i32(src), i32(shared), sk_max, B, H, Hkv, hd, st, scratch, ctr)
    if ctr is not None:
        assert int(ctr.abs().sum()) == 0, "the arrival counters are left at zero"
    assert torch.isfinite(want.float()).all() and torch.isfinite(got.float()).all(), "a NaN: a poisoned position was read"
    assert torch.equal(got, want), (case, eff)
    for b, n in enumerate(sk):
        if n <= 0:
            assert float(got[b].float().abs().sum()) == 0, "idle row"
    if any(eff):                                       # the poison is where the plain entry reads
        plain = torch.empty_like(got)
        ops.attention_decode_rows(q, kp, vp, plain, i32(sk), sk_max, B, H, Hkv, hd, st, scratch, ctr)
        assert not torch.isfinite(plain.float()).all()
    # src_row None is the plain entry
    rc = lib.load().a3v_attention_decode_rows_shared(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), got.data_ptr(), i32(sk).data_ptr(), None, None,
                                                     sk_max, B, H, Hkv, hd, ops._Strides(*st), ops._p(scratch), ops._p(ctr), ops.dt(q),
                                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(got, want)


@pytest.mark.parametrize("sk_max", [64, 300], ids=["one-split", "many-splits"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2)], ids=["mha", "gqa"])
@pytest.mark.parametrize("hd", [64, 128])
def test_attention_shared_equals_plain_on_copied_caches(hd, H, Hkv, case, sk_max):
    ns = ops.attention_decode_rows_splits(4, H, sk_max)
    assert (ns == 1) if sk_max == 64 else (ns > 1), ns
    _attn_case(case, hd, H, Hkv, sk_max, BF)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype,hd", [(torch.float32, 16), (BF, 32)], ids=["fp32-hd16", "bf16-hd32"])
def test_attention_shared_generic_forms(dtype, hd, case):
    _attn_case(case, hd, 8, 2, 300, dtype)


# ------------------------------------------------------------------ 2. kv_copy_span
@pytest.mark.parametrize("lo,hi", [(64, 64), (64, 65), (64, 127), (0, 63), (128, 131)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_kv_copy_span_writes_exactly_the_span(dtype, hd, lo, hi):
    B, Hkv, Smax, layers, src = 5, 2, 192, 3, 2
    dst = [0, 3, 9, -1, 2]                               # one out of range on either side, and the source itself
    ks = [gen(B, Hkv, Smax, hd, seed=10 + i).to(dtype).to(DEV) for i in range(layers)]      # canaries: every element its own value
    vs = [gen(B, Hkv, hd, Smax, seed=20 + i).to(dtype).to(DEV) for i in range(layers)]
    wk, wv = [k.clone() for k in ks], [v.clone() for v in vs]
    for k, v in zip(wk, wv):
        for r in (0, 3):
            k[r, :, lo:hi] = k[src, :, lo:hi]
            v[r, :, :, lo:hi] = v[src, :, :, lo:hi]
    ops.kv_copy_span(ks, vs, src, i32(dst), lo, hi)
    torch.cuda.synchronize()
    for i in range(layers):
        assert torch.equal(ks[i], wk[i]) and torch.equal(vs[i], wv[i]), i
    if hi > lo:
        assert not torch.equal(ks[0][0], gen(B, Hkv, Smax, hd, seed=10).to(dtype).to(DEV)[0]), "something was copied"


# ------------------------------------------------------------------ 3. the step
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}


def _model(hd, weights=None, dtype=BF, max_seq_len=256, max_batch_size=32):
    oargs = ref_cpu.OracleArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, **GEOM[hd])
    sd = ref_cpu.make_decoder_weights(oargs, seed=0, std=0.05)
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, max_batch_size=max_batch_size, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(dtype).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    return m


# (pos, src_row, shared) per row
STEP3 = [(150, 0, 0), (70, 0, 64), (129, 0, 128)]
STEP20 = ([(40, 0, 0), (5, 1, 0), (200, 2, 0), (100, 2, 64), (-1, 2, 128)] + [(10 + b, b, 0) for b in range(5, 10)]
          + [(64, 2, 64), (-1, 11, 0), (130, 2, 128), (90, 30, 64), (17, -4, 64), (200, 2, 128), (255, 2, 192), (33, 17, 0), (127, 2, 64), (191, 2, 128)])


@pytest.mark.parametrize("rows", [STEP3, STEP20], ids=["B3", "B20-two-chunks"])
@pytest.mark.parametrize("weights", [None, "fp8", "nf4"])
@pytest.mark.parametrize("hd", [64, 128])
def test_step_shared_equals_the_plain_step_on_copied_caches(hd, weights, rows):
    """forward_inference_rows(..., src_row, shared) on a NaN-poisoned sibling prefix == the plain call on physically copied caches:
    logits and whole caches, from the fused C step (B 20: two chunks, siblings in the second whose leader, row 2, is in the first)
    and kernel by kernel."""
    m = _model(hd, weights)
    B = len(rows)
    pos, src, shared = (list(x) for x in zip(*rows))
    if B == 20:
        assert src[15] == 2 and src[16] == 2 and pos[15] > 0, "a sibling in the second chunk (rows 10..19), its leader in the first"
    w8 = {None: 0, "fp8": 1, "nf4": 2}[weights]
    form = lib.load().a3v_llama_decode_step_rows_form(B, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, w8)
    if hd == 128 or weights is None:     # (the dim-256 geometry has no fused form for weight images: it runs kernel by kernel both times)
        assert form == 2, "the fused C step is what the first pass below runs"
    m.allocate_rows(B)
    pos_max = max(pos)
    eff = _effective(src, shared, [p + 1 for p in pos], pos_max + 1, B)
    assert sum(e > 0 for e in eff) >= 2
    copied, poisoned = [], []
    for i in range(m.n_layers):                              # an arbitrary earlier context in every cache row
        k = gen(*m._k_cache[i].shape, seed=20 + i).to(BF).to(DEV)
        v = gen(*m._vt_cache[i].shape, seed=30 + i).to(BF).to(DEV)
        kc, vc, kp, vp = _copied_and_poisoned(k, v, src, eff)
        copied.append((kc, vc))
        poisoned.append((kp, vp))
    tok = torch.randint(3, VOCAB, (B,), generator=torch.Generator().manual_seed(B)).to(DEV)
    p, s, sh = i32(pos), i32(src), i32(shared)

    def run(caches, **kw):
        for i, (k, v) in enumerate(caches):
            m._k_cache[i].copy_(k)
            m._vt_cache[i].copy_(v)
        out = m.forward_inference_rows(tok, p, pos_max, **kw).clone()
        return out, [(k.clone(), v.clone()) for k, v in zip(m._k_cache, m._vt_cache)]

    for per_kernel in (False, True):
        m._per_kernel_decode = per_kernel
        want, cw = run(copied)
        got, cg = run(poisoned, src_row=s, shared=sh)
        live = [b for b in range(B) if pos[b] >= 0]
        assert torch.isfinite(want[live]).all() and torch.isfinite(got[live]).all(), per_kernel
        assert torch.equal(got, want), (per_kernel, float((got - want).abs().max()))
        for i in range(m.n_layers):                          # the step wrote the new position of every row's own cache, nothing else
            for b in range(B):
                e = eff[b]
                assert torch.equal(cg[i][0][b][:, e:], cw[i][0][b][:, e:]) and torch.equal(cg[i][1][b][:, :, e:], cw[i][1][b][:, :, e:]), (i, b)
                assert torch.isnan(cg[i][0][b][:, :e].float()).all(), "the sibling's own prefix is never written"
    with pytest.raises(ValueError, match="together"):
        m.forward_inference_rows(tok, p, pos_max, src_row=s)


def test_share_prefix_copies_the_tail_and_returns_the_boundary():
    m = _model(64)
    m.allocate_rows(4)
    for i in range(m.n_layers):
        m._k_cache[i].copy_(gen(*m._k_cache[i].shape, seed=40 + i).to(BF))
        m._vt_cache[i].copy_(gen(*m._vt_cache[i].shape, seed=50 + i).to(BF))
    before = [(k.clone(), v.clone()) for k, v in zip(m._k_cache, m._vt_cache)]
    assert m.share_prefix(1, [0, 3], 150) == 128
    assert m.share_prefix(1, [2], 128) == 128 and m.share_prefix(1, [], 77) == 64
    for i, (k, v) in enumerate(before):
        for r in (0, 3):
            k[r, :, 128:150] = k[1, :, 128:150]
            v[r, :, :, 128:150] = v[1, :, :, 128:150]
        assert torch.equal(m._k_cache[i], k) and torch.equal(m._vt_cache[i], v), i


# ------------------------------------------------------------------ 4. model level
def _tiny_meta(max_seq_len=192):
    cfg = os.path.join(GD, "tiny_params.json")
    mm = MetaModel("llama_ens5", cfg, os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=max_seq_len)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(torch.float32).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": max_seq_len}), sd)
    return mm, dec


LONG = "Where is the drawer handle of the cabinet, and which way does it open? " * 2       # 85 tokens: a shared prefix of 64
PROMPTS = ["Detect the lid", LONG, "Open", "Find the door of the microwave"]
GEN = [3, 7, 2, 5]
N_S, T, TOP_P = 3, 1.0, 0.9


def _count_prefills(mm):
    calls = []
    orig = mm.llma.prefill_row

    def counted(row, *a, **k):
        calls.append(row)
        return orig(row, *a, **k)
    mm.llma.prefill_row = counted
    return calls


@pytest.fixture(scope="module")
def text_case():
    mm, dec = _tiny_meta()
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in PROMPTS]
    assert 64 + 2 < max(map(len, pt)) < 150, "one prompt reaches past the first 64 boundary, uncut"
    U = torch.rand(len(PROMPTS), N_S, max(GEN) + 3, generator=torch.Generator().manual_seed(17))
    want = []
    for i, (t, g) in enumerate(zip(pt, GEN)):
        per = []
        for s in range(N_S):
            def sampler(step, logits, i=i, s=s):
                return ref_cpu.sample_top_p_at(torch.softmax(logits / T, dim=-1), TOP_P, U[i, s, step:step + 1])
            per.append(ref_cpu.generate_greedy(dec, [t], max_gen_len=g, eos_id=mm.tokenizer.eos_id, sampler=sampler)[1][0])
        want.append(per)
    assert any(len({tuple(x) for x in per}) > 1 for per in want), "the samples of a prompt differ"
    return mm, U, want


def _repeated(mm, U, rows, **kw):
    """the same prompts repeated N_S times through n = 1, regrouped per prompt"""
    rep = [p for p in PROMPTS for _ in range(N_S)]
    gens = [g for g in GEN for _ in range(N_S)]
    _, ids, sc = mm.generate_many(rep, None, batch_rows=rows, max_gen_len=gens, temperature=T, top_p=TOP_P, return_ids=True,
                                  return_logprobs=True, sample_uniforms=U.reshape(len(rep), -1), **kw)
    grp = lambda x: [x[i * N_S:(i + 1) * N_S] for i in range(len(PROMPTS))]
    return grp(ids), grp(sc)


@pytest.mark.parametrize("rows", [4, 6])
def test_generate_many_n3_equals_repeated_prompts_and_the_oracle(text_case, rows):
    mm, U, want = text_case
    calls = _count_prefills(mm)
    try:
        texts, ids, sc = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, temperature=T, top_p=TOP_P, return_ids=True,
                                          return_logprobs=True, sample_uniforms=U, n=N_S)
        assert len(calls) == len(PROMPTS), "one prefill per prompt, not per sample"
    finally:
        del mm.llma.prefill_row
    assert ids == want, (rows, ids, want)
    assert texts == [[mm.tokenizer.decode(t) for t in per] for per in want]
    rid, rsc = _repeated(mm, U, rows)
    assert ids == rid and sc == rsc, "ids and log-probs of every (prompt, sample), exactly"
    assert all(len(per) == N_S and all(len(s["logprobs"]) == len(t) for s, t in zip(per, pid)) for per, pid in zip(sc, ids))


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.3), dict(top_k=5)], ids=["penalty", "top-k"])
def test_generate_many_n3_with_controls_equals_repeated_prompts(text_case, kw):
    mm, U, _ = text_case
    _, ids, sc = mm.generate_many(PROMPTS, None, batch_rows=4, max_gen_len=GEN, temperature=T, top_p=TOP_P, return_ids=True,
                                  return_logprobs=True, sample_uniforms=U, n=N_S, **kw)
    rid, rsc = _repeated(mm, U, 4, **kw)
    assert ids == rid and sc == rsc


def test_generate_many_n3_with_image_equals_repeated_prompts_and_the_oracle():
    TK = dict(dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=256)
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
    m = plugin.Transformer(plugin.ModelArgs(**TK, vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1), with_visual=True)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(**TK), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    m.load_state_dict({**sd, **vsd})
    mm.llma = m.to(DEV)
    prompts, gens = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open"], [5, 2, 4]
    img = synth_image(3, size=112, seed=3)
    itok = ref_cpu.assemble_image_tokens(ref_cpu.encode_image(img, vsd, vit_layers=2, vit_heads=4, n_views=1), vsd["start_img"], vsd["end_img"])
    assert itok.shape[1] >= 64, "the image words alone reach past the first 64 boundary: every sibling reads a shared prefix"
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(**TK), sd)
    U = torch.rand(len(prompts), N_S, max(gens) + 2, generator=torch.Generator().manual_seed(5))
    want = []
    for i, (p, g) in enumerate(zip(prompts, gens)):
        t = mm.tokenizer.encode(p, bos=True, eos=False)
        per = []
        for s in range(N_S):
            def sampler(step, logits, i=i, s=s):
                return ref_cpu.sample_top_p_at(torch.softmax(logits / T, dim=-1), TOP_P, U[i, s, step:step + 1])
            per.append(ref_cpu.generate_greedy(dec, [t], image_tokens=itok[i:i + 1], image_words=itok.shape[1], max_gen_len=g,
                                               eos_id=mm.tokenizer.eos_id, sampler=sampler)[1][0])
        want.append(per)
    rep = [p for p in prompts for _ in range(N_S)]
    for rows in (4, 6):
        calls = _count_prefills(mm)
        _, ids, sc = mm.generate_many(prompts, img, batch_rows=rows, max_gen_len=gens, temperature=T, top_p=TOP_P, return_ids=True,
                                      return_logprobs=True, sample_uniforms=U, n=N_S)
        del mm.llma.prefill_row
        assert len(calls) == len(prompts)
        assert ids == want, (rows, ids, want)
        _, rid, rsc = mm.generate_many(rep, img.repeat_interleave(N_S, dim=0), batch_rows=rows, max_gen_len=[g for g in gens for _ in range(N_S)],
                                       temperature=T, top_p=TOP_P, return_ids=True, return_logprobs=True,
                                       sample_uniforms=U.reshape(len(rep), -1))
        assert [x for per in ids for x in per] == rid and [x for per in sc for x in per] == rsc, rows


# ------------------------------------------------------------------ 5. the eval entry
def test_eval_entry_num_samples(tmp_path):
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd import eval_affordance_v2 as ev
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
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "10", "--max_seq_len", "512",
           "--temperature", "0.7", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32",
           "--continuous_rows", "2"]
    for flag, extra in (("rows", []), ("one", ["--num_samples", "1"]), ("two", ["--num_samples", "2"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = open(tmp_path / "logs" / "rows" / "demo.json", "rb").read()
    assert a == open(tmp_path / "logs" / "one" / "demo.json", "rb").read(), "the default writes the bytes it wrote"
    for rec in json.loads(a):
        assert sorted(rec) == sorted(["answer", "format_answer", "annotation", "question", "image", "fail"])
    recs = json.loads(open(tmp_path / "logs" / "two" / "demo.json").read())
    assert len(recs) == 3
    for rec in recs:
        ss = rec["samples"]
        assert len(ss) == 2 and all(sorted(s) == ["answer", "fail", "format_answer", "logprob_sum"] for s in ss)
        b = ss[ev.select_sample(ss)]
        assert (rec["answer"], rec["format_answer"], rec["fail"]) == (b["answer"], b["format_answer"], b["fail"])
        assert "logprobs" not in rec and "logprob_sum" not in rec, "--save_scores was not given"
    r = subprocess.run(cmd + ["--addition_flag", "bad", "--num_samples", "3"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--continuous_rows" in r.stderr


# ------------------------------------------------------------------ 6. refusals
def test_refusals_raise_with_nothing_allocated():
    mm, _ = _tiny_meta()
    with pytest.raises(ValueError, match="temperature > 0"):
        mm.generate_many(["Lid?"], None, batch_rows=2, max_gen_len=2, n=2, temperature=0)
    with pytest.raises(ValueError, match="batch_rows"):
        mm.generate_many(["Lid?"], None, batch_rows=2, max_gen_len=2, n=3, temperature=0.5)
    assert mm.llma._cache_shape is None and not mm.llma._k_cache, "nothing was allocated"
