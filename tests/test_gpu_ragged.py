"""-m gpu: ragged decode (a3v_ragged.hip, Transformer.prefill_row / forward_inference_rows, MetaModel.generate_many) -- the per-row
kernels against the uniform entries they restate (bit for bit where the walk is the same) and against the fp64 / integer
restatements of tests/ragged_ref.py, the step against the per-kernel sequence, the model level against the oracle."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import ragged_ref as R
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


# ------------------------------------------------------------------ 1. rope_kvcache_rows
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kvcache_rows_equals_the_uniform_entry_row_by_row(hd, dtype):
    B, H, Hkv, Smax = 5, 4, 2, 128
    pos = [0, 127, 63, -1, 64]
    qkv = gen(B, (H + 2 * Hkv) * hd, seed=hd).to(dtype).to(DEV)
    cs = plugin.precompute_cos_sin(hd, Smax, 10000.0, None).to(DEV)
    k0 = gen(B, Hkv, Smax, hd, seed=1).to(dtype).to(DEV)
    v0 = gen(B, Hkv, hd, Smax, seed=2).to(dtype).to(DEV)
    # five uniform calls (S = 1), each on a one-row view of the caches
    kw, vw, qw = k0.clone(), v0.clone(), torch.zeros(B, H * hd, dtype=dtype, device=DEV)
    for b, p in enumerate(pos):
        if p >= 0:
            ops.rope_kvcache(qkv[b:b + 1], qw[b:b + 1], kw[b:b + 1], vw[b:b + 1], cs, 1, 1, H, Hkv, hd, p, p)
    kg, vg = k0.clone(), v0.clone()
    qg = torch.full((B, H * hd), 7.0, dtype=dtype, device=DEV)
    ops.rope_kvcache_rows(qkv, qg, kg, vg, cs, i32(pos), B, H, Hkv, hd)
    assert torch.equal(qg, qw), "q rows (the idle row: zeros)"
    assert torch.equal(kg, kw) and torch.equal(vg, vw), "whole caches: the written positions and every other byte"
    assert torch.equal(kg[3], k0[3]) and torch.equal(vg[3], v0[3]), "idle row"
    # against the fp64 restatement (one rounding of the rotated value)
    q64, writes = R.rope_rows_fp64(qkv.cpu(), cs.cpu(), pos, H, Hkv, hd, Smax)
    tol = 2 ** -8 if dtype == BF else 1e-6
    assert float((qg.double().cpu().view(B, H, hd) - q64).abs().max()) <= tol * float(q64.abs().max())
    for (b, p), (k64, v64) in writes.items():
        assert float((kg[b, :, p].double().cpu() - k64).abs().max()) <= tol * float(k64.abs().max())
        assert torch.equal(vg[b, :, :, p].double().cpu(), v64)
    # a position of Smax is an idle row: nothing is written
    kg2, vg2 = k0.clone(), v0.clone()
    ops.rope_kvcache_rows(qkv, qg, kg2, vg2, cs, i32([Smax, Smax + 5, -7, 2 ** 31 - 1, Smax]), B, H, Hkv, hd)
    assert torch.equal(kg2, k0) and torch.equal(vg2, v0) and float(qg.float().abs().sum()) == 0


# ------------------------------------------------------------------ 2. attention_decode_rows
def _caches(B, Hkv, hd, Smax, sk, seed, dtype=BF):
    """bf16-exact K / V^T caches whose positions behind sk[b] hold NaN bits"""
    k = gen(B, Hkv, Smax, hd, seed=seed).to(dtype)
    vt = gen(B, Hkv, hd, Smax, seed=seed + 1).to(dtype)
    for b, n in enumerate(sk):
        k[b, :, max(n, 0):] = float("nan")
        vt[b, :, :, max(n, 0):] = float("nan")
    return k.to(DEV), vt.to(DEV)


def _strides(H, Hkv, hd, Smax):
    return (H * hd, H * hd, hd, Hkv * Smax * hd, Smax * hd, hd, Hkv * hd * Smax, hd * Smax, Smax, H * hd, H * hd, hd)


def _rows(q, k, vt, sk, sk_max, H, Hkv, hd, poison=True):
    B, Smax = q.shape[0], k.shape[2]
    out = torch.full((B, H * hd), float("nan"), dtype=q.dtype, device=DEV)
    scratch = ctr = None
    if q.dtype == BF:
        scratch = torch.full((ops.attention_scratch_floats(B, H, hd, sk_max),), float("nan") if poison else 0.0, dtype=torch.float32, device=DEV)
        ctr = torch.zeros(B * H, dtype=torch.int32, device=DEV)
    ops.attention_decode_rows(q, k, vt, out, i32(sk), sk_max, B, H, Hkv, hd, _strides(H, Hkv, hd, Smax), scratch, ctr)
    if ctr is not None:
        assert int(ctr.abs().sum()) == 0, "the arrival counters are left at zero"
    return out


def _uniform(q, k, vt, Sk, H, Hkv, hd):
    """the public a3v_attention at S = 1 in its wave-streaming form"""
    B, Smax = q.shape[0], k.shape[2]
    out = torch.full((B, H * hd), float("nan"), dtype=BF, device=DEV)
    scratch = torch.empty(ops.attention_scratch_floats(B, H, hd, Sk), dtype=torch.float32, device=DEV)
    with lib.env(A3V_ATTN_DECODE_WAVE_STANDALONE="1"):
        ops.attention(q, k, vt, out, B, 1, Sk, H, Hkv, hd, _strides(H, Hkv, hd, Smax), False, scratch)
    return out


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_rows_one_split_is_bit_equal_to_the_uniform_kernel(hd):
    """One key range per (batch, head): a wave's tile walk depends on the row's own key count only, so row b equals the uniform
    kernel at Sk = sk[b] bit for bit."""
    B, H, Hkv, Smax = 8, 32, 8, 640
    sk = [1, 63, 64, 65, 511, 512, 513, 640]
    assert ops.attention_decode_rows_splits(B, H, max(sk)) == 1
    q = gen(B, H * hd, seed=3).to(BF).to(DEV)
    k, vt = _caches(B, Hkv, hd, Smax, sk, seed=4)
    got = _rows(q, k, vt, sk, max(sk), H, Hkv, hd)
    assert torch.isfinite(got.float()).all()
    for b, n in enumerate(sk):
        assert torch.equal(got[b], _uniform(q, k, vt, n, H, Hkv, hd)[b]), (b, n)


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_rows_many_splits(hd):
    """Reference: fp64 softmax over the row's own keys; bound: the S = 1 parity test of a3v_attention (tests/test_gpu_kernels.py,
    rtol 2^-7, atol 4e-3).  Row 1 has three keys: five of its six key ranges are empty."""
    B, H, Hkv, Smax = 2, 4, 2, 704
    sk = [700, 3]
    ns = ops.attention_decode_rows_splits(B, H, max(sk))
    assert ns > 1, ns
    q = gen(B, H * hd, seed=5).to(BF).to(DEV)
    k, vt = _caches(B, Hkv, hd, Smax, sk, seed=6)
    got = _rows(q, k, vt, sk, max(sk), H, Hkv, hd).float().cpu().view(B, H, hd)
    want = R.decode_attention_rows_fp64(q.float().cpu().view(B, H, hd), k.cpu(), vt.cpu(), sk).float()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    print(f"hd {hd}, {ns} key ranges: max err {float(err.max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    assert bool((err <= 4e-3 + 2 ** -7 * want.abs()).all()), float(err.max())
    # every row at sk_max: the uniform kernel's plan and walk, bit for bit
    k2, vt2 = _caches(B, Hkv, hd, Smax, [700, 700], seed=7)
    assert torch.equal(_rows(q, k2, vt2, [700, 700], 700, H, Hkv, hd), _uniform(q, k2, vt2, 700, H, Hkv, hd))


@pytest.mark.parametrize("sk_max", [5, 300])
def test_attention_rows_idle_rows_are_zero(sk_max):
    B, H, Hkv, hd, Smax = 3, 4, 2, 64, 320
    sk = [0, 5, -1]
    q = gen(B, H * hd, seed=8).to(BF).to(DEV)
    k, vt = _caches(B, Hkv, hd, Smax, sk, seed=9)
    got = _rows(q, k, vt, sk, sk_max, H, Hkv, hd).float().cpu().view(B, H, hd)
    assert torch.isfinite(got).all() and float(got[0].abs().sum()) == 0 and float(got[2].abs().sum()) == 0
    want = R.decode_attention_rows_fp64(q.float().cpu().view(B, H, hd), k.cpu(), vt.cpu(), sk).float()
    assert bool(((got - want).abs() <= 4e-3 + 2 ** -7 * want.abs()).all())
    assert float(want[1].abs().max()) > 0


def test_attention_rows_fp32():
    """fp32 parity form against fp64 within the fp32 attention kernel's bound (tests/test_gpu_kernels.py: rtol 1e-4, atol 2e-5)."""
    B, H, Hkv, hd, Smax = 3, 4, 2, 64, 128
    sk = [97, 1, 0]
    q = gen(B, H * hd, seed=10).to(DEV)
    k, vt = _caches(B, Hkv, hd, Smax, sk, seed=11, dtype=torch.float32)
    got = _rows(q, k, vt, sk, 100, H, Hkv, hd).cpu().view(B, H, hd)
    want = R.decode_attention_rows_fp64(q.cpu().view(B, H, hd), k.cpu(), vt.cpu(), sk).float()
    assert torch.isfinite(got).all() and float(got[2].abs().sum()) == 0
    assert bool(((got - want).abs() <= 2e-5 + 1e-4 * want.abs()).all()), float((got - want).abs().max())


# ------------------------------------------------------------------ 3. generate_step_rows
@pytest.mark.parametrize("use_sampled", [False, True], ids=["argmax", "sampled"])
def test_generate_step_rows_is_the_integer_restatement(use_sampled):
    """One launch on a batch that holds, together: a running row, a row completing a two-token stop sequence, a row stopped on
    entry, a row reaching its limit, a row emitting EOS, and a row whose cur is already at its limit."""
    V, stop = 300, [[2], [7, 8]]
    tokens = [[1, 5, 0, 0, 0], [1, 7, 0, 0, 0], [1, 9, 9, 9, 9], [1, 4, 0, 0, 0], [1, 4, 0, 0, 0], [1, 4, 6, 0, 0]]
    cur, limit = [2, 2, 3, 2, 2, 3], [5, 5, 5, 3, 5, 3]
    stopped, stop_pos = [False, False, True, False, False, False], [0, 0, 2, 0, 0, 0]
    want_next = [3, 8, 11, 299, 2, 17]
    logits = gen(len(tokens), V, seed=12)
    for b, t in enumerate(want_next):
        logits[b, t] = 50.0
    logits[3, 150] = 50.0                                       # a tie: the first index wins ... but index 150 < 299
    want_next[3] = 150
    B = len(tokens)
    d = dict(tokens=torch.tensor(tokens, device=DEV), cur=i32(cur), limit=i32(limit), stopped=torch.tensor(stopped, device=DEV),
             stop_pos=torch.tensor(stop_pos, device=DEV), live=i32([5]), next_tok=torch.full((B,), -5, dtype=torch.long, device=DEV),
             pos=i32([-9] * B))
    sampled = torch.tensor(want_next, device=DEV) if use_sampled else None
    ops.generate_step_rows(None if use_sampled else logits.to(DEV), sampled, d["tokens"], d["cur"], d["limit"], 10,
                           torch.tensor([t for s in stop for t in s], device=DEV), i32([0, 1, 3]), len(stop), d["stopped"], d["stop_pos"],
                           d["live"], d["next_tok"], d["pos"])
    nt, pos = R.generate_step_rows(None if use_sampled else logits.tolist(), want_next if use_sampled else None, tokens, cur, limit, 10, stop,
                                   stopped, stop_pos)
    assert d["tokens"].tolist() == tokens and d["cur"].tolist() == cur
    assert d["stopped"].tolist() == stopped == [False, True, True, True, True, True]
    assert d["stop_pos"].tolist() == stop_pos
    assert d["next_tok"].tolist() == nt and d["pos"].tolist() == pos and pos[0] == 12
    assert int(d["live"]) == 5 - 4, "live counts the rows that stopped in this step"


# ------------------------------------------------------------------ models
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}


def _model(hd, weights=None, dtype=BF, max_seq_len=128, max_batch_size=32):
    oargs = ref_cpu.OracleArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, **GEOM[hd])
    sd = ref_cpu.make_decoder_weights(oargs, seed=0, std=0.05)
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, max_batch_size=max_batch_size, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(dtype).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    return m, oargs, sd


# ------------------------------------------------------------------ 4. the step
def _per_kernel_step_rows(m, tok, pos, pos_max):
    """One ragged step as the sequence of public entries (no fused GEMV forms): rmsnorm, GEMV, a3v_rope_kvcache_rows,
    a3v_attention_decode_rows, GEMV + residual, rmsnorm, GEMV SwiGLU, GEMV + residual; 17..32 rows as the two row chunks of the C call."""
    a = m.args
    B = tok.shape[0]
    H, Hkv, hd, dim = m.n_heads, m.n_kv_heads, m.head_dim, a.dim
    hh = torch.empty(B, dim, dtype=BF, device=DEV)
    ops.embed_assemble(tok.view(B, 1).contiguous(), m.tok_embeddings.weight, hh, B, 1, 0, dim)
    pk, fmt, images = m._pack(), m.weight_format, None if m._weights is None else m._weights.images
    Bc = B if B <= 16 else (B + 1) // 2
    for b0 in range(0, B, Bc):
        nb = min(Bc, B - b0)
        h, p = hh[b0:b0 + nb], pos[b0:b0 + nb].contiguous()
        sk = p + 1
        xn, qkv = torch.empty_like(h), torch.empty(nb, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
        att, act = torch.empty(nb, H * hd, dtype=BF, device=DEV), torch.empty(nb, m.ffn, dtype=BF, device=DEV)
        scratch = torch.empty(ops.attention_scratch_floats(nb, H, hd, pos_max + 1), dtype=torch.float32, device=DEV)
        ctr = torch.zeros(nb * H, dtype=torch.int32, device=DEV)

        def lin(x, i, key, out, **kw):
            idx = ("wqkv", "wo", "w13", "w2").index(key)
            ws = m._skinny_ws(nb, out.shape[1] * (2 if kw.get("epilogue") == ops.EPI_SWIGLU else 1), x.shape[1])
            if fmt == "nf4":
                return ops.gemm_skinny_nf4(x, *images[f"{key}.{i}"], out, ws, **kw)
            if fmt == "fp8":
                return ops.gemm_skinny_fp8(x, *images[f"{key}.{i}"], out, ws, **kw)
            assert fmt == "bf16"
            lyr = m.layers[i]
            w = (pk[f"wqkv.{i}"], lyr.attention.wo.weight, pk[f"w13.{i}"], lyr.feed_forward.w2.weight)[idx]
            return ops.gemm_skinny(x, w, out, ws, **kw)
        for i, lyr in enumerate(m.layers):
            kc, vc = m._k_cache[i][b0:b0 + nb], m._vt_cache[i][b0:b0 + nb]
            ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
            lin(xn, i, "wqkv", qkv)
            ops.rope_kvcache_rows(qkv, qkv, kc, vc, m._cos_sin_dev(), p, nb, H, Hkv, hd)
            ops.attention_decode_rows(qkv, kc, vc, att, sk, pos_max + 1, nb, H, Hkv, hd,
                                      ((H + 2 * Hkv) * hd, (H + 2 * Hkv) * hd, hd) + _strides(H, Hkv, hd, kc.shape[2])[3:], scratch, ctr)
            lin(att, i, "wo", h, residual=h, epilogue=ops.EPI_RESIDUAL)
            ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
            lin(xn, i, "w13", act, epilogue=ops.EPI_SWIGLU)
            lin(act, i, "w2", h, residual=h, epilogue=ops.EPI_RESIDUAL)
        assert int(ctr.abs().sum()) == 0
    xn = torch.empty_like(hh)
    ops.rmsnorm(hh, m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(B, a.vocab_size, dtype=torch.float32, device=DEV)
    m._lm_head_f32(xn, logits)
    return logits


@pytest.mark.parametrize("B,pos", [(3, [5, 0, 40]), (20, [5, 0, 40, -1, 127, 64, 63, 1, 2, 3, 90, -1, 17, 18, 19, 100, 101, 33, 65, 126])],
                         ids=["B3", "B20-two-chunks"])
@pytest.mark.parametrize("weights", [None, "fp8", "nf4"])
def test_step_rows_equals_the_per_kernel_sequence(weights, B, pos):
    """a3v_llama_decode_step_rows (through forward_inference_rows) == the per-kernel sequence of public entries, logits and whole
    caches, bit for bit (the geometry of the fp8-KV step test); only position pos[b] of cache row b changes, nothing of an idle row."""
    m, _, _ = _model(128, weights)
    w8 = {None: 0, "fp8": 1, "nf4": 2}[weights]
    assert lib.load().a3v_llama_decode_step_rows_form(B, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, w8) == 2
    m.allocate_rows(B)
    before = []
    for i in range(m.n_layers):                              # an arbitrary earlier context in every cache row
        m._k_cache[i].copy_(gen(*m._k_cache[i].shape, seed=20 + i).to(BF))
        m._vt_cache[i].copy_(gen(*m._vt_cache[i].shape, seed=30 + i).to(BF))
        before.append((m._k_cache[i].clone(), m._vt_cache[i].clone()))
    tok = torch.randint(3, VOCAB, (B,), generator=torch.Generator().manual_seed(B)).to(DEV)
    p = i32(pos)
    pos_max = max(pos)
    fused = m.forward_inference_rows(tok, p, pos_max).clone()
    after = [(k.clone(), v.clone()) for k, v in zip(m._k_cache, m._vt_cache)]
    for i, (k, v) in enumerate(before):
        m._k_cache[i].copy_(k)
        m._vt_cache[i].copy_(v)
    per = _per_kernel_step_rows(m, tok, p, pos_max)
    assert torch.isfinite(fused).all()
    print(f"weights {weights}, B {B}: max |fused - per kernel| = {float((fused - per).abs().max()):.3e} of max |logit| {float(fused.abs().max()):.3e}")
    for i, (k, v) in enumerate(after):
        assert torch.equal(m._k_cache[i], k) and torch.equal(m._vt_cache[i], v), i
        for b, pb in enumerate(pos):                         # only position pos[b] of row b changed
            keep = torch.ones(k.shape[2], dtype=torch.bool, device=DEV)
            if pb >= 0:
                keep[pb] = False
            assert torch.equal(k[b][:, keep], before[i][0][b][:, keep]) and torch.equal(v[b][:, :, keep], before[i][1][b][:, :, keep]), (i, b)
    assert torch.equal(fused, per)
    if weights is None and B == 3:                            # the plugin's own kernel-by-kernel path (geometries without the fused form)
        for i, (k, v) in enumerate(before):
            m._k_cache[i].copy_(k)
            m._vt_cache[i].copy_(v)
        m._per_kernel_decode = True
        assert torch.equal(m.forward_inference_rows(tok, p, pos_max), per)


# ------------------------------------------------------------------ 5. model level
def _tiny_meta(dtype=torch.float32, max_seq_len=96):
    cfg = os.path.join(GD, "tiny_params.json")
    mm = MetaModel("llama_ens5", cfg, os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=max_seq_len)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(dtype).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": max_seq_len}), sd)
    return mm, dec


PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
GEN = [3, 9, 2, 6, 4]               # rows 2: prompt 1 is mid-answer while row 0 is refilled with prompts 2, 3 and 4


@pytest.fixture(scope="module")
def text_case():
    mm, dec = _tiny_meta()
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in PROMPTS]
    assert len(set(map(len, pt))) == len(pt), "prompts of different lengths"
    want = [ref_cpu.generate_greedy(dec, [t], max_gen_len=g, eos_id=mm.tokenizer.eos_id)[1][0] for t, g in zip(pt, GEN)]
    return mm, dec, pt, want


@pytest.mark.parametrize("rows", [1, 2, 4])
def test_generate_many_fp32_equals_the_oracle_per_prompt(text_case, rows):
    mm, _, _, want = text_case
    texts, ids = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True)
    assert ids == want, (rows, ids, want)
    assert texts == [mm.tokenizer.decode(t) for t in want]
    if rows == 2:
        for pe in (1, 3):
            assert mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, poll_every=pe)[1] == want, pe
        # stop strings and a uniform max_gen_len: generate()'s answers for the same prompts one by one
        stops = ("li", "ab")
        one = [mm.generate([p], None, max_gen_len=12, additional_stop_symbols=stops, return_ids=True)[1][0] for p in PROMPTS]
        assert mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=12, additional_stop_symbols=stops, return_ids=True)[1] == one


def test_generate_many_fp32_with_image_equals_the_oracle():
    TK = dict(dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=256)
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
    m = plugin.Transformer(plugin.ModelArgs(**TK, vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1), with_visual=True)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(**TK), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    m.load_state_dict({**sd, **vsd})
    mm.llma = m.to(DEV)
    prompts, gens = PROMPTS[:3], [5, 2, 4]
    img = synth_image(3, size=112, seed=3)
    itok = ref_cpu.assemble_image_tokens(ref_cpu.encode_image(img, vsd, vit_layers=2, vit_heads=4, n_views=1), vsd["start_img"], vsd["end_img"])
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(**TK), sd)
    want = []
    for i, (p, g) in enumerate(zip(prompts, gens)):
        t = mm.tokenizer.encode(p, bos=True, eos=False)
        want.append(ref_cpu.generate_greedy(dec, [t], image_tokens=itok[i:i + 1], image_words=itok.shape[1], max_gen_len=g,
                                            eos_id=mm.tokenizer.eos_id)[1][0])
    for rows in (1, 2):
        assert mm.generate_many(prompts, img, batch_rows=rows, max_gen_len=gens, return_ids=True)[1] == want, rows


def test_generate_many_sampled_equals_the_oracle_replay(text_case):
    """Uniforms are indexed [prompt, generated index]: the oracle replays every prompt alone with its own row of them, and the ids do
    not depend on batch_rows."""
    mm, dec, pt, _ = text_case
    T, p = 1.0, 0.9
    U = torch.rand(len(PROMPTS), max(GEN) + 3, generator=torch.Generator().manual_seed(17))
    want = []
    for i, (t, g) in enumerate(zip(pt, GEN)):
        def sampler(step, logits, i=i):
            return ref_cpu.sample_top_p_at(torch.softmax(logits / T, dim=-1), p, U[i, step:step + 1])
        want.append(ref_cpu.generate_greedy(dec, [t], max_gen_len=g, eos_id=mm.tokenizer.eos_id, sampler=sampler)[1][0])
    assert want != text_case[3], "the draw matters: not the greedy sequence"
    for rows in (1, 2, 4):
        got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, temperature=T, top_p=p, return_ids=True, sample_uniforms=U)[1]
        assert got == want, rows


def test_forward_inference_rows_bf16_against_the_oracle():
    """Rows prefilled with prompts of different lengths, then one ragged step: logits against the oracle (bf16 weights) within the
    bf16 model bound of tests/test_gpu_model.py (4e-2 of max |logit|)."""
    m, oargs, sd = _model(64)
    sdb = {k: v.to(BF) for k, v in sd.items()}
    lens = [9, 1, 30, 17]
    B = len(lens)
    ex = torch.randint(3, VOCAB, (B, 40), generator=torch.Generator().manual_seed(3))
    ex[:, 0] = 1
    assert lib.load().a3v_llama_decode_step_rows_form(B, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, 0) == 2
    m.allocate_rows(B)
    pre = [m.prefill_row(b, ex[b:b + 1, :n].to(DEV)) for b, n in enumerate(lens)]
    step = m.forward_inference_rows(torch.stack([ex[b, n] for b, n in enumerate(lens)]).to(DEV), i32(lens), max(lens))
    for b, n in enumerate(lens):
        d = ref_cpu.OracleDecoder(oargs, sdb)
        w0 = d.forward_inference(ex[b:b + 1, :n], 0).float()
        w1 = d.forward_inference(ex[b:b + 1, n:n + 1], n).float()
        e0 = float((pre[b].cpu() - w0).abs().max() / w0.abs().max())
        e1 = float((step[b:b + 1].cpu() - w1).abs().max() / w1.abs().max())
        print(f"row {b} (prompt of {n}): prefill_row {e0:.3e}, ragged step {e1:.3e} of max |logit| {float(w0.abs().max()):.3e} / {float(w1.abs().max()):.3e}"
              f" (got {float(pre[b].abs().max()):.3e} / {float(step[b].abs().max()):.3e})")
        assert e0 < 4e-2 and e1 < 4e-2, (b, e0, e1)


def test_refusals_raise_before_any_launch(tmp_path):
    from a3vlm_amd.model.LLM import llama_ens5_2images as plugin2
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    m, _, _ = _model(64)
    m.quantize_kv_cache("fp8")
    tok, p = torch.zeros(2, dtype=torch.long, device=DEV), i32([0, 0])
    for call in (lambda: m.allocate_rows(2), lambda: m.prefill_row(0, tok[None, :1]), lambda: m.forward_inference_rows(tok, p, 0)):
        with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
            call()
    assert m._cache_shape is None, "nothing was allocated"
    m2 = plugin2.Transformer(plugin2.ModelArgs(vocab_size=VOCAB, max_seq_len=128, **GEOM[64]))
    with pytest.raises(NotImplementedError, match="two-image"):
        m2.allocate_rows(2)
    mp = peft.Transformer(peft.ModelArgs(vocab_size=VOCAB, max_seq_len=128, lora_rank=8, **GEOM[64]))
    with pytest.raises(NotImplementedError, match=r"merge_adapters\(\)"):
        mp.forward_inference_rows(tok, p, 0)
    mm, _ = _tiny_meta()
    mm.llma = m                                               # (the tiny fixture model has head_dim 16: no fp8 cache there)
    with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
        mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=2)


# ------------------------------------------------------------------ 6. the eval entry
def test_eval_entry_continuous_rows_writes_the_same_records(tmp_path):
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
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "10", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32"]
    for flag, extra in (("plain", []), ("rows", ["--continuous_rows", "2"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = open(tmp_path / "logs" / "plain" / "demo.json", "rb").read()
    b = open(tmp_path / "logs" / "rows" / "demo.json", "rb").read()
    assert len(json.loads(a)) == 3 and a == b
