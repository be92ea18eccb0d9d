"""-m gpu: the fp8 KV cache (a3v_kv8.hip, Transformer.quantize_kv_cache) -- the quantising cache write and its inverse against the
host restatement (tests/kv8_ref.py), decode attention on the fp8 bytes against an fp64 attention over the very bytes the GPU
quantiser produced, prefill left bit-identical, the structure of a3v_llama_decode_step_kv8, accuracy against a fake-quantised
oracle, and the user-facing entry points."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import kv8_ref as R
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
CANARY_BYTE, CANARY_SCALE = 0x5A, 123.0


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rt(x):
    return x.to(BF).float()


# ------------------------------------------------------------------ 1. quantiser
# (B, Hkv, hd, S, dst_pos, Smax) -> (Smax_src, src_pos): S = 1 reads the one-position staging pair; 37 @ 0 an aligned source (16-B
# loads), 37 @ 27 a source whose offset to the destination is a multiple of 8 but not of 64, 130 @ 61 a source row of 130 (no
# vector loads) and a run that covers a ragged head, whole tiles and a ragged tail
QUANT_CASES = {(1, 2, 64, 1, 0, 64): (1, 0), (2, 2, 128, 1, 63, 64): (1, 0), (2, 1, 128, 37, 0, 128): (128, 0),
               (3, 2, 64, 37, 27, 128): (48, 3), (1, 2, 128, 130, 61, 256): (130, 0)}


def _kv_rows(B, Hkv, S, hd, seed):
    """k, v [B,Hkv,S,hd] bf16-exact, rows of very different magnitude, one all-zero row in each"""
    k = rt(gen(B, Hkv, S, hd, seed=seed) * (gen(B, Hkv, S, 1, seed=seed + 1).abs() * 3 + 0.01))
    v = rt(gen(B, Hkv, S, hd, seed=seed + 2) * (gen(B, Hkv, S, 1, seed=seed + 3).abs() * 3 + 0.01))
    k[0, 0, 0] = 0
    v[0, Hkv - 1, S - 1] = 0
    return k, v


def _src_pair(k, v, Smax_src, src_pos):
    """the rows at src_pos .. of a bf16 K / V^T pair whose other positions hold other numbers"""
    B, Hkv, S, hd = k.shape
    ks = rt(gen(B, Hkv, Smax_src, hd, seed=90) * 50)
    vs = rt(gen(B, Hkv, hd, Smax_src, seed=91) * 50)
    ks[:, :, src_pos:src_pos + S] = k
    vs[:, :, :, src_pos:src_pos + S] = v.transpose(2, 3)
    return ks.to(BF).to(DEV).contiguous(), vs.to(BF).to(DEV).contiguous()


def _caches(B, Hkv, hd, Smax, byte=CANARY_BYTE, scale=CANARY_SCALE):
    return (torch.full((B, Hkv, Smax, hd), byte, dtype=torch.uint8, device=DEV), torch.full((B, Hkv, hd, Smax), byte, dtype=torch.uint8, device=DEV),
            torch.full((B, Hkv, Smax), scale, dtype=torch.float32, device=DEV), torch.full((B, Hkv, Smax), scale, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("case", list(QUANT_CASES), ids=lambda c: "-".join(map(str, c)))
def test_quantizer_and_dequantizer(case):
    B, Hkv, hd, S, dst, Smax = case
    Smax_src, src_pos = QUANT_CASES[case]
    k, v = _kv_rows(B, Hkv, S, hd, seed=sum(case))
    ksrc, vsrc = _src_pair(k, v, Smax_src, src_pos)
    kq, vq, ks, vs = _caches(B, Hkv, hd, Smax)
    ops.kv_quantize_fp8(ksrc, vsrc, src_pos, kq, vq, ks, vs, S, dst)
    torch.cuda.synchronize()
    kq_c, vq_c, ks_c, vs_c = kq.cpu(), vq.cpu(), ks.cpu(), vs.cpu()
    sl = slice(dst, dst + S)
    for name, x, codes, sc in (("k", k, kq_c[:, :, sl], ks_c[:, :, sl]), ("v", v, vq_c[:, :, :, sl].transpose(2, 3), vs_c[:, :, sl])):
        amax = x.abs().amax(-1)
        torch.testing.assert_close(sc, amax.clamp_min(1e-12) / 448, rtol=1e-6, atol=0, msg=f"{name} scales")
        code = codes.contiguous().view(F8).float()
        dq = code * sc[..., None]
        assert torch.isfinite(dq).all() and torch.isfinite(sc).all(), name
        err, bound = (dq - x).abs().double(), R.half_step_bound(x, sc)
        print(f"{name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
        assert bool((code.abs().amax(-1)[amax > 0] == 448).all()), f"{name}: the row maximum maps to +-448"
        assert float(dq[amax == 0].abs().sum()) == 0 and int((amax == 0).sum()) >= 1, f"{name}: all-zero row"
    # nothing outside the S positions was touched (the V^T edges are byte runs inside 16-B words)
    out = torch.ones(Smax, dtype=torch.bool)
    out[sl] = False
    assert bool((kq_c[:, :, out] == CANARY_BYTE).all()) and bool((vq_c[:, :, :, out] == CANARY_BYTE).all())
    assert bool((ks_c[:, :, out] == CANARY_SCALE).all()) and bool((vs_c[:, :, out] == CANARY_SCALE).all())
    # the inverse: positions 0 .. n-1 (canary codes in front of dst included), bit-equal to bf16(float(q) * scale)
    n = dst + S
    Smax_dst = n + 3 if S % 2 else (n + 7) // 8 * 8 + 8
    kd = torch.full((B, Hkv, Smax_dst, hd), 7.0, dtype=BF, device=DEV)
    vd = torch.full((B, Hkv, hd, Smax_dst), 7.0, dtype=BF, device=DEV)
    ops.kv_dequantize_fp8(kq, vq, ks, vs, kd, vd, n)
    want_k = (kq_c[:, :, :n].view(F8).float() * ks_c[:, :, :n, None]).to(BF)
    want_v = (vq_c[:, :, :, :n].contiguous().view(F8).float() * vs_c[:, :, None, :n]).to(BF)
    assert torch.equal(kd.cpu()[:, :, :n], want_k) and torch.equal(vd.cpu()[:, :, :, :n], want_v)
    assert bool((kd.cpu()[:, :, n:] == 7).all()) and bool((vd.cpu()[:, :, :, n:] == 7).all())


# ------------------------------------------------------------------ 2. decode attention
def _attn_case(B, H, Hkv, hd, Sk, seed):
    """caches whose tail (positions >= Sk, scales included) holds the e4m3 NaN code / inf, and the same with a zero tail"""
    Smax = (Sk + 63) // 64 * 64 + 64
    k, v = _kv_rows(B, Hkv, Sk, hd, seed=seed)
    ksrc, vsrc = _src_pair(k, v, Sk, 0)
    bad = _caches(B, Hkv, hd, Smax, byte=R.NAN_BYTE, scale=float("inf"))
    ops.kv_quantize_fp8(ksrc, vsrc, 0, *bad, Sk, 0)
    clean = [t.clone() for t in bad]
    for t, dim in zip(clean, (2, 3, 2, 2)):
        t.narrow(dim, Sk, Smax - Sk).zero_()
    q = rt(gen(B, H, hd, seed=seed + 7))
    return q, bad, clean


def _run_attn(q, caches, B, H, Hkv, hd, Sk, fused):
    qd = q.to(BF).to(DEV).view(B, H * hd)
    out = torch.full((B, H * hd), float("nan"), dtype=BF, device=DEV)
    scratch = torch.full((ops.attention_scratch_floats(B, H, hd, Sk),), float("nan"), dtype=torch.float32, device=DEV)
    ctr = torch.zeros(B * H, dtype=torch.int32, device=DEV) if fused else None
    ops.attention_decode_fp8kv(qd, *caches, out, B, Sk, H, Hkv, hd, scratch, ctr)
    if fused:
        assert int(ctr.abs().sum()) == 0, "the arrival counters are left at zero"
    return out.float().cpu().view(B, H, hd)


ATTN_SHAPES = [(1, 2, 2, 64, 1), (2, 4, 2, 128, 7), (3, 8, 8, 128, 65), (1, 2, 1, 64, 513), (2, 32, 32, 128, 577),
               (1, 2, 2, 128, 1500)]            # the last one: few (batch, head) pairs and a long context -> more than 8 key ranges


@pytest.mark.parametrize("B,H,Hkv,hd,Sk", ATTN_SHAPES)
def test_decode_attention_fp8kv(B, H, Hkv, hd, Sk):
    """Reference: fp64 attention over the cache bytes the GPU quantiser wrote, so the inputs are exact and only the fp32 order
    differs; the bound is the bf16 decode-attention test's against its oracle (tests/test_gpu_kernels.py: rtol 2^-7, atol 4e-3)."""
    q, bad, clean = _attn_case(B, H, Hkv, hd, Sk, seed=B + H + Sk)
    want = R.decode_attention_fp64(q, *[t.cpu() for t in clean], Sk).float()
    ns = ops.attention_decode_fp8kv_splits(B, H, Sk)
    if Sk == 1500:
        assert ns > 8, ns
    if Sk == 513:
        assert 1 < ns <= 8, ns
    got = _run_attn(q, bad, B, H, Hkv, hd, Sk, fused=False)
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    print(f"nsplit {ns}: max err {float(err.max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    assert bool((err <= 4e-3 + 2 ** -7 * want.abs()).all()), float(err.max())
    assert torch.equal(got, _run_attn(q, clean, B, H, Hkv, hd, Sk, fused=False)), "the cache tail must not reach the result"
    assert torch.equal(got, _run_attn(q, bad, B, H, Hkv, hd, Sk, fused=True)), "fused-combine form != stand-alone form"


# ------------------------------------------------------------------ models
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}


def _weights(hd, seed=0, std=0.05, vocab=VOCAB, max_seq_len=128):
    oargs = ref_cpu.OracleArgs(vocab_size=vocab, max_seq_len=max_seq_len, **GEOM[hd])
    return oargs, ref_cpu.make_decoder_weights(oargs, seed=seed, std=std)


def _model(hd, sd, kv=None, weights=None, vocab=VOCAB, max_seq_len=128):
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=vocab, max_seq_len=max_seq_len, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    if kv is not None:
        m.quantize_kv_cache(kv)
    return m


def _tokens(B, T, seed, vocab=VOCAB):
    ex = torch.randint(3, vocab, (B, T), generator=torch.Generator().manual_seed(seed))
    ex[:, 0] = 1
    return ex.to(DEV)


def _kv8_clone(m):
    return {k: [t.clone() for t in m._kv8[k]] for k in ("k_q", "vt_q", "k_scale", "v_scale")}


# ------------------------------------------------------------------ 3. prefill untouched
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_is_bit_identical_and_fills_the_fp8_cache(hd):
    _, sd = _weights(hd)
    ma, mb = _model(hd, sd), _model(hd, sd, kv="fp8")
    B, T = 2, 21
    ex = _tokens(B, T, seed=5)
    la, lb = ma.forward_inference(ex, 0), mb.forward_inference(ex, 0)
    assert torch.equal(la, lb), "prefill logits with an fp8 KV cache must equal the bf16-cache model's bit for bit"
    assert mb._kv8 is not None and mb._k_cache[0] is mb._k_cache[1], "one shared bf16 pair"
    Hkv, Smax = ma.n_kv_heads, ma._k_cache[0].shape[2]
    for i in range(ma.n_layers):
        kq, vq, ks, vs = _caches(B, Hkv, hd, Smax, byte=0, scale=0.0)
        ops.kv_quantize_fp8(ma._k_cache[i], ma._vt_cache[i], 0, kq, vq, ks, vs, T, 0)
        for name, want in (("k_q", kq), ("vt_q", vq), ("k_scale", ks), ("v_scale", vs)):
            assert torch.equal(mb._kv8[name][i], want), (i, name)
    # None restores the bf16 cache (and drops the fp8 one)
    mb.quantize_kv_cache(None)
    assert mb._kv8 is None and mb._cache_shape is None
    assert torch.equal(mb.forward_inference(ex, 0), la) and mb._k_cache[0] is not mb._k_cache[1]


# ------------------------------------------------------------------ 4. step structure
def _per_kernel_step(m, tok, pos):
    """One decode step of an fp8-KV model as the sequence of public entries (no fused GEMV forms): rmsnorm, GEMV, rope_kvcache into
    the staging pair, a3v_kv_quantize_fp8, a3v_attention_decode_fp8kv, GEMV + residual, rmsnorm, GEMV SwiGLU, GEMV + residual."""
    a, kv8 = m.args, m._kv8
    B = tok.shape[0]
    H, Hkv, hd, dim = m.n_heads, m.n_kv_heads, m.head_dim, a.dim
    h = torch.empty(B, dim, dtype=BF, device=DEV)
    ops.embed_assemble(tok.contiguous(), m.tok_embeddings.weight, h, B, 1, 0, dim)
    xn, qkv = torch.empty_like(h), torch.empty(B, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
    att, act = torch.empty(B, H * hd, dtype=BF, device=DEV), torch.empty(B, m.ffn, dtype=BF, device=DEV)
    scratch = torch.empty(ops.attention_scratch_floats(B, H, hd, pos + 1), dtype=torch.float32, device=DEV)
    pk, fmt, images = m._pack(), m.weight_format, None if m._weights is None else m._weights.images

    def lin(x, i, key, out, **kw):
        idx = ("wqkv", "wo", "w13", "w2").index(key)
        ws = m._skinny_ws(B, out.shape[1] * (2 if kw.get("epilogue") == ops.EPI_SWIGLU else 1), x.shape[1])
        if fmt == "nf4":
            return ops.gemm_skinny_nf4(x, *images[f"{key}.{i}"], out, ws, **kw)
        if fmt == "fp8":
            return ops.gemm_skinny_fp8(x, *images[f"{key}.{i}"], out, ws, **kw)
        assert fmt == "bf16"
        lyr = m.layers[i]
        w = (pk[f"wqkv.{i}"], lyr.attention.wo.weight, pk[f"w13.{i}"], lyr.feed_forward.w2.weight)[idx]
        return ops.gemm_skinny(x, w, out, ws, **kw)
    for i, lyr in enumerate(m.layers):
        fp8c = (kv8["k_q"][i], kv8["vt_q"][i], kv8["k_scale"][i], kv8["v_scale"][i])
        ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
        lin(xn, i, "wqkv", qkv)
        ops.rope_kvcache(qkv, qkv, kv8["stage_k"], kv8["stage_vt"], m._cos_sin_dev(), B, 1, H, Hkv, hd, 0, pos)
        ops.kv_quantize_fp8(kv8["stage_k"], kv8["stage_vt"], 0, *fp8c, 1, pos)
        ops.attention_decode_fp8kv(qkv, *fp8c, att, B, pos + 1, H, Hkv, hd, scratch)
        lin(att, i, "wo", h, residual=h, epilogue=ops.EPI_RESIDUAL)
        ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
        lin(xn, i, "w13", act, epilogue=ops.EPI_SWIGLU)
        lin(act, i, "w2", h, residual=h, epilogue=ops.EPI_RESIDUAL)
    ops.rmsnorm(h, m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(B, a.vocab_size, dtype=torch.float32, device=DEV)
    m._lm_head_f32(xn, logits)
    return logits


@pytest.mark.parametrize("weights", [None, "fp8", "nf4"])
def test_step_kv8_equals_the_per_kernel_sequence(weights):
    _, sd = _weights(128)
    m = _model(128, sd, kv="fp8", weights=weights)
    B, T = 4, 20
    from a3vlm_amd import lib
    w8 = {None: 0, "fp8": 1, "nf4": 2}[weights]
    assert lib.load().a3v_llama_decode_step_form(B, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, w8) == 2
    ex = _tokens(B, T, seed=6)
    m.forward_inference(ex[:, :T - 1], 0)
    after_prefill = _kv8_clone(m)
    fused = m.forward_inference(ex[:, T - 1:], T - 1).clone()
    cache_fused = _kv8_clone(m)
    for k, ts in after_prefill.items():                     # same cache state, then the same step kernel by kernel
        for t, src in zip(m._kv8[k], ts):
            t.copy_(src)
    per = _per_kernel_step(m, ex[:, T - 1:], T - 1)
    print(f"weights {weights}: max |fused - per kernel| = {float((fused - per).abs().max()):.3e} of max |logit| {float(fused.abs().max()):.3e}")
    for k in cache_fused:
        for i, (x, y) in enumerate(zip(cache_fused[k], m._kv8[k])):
            assert torch.equal(x, y), (k, i)
    assert torch.equal(fused, per)


def test_step_kv8_two_row_chunks():
    """B = 18 runs as two chunks of 9 rows inside the C call: equal to two B = 9 steps on the same cache rows (offsets of caches, scales,
    staging pair and activations)."""
    _, sd = _weights(128)
    m = _model(128, sd, kv="fp8")
    B, T = 18, 12
    ex = _tokens(B, T, seed=7)
    m.forward_inference(ex[:, :T - 1], 0)
    big = _kv8_clone(m)
    l18 = m.forward_inference(ex[:, T - 1:], T - 1).clone()
    new18 = _kv8_clone(m)
    for r0 in (0, 9):
        m._allocate_kv_cache(9)                             # fresh caches of 9 rows, filled with the rows the B = 18 prefill wrote
        for k in big:
            for t, src in zip(m._kv8[k], big[k]):
                t.copy_(src[r0:r0 + 9])
        l9 = m.forward_inference(ex[r0:r0 + 9, T - 1:], T - 1)
        assert torch.equal(l9, l18[r0:r0 + 9]), r0
        for k in big:
            for t, src in zip(m._kv8[k], new18[k]):
                assert torch.equal(t, src[r0:r0 + 9]), (k, r0)


def test_continuation_of_five_tokens():
    """S = 5 at start_pos = 11: each layer's prefix is dequantised into the shared pair, the layer runs in bf16, the five new positions
    are quantised.  Layer 0's K / V do not depend on the cache, so its fp8 rows equal the quantiser over the bf16 model's; in the last
    layer (whose bf16 K / V the shared pair still holds) the two models' rows differ by the prefix's quantisation noise, and the
    dequantised rows then differ by at most that difference plus one e4m3 step (two roundings to nearest of half a step each)."""
    hd = 64
    _, sd = _weights(hd)
    ma, mb = _model(hd, sd), _model(hd, sd, kv="fp8")
    B, P, S = 2, 11, 5
    ex = _tokens(B, P + S, seed=8)
    for m in (ma, mb):
        m.forward_inference(ex[:, :P], 0)
    la, lb = ma.forward_inference(ex[:, P:], P), mb.forward_inference(ex[:, P:], P)
    assert torch.isfinite(lb).all()
    scale = float(la.abs().max())
    print(f"continuation logits: max |fp8 kv - bf16 kv| / max |logit| = {float((la - lb).abs().max()) / scale:.3e}")
    Hkv, Smax, L = ma.n_kv_heads, ma._k_cache[0].shape[2], ma.n_layers
    sl = slice(P, P + S)
    for i in (0, L - 1):
        kq, vq, ks, vs = _caches(B, Hkv, hd, Smax, byte=0, scale=0.0)
        ops.kv_quantize_fp8(ma._k_cache[i], ma._vt_cache[i], P, kq, vq, ks, vs, S, P)
        got = [mb._kv8[k][i] for k in ("k_q", "vt_q", "k_scale", "v_scale")]
        if i == 0:
            assert torch.equal(got[0][:, :, sl], kq[:, :, sl]) and torch.equal(got[1][:, :, :, sl], vq[:, :, :, sl])
            assert torch.equal(got[2][:, :, sl], ks[:, :, sl]) and torch.equal(got[3][:, :, sl], vs[:, :, sl])
            continue
        xa = (ma._k_cache[i][:, :, sl].float().cpu(), ma._vt_cache[i][:, :, :, sl].float().cpu().transpose(2, 3))
        xb = (mb._k_cache[i][:, :, sl].float().cpu(), mb._vt_cache[i][:, :, :, sl].float().cpu().transpose(2, 3))
        codes_a = (kq[:, :, sl].cpu(), vq[:, :, :, sl].cpu().transpose(2, 3).contiguous())
        codes_b = (got[0][:, :, sl].cpu(), got[1][:, :, :, sl].cpu().transpose(2, 3).contiguous())
        for j, (sa, sb) in enumerate(((ks, got[2]), (vs, got[3]))):
            sa, sb = sa[:, :, sl].cpu(), sb[:, :, sl].cpu()
            da, db = codes_a[j].view(F8).float() * sa[..., None], codes_b[j].view(F8).float() * sb[..., None]
            same = (xa[j] == xb[j]).all(-1)                                    # rows whose bf16 values agree: the same codes
            assert torch.equal(codes_a[j][same], codes_b[j][same]) and torch.equal(sa[same], sb[same])
            step = torch.maximum(R.e4m3_step(xa[j].double() / sa[..., None].double()) * sa[..., None].double(),
                                 R.e4m3_step(xb[j].double() / sb[..., None].double()) * sb[..., None].double())
            assert bool(((da - db).abs().double() <= (xa[j] - xb[j]).abs().double() + step * (1 + 1e-6)).all()), ("kv"[j], i)


# ------------------------------------------------------------------ 5. accuracy
class _FakeQuantOracle(ref_cpu.OracleDecoder):
    """OracleDecoder whose cache rows go through quantise -> dequantise (tests/kv8_ref.py) after every write.  As in the product, a
    prefill attends over the rows it has just computed and the cache keeps their quantised form; a decode step reads every key,
    the new one included, from the cache."""

    def attention(self, i, x, start_pos, freqs_cis, mask):
        p = f"layers.{i}.attention."
        bsz, seqlen, _ = x.shape
        xq = self.lin(x, p + "wq").view(bsz, seqlen, self.args.n_heads, self.head_dim)
        xk = self.lin(x, p + "wk").view(bsz, seqlen, self.n_kv_heads, self.head_dim)
        xv = self.lin(x, p + "wv").view(bsz, seqlen, self.n_kv_heads, self.head_dim)
        xq, xk = ref_cpu.apply_rotary_emb(xq, xk, freqs_cis)
        self.k_cache[i] = self.k_cache[i].to(xk)
        self.v_cache[i] = self.v_cache[i].to(xv)
        sl = slice(start_pos, start_pos + seqlen)
        self.k_cache[i][:bsz, sl] = R.fake_quant(xk)
        self.v_cache[i][:bsz, sl] = R.fake_quant(xv)
        keys = self.k_cache[i][:bsz, :start_pos + seqlen].clone()
        values = self.v_cache[i][:bsz, :start_pos + seqlen].clone()
        if seqlen > 1:
            keys[:, sl], values[:, sl] = xk, xv
        keys = ref_cpu.repeat_kv(keys, self.n_rep).transpose(1, 2)
        values = ref_cpu.repeat_kv(values, self.n_rep).transpose(1, 2)
        m = ref_cpu.make_causal_mask(seqlen, keys.size(2)) if mask == "causal" else None
        out = ref_cpu.sdpa(xq.transpose(1, 2), keys, values, m).transpose(1, 2).contiguous().view(bsz, seqlen, -1)
        return self.lin(out, p + "wo")


# weights / vocabulary chosen on the CPU from the oracle alone: with these, 10 of the 16 (step, row) argmaxes have a top-2 margin above
# twice the bound (a small vocabulary keeps the margins wide, a small std keeps the attention flat and D small)
ACC = dict(hd=64, seed=11, std=0.03, vocab=16, B=2, T0=9, steps=8)


def _oracle_runs():
    """Greedy decode of the fake-quantised oracle (bf16 weights, as the bf16 model test) and the plain oracle fed the SAME tokens:
    (prompt, ids [steps, B], fake-quantised logits per step, D = their largest deviation)."""
    c = ACC
    oargs, sd = _weights(c["hd"], seed=c["seed"], std=c["std"], vocab=c["vocab"])
    sdb = {k: v.to(BF) for k, v in sd.items()}
    fq, plain = _FakeQuantOracle(oargs, sdb), ref_cpu.OracleDecoder(oargs, sdb)
    ex = _tokens(c["B"], c["T0"], seed=12, vocab=c["vocab"]).cpu()
    lq, lp = [fq.forward_inference(ex, 0).float()], [plain.forward_inference(ex, 0).float()]
    ids = []
    for t in range(c["steps"] - 1):
        ids.append(lq[-1].argmax(-1))
        lq.append(fq.forward_inference(ids[-1][:, None], c["T0"] + t).float())
        lp.append(plain.forward_inference(ids[-1][:, None], c["T0"] + t).float())
    ids.append(lq[-1].argmax(-1))
    D = max(float((a - b).abs().max()) for a, b in zip(lq, lp))
    return sd, ex, torch.stack(ids), lq, D


def test_greedy_decode_against_the_fake_quantised_oracle():
    """Allowed deviation of a step's logits: the bf16 model test's bound against its oracle (4e-2 of max |logit|,
    tests/test_gpu_model.py) plus D, the deviation between the fake-quantised and the plain oracle on the same inputs -- a bf16
    rounding difference in K can flip an e4m3 code, an error of the size of the quantisation noise itself."""
    c = ACC
    sd, ex, ids, want, D = _oracle_runs()
    scale = max(float(w.abs().max()) for w in want)
    bound = 4e-2 * scale + D
    m = _model(c["hd"], sd, kv="fp8", vocab=c["vocab"])
    got = [m.forward_inference(ex.to(DEV), 0).float().cpu()]
    for t in range(c["steps"] - 1):
        got.append(m.forward_inference(ids[t][:, None].to(DEV), c["T0"] + t).float().cpu())
    decided = 0
    for t, (g_, w) in enumerate(zip(got, want)):
        err = float((g_ - w).abs().max())
        top = w.topk(2, dim=-1).values
        sure = (top[:, 0] - top[:, 1]) > 2 * bound
        print(f"step {t}: err {err:.3e} (bound {bound:.3e} = 4e-2 * {scale:.3e} + D {D:.3e}); decided rows {int(sure.sum())}/{len(sure)}")
        assert err <= bound, (t, err, bound)
        assert torch.equal(g_.argmax(-1)[sure], w.argmax(-1)[sure]), t
        decided += int(sure.sum())
    assert 2 * decided >= c["steps"] * c["B"], decided


# ------------------------------------------------------------------ 6. entry points
DEC = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256, norm_eps=1e-5, rope_theta=10000.0)
VIT = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    tmp = tmp_path_factory.mktemp("kv8ck")
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps({**DEC, **VIT}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=512, **DEC), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(DEC["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    args = types.SimpleNamespace(precision="tf32", only_save_trainable=False)
    ckdir = ck.save_checkpoint(str(tmp / "ck"), args, mm, None, None, None, epoch=0)
    return cfgp, ckdir, tmp


@pytest.mark.parametrize("quant", [None, True, "nf4"])
def test_from_pretrained_kv_quant_generate(ckpt, quant):
    from a3vlm_amd.model.meta import MetaModel
    cfgp, ckdir, _ = ckpt
    mm = MetaModel.from_pretrained(ckdir, llama_type="llama_ens5", llama_config=[str(cfgp)], tokenizer_path=os.path.join(GD, "tokenizer.model"),
                                   with_visual=True, max_seq_len=512, quant=quant or False, kv_quant="fp8")
    assert mm.llma._kv_quant == "fp8"
    assert mm.llma.weight_format == {None: "bf16", True: "fp8", "nf4": "nf4"}[quant]
    prompt, n = "Detect all manipulable object parts.", 10
    _, ids = mm.generate([prompt], None, max_gen_len=n, temperature=0, return_ids=True)
    assert mm.llma._kv8 is not None and mm.llma._kv8["k_q"][0].dtype == torch.uint8
    tok = mm.tokenizer.encode(prompt, bos=True, eos=False)
    seq, step_ids = torch.tensor([tok], device=DEV), []
    logits = mm.llma.forward_inference(seq, 0)                       # the same object driven step by step
    for j in range(n):
        nxt = int(logits.argmax(-1))
        if nxt == mm.tokenizer.eos_id:
            break
        step_ids.append(nxt)
        logits = mm.llma.forward_inference(torch.tensor([[nxt]], device=DEV), len(tok) + j)
    assert ids[0] == step_ids and len(step_ids) > 0, (ids[0], step_ids)


def test_eval_affordance_with_quant_kv_quant_demo(ckpt):
    cfgp, ckdir, tmp = ckpt
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_with_quant", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2",
           "--num_workers", "0", "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224",
           "--max_gen_len", "10", "--max_seq_len", "512", "--temperature", "0", "--image_root", os.path.join(GD, "demo"),
           "--output_root", str(tmp / "logs"), "--precision", "bf16", "--addition_flag", "kv8", "--kv_quant", "fp8"]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = json.load(open(tmp / "logs" / "kv8" / "demo.json"))
    assert len(recs) == 3 and set(recs[0]) == {"answer", "format_answer", "annotation", "question", "image", "fail"}
    assert recs[0]["answer"] == recs[1]["answer"]          # the three demo items share image and question
