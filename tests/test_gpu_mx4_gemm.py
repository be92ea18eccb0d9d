"""The W4A8 GEMM on MXFP4 images on the GPU: the MXFP8 row quantiser bit-equal to tests/mx4_gemm_ref.py (and, with its RMSNorm prologue,
to a3v_rmsnorm followed by the plain form); a3v_gemm_nt_mxfp4 bit-exact on an exactly representable family at every tile edge of its
plan, inside the derived bound on reals, equal to the decode GEMV where both run, repeatable; the model paths of
quantize_decode_weights("mxfp4", prefill=True) against the sequence of public ops and a fake-quantised oracle."""
import os

import numpy as np
import pytest
import torch

import mx4_gemm_ref as G
import mx4_ref as R
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPIS = {"none": 0, "residual": ops.EPI_RESIDUAL, "swiglu": ops.EPI_SWIGLU, "f32": ops.EPI_OUT_F32}


def _bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(BF)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _image_on_gpu(q, s, pad=32):
    """Codes in a 0xFF-filled buffer with a padded row stride, scales with 0xFF margins (0xFF = the NaN scale: never to be read)."""
    N, K2 = q.shape
    qb = torch.full((N + 2, K2 + pad), 0xFF, dtype=torch.uint8, device=DEV)
    qb[1:N + 1, :K2] = torch.from_numpy(q).to(DEV)
    sb = torch.full((s.size + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    sb[32:32 + s.size] = torch.from_numpy(s.reshape(-1)).to(DEV)
    return qb[1:N + 1, :K2], sb[32:32 + s.size].view(s.shape)


# ------------------------------------------------------------------ row quantiser
def _quantise_on_gpu(x, norm_w=None, eps=0.0):
    """x [rows, K] bf16 (CPU) in a NaN-filled buffer with a padded stride; codes and exponents in 0xA5-filled buffers: the windows (GPU)
    after checking that nothing outside them was written."""
    rows, K = x.shape
    xb = torch.full((rows + 2, K + 8), float("nan"), dtype=BF, device=DEV)
    xb[1:rows + 1, :K] = x.to(DEV)
    qb = torch.full((rows + 2, K + 48), 0xA5, dtype=torch.uint8, device=DEV)
    eb = torch.full((rows * (K // 32) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    q, e = qb[1:rows + 1, :K], eb[32:32 + rows * (K // 32)].view(rows, K // 32)
    ops.quantize_rows_mxfp8(xb[1:rows + 1, :K], q, e, None if norm_w is None else norm_w.to(DEV), eps)
    torch.cuda.synchronize()
    assert bool((qb[0] == 0xA5).all() and (qb[-1] == 0xA5).all() and (qb[:, K:] == 0xA5).all()), "codes: nothing outside the window"
    assert bool((eb[:32] == 0xA5).all() and (eb[-32:] == 0xA5).all()), "exponents: nothing outside the window"
    return q, e


def _rows_input(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-12, 9, (rows, K // 32, 1), generator=g).float()).expand(rows, K // 32, 32).reshape(rows, K)
    x = x.to(BF).float()
    x[0, :32] = 0.0                                                 # zero block
    x[0, 32:64] = -0.0                                              # a zero block of negative zeros
    x[0, 64:96] = 0.0                                               # saturation edge at E = 0: 448 < 464, 480, 500 -> 448; 449 is no bf16 value
    x[0, 64:70] = torch.tensor([500.0, 464.0, -480.0, 448.0, 432.0, 440.0])
    x[0, 96:128] = 0.0                                              # e4m3 subnormals at E = 0 (max 256): below 2^-6 the step is 2^-9
    x[0, 96:104] = torch.tensor([256.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10, -(2.0 ** -11), 5 * 2.0 ** -10, -(2.0 ** -7)])
    r = rows - 1                                                    # the last row too (rows = 1: the same row, other blocks where K allows)
    if K >= 256:
        x[r, K - 32:] = 0.0
        x[r, K - 64:K - 32] = 0.0
        x[r, K - 64:K - 60] = torch.tensor([3.0e38, 1.0, -2.0 ** -120, 2.0 ** 100])    # one huge element: E = 126 - 8
        x[r, K - 96:K - 64] = torch.tensor(2.0 ** -130)             # bf16 denormals: E = -138 clamps to -127
    return x.to(BF)


@pytest.mark.parametrize("rows,K", [(1, 128), (33, 384), (5, 11008)])
def test_row_quantiser_equals_the_restatement(rows, K):
    x = _rows_input(rows, K, seed=rows + K)
    aq, ea = G.quant_rows(_np(x))
    q, e = _quantise_on_gpu(x)
    assert np.array_equal(e.cpu().numpy(), (ea + 127).astype(np.uint8)), "block exponents"
    assert np.array_equal(q.cpu().numpy(), G.e4m3_bytes(aq)), "e4m3 codes"
    assert int(e[0, 0]) == 127 and int(e[0, 1]) == 127 and not q[0, :64].any(), "zero blocks: byte 127, codes 0"
    assert not (e == 0xFF).any()


@pytest.mark.parametrize("rows,K", [(1, 128), (33, 384), (5, 8192)])      # 8192: the widest row a3v_rmsnorm itself takes
def test_rmsnorm_prologue_equals_rmsnorm_then_the_plain_quantiser(rows, K):
    g = torch.Generator().manual_seed(rows * K)
    x = (torch.randn(rows, K, generator=g) * 3.0).to(BF)
    x[0, :32] = 0.0
    w = (1.0 + 0.2 * torch.randn(K, generator=g)).to(BF)
    w[40:44] = 0.0                                                  # a zero weight inside a block
    q1, e1 = _quantise_on_gpu(x, w, 1e-5)
    y = torch.empty(rows, K, dtype=BF, device=DEV)
    ops.rmsnorm(x.to(DEV), w.to(DEV), y, 1e-5)
    q2, e2 = _quantise_on_gpu(y.cpu())
    assert torch.equal(q1, q2) and torch.equal(e1, e2)
    aq, ea = G.quant_rows(_np(y))
    assert np.array_equal(q1.cpu().numpy(), G.e4m3_bytes(aq)) and np.array_equal(e1.cpu().numpy(), (ea + 127).astype(np.uint8))


# ------------------------------------------------------------------ GEMM
def _run_gemm(a, q, s, epi, res=None):
    """a [M, K] bf16 (CPU) quantised on the GPU, the output in a sentinel-filled buffer; returns the window (CPU) after checking the rest."""
    M, K = a.shape
    N = q.shape[0]
    aq, ea = _quantise_on_gpu(a)
    ncol = N // 2 if epi == ops.EPI_SWIGLU else N
    odt = torch.float32 if epi & ops.EPI_OUT_F32 else BF
    cb = torch.full((M + 2, ncol + 8), -12345.0, dtype=odt, device=DEV)
    ops.gemm_nt_mxfp4(aq, ea, q, s, cb[1:M + 1, :ncol], residual=None if res is None else res.to(DEV), epilogue=epi & ~ops.EPI_RESIDUAL)
    torch.cuda.synchronize()
    assert bool((cb[0] == -12345.0).all() and (cb[-1] == -12345.0).all() and (cb[:, ncol:] == -12345.0).all()), "nothing outside the output window"
    return cb[1:M + 1, :ncol].cpu()


def _run_gemv(a, q, s, epi, res=None):
    """The decode GEMV (a3v_gemm_skinny_mxfp4) on the same operands, 16 rows per call."""
    M, K = a.shape
    N = q.shape[0]
    ncol = N // 2 if epi == ops.EPI_SWIGLU else N
    out = torch.empty(M, ncol, dtype=torch.float32 if epi & ops.EPI_OUT_F32 else BF, device=DEV)
    ws = torch.zeros((ops.gemm_skinny_mxfp4_ws_bytes(min(M, 16), N, K) + 3) // 4, dtype=torch.float32, device=DEV)
    ad = a.to(DEV)
    for r0 in range(0, M, 16):
        ops.gemm_skinny_mxfp4(ad[r0:r0 + 16], q, s, out[r0:r0 + 16], ws, residual=None if res is None else res[r0:r0 + 16].to(DEV),
                              epilogue=epi & ~ops.EPI_RESIDUAL)
    return out.cpu()


def _exact_case(M, N, K, seed):
    """Weights on the e2m1 grid times block powers of two in 2^-6 .. 2^6, activations integers |a| <= 8 times block powers of two: every
    product is a multiple of one quantum and sum |a w| stays below 2^24 quanta, so fp32 accumulation is exact in any order."""
    rng = np.random.default_rng(seed)
    nb = K // 32
    grid = np.concatenate([R.E2M1, -R.E2M1[1:]])
    ew = rng.integers(-6, -2, size=(N, nb))
    for r in range(N):                                              # two blocks per row anywhere in the range
        ew[r, rng.integers(0, nb, size=2)] = rng.integers(-6, 5, size=2)
    wv = grid[rng.integers(0, 15, size=(N, nb, 32))]
    rs, bs = N // 2 + 1, nb // 2                                    # the one block with the top scale holds one value no other block can have
    ew[rs, bs] = 6
    wv[rs, bs] = 0.0
    wv[rs, bs, 13] = -6.0
    W = np.ldexp(wv, ew[..., None]).reshape(N, K)
    ea = rng.integers(-1, 2, size=(M, nb))
    ai = rng.integers(-8, 9, size=(M, nb, 32))
    ai[:, bs, 13] = rng.choice([-7, -5, -3, 3, 5, 7], size=M)       # the marker weight always meets a nonzero activation
    A = np.ldexp(ai.astype(np.float64), ea[..., None]).reshape(M, K)
    quantum = 2.0 ** (-6 - 1 - 1)
    assert (np.abs(A) @ np.abs(W).T).max() / quantum < 2 ** 24
    q, s = R.quantize(W)
    assert np.array_equal(R.dequantize(q, s), W) and np.array_equal(R.fake_quant_act(A), A), "both operands are exact in their MX formats"
    return A, q, s


def _plan_edges():
    """What the exact family walks, read from the planner: every tile-row count it returns (over M 1..600 of the five 7B shapes), the
    tile columns of the plain and the SwiGLU form, the K stage."""
    rows, cols, cols_sw, stage, slices = set(), set(), set(), set(), set()
    for N, K, epi in ((12288, 4096, 0), (4096, 4096, ops.EPI_RESIDUAL), (22016, 4096, ops.EPI_SWIGLU), (4096, 11008, ops.EPI_RESIDUAL),
                      (32000, 4096, ops.EPI_OUT_F32)):
        for M in range(1, 601):
            rc, p = ops.mx4_gemm_plan(M, N, K, epi)
            assert rc == 0
            rows.add(p[0]); (cols_sw if epi == ops.EPI_SWIGLU else cols).add(p[1]); stage.add(p[2]); slices.add(p[6])
    assert len(cols) == 1 and len(cols_sw) == 1 and len(stage) == 1
    assert slices == {1}, "a split-K plan exists: the exact family must include a shape that takes it"
    return sorted(rows), cols.pop(), cols_sw.pop(), stage.pop()


ROWS, COLS, COLS_SW, STAGE = _plan_edges()
EXACT_M = sorted({1, 17, 33} | {r + d for r in ROWS for d in (-1, 0, 1)})
EXACT_K = (128, STAGE, STAGE + 128, 3 * STAGE)


def _exact_check(M, N, K, name, gemv=False):
    """One exact case, one epilogue: the GEMM's bits against the restatement's; SwiGLU (no correctly rounded silu on the device) against
    the decode GEMV's SwiGLU epilogue on the same exact accumulators -- the same device expression -- and within the bound."""
    epi = EPIS[name]
    A, q, s = _exact_case(M, N, K, seed=M * 7 + N + K + (epi != 0))
    aq, ea = G.quant_rows(A)
    qd, sd = _image_on_gpu(q, s)
    a = _bf(A)
    acc = A @ R.dequantize(q, s).T
    res = _bf(np.random.default_rng(1).standard_normal((M, N)) * np.abs(acc).max()) if name == "residual" else None
    r = G.reference(aq, ea, q, s, epi, None if res is None else _np(res))
    got = _run_gemm(a, qd, sd, epi, res)
    if name == "swiglu":
        want = _run_gemv(a, qd, sd, epi)
        assert torch.equal(got, want), (M, N, K, name, float((got.float() - want.float()).abs().max()))
        assert G.ratio(_np(got), r) <= 1.0
        cpu = G.swiglu_on_exact(acc)
        assert (np.abs(_np(got) - cpu) <= 2.0 ** -6 * np.abs(cpu) + 1e-30).all(), "two bf16 steps of the CPU SwiGLU"
        return
    assert got.dtype == (torch.float32 if name == "f32" else BF)
    assert np.array_equal(_np(got), r["bits"]), (M, N, K, name, float(np.abs(_np(got) - r["bits"]).max()))
    if gemv:
        assert torch.equal(got, _run_gemv(a, qd, sd, epi, res)), (M, N, K, name)


@pytest.mark.parametrize("M", EXACT_M)
def test_gemm_exact_family(M):
    rc, plan = ops.mx4_gemm_plan(M, COLS + 16, 3 * STAGE)
    print(f"M {M}: tile {plan[0]} x {plan[1]}, K stage {plan[2]}, grid {plan[3]}, {plan[6]} K slice(s)")
    for K in EXACT_K:
        for N in (16, 48, COLS + 16):
            for name in ("none", "residual", "f32"):
                _exact_check(M, N, K, name)
        for N in (32, 64, COLS_SW + 32):                           # SwiGLU: N counts gate / up rows in 16-row pairs
            _exact_check(M, N, K, "swiglu")


RANDOM = [(5, 48, 640), (24, 80, 1152), (40, 96, 512), (200, 144, 1536)]


def _random_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
    q, s = R.quantize(_np(w))
    aq, ea = G.quant_rows(_np(a))
    return a, q, s, aq, ea, g


@pytest.mark.parametrize("M,N,K", RANDOM, ids=lambda v: str(v))
def test_gemm_random_family_inside_the_derived_bound(M, N, K):
    rc, plan = ops.mx4_gemm_plan(M, N, K)
    assert plan[0] == {5: 16, 24: 32, 40: 64, 200: 128}[M], "one shape per plan family"
    a, q, s, aq, ea, g = _random_case(M, N, K, seed=M + N + K)
    qd, sd = _image_on_gpu(q, s)
    res = torch.randn(M, N, generator=g).to(BF)
    for name in ("none", "residual", "f32"):
        r = G.reference(aq, ea, q, s, EPIS[name], _np(res) if name == "residual" else None)
        got = _run_gemm(a, qd, sd, EPIS[name], res if name == "residual" else None)
        rt = G.ratio(_np(got), r)
        print(f"{name}: max err / bound {rt:.3f}")
        assert rt <= 1.0, name
    Ns = (N + 31) // 32 * 32
    a, q, s, aq, ea, g = _random_case(M, Ns, K, seed=M + N + K + 1)
    qd, sd = _image_on_gpu(q, s)
    rt = G.ratio(_np(_run_gemm(a, qd, sd, ops.EPI_SWIGLU)), G.reference(aq, ea, q, s, ops.EPI_SWIGLU))
    print(f"swiglu (N {Ns}): max err / bound {rt:.3f}")
    assert rt <= 1.0


def test_lm_head_like_shape_inside_the_bound():
    M, N, K = 40, 2000, 512                                        # a vocabulary that is a multiple of 16 and of nothing larger
    a, q, s, aq, ea, g = _random_case(M, N, K, seed=4)
    got = _run_gemm(a, *_image_on_gpu(q, s), ops.EPI_OUT_F32)
    rt = G.ratio(_np(got), G.reference(aq, ea, q, s, ops.EPI_OUT_F32))
    print(f"max err / bound {rt:.3f}")
    assert got.dtype == torch.float32 and rt <= 1.0


@pytest.mark.parametrize("M", [1, 8, 16])
def test_gemv_and_gemm_agree(M):
    N, K = 96, 1152
    for name in EPIS:                                               # exact inputs: bit-equal (and equal to the restatement)
        _exact_check(M, N, K, name, gemv=True)
    a, q, s, aq, ea, g = _random_case(M, N, K, seed=M)
    qd, sd = _image_on_gpu(q, s)
    res = torch.randn(M, N, generator=g).to(BF)
    for name, epi in EPIS.items():
        rr = res if name == "residual" else None
        r = G.reference(aq, ea, q, s, epi, None if rr is None else _np(rr))
        rg, rv = G.ratio(_np(_run_gemm(a, qd, sd, epi, rr)), r), G.ratio(_np(_run_gemv(a, qd, sd, epi, rr)), r)
        print(f"{name}: GEMM {rg:.3f}, GEMV {rv:.3f} of the bound")
        assert rg <= 1.0 and rv <= 1.0, name


def test_calls_are_repeatable():
    for (M, N, K), epi in (((200, 144, 1536), 0), ((40, 96, 640), ops.EPI_SWIGLU), ((33, 80, 4096), ops.EPI_RESIDUAL)):
        a, q, s, aq, ea, g = _random_case(M, N, K, seed=9)
        qd, sd = _image_on_gpu(q, s)
        res = torch.randn(M, N, generator=g).to(BF) if epi == ops.EPI_RESIDUAL else None
        assert torch.equal(_run_gemm(a, qd, sd, epi, res), _run_gemm(a, qd, sd, epi, res)), (M, N, K, epi)


# ------------------------------------------------------------------ model
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}
LINEARS = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2", "feed_forward.w3")


def _model(hd, sd, prefill, vocab=VOCAB):
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=vocab, max_seq_len=128, max_batch_size=40, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    if prefill is not None:
        m.quantize_decode_weights("mxfp4", prefill=prefill)
    return m


def _weights(hd, seed=0):
    oargs = ref_cpu.OracleArgs(vocab_size=VOCAB, max_seq_len=128, **GEOM[hd])
    return ref_cpu.make_decoder_weights(oargs, seed=seed, std=0.05)


def _wd_state(sd, n_layers):
    """The state dict with every decoder linear and the LM head replaced by its Wd (tests/mx4_ref.py on the bf16 weight)."""
    out = dict(sd)
    for k in [f"layers.{i}.{n}.weight" for i in range(n_layers) for n in LINEARS] + ["output.weight"]:
        w = _np(sd[k].to(BF))
        out[k] = torch.from_numpy(R.dequantize(*R.quantize(w)).astype(np.float32))
    return out


def _tokens(B, T, seed):
    ex = torch.randint(3, VOCAB, (B, T), generator=torch.Generator().manual_seed(seed))
    ex[:, 0] = 1
    return ex.to(DEV)


def _public_ops_forward(m, tok, pos):
    """forward_inference(tok [B, S], pos) of a prefill=True model as the sequence of public ops on the model's caches: fp32 logits [B, V]."""
    a, mx, hd = m.args, m._weights.images, m.head_dim
    H, Hkv, dim = m.n_heads, m.n_kv_heads, a.dim
    B, S = tok.shape
    rows = B * S
    h = torch.empty(rows, dim, dtype=BF, device=DEV)
    ops.embed_assemble(tok.contiguous(), m.tok_embeddings.weight, h, B, S, 0, dim)
    qkv = torch.empty(rows, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
    att, act = torch.empty(rows, H * hd, dtype=BF, device=DEV), torch.empty(rows, m.ffn, dtype=BF, device=DEV)
    scratch = torch.empty(2 * ops.attention_scratch_floats(B, H, hd, a.max_seq_len + 64), dtype=torch.float32, device=DEV) if S == 1 else None

    def lin(x, img, out, norm_w=None, **kw):
        xq, xe = ops.quantize_rows_mxfp8(x, None, None, norm_w, a.norm_eps if norm_w is not None else 0.0)
        ops.gemm_nt_mxfp4(xq, xe, img.q, img.s, out, **kw)
    for i, lyr in enumerate(m.layers):
        kc, vc = m._k_cache[i], m._vt_cache[i]
        smax, ldq = kc.shape[2], qkv.stride(0)
        strides = (S * ldq, ldq, hd, Hkv * smax * hd, smax * hd, hd, Hkv * hd * smax, hd * smax, smax, S * H * hd, H * hd, hd)
        lin(h, mx[f"wqkv.{i}"], qkv, lyr.attention_norm.weight)
        ops.rope_kvcache(qkv, qkv, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, pos, pos)
        ops.attention(qkv, kc, vc, att, B, S, pos + S, H, Hkv, hd, strides, S > 1, scratch)
        lin(att, mx[f"wo.{i}"], h, residual=h)
        lin(h, mx[f"w13.{i}"], act, lyr.ffn_norm.weight, epilogue=ops.EPI_SWIGLU)
        lin(act, mx[f"w2.{i}"], h, residual=h)
    xn = torch.empty(B, dim, dtype=BF, device=DEV)
    ops.rmsnorm(h.view(B, S, dim)[:, -1, :], m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(B, a.vocab_size, dtype=torch.float32, device=DEV)
    lin(xn, mx["output"], logits, epilogue=ops.EPI_OUT_F32)
    return logits


def _against_public_ops(m, tok, pos):
    """The model's forward_inference against _public_ops_forward from the same cache state: logits and caches bit-equal."""
    if pos == 0:
        m.forward_inference(tok, 0)                                 # allocates the caches
        for t in m._k_cache + m._vt_cache:
            t.zero_()
    k0, v0 = [t.clone() for t in m._k_cache], [t.clone() for t in m._vt_cache]
    got = m.forward_inference(tok, pos).clone()
    k1, v1 = [t.clone() for t in m._k_cache], [t.clone() for t in m._vt_cache]
    for t, src in zip(m._k_cache + m._vt_cache, k0 + v0):
        t.copy_(src)
    want = _public_ops_forward(m, tok, pos)
    assert torch.equal(got, want), float((got - want).abs().max())
    for x, y in zip(k1 + v1, m._k_cache + m._vt_cache):
        assert torch.equal(x, y)


@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_and_33_row_step_equal_the_sequence_of_public_ops(hd):
    m = _model(hd, _weights(hd), True)
    assert m.weight_format == "mxfp4" and m._weights.images and m._weights.prefill is True
    _against_public_ops(m, _tokens(2, 21, seed=5), 0)               # 42 rows at S = 21
    B, T = 33, 6
    ex = _tokens(B, T, seed=9)
    _against_public_ops(m, ex[:, :T - 1], 0)                        # 165 rows
    _against_public_ops(m, ex[:, T - 1:], T - 1)                    # the 33-row decode step: S = 1, rows > 32
    assert "nf4_scratch" not in m._ws, "a prefill=True model never allocates the dequantisation scratch"


def test_teacher_forced_forward_and_ragged_rows_never_dequantise():
    hd = 64
    m = _model(hd, _weights(hd), True)
    ex = _tokens(2, 21, seed=5)
    out = m.forward(ex)                                             # compute_logits / evaluate_examples: every position's logits
    assert out.shape == (2, 21, VOCAB) and out.dtype == BF and bool(torch.isfinite(out.float()).all())
    assert torch.equal(out, m.forward(ex)) and "nf4_scratch" not in m._ws
    m.allocate_rows(33)
    for b in range(33):
        m.prefill_row(b, ex[:1, :4 + b % 3])
    pos = torch.tensor([4 + b % 3 for b in range(33)], dtype=torch.int32, device=DEV)
    lg = m.forward_inference_rows(ex[0, :1].repeat(33), pos, 6)
    assert bool(torch.isfinite(lg).all()) and torch.equal(lg[0], lg[3]), "rows in the same state give the same logits"
    assert "nf4_scratch" not in m._ws


@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_false_beside_it_is_still_weight_only(hd):
    """The default path next to a prefill=True model: bit-equal to the bf16 model that holds Wd, through the dequantisation scratch."""
    sd = _weights(hd)
    mp, mq, md = _model(hd, sd, True), _model(hd, sd, False), _model(hd, _wd_state(sd, 2), None)
    ex = _tokens(2, 21, seed=5)
    lp, lq, ld = mp.forward_inference(ex, 0), mq.forward_inference(ex, 0), md.forward_inference(ex, 0)
    assert torch.equal(lq, ld), "prefill=False: weight-only, the logits of the bf16 model on Wd"
    assert "nf4_scratch" in mq._ws and "nf4_scratch" not in mp._ws
    assert mq._weights.prefill is False and not torch.equal(lp, ld), "prefill=True quantises the activations: other logits"


class _FakeQuantOracle(ref_cpu.OracleDecoder):
    """OracleDecoder whose linears, the LM head included, see MXFP8 fake-quantised inputs (tests/mx4_ref.py quant_act_mxfp8) at every S:
    what a prefill=True model multiplies in its W4A8 GEMMs and in its decode GEMVs alike."""

    @staticmethod
    def _fq(x):
        flat = x.reshape(-1, x.shape[-1])
        return torch.from_numpy(R.fake_quant_act(_np(flat)).astype(np.float32)).to(x.dtype).view(x.shape)

    def lin(self, x, name):
        return super().lin(self._fq(x), name)

    def forward_inference(self, tokens, start_pos, image_tokens=None):
        assert image_tokens is None
        bsz, seqlen = tokens.shape
        if start_pos == 0:
            self.allocate_kv_cache(bsz)
            self.cache_image_words = 0
        h = self.embed(tokens)
        freqs_cis = self.freqs_cis[start_pos:start_pos + seqlen]
        for i in range(self.args.n_layers):
            h = self.block(i, h, start_pos, freqs_cis, None if seqlen == 1 else "causal")
        h = ref_cpu.rmsnorm(h, self.sd["norm.weight"], self.args.norm_eps)
        return torch.nn.functional.linear(self._fq(h[:, -1:, :]), self.sd["output.weight"])[:, 0].float()


# the configuration of tests/test_gpu_mx4.py's oracle test (a small vocabulary keeps the top-2 margins wide) with another weight seed:
# with every linear input quantised at every S, D is larger than there and seed 11 leaves no row whose margin exceeds twice the bound;
# of the seeds 0..9 seed 1 decides the most rows ON THE CPU ORACLE (14 of 16) -- chosen from the reference alone, before any GPU run
ACC = dict(hd=64, seed=1, std=0.03, vocab=16, B=2, T0=9, steps=8)


def _oracle_runs():
    """Greedy decode of the fake-quantised oracle on Wd (bf16) and the plain oracle on Wd fed the SAME tokens: (state dict, prompt,
    ids [steps, B], fake-quantised logits per step, D = their largest deviation).  All on the CPU."""
    c = ACC
    oargs = ref_cpu.OracleArgs(vocab_size=c["vocab"], max_seq_len=128, **GEOM[c["hd"]])
    sd = ref_cpu.make_decoder_weights(oargs, seed=c["seed"], std=c["std"])
    sdb = {k: v.to(BF) for k, v in _wd_state(sd, oargs.n_layers).items()}
    fq, plain = _FakeQuantOracle(oargs, sdb), ref_cpu.OracleDecoder(oargs, sdb)
    ex = torch.randint(3, c["vocab"], (c["B"], c["T0"]), generator=torch.Generator().manual_seed(12))
    ex[:, 0] = 1
    lq, lp = [fq.forward_inference(ex, 0).float()], [plain.forward_inference(ex, 0).float()]
    ids = []
    for t in range(c["steps"] - 1):
        ids.append(lq[-1].argmax(-1))
        lq.append(fq.forward_inference(ids[-1][:, None], c["T0"] + t).float())
        lp.append(plain.forward_inference(ids[-1][:, None], c["T0"] + t).float())
    ids.append(lq[-1].argmax(-1))
    D = max(float((a - b).abs().max()) for a, b in zip(lq, lp))
    return sd, ex, torch.stack(ids), lq, D


def test_greedy_decode_against_the_oracle_that_quantises_every_linear_input():
    """Eight greedy steps of a prefill=True model.  Allowed deviation of a step's logits from the fake-quantised oracle: the bound of
    tests/test_gpu_mx4.py test_greedy_decode_against_the_fake_quantised_oracle, 4e-2 of max |logit| plus D, the deviation between the
    fake-quantised and the plain oracle on Wd for the same tokens (computed on the CPU).  Rows whose top-2 margin exceeds twice the
    bound must pick the oracle's token, and there must be such rows."""
    c = ACC
    sd, ex, ids, want, D = _oracle_runs()
    scale = max(float(w.abs().max()) for w in want)
    bound = 4e-2 * scale + D
    m = _model(c["hd"], sd, True, vocab=c["vocab"])
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
    print(f"decided (step, row) pairs: {decided} of {c['steps'] * c['B']}")
    assert decided > 0, "no decided row: the comparison of tokens checked nothing"
    assert "nf4_scratch" not in m._ws


def test_refusals_stay():
    sd = _weights(64)
    m32 = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=128, **GEOM[64]))
    m32.load_state_dict(sd)
    m32.to(DEV)
    with pytest.raises(ValueError, match="fp32"):
        m32.quantize_decode_weights("mxfp4", prefill=True)
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    mp = peft.Transformer(peft.ModelArgs(vocab_size=VOCAB, max_seq_len=128, lora_rank=8, **GEOM[64]))
    with pytest.raises(NotImplementedError, match=r"merge_adapters\(\)"):
        mp.quantize_decode_weights("mxfp4", prefill=True)


DEC = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256, norm_eps=1e-5, rope_theta=10000.0)
VIT = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    import json
    import types
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    tmp = tmp_path_factory.mktemp("mx4gemmck")
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps({**DEC, **VIT}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=512, **DEC), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(DEC["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    args = types.SimpleNamespace(precision="tf32", only_save_trainable=False)
    return cfgp, ck.save_checkpoint(str(tmp / "ck"), args, mm, None, None, None, epoch=0)


def test_from_pretrained_quant_prefill_generates(ckpt):
    from a3vlm_amd.model.meta import MetaModel
    cfgp, ckdir = ckpt
    kw = dict(llama_type="llama_ens5", llama_config=[str(cfgp)], tokenizer_path=os.path.join(GD, "tokenizer.model"), with_visual=True,
              max_seq_len=512)
    with pytest.raises(ValueError, match="MXFP4 option"):
        MetaModel.from_pretrained(ckdir, quant="nf4", quant_prefill=True, **kw)
    mm = MetaModel.from_pretrained(ckdir, quant="mxfp4", quant_prefill=True, **kw)
    assert mm.llma.weight_format == "mxfp4" and mm.llma._weights.images and mm.llma._weights.prefill is True
    prompts, n = ["Detect all manipulable object parts.", "Lid?"], 8
    ids = [mm.generate([p], None, max_gen_len=n, temperature=0, return_ids=True)[1][0] for p in prompts]
    assert all(len(i) > 0 for i in ids)
    assert mm.generate_many(prompts, None, batch_rows=2, max_gen_len=n, return_ids=True)[1] == ids
    assert "nf4_scratch" not in mm.llma._ws
