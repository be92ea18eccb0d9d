"""MXFP4 on the GPU: quantiser / dequantiser bit-equal to tests/mx4_ref.py; the scaled-MFMA decode GEMV bit-exact on an exactly
representable family (lane map, nibble order, scale bytes), inside derived bounds on reals, deterministic under split-K; the model
paths of quantize_decode_weights("mxfp4")."""
import os

import numpy as np
import pytest
import torch

import mx4_ref as R
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


# ------------------------------------------------------------------ quantiser / dequantiser
def _quant_input(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-8, 9, (N, K // 32, 1), generator=g).float()).expand(N, K // 32, 32).reshape(N, K)
    w = w.to(BF).float()
    w[0, :32] = 0.0                                                 # zero block
    w[1, 32:64] = 0.0
    w[1, 40] = -0.0
    w[2, 64:96] = 0.0
    w[2, 70] = 3.0e38                                               # a block of one huge element
    w[3, :12] = torch.tensor([7.5, -7.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.0, -5.0])   # ties and saturation at E = 0
    w[3, 12:32] = 0.0
    w[4, 96:128] = torch.tensor(2.0 ** -130)                        # bf16 denormals
    w[5, :32] = -0.0
    w[6, :32] = 0.0                                                 # maximum in [2^-125, 2^-124): E = -127, scale byte 0, nonzero codes
    w[6, :6] = torch.tensor([1.5 * 2.0 ** -125, -2.0 ** -125, 2.0 ** -126, -2.0 ** -127, 2.0 ** -128, 1.5 * 2.0 ** -127])
    return w.to(BF)


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (33 * 16, 11008)])
def test_quantiser_and_dequantiser_equal_the_restatement(N, K):
    w = _quant_input(N, K, seed=N + K)
    want_q, want_s = R.quantize(_np(w))
    ldq = K // 2 + 48
    qb = torch.full((N + 2, ldq), 0xA5, dtype=torch.uint8, device=DEV)
    sb = torch.full((N * (K // 32) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    q, s = qb[1:N + 1, :K // 2], sb[32:32 + N * (K // 32)].view(N, K // 32)
    ops.quantize_mxfp4(w.to(DEV), q, s)
    assert np.array_equal(q.cpu().numpy(), want_q) and np.array_equal(s.cpu().numpy(), want_s)
    assert not (s == 0xFF).any()
    assert bool((qb[0] == 0xA5).all() and (qb[-1] == 0xA5).all() and (qb[:, K // 2:] == 0xA5).all()), "codes: nothing outside the window"
    assert bool((sb[:32] == 0xA5).all() and (sb[-32:] == 0xA5).all()), "scales: nothing outside the window"
    ob = torch.full((N + 2, K + 8), 777.0, dtype=BF, device=DEV)
    out = ob[1:N + 1, :K]
    ops.dequantize_mxfp4(q, s, out)
    wd = R.dequantize(want_q, want_s)
    assert np.array_equal(_np(out), wd), "Wd is exact in bf16"
    assert bool((ob[0] == 777.0).all() and (ob[-1] == 777.0).all() and (ob[:, K:] == 777.0).all())


# ------------------------------------------------------------------ GEMV
EPIS = {"none": 0, "residual": ops.EPI_RESIDUAL, "swiglu": ops.EPI_SWIGLU, "f32": ops.EPI_OUT_F32}


def _run_gemv(a, q, s, epi, res=None, N=None):
    """a [M, K] bf16 (CPU) in a NaN-filled buffer, output in a sentinel-filled one; returns the window (CPU) after checking the rest."""
    M, K = a.shape
    N = q.shape[0]
    ab = torch.full((M + 2, K + 8), float("nan"), dtype=BF, device=DEV)
    ab[1:M + 1, :K] = a.to(DEV)
    ncol = N // 2 if epi == ops.EPI_SWIGLU else N
    odt = torch.float32 if epi & ops.EPI_OUT_F32 else BF
    cb = torch.full((M + 2, ncol + 8), -12345.0, dtype=odt, device=DEV)
    ws = torch.zeros((ops.gemm_skinny_mxfp4_ws_bytes(M, N, K) + 3) // 4, dtype=torch.float32, device=DEV)
    ops.gemm_skinny_mxfp4(ab[1:M + 1, :K], q, s, cb[1:M + 1, :ncol], ws, residual=None if res is None else res.to(DEV), epilogue=epi & ~ops.EPI_RESIDUAL)
    torch.cuda.synchronize()
    assert bool((cb[0] == -12345.0).all() and (cb[-1] == -12345.0).all() and (cb[:, ncol:] == -12345.0).all()), "nothing outside the output window"
    assert not ws[:4096].any(), "the arrival counters are left zero"
    return cb[1:M + 1, :ncol].cpu()


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
    return A, W, q, s


def _epilogue(acc, epi, res):
    """The rounding sequence of the bf16 GEMV on an exact accumulator (torch CPU, fp32)."""
    y = torch.from_numpy(acc.astype(np.float32)).to(BF).float()
    if epi & ops.EPI_RESIDUAL:
        y = y + res.float()
    return y if epi & ops.EPI_OUT_F32 else y.to(BF)


EXACT = [(M, N, K) for M in (1, 5, 16) for N in (16, 48, 4112) for K in (128, 384, 4096)] + [(M, 48, 11008) for M in (1, 5, 16)]


@pytest.mark.parametrize("M,N,K", EXACT, ids=lambda v: str(v))
def test_gemv_exact_family(M, N, K):
    A, W, q, s = _exact_case(M, N, K, seed=M * 7 + N + K)
    acc = A @ W.T
    qd, sd = _image_on_gpu(q, s)
    rc, plan = ops.mx4_gemv_plan(M, N, K)
    print(f"M {M} N {N} K {K}: {plan[2]} K slice(s), grid {plan[0]}")
    res = _bf(np.random.default_rng(1).standard_normal((M, N)) * np.abs(acc).max())
    a = _bf(A)
    for name, epi in EPIS.items():
        if name == "swiglu":
            # N counts gate / up rows in 16-row pairs: the same family at the next multiple of 32 rows
            N = (N + 31) // 32 * 32
            A, W, q, s = _exact_case(M, N, K, seed=M * 7 + N + K + 1)
            acc, a = A @ W.T, _bf(A)
            qd, sd = _image_on_gpu(q, s)
            print(f"  SwiGLU at N {N}: {ops.mx4_gemv_plan(M, N, K, ops.EPI_SWIGLU)[1][2]} K slice(s)")
            # the same exact accumulators through the bf16 GEMV's own SwiGLU epilogue (its silu is a device expression)
            wd = _bf(W).to(DEV)
            want = torch.empty(M, N // 2, dtype=BF, device=DEV)
            ops.gemm_skinny(a.to(DEV), wd, want, ops.gemm_skinny_workspace(M, N, K, DEV), epilogue=ops.EPI_SWIGLU)
            want = want.cpu()
            nb16 = N // 32
            gu = torch.from_numpy(acc.astype(np.float32)).to(BF).float().view(M, nb16, 2, 16)
            cpu = (torch.nn.functional.silu(gu[:, :, 0]).to(BF).float() * gu[:, :, 1]).reshape(M, N // 2)
            # the reference itself against a CPU SwiGLU: the device silu (v_exp, v_rcp: a few fp32 ulps) can move bf16(silu(gate)) by
            # one bf16 step (<= 2^-7 relative) and the rounding of the product by one more
            assert bool(((want.float() - cpu).abs() <= 2.0 ** -6 * cpu.abs() + 1e-30).all()), "the reference: two bf16 steps of the CPU SwiGLU"
        else:
            want = _epilogue(acc, epi, res)
        got = _run_gemv(a, qd, sd, epi, res if epi & ops.EPI_RESIDUAL else None)
        assert got.dtype == want.dtype and torch.equal(got, want), (name, float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("M", [1, 8])
def test_gemv_exact_ring_steady_state(M):
    """N 16384, K 4096: two K slices of FOUR 512-k units each (what 7B w13 and the LM head run), so every ring slot is refilled while
    later stages are in flight.  The image is 16 row-rolled copies of one exact 1024-row case (generated once per M); every 16-row
    tile of every copy must give the base case's bits."""
    N0, K, copies = 1024, 4096, 16
    N = N0 * copies
    for epi in (0, ops.EPI_SWIGLU):
        rc, plan = ops.mx4_gemv_plan(M, N, K, epi)
        assert rc == 0 and plan[2] == 2 and plan[7] == 4, plan
    A, W, q, s = _exact_case(M, N0, K, seed=77 + M)
    acc = A @ W.T
    a = _bf(A)
    # copy j holds the base rows rolled by 32 j (whole gate / up pairs): row n of copy j is base row (n + 32 j) % N0
    idx = np.concatenate([(np.arange(N0) + 32 * j) % N0 for j in range(copies)])
    qd, sd = _image_on_gpu(q[idx], s[idx])
    acc_all = acc[:, idx]
    got = _run_gemv(a, qd, sd, 0)
    want = _epilogue(acc_all, 0, None)
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    wd = _bf(W[idx]).to(DEV)
    want = torch.empty(M, N // 2, dtype=BF, device=DEV)
    ops.gemm_skinny(a.to(DEV), wd, want, ops.gemm_skinny_workspace(M, N, K, DEV), epilogue=ops.EPI_SWIGLU)
    got = _run_gemv(a, qd, sd, ops.EPI_SWIGLU)
    assert torch.equal(got, want.cpu())
    gu = torch.from_numpy(acc_all.astype(np.float32)).to(BF).float().view(M, N // 32, 2, 16)
    cpu = (torch.nn.functional.silu(gu[:, :, 0]).to(BF).float() * gu[:, :, 1]).reshape(M, N // 2)
    assert bool(((got.float() - cpu).abs() <= 2.0 ** -6 * cpu.abs() + 1e-30).all()), "within two bf16 steps of the CPU SwiGLU (as the exact family)"


@pytest.mark.parametrize("M,N,K", [(5, 48, 384), (16, 80, 4096), (3, 48, 11008)])
def test_gemv_bounded_family(M, N, K):
    g = torch.Generator().manual_seed(K + M)
    def reals(r):
        x = torch.randn(r, K, generator=g) * torch.exp2(torch.randint(-8, 9, (r, K // 32, 1), generator=g).float()).expand(r, K // 32, 32).reshape(r, K)
        return x.to(BF)
    a, w = reals(M), reals(N) * 0.05
    q, s = R.quantize(_np(w))
    Wd = R.dequantize(q, s)
    aq, ea = R.quant_act_mxfp8(_np(a))
    Aq = R.dequant_act(aq, ea)
    ref_q = Aq @ Wd.T                                               # fp64 on the restated codes of both operands
    acc_bound = (K - 1) * 2.0 ** -23 * (np.abs(Aq) @ np.abs(Wd).T)  # fp32 accumulation, tests/gemm_ref.py
    E = np.repeat(ea, 32, axis=1)
    act_bound = np.maximum(2.0 ** -4 * np.abs(_np(a)), np.ldexp(1.0, E - 10)) @ np.abs(Wd).T
    ref_u = _np(a) @ Wd.T
    qd, sd = _image_on_gpu(q, s)
    res = (torch.randn(M, N, generator=g) * float(np.abs(ref_q).mean())).to(BF)
    for name in ("none", "f32", "residual"):
        epi = EPIS[name]
        got = _np(_run_gemv(a, qd, sd, epi, res if name == "residual" else None))
        r = _np(res) if name == "residual" else 0.0
        # bf16(acc) (+ residual, rounded again): half a bf16 step each, 2^-8 |x| (8 significant bits)
        out = 2.0 ** -8 * np.abs(ref_q) + acc_bound * (1 + 2.0 ** -8)
        if name == "residual":
            out = out + 2.0 ** -8 * (np.abs(ref_q + r) + out)
        e1 = np.abs(got - (ref_q + r))
        print(f"{name}: max err / bound vs restated codes {float((e1 / out).max()):.3f}; vs unquantised A {float((np.abs(got - (ref_u + r)) / (out + act_bound)).max()):.3f}")
        assert (e1 <= out).all(), name
        assert (np.abs(got - (ref_u + r)) <= out + act_bound).all(), name


def test_split_plan_is_deterministic():
    M, N, K = 8, 64, 4096
    assert ops.mx4_gemv_plan(M, N, K)[1][2] > 1
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(M, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * 0.05).to(BF)
    q, s = ops.quantize_mxfp4(w.to(DEV))
    runs = [_run_gemv(a, q, s, ops.EPI_SWIGLU) for _ in range(2)] + [_run_gemv(a, q, s, 0) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[2], runs[3])


# ------------------------------------------------------------------ model
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}
LINEARS = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2", "feed_forward.w3")


def _model(hd, sd, weights=None, kv=None):
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=128, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    if kv is not None:
        m.quantize_kv_cache(kv)
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


@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_equals_the_bf16_model_holding_wd(hd):
    sd = _weights(hd)
    mq, md = _model(hd, sd, "mxfp4"), _model(hd, _wd_state(sd, 2))
    assert mq.weight_format == "mxfp4" and mq._weights.images and not hasattr(mq.layers[0].attention.wq, "weight") and "output.weight" not in mq.state_dict()
    ex = _tokens(2, 21, seed=5)
    assert torch.equal(mq.forward_inference(ex, 0), md.forward_inference(ex, 0)), "prefill is weight-only: bit-equal logits"
    for i in range(2):
        assert torch.equal(mq._k_cache[i], md._k_cache[i]) and torch.equal(mq._vt_cache[i], md._vt_cache[i]), i


def test_decode_step_above_32_rows_is_weight_only_end_to_end():
    """More than 32 decode rows have no GEMV form: layers AND head run on the dequantised weights, bit-equal to the bf16 model on Wd."""
    hd, B, T = 64, 33, 6
    sd = _weights(hd)
    mq, md = _model(hd, sd, "mxfp4"), _model(hd, _wd_state(sd, 2))
    ex = _tokens(B, T, seed=9)
    for m in (mq, md):
        m.forward_inference(ex[:, :T - 1], 0)
    assert torch.equal(mq.forward_inference(ex[:, T - 1:], T - 1), md.forward_inference(ex[:, T - 1:], T - 1))


@pytest.mark.parametrize("B", [4, 18])
def test_decode_step_equals_the_sequence_of_public_ops(B):
    hd = 128
    m = _model(hd, _weights(hd), "mxfp4")
    T = 12
    ex = _tokens(B, T, seed=6)
    m.forward_inference(ex[:, :T - 1], 0)
    kc0, vc0 = [t.clone() for t in m._k_cache], [t.clone() for t in m._vt_cache]
    got = m.forward_inference(ex[:, T - 1:], T - 1).clone()
    kc1 = [t.clone() for t in m._k_cache]
    for t, src in zip(m._k_cache + m._vt_cache, kc0 + vc0):
        t.copy_(src)
    a, mx = m.args, m._weights.images
    H, Hkv, dim, pos = m.n_heads, m.n_kv_heads, a.dim, T - 1
    h = torch.empty(B, dim, dtype=BF, device=DEV)
    ops.embed_assemble(ex[:, T - 1:].contiguous(), m.tok_embeddings.weight, h, B, 1, 0, dim)
    xn, qkv = torch.empty_like(h), torch.empty(B, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
    att, act = torch.empty(B, H * hd, dtype=BF, device=DEV), torch.empty(B, m.ffn, dtype=BF, device=DEV)
    scratch = torch.empty(2 * ops.attention_scratch_floats(B, H, hd, a.max_seq_len + 64), dtype=torch.float32, device=DEV)

    def lin(x, img, out, **kw):
        ws = torch.zeros((ops.gemm_skinny_mxfp4_ws_bytes(16, img.q.shape[0], x.shape[1]) + 3) // 4, dtype=torch.float32, device=DEV)
        for r0 in range(0, B, 16):
            r = kw.get("residual")
            ops.gemm_skinny_mxfp4(x[r0:r0 + 16], img.q, img.s, out[r0:r0 + 16], ws, residual=None if r is None else r[r0:r0 + 16],
                                  epilogue=kw.get("epilogue", 0))
    for i, lyr in enumerate(m.layers):
        kc, vc = m._k_cache[i], m._vt_cache[i]
        smax, ldq = kc.shape[2], qkv.stride(0)
        strides = (ldq, ldq, hd, Hkv * smax * hd, smax * hd, hd, Hkv * hd * smax, hd * smax, smax, H * hd, H * hd, hd)
        ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
        lin(xn, mx[f"wqkv.{i}"], qkv)
        ops.rope_kvcache(qkv, qkv, kc, vc, m._cos_sin_dev(), B, 1, H, Hkv, hd, pos, pos)
        ops.attention(qkv, kc, vc, att, B, 1, pos + 1, H, Hkv, hd, strides, False, scratch)
        lin(att, mx[f"wo.{i}"], h, residual=h)
        ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
        lin(xn, mx[f"w13.{i}"], act, epilogue=ops.EPI_SWIGLU)
        lin(act, mx[f"w2.{i}"], h, residual=h)
    ops.rmsnorm(h, m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(B, a.vocab_size, dtype=torch.float32, device=DEV)
    lin(xn, mx["output"], logits, epilogue=ops.EPI_OUT_F32)
    assert torch.equal(got, logits)
    for x, y in zip(kc1, m._k_cache):
        assert torch.equal(x, y)


class _FakeQuantOracle(ref_cpu.OracleDecoder):
    """OracleDecoder whose linears see MXFP8 fake-quantised inputs (tests/mx4_ref.py quant_act_mxfp8) at S = 1, the LM head included --
    what the product's decode GEMVs multiply; a multi-token forward is weight-only and stays the plain oracle."""

    @staticmethod
    def _fq(x):
        if x.shape[1] != 1:
            return x
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
        hl = h[:, -1:, :]
        return torch.nn.functional.linear(self._fq(hl) if seqlen == 1 else hl, self.sd["output.weight"])[:, 0].float()


# the configuration of tests/test_gpu_kv8.py's cache-oracle test: a small vocabulary keeps the top-2 margins wide
ACC = dict(hd=64, seed=11, std=0.03, vocab=16, B=2, T0=9, steps=8)


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


def test_greedy_decode_against_the_fake_quantised_oracle():
    """Eight greedy steps.  Allowed deviation of a step's logits from the fake-quantised oracle: the bf16 model test's bound against
    its oracle (4e-2 of max |logit|, tests/test_gpu_model.py) plus D, the deviation between the fake-quantised and the plain oracle
    on Wd for the same tokens -- a bf16 rounding difference in a linear's input can flip an e4m3 code or a block exponent, an error
    of the size of the quantisation noise itself.  Rows whose top-2 margin exceeds twice the bound must pick the oracle's token."""
    c = ACC
    sd, ex, ids, want, D = _oracle_runs()
    scale = max(float(w.abs().max()) for w in want)
    bound = 4e-2 * scale + D
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=c["vocab"], max_seq_len=128, **GEOM[c["hd"]]))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    m.quantize_decode_weights("mxfp4")
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


DEC = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256, norm_eps=1e-5, rope_theta=10000.0)
VIT = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    import json
    import types
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    tmp = tmp_path_factory.mktemp("mx4ck")
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps({**DEC, **VIT}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=512, **DEC), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(DEC["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    args = types.SimpleNamespace(precision="tf32", only_save_trainable=False)
    return cfgp, ck.save_checkpoint(str(tmp / "ck"), args, mm, None, None, None, epoch=0)


@pytest.mark.parametrize("kv", [None, "fp8"])
def test_from_pretrained_mxfp4_generates(ckpt, kv):
    from a3vlm_amd.model.meta import MetaModel
    cfgp, ckdir = ckpt
    mm = MetaModel.from_pretrained(ckdir, llama_type="llama_ens5", llama_config=[str(cfgp)], tokenizer_path=os.path.join(GD, "tokenizer.model"),
                                   with_visual=True, max_seq_len=512, quant="mxfp4", kv_quant=kv)
    assert mm.llma.weight_format == "mxfp4" and mm.llma._weights.images and mm.llma._kv_quant == kv
    prompts, n = ["Detect all manipulable object parts.", "Lid?"], 8
    ids = [mm.generate([p], None, max_gen_len=n, temperature=0, return_ids=True)[1][0] for p in prompts]
    tok = mm.tokenizer.encode(prompts[0], bos=True, eos=False)
    logits, step_ids = mm.llma.forward_inference(torch.tensor([tok], device=DEV), 0), []
    for j in range(n):
        nxt = int(logits.argmax(-1))
        if nxt == mm.tokenizer.eos_id:
            break
        step_ids.append(nxt)
        logits = mm.llma.forward_inference(torch.tensor([[nxt]], device=DEV), len(tok) + j)
    assert ids[0] == step_ids and len(step_ids) > 0
    if kv is None:                                                  # ragged decode (bf16 cache): the ids of generate(), prompt by prompt
        assert mm.generate_many(prompts, None, batch_rows=2, max_gen_len=n, return_ids=True)[1] == ids
    with pytest.raises(RuntimeError, match="MXFP4"):
        mm.train_engine()


def test_refusals_raise_before_any_launch():
    sd = _weights(64)
    m = _model(64, sd, "mxfp4")
    for mode in ("mxfp4", "nf4", "fp8"):
        with pytest.raises(RuntimeError, match="holds MXFP4"):
            m.quantize_decode_weights(mode)
    m = _model(128, _weights(128), "nf4")
    with pytest.raises(RuntimeError, match="holds NF4"):
        m.quantize_decode_weights("mxfp4")
    m32 = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=128, **GEOM[64]))
    m32.load_state_dict(sd)
    m32.to(DEV)
    with pytest.raises(ValueError, match="fp32"):
        m32.quantize_decode_weights("mxfp4")
    odd = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=128, dim=192, n_layers=1, n_heads=3, multiple_of=64)).to(BF).to(DEV)
    with pytest.raises(ValueError, match="multiples of 128"):
        odd.quantize_decode_weights("mxfp4")
    assert hasattr(odd.layers[0].attention.wq, "weight"), "a refused model keeps its weights"
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    mp = peft.Transformer(peft.ModelArgs(vocab_size=VOCAB, max_seq_len=128, lora_rank=8, **GEOM[64]))
    with pytest.raises(NotImplementedError, match=r"merge_adapters\(\)"):
        mp.quantize_decode_weights("mxfp4")
