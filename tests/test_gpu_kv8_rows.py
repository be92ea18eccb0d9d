"""-m gpu: the fp8 KV cache on the ragged decode path (a3v_kv8_rows.hip, Transformer.quantize_kv_cache("fp8", rows=True)).  The write
kernel, the span copy and the fused step are held to equalities against the entries they restate; the attention to the fp64
reference of tests/kv8_rows_ref.py (exact family bit for bit, partial slots included; bounded and stress inside the derived bound)
and to its four contracts as equalities; the model to the bf16-cache model (prefill), to the fake-quantised oracle (decode) and to
itself without shared keys (parallel sampling)."""
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import kv8_ref
import kv8_rows_ref as R
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def plan(B, H, Sk):
    return ops.attention_decode_plan(B, H, Sk)


# ------------------------------------------------------------------ 1. the quantising write
@pytest.mark.parametrize("pos", [(0, 63, -1, 128), (64, 127, 128, -5)], ids=["0-63-idle-Smax", "64-last-Smax-idle"])
@pytest.mark.parametrize("hd", [64, 128])
def test_write_equals_rope_rows_then_quantize(hd, pos):
    B, H, Hkv, Smax = 4, 4, 2, 128
    g = torch.Generator().manual_seed(hd + pos[0])
    qkv = (torch.randn(B, (H + 2 * Hkv) * hd, generator=g) * 2).to(BF).to(DEV)
    ang = torch.rand(Smax, hd // 2, generator=g) * 6.28
    cs = torch.stack((ang.cos(), ang.sin()), -1).contiguous().to(DEV)
    p = i32(pos)
    # the entries it restates: rope into a bf16 cache, then the S = 1 quantiser at the row's position
    kc = torch.zeros(B, Hkv, Smax, hd, dtype=BF, device=DEV)
    vc = torch.zeros(B, Hkv, hd, Smax, dtype=BF, device=DEV)
    q_want = torch.full((B, H * hd), 7.0, dtype=BF, device=DEV)
    ops.rope_kvcache_rows(qkv, q_want, kc, vc, cs, p, B, H, Hkv, hd)
    canary = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, generator=g).to(DEV)
    fcan = lambda *s: torch.randn(*s, generator=g).to(DEV)
    got = [canary(B, Hkv, Smax, hd), canary(B, Hkv, hd, Smax), fcan(B, Hkv, Smax), fcan(B, Hkv, Smax)]
    want = [t.clone() for t in got]
    for b, pb in enumerate(pos):
        if 0 <= pb < Smax:
            ops.kv_quantize_fp8(kc[b:b + 1], vc[b:b + 1], pb, *(t[b:b + 1] for t in want), 1, pb)
    before = [t.clone() for t in got]
    q_got = qkv.clone()
    ops.rope_kvquant_rows(q_got, q_got, *got, cs, p, B, H, Hkv, hd)          # q in place, as the step runs it
    assert torch.equal(q_got[:, :H * hd], q_want), "q_out"
    assert torch.equal(q_got[:, H * hd:], qkv[:, H * hd:]), "the k / v columns of the qkv buffer are not written"
    for name, a, b_ in zip(("k_q", "vt_q", "k_scale", "v_scale"), got, want):
        assert torch.equal(a, b_), name                                       # codes, scales, and every canary outside pos[b]
    for b, pb in enumerate(pos):
        if not 0 <= pb < Smax:
            assert all(torch.equal(a[b], c[b]) for a, c in zip(got, before)), "an idle row's cache arrays are untouched"
            assert float(q_got[b, :H * hd].float().abs().sum()) == 0, "an idle row's q is zeros"
        else:
            assert not torch.equal(got[0][b, :, pb], before[0][b, :, pb])
    # and against the host restatement (oracle.quant_fp8 on the bf16-rounded rotated k).  v is not rotated: its codes and scales are
    # the oracle's exactly.  The rotation is a fused multiply-add on the device and two roundings in torch, so a rotated value may
    # land on the neighbouring bf16 (2^-8 relative): q within one bf16 ulp; a k scale within 2^-7 relative (one bf16 ulp of amax);
    # a dequantised k value within one e4m3 step of the neighbouring code (at most twice the step at x, across a binade edge) plus
    # 2^-7 |x| (the moved input and the moved scale)
    q_ref, writes = R.rope_kvquant_rows_ref(qkv.cpu(), cs.cpu(), pos, H, Hkv, hd, Smax)
    qg = q_got[:, :H * hd].float().cpu()
    assert bool(((qg - q_ref.float()).abs() <= 2.0 ** -7 * q_ref.float().abs() + 2.0 ** -18).all())   # (+ fp32 rounding of products of |x| < 16 where the two cancel)
    exact = 0
    for b, w in enumerate(writes):
        if w is None:
            continue
        pb, kq, ks, vq, vs = w
        assert torch.equal(got[1][b, :, :, pb].cpu(), vq) and torch.equal(got[3][b, :, pb].cpu(), vs), ("v", b)
        gks, gkq = got[2][b, :, pb].cpu(), got[0][b, :, pb].cpu()
        assert bool(((gks - ks).abs() <= 2.0 ** -7 * ks).all()), ("k scale", b)
        x = kv8_ref.dequantize_rows(kq, ks)
        step = kv8_ref.e4m3_step(x.double() / ks[:, None].double()) * ks[:, None].double()
        assert bool(((kv8_ref.dequantize_rows(gkq, gks) - x).abs().double() <= 2 * step + 2.0 ** -7 * x.abs().double()).all()), ("k", b)
        exact += int(torch.equal(gkq, kq) and torch.equal(gks, ks))
    print(f"hd {hd} pos {pos}: k rows whose codes and scales equal the host restatement exactly: {exact} of {sum(w is not None for w in writes)}")


# ------------------------------------------------------------------ 2. the attention
def _edge_cases():
    """sk at every edge of the exported plan: one geometry with ONE key range at any sk_max (B * H = 256), one with >= 2"""
    out = []
    ns, ch = plan(32, 8, 200)
    assert ns == 1
    edges = [1, 63, 64, 65, 127, 128, 129, 199, 200, 0, 500]
    sk = [edges[b % len(edges)] for b in range(32)]
    out.append(R.make_case("one-range", 8, 2, 128, sk, 200, plan, src=[0] * 32, shared=[0] + [(64, 128, 192, 100)[b % 4] for b in range(1, 32)]))
    ns, ch = plan(4, 4, 400)
    assert ns >= 2, (ns, ch)
    e = sorted({x for s in range(1, ns + 1) for x in (s * ch - 1, s * ch, s * ch + 1) if 0 < x <= 400} | {400})
    for i in range(0, len(e), 3):
        sk = (400,) + tuple(e[i:i + 3]) + (e[-1],) * (3 - len(e[i:i + 3]))
        out.append(R.make_case(f"range-edges-{i}", 4, 2, 64, sk, 400, plan))
        out.append(R.make_case(f"range-edges-{i}-shared", 4, 2, 64, sk, 400, plan, src=(0, 0, 0, 0), shared=(0, 64, 10 ** 6, ch)))
    return out


@pytest.fixture(scope="module")
def attn_cases():
    return {c.id: c for c in R.cpu_cases(plan) + _edge_cases()}


CASE_IDS = ["kv8rows-" + t for t in "abcdef"] + ["kv8rows-one-range"] + [f"kv8rows-range-edges-{i}{s}" for i in (0, 3, 6) for s in ("", "-shared")]


def _dev_inputs(c, inp):
    q = inp["q"].to(BF).reshape(c.B, c.H * c.hd).contiguous().to(DEV)
    return q, [inp[k].contiguous().to(DEV) for k in ("kq", "vtq", "ks", "vs")]


def _run_rows(c, q, arrays, src=None, shared=None, sk=None, raw_shared_entry=False):
    """-> (out bf16 [B, H, hd] on the CPU, partial slots [B, H, nsplit, hd + 2], counters)"""
    B, H, Hkv, hd = c.B, c.H, c.Hkv, c.hd
    n = ops.attention_scratch_floats(B, H, hd, c.sk_max)
    scratch = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    counters = torch.zeros(B * H, dtype=torch.int32, device=DEV)
    out = torch.full((B, H * hd), float("nan"), dtype=BF, device=DEV)
    skd = i32(c.sk if sk is None else sk)
    if raw_shared_entry:                                      # contract (d): the shared entry with src_row == NULL
        P = lambda t: None if t is None else t.data_ptr()
        rc = lib.load().a3v_attention_decode_rows_fp8kv_shared(P(q), q.stride(0), *(P(t) for t in arrays), P(out), out.stride(0), P(skd), None,
                                                               P(skd), c.sk_max, B, H, Hkv, hd, arrays[0].shape[2], P(scratch), P(counters),
                                                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        ops.attention_decode_rows_fp8kv(q, *arrays, out, skd, c.sk_max, B, H, Hkv, hd, scratch, counters, src, shared)
    torch.cuda.synchronize()
    part = scratch[:B * H * c.nsplit * (hd + 2)].view(B, H, c.nsplit, hd + 2).cpu()
    return out.view(B, H, hd).cpu(), part, counters.cpu()


def _copied(c, inp):
    """the caches with bytes AND scales of [0, S_b) of row src_row[b] physically copied into row b"""
    kq, vq, ks, vs = (inp[k].clone() for k in ("kq", "vtq", "ks", "vs"))
    for b in range(c.B):
        s, S = c.shared_len(b)
        if s != b and S > 0:
            kq[b, :, :S], vq[b, :, :, :S], ks[b, :, :S], vs[b, :, :S] = inp["kq"][s, :, :S], inp["vtq"][s, :, :, :S], inp["ks"][s, :, :S], inp["vs"][s, :, :S]
    return dict(q=inp["q"], kq=kq, vtq=vq, ks=ks, vs=vs)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_attention_against_the_fp64_reference_and_its_contracts(attn_cases, cid, family):
    c = attn_cases[cid]
    ref = R.reference(c, family)
    inp = ref["inp"]
    q, arrays = _dev_inputs(c, inp)
    src, shared = (i32(c.src), i32(c.shared)) if c.src else (None, None)
    out, part, ctr = _run_rows(c, q, arrays, src, shared)
    ok, ratio, why = R.judge(c, family, ref, out, part if c.nsplit > 1 else None)
    print(f"{c.id} {family}: nsplit {c.nsplit} chunk {c.chunk}, err / bound {ratio:.3f}")
    assert ok, (c.id, family, ratio, why)
    assert int(ctr.abs().sum()) == 0, "counters are left zero"
    idle = torch.tensor([k <= 0 for k in c.keys()])
    assert float(out[idle].float().abs().sum()) == 0 if bool(idle.any()) else True
    keys = c.keys()
    if c.src:
        # (c) bit-equal to the plain entry on physically copied caches -- while the sibling's own [0, S_b) holds 0x7F / inf here
        _, carr = _dev_inputs(c, _copied(c, inp))
        plain, ppart, _ = _run_rows(c, q, carr)
        assert torch.equal(out, plain), "(c) shared != plain on copied caches"
        live = torch.tensor([k > 0 for k in keys])
        if c.nsplit > 1:
            assert torch.equal(part[live], ppart[live]), "(c) partial slots"
        # (d) src_row == NULL: the call is the plain one
        d_out, _, _ = _run_rows(c, q, carr, raw_shared_entry=True)
        assert torch.equal(d_out, plain), "(d)"
        arrays = carr
    if family != "bounded":
        return
    # (b) every row at sk_max: the uniform launch, bit for bit (fresh inputs: every position below sk_max is live)
    full = R.make_case(c.id[8:] + "-full", c.H, c.Hkv, c.hd, (c.sk_max,) * c.B, c.sk_max, plan)
    finp = R.inputs(full, family)
    fq, farr = _dev_inputs(full, finp)
    rows_out, _, _ = _run_rows(full, fq, farr)
    scratch = torch.empty(ops.attention_scratch_floats(c.B, c.H, c.hd, c.sk_max), dtype=torch.float32, device=DEV)
    for counters in (torch.zeros(c.B * c.H, dtype=torch.int32, device=DEV), None):
        uni = torch.empty(c.B, c.H * c.hd, dtype=BF, device=DEV)
        ops.attention_decode_fp8kv(fq, *farr, uni, c.B, c.sk_max, c.H, c.Hkv, c.hd, scratch, counters)
        assert torch.equal(uni.view(c.B, c.H, c.hd).cpu(), rows_out), "(b) rows at sk_max != the uniform launch"
    # (a) one key range: row b is the uniform launch at Sk = sk[b] (its other rows read dead positions: only row b is compared)
    if c.nsplit == 1:
        for n in sorted({k for k in keys if k > 0}):
            if plan(c.B, c.H, n)[0] != 1:
                continue
            uni = torch.empty(c.B, c.H * c.hd, dtype=BF, device=DEV)
            ops.attention_decode_fp8kv(q, *arrays, uni, c.B, n, c.H, c.Hkv, c.hd, scratch, torch.zeros(c.B * c.H, dtype=torch.int32, device=DEV))
            uni = uni.view(c.B, c.H, c.hd).cpu()
            for b in [b for b, k in enumerate(keys) if k == n]:
                assert torch.equal(uni[b], out[b]), ("(a)", b, n)


# ------------------------------------------------------------------ 3. the span copy
@pytest.mark.parametrize("lo", [64, 77], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("hd", [64, 128])
def test_kv8_copy_span_writes_exactly_the_span(hd, lo):
    B, Hkv, Smax, L = 4, 2, 256, 2
    g = torch.Generator().manual_seed(hd + lo)
    mk = lambda: [[torch.randint(0, 256, (B, Hkv, Smax, hd), dtype=torch.uint8, generator=g).to(DEV) for _ in range(L)],
                  [torch.randint(0, 256, (B, Hkv, hd, Smax), dtype=torch.uint8, generator=g).to(DEV) for _ in range(L)],
                  [torch.randn(B, Hkv, Smax, generator=g).to(DEV) for _ in range(L)],
                  [torch.randn(B, Hkv, Smax, generator=g).to(DEV) for _ in range(L)]]
    dst = i32([0, 3, 1, 7, -1])                               # 1 is the source, 7 and -1 are outside: skipped
    for n in (0, 1, 15, 16, 17, 63):
        arrays = mk()
        want = [[t.clone() for t in ts] for ts in arrays]
        hi = lo + n
        for i in range(L):
            for r in (0, 3):
                want[0][i][r, :, lo:hi] = want[0][i][1, :, lo:hi]
                want[1][i][r, :, :, lo:hi] = want[1][i][1, :, :, lo:hi]
                want[2][i][r, :, lo:hi] = want[2][i][1, :, lo:hi]
                want[3][i][r, :, lo:hi] = want[3][i][1, :, lo:hi]
        ptrs = ops.kv8_copy_span(*arrays, 1, dst, lo, hi)
        assert tuple(ptrs.shape) == (4, L)
        for name, a, w in zip(("k_q", "vt_q", "k_scale", "v_scale"), arrays, want):
            for i in range(L):
                assert torch.equal(a[i], w[i]), (name, i, n)
    arrays = mk()
    keep = [[t.clone() for t in ts] for ts in arrays]
    ops.kv8_copy_span(*arrays, 1, dst[:0], lo, lo + 5)         # no destination: nothing launched
    assert all(torch.equal(a, k) for ts, ks in zip(arrays, keep) for a, k in zip(ts, ks))


# ------------------------------------------------------------------ 4. the fused step
VOCAB = 640
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}
# (pos, src_row, shared) per row
STEP3 = [(150, 0, 0), (70, 0, 64), (129, 0, 128)]
STEP17 = ([(200, 0, 0), (5, 1, 0), (100, 0, 64), (-1, 2, 128), (64, 0, 64), (130, 0, 128), (90, 30, 64), (17, -4, 64)]
          + [(10 + b, b, 0) for b in range(8, 12)] + [(200, 0, 128), (255, 0, 192), (127, 0, 64), (191, 9, 0), (66, 0, 64)])


def _weights(hd, seed=0, std=0.05, vocab=VOCAB, max_seq_len=256):
    oargs = ref_cpu.OracleArgs(vocab_size=vocab, max_seq_len=max_seq_len, **GEOM[hd])
    return oargs, ref_cpu.make_decoder_weights(oargs, seed=seed, std=std)


def _model(hd, sd, kv="rows", weights=None, vocab=VOCAB, max_seq_len=256):
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=vocab, max_seq_len=max_seq_len, max_batch_size=32, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    if kv == "rows":
        m.quantize_kv_cache("fp8", rows=True)
    return m


KV8 = ("k_q", "vt_q", "k_scale", "v_scale")


def _fill_random(m, seed):
    """finite codes (no 0x7F / 0xFF) and positive scales in every position of every row"""
    g = torch.Generator().manual_seed(seed)
    for i in range(m.n_layers):
        for k in KV8[:2]:
            t = m._kv8[k][i]
            b = torch.randint(0, 0x7F, t.shape, dtype=torch.uint8, generator=g) | (torch.randint(0, 2, t.shape, dtype=torch.uint8, generator=g) << 7)
            t.copy_(b.to(DEV))
        for k in KV8[2:]:
            t = m._kv8[k][i]
            t.copy_((torch.rand(t.shape, generator=g) * 0.01 + 0.001).to(DEV))


def _snapshot(m):
    return {k: [t.clone() for t in m._kv8[k]] for k in KV8}


def _restore(m, snap):
    for k in KV8:
        for t, s in zip(m._kv8[k], snap[k]):
            t.copy_(s)


def _step(m, rows, shared, tok, per_kernel=False):
    pos = i32([r[0] for r in rows])
    kw = dict(src_row=i32([r[1] for r in rows]), shared=i32([r[2] for r in rows])) if shared else {}
    m._per_kernel_decode = per_kernel
    try:
        return m.forward_inference_rows(tok, pos, max(r[0] for r in rows), **kw).clone()
    finally:
        m._per_kernel_decode = False


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("weights", [None, "nf4"])
def test_fused_step_equals_the_per_kernel_sequence_B3(weights, shared):
    hd = 128
    m = _model(hd, _weights(hd)[1], weights=weights)
    B = len(STEP3)
    w8 = {None: 0, "nf4": 2}[weights]
    assert lib.load().a3v_llama_decode_step_rows_kv8_form(B, m.args.dim, m.n_heads, m.n_kv_heads, hd, m.ffn, w8) == 2
    m.allocate_rows(B)
    assert m._k_cache[0].shape[0] == 1 and "stage_k" not in m._kv8, "a one-row bf16 pair and no staging pair"
    _fill_random(m, 3)
    start = _snapshot(m)
    tok = torch.randint(3, VOCAB, (B,), generator=torch.Generator().manual_seed(4)).to(DEV)
    fused = _step(m, STEP3, shared, tok)
    after = _snapshot(m)
    _restore(m, start)
    per = _step(m, STEP3, shared, tok, per_kernel=True)
    print(f"weights {weights} shared {shared}: max |fused - per kernel| = {float((fused - per).abs().max()):.3e}")
    assert torch.equal(fused, per)
    for k in KV8:
        for i in range(m.n_layers):
            assert torch.equal(after[k][i], m._kv8[k][i]), (k, i)
            assert not torch.equal(after[k][i], start[k][i]), "the step wrote the new positions"


def _per_kernel_step_rows_kv8(m, tok, pos, pos_max):
    """One ragged step over the fp8 rows cache as the sequence of PUBLIC entries (no fused GEMV forms): rmsnorm, GEMV,
    a3v_rope_kvquant_rows, a3v_attention_decode_rows_fp8kv, GEMV + residual, rmsnorm, GEMV SwiGLU, GEMV + residual; 17..32 rows as
    the two row chunks of the C call, every array addressed through its view of the chunk's rows (the restatement of
    tests/test_gpu_ragged.py's for the bf16 cache).  -> (logits, hidden state behind the last layer)"""
    a, kv8 = m.args, m._kv8
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
            fp8c = [kv8[k][i][b0:b0 + nb] for k in KV8]
            ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
            lin(xn, i, "wqkv", qkv)
            ops.rope_kvquant_rows(qkv, qkv, *fp8c, m._cos_sin_dev(), p, nb, H, Hkv, hd)
            ops.attention_decode_rows_fp8kv(qkv, *fp8c, att, sk, pos_max + 1, nb, H, Hkv, hd, scratch, ctr)
            lin(att, i, "wo", h, residual=h, epilogue=ops.EPI_RESIDUAL)
            ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
            lin(xn, i, "w13", act, epilogue=ops.EPI_SWIGLU)
            lin(act, i, "w2", h, residual=h, epilogue=ops.EPI_RESIDUAL)
        assert int(ctr.abs().sum()) == 0
    xn = torch.empty_like(hh)
    ops.rmsnorm(hh, m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(B, a.vocab_size, dtype=torch.float32, device=DEV)
    m._lm_head_f32(xn, logits)
    return logits, hh


def _shared_eff(rows):
    """(source row, S_b) per row of a (pos, src_row, shared) table"""
    B, eff = len(rows), []
    for b, (p, s, sh) in enumerate(rows):
        s = s if 0 <= s < B else b
        eff.append((s, 0 if s == b or p < 0 else min(sh, p + 1) & ~63))
    return eff


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("rows", [STEP3, STEP17], ids=["B3", "B17-two-chunks"])
@pytest.mark.parametrize("weights", [None, "fp8"])
def test_fused_step_equals_the_sequence_of_public_entries(weights, rows, shared):
    """a3v_llama_decode_step_rows_kv8 (through forward_inference_rows) == the per-kernel sequence of the public entries run in the C
    call's row chunks (B = 17: 9 + 8): logits, the hidden state behind the last layer and all four arrays of every layer, bit for
    bit.  Shared: the fused step runs on caches where every sibling's own [0, S_b) holds 0x7F bytes and inf scales (a sibling in the
    second chunk reads the leader in the first); the sequence of public entries, whose shared attention has no row offset, runs the
    PLAIN entries on caches into which bytes and scales of [0, S_b) of the source row were physically copied -- contract (c).
    hd 128 / dim 512, the geometry of tests/test_gpu_ragged.py's step test: the stand-alone fp8 GEMV entry refuses dim 256."""
    hd = 128
    m = _model(hd, _weights(hd)[1], weights=weights)
    B = len(rows)
    m.allocate_rows(B)
    _fill_random(m, 5)
    eff = _shared_eff(rows) if shared else [(b, 0) for b in range(B)]
    if B == 17:
        assert any(s == 0 and S > 0 for s, S in eff[9:]) or not shared
    copied = _snapshot(m)                                     # what the public entries see
    for i in range(m.n_layers):
        for b, (s, S) in enumerate(eff):
            if S:
                for k in KV8:
                    t = copied[k][i]
                    if k == "vt_q":
                        t[b, :, :, :S] = t[s, :, :, :S]
                    else:
                        t[b, :, :S] = t[s, :, :S]
                m._kv8["k_q"][i][b, :, :S] = 0x7F            # what the fused shared step must never read
                m._kv8["vt_q"][i][b, :, :, :S] = 0x7F
                m._kv8["k_scale"][i][b, :, :S] = float("inf")
                m._kv8["v_scale"][i][b, :, :S] = float("inf")
    tok = torch.randint(3, VOCAB, (B,), generator=torch.Generator().manual_seed(6)).to(DEV)
    pos, pos_max = i32([r[0] for r in rows]), max(r[0] for r in rows)
    fused = _step(m, rows, shared, tok)
    fused_h = m._buf("h", (B, m.args.dim)).clone()
    after = _snapshot(m)
    _restore(m, copied)
    per, per_h = _per_kernel_step_rows_kv8(m, tok, pos, pos_max)
    live = torch.tensor([r[0] >= 0 for r in rows], device=DEV)
    print(f"weights {weights} B {B} shared {shared}: max |fused - per kernel| = {float((fused[live] - per[live]).abs().max()):.3e}")
    assert torch.isfinite(fused[live]).all()
    assert torch.equal(fused_h[live], per_h[live]), "hidden state"
    assert torch.equal(fused[live], per[live]), "logits"
    for i in range(m.n_layers):
        for b, ((s, S), (p, _, _)) in enumerate(zip(eff, rows)):
            for k in KV8:
                x, y = after[k][i][b], m._kv8[k][i][b]
                if k == "vt_q":
                    x, y = x[:, :, S:], y[:, :, S:]
                else:
                    x, y = x[:, S:], y[:, S:]
                assert torch.equal(x, y), (k, i, b)            # the new position and everything the step must leave alone
            if p >= 0:
                assert not torch.equal(after["k_q"][i][b, :, p], copied["k_q"][i][b, :, p]), "the step wrote position pos[b]"



def test_form_query_refuses_and_touches_nothing():
    hd = 64
    m = _model(hd, _weights(hd)[1])
    B = 2
    m.allocate_rows(B)
    _fill_random(m, 7)
    start = _snapshot(m)
    L = lib.load()
    assert L.a3v_llama_decode_step_rows_kv8_form(B, 100, 2, 2, 50, 128, 0) == 0
    assert L.a3v_llama_decode_step_rows_kv8_form(33, m.args.dim, m.n_heads, m.n_kv_heads, hd, m.ffn, 0) == 0
    tab = m._llama_layer_table()
    h = torch.full((B, 100), 3.0, dtype=BF, device=DEV)
    bufs = m._decode_step_buffers(B)
    pos = i32([5, 9])
    rc = L.a3v_llama_decode_step_rows_kv8(tab, m._kv8_tab, m.n_layers, h.data_ptr(), *(t.data_ptr() for t in bufs), m._cos_sin_dev().data_ptr(),
                                          pos.data_ptr(), None, None, 9, B, 100, 2, 2, 50, 128, m._k_cache[0].shape[2], 1e-5,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and float((h.float() - 3.0).abs().sum()) == 0
    for k in KV8:
        for t, s in zip(m._kv8[k], start[k]):
            assert torch.equal(t, s)


# ------------------------------------------------------------------ 5. the model
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_row_is_bit_identical_and_fills_one_row(hd):
    _, sd = _weights(hd)
    ma, mb = _model(hd, sd, kv=None), _model(hd, sd)
    R_, T, row = 3, 70, 1
    tok = torch.randint(3, VOCAB, (1, T), generator=torch.Generator().manual_seed(5)).to(DEV)
    tok[0, 0] = 1
    for m in (ma, mb):
        m.allocate_rows(R_)
    for i in range(mb.n_layers):
        for k in KV8[:2]:
            mb._kv8[k][i].fill_(0x55)
        for k in KV8[2:]:
            mb._kv8[k][i].fill_(-3.0)
    la, lb = ma.prefill_row(row, tok), mb.prefill_row(row, tok)
    assert torch.equal(la, lb), "prefill_row logits over an fp8 rows cache must equal the bf16-cache model's bit for bit"
    assert mb._k_cache[0].shape[0] == 1 and mb._k_cache[0] is mb._k_cache[1], "one shared one-row bf16 pair"
    for i in range(ma.n_layers):
        k = ma._k_cache[i][row:row + 1, :, :T].float().cpu()
        v = ma._vt_cache[i][row:row + 1, :, :, :T].float().cpu().transpose(2, 3).contiguous()
        kq, vtq, ks, vs = kv8_ref.quantize_kv(k, v)
        g = {n: mb._kv8[n][i].cpu() for n in KV8}
        assert torch.equal(g["k_q"][row:row + 1, :, :T], kq) and torch.equal(g["vt_q"][row:row + 1, :, :, :T], vtq), i
        assert torch.equal(g["k_scale"][row:row + 1, :, :T], ks) and torch.equal(g["v_scale"][row:row + 1, :, :T], vs), i
        for r in (0, 2):
            assert bool((g["k_q"][r] == 0x55).all()) and bool((g["vt_q"][r] == 0x55).all()) and bool((g["k_scale"][r] == -3).all())
        assert bool((g["k_q"][row, :, T:] == 0x55).all()) and bool((g["vt_q"][row, :, :, T:] == 0x55).all()) and bool((g["v_scale"][row, :, T:] == -3).all())


class _FakeQuantOracle(ref_cpu.OracleDecoder):
    """OracleDecoder whose cache rows go through quantise -> dequantise (tests/kv8_ref.py) after every write (the restatement of
    tests/test_gpu_kv8.py's): a prefill attends over the rows it has just computed and the cache keeps their quantised form; a
    decode step reads every key, the new one included, from the cache."""

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
        self.k_cache[i][:bsz, sl] = kv8_ref.fake_quant(xk)
        self.v_cache[i][:bsz, sl] = kv8_ref.fake_quant(xv)
        keys = self.k_cache[i][:bsz, :start_pos + seqlen].clone()
        values = self.v_cache[i][:bsz, :start_pos + seqlen].clone()
        if seqlen > 1:
            keys[:, sl], values[:, sl] = xk, xv
        keys = ref_cpu.repeat_kv(keys, self.n_rep).transpose(1, 2)
        values = ref_cpu.repeat_kv(values, self.n_rep).transpose(1, 2)
        m = ref_cpu.make_causal_mask(seqlen, keys.size(2)) if mask == "causal" else None
        out = ref_cpu.sdpa(xq.transpose(1, 2), keys, values, m).transpose(1, 2).contiguous().view(bsz, seqlen, -1)
        return self.lin(out, p + "wo")


# weights, vocabulary, seeds and lengths chosen on the CPU from the oracle alone (a small vocabulary keeps the margins wide, a small
# std keeps the attention flat and D small): with these, ACC_DECIDED of the 16 (step, row) argmaxes have a top-2 margin above twice
# the bound -- asserted from the oracle before the device is asked
ACC = dict(hd=64, seed=11, std=0.03, vocab=16, T0=(9, 14), steps=8)
ACC_DECIDED = 15


def _oracle_runs():
    """Per prompt at batch 1: greedy decode of the fake-quantised oracle and the plain oracle fed the SAME tokens ->
    (weights, prompts, ids [steps] per prompt, fake-quantised logits per step per prompt, D = their largest deviation)."""
    c = ACC
    oargs, sd = _weights(c["hd"], seed=c["seed"], std=c["std"], vocab=c["vocab"], max_seq_len=128)
    sdb = {k: v.to(BF) for k, v in sd.items()}
    prompts, ids, logits, D = [], [], [], 0.0
    for r, T0 in enumerate(c["T0"]):
        fq, plain = _FakeQuantOracle(oargs, sdb), ref_cpu.OracleDecoder(oargs, sdb)
        ex = torch.randint(3, c["vocab"], (1, T0), generator=torch.Generator().manual_seed(12 + r))
        ex[:, 0] = 1
        lq, lp, idr = [fq.forward_inference(ex, 0).float()], [plain.forward_inference(ex, 0).float()], []
        for t in range(c["steps"] - 1):
            idr.append(lq[-1].argmax(-1))
            lq.append(fq.forward_inference(idr[-1][:, None], T0 + t).float())
            lp.append(plain.forward_inference(idr[-1][:, None], T0 + t).float())
        D = max(D, max(float((a - b).abs().max()) for a, b in zip(lq, lp)))
        prompts.append(ex)
        ids.append(idr)
        logits.append(lq)
    return sd, prompts, ids, logits, D


def test_ragged_greedy_decode_against_the_fake_quantised_oracle():
    """Two rows with prompts of different lengths, teacher-forced on the oracle's ids.  Allowed deviation of a step's logits, by
    the construction of tests/test_gpu_kv8.py: 4e-2 of max |logit| (the bf16 model test's bound against its oracle) plus D, the
    deviation between the fake-quantised and the plain oracle on the same inputs.  The argmax must agree wherever the oracle's top-2
    margin exceeds twice the bound."""
    c = ACC
    sd, prompts, ids, want, D = _oracle_runs()
    scale = max(float(w.abs().max()) for lq in want for w in lq)
    bound = 4e-2 * scale + D
    sure = [[float(w.topk(2, dim=-1).values[0, 0] - w.topk(2, dim=-1).values[0, 1]) > 2 * bound for w in lq] for lq in want]
    decided = sum(map(sum, sure))
    print(f"bound {bound:.3e} = 4e-2 * {scale:.3e} + D {D:.3e}; decided (step, row) choices {decided}/{2 * c['steps']}")
    assert decided >= ACC_DECIDED and 2 * decided >= 2 * c["steps"], decided
    m = _model(c["hd"], sd, vocab=c["vocab"], max_seq_len=128)
    m.allocate_rows(2)
    got = [[m.prefill_row(r, prompts[r].to(DEV)).float().cpu()] for r in range(2)]
    for t in range(c["steps"] - 1):
        tok = torch.stack([ids[r][t][0] for r in range(2)]).to(DEV)
        pos = [c["T0"][r] + t for r in range(2)]
        lg = m.forward_inference_rows(tok, i32(pos), max(pos)).float().cpu()
        for r in range(2):
            got[r].append(lg[r:r + 1])
    for r in range(2):
        for t, (g_, w) in enumerate(zip(got[r], want[r])):
            err = float((g_ - w).abs().max())
            print(f"row {r} step {t}: err {err:.3e} (bound {bound:.3e}); decided {sure[r][t]}")
            assert err <= bound, (r, t, err, bound)
            if sure[r][t]:
                assert int(g_.argmax(-1)) == int(w.argmax(-1)), (r, t)


DEC = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256, norm_eps=1e-5, rope_theta=10000.0)
VIT = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)
LONG = "Where is the drawer handle of the cabinet, and which way does it open? " * 2       # 85 tokens: a shared prefix of 64
PROMPTS = ["Detect the lid", LONG, "Open"]
GEN = [3, 6, 2]
N_S, TEMP, TOP_P = 4, 1.0, 0.9


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kv8rows")
    cfgp = tmp / "dec.json"
    cfgp.write_text(json.dumps(DEC))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=192)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, max_seq_len=192, **DEC), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(BF).to(DEV)
    mm.llma.quantize_kv_cache("fp8", rows=True)
    return mm


def test_generate_many_n4_equals_rows_that_hold_their_whole_prompt(meta):
    """n = 4 answers per prompt from ONE prefill, siblings reading the leader's keys below the last 64 boundary -- against the same
    loop (forward_inference_rows, the same uniforms) over rows that each hold the whole prompt physically: the prompts repeated four
    times through n = 1, where nothing is shared.  Ids and log-probs are equal, exactly."""
    mm = meta
    assert max(len(mm.tokenizer.encode(p, bos=True, eos=False)) for p in PROMPTS) > 66
    U = torch.rand(len(PROMPTS), N_S, max(GEN) + 3, generator=torch.Generator().manual_seed(17))
    calls, orig = [], mm.llma.prefill_row

    def counted(row, *a, **k):
        calls.append(row)
        return orig(row, *a, **k)
    mm.llma.prefill_row = counted
    try:
        texts, ids, sc = mm.generate_many(PROMPTS, None, batch_rows=8, max_gen_len=GEN, temperature=TEMP, top_p=TOP_P, return_ids=True,
                                          return_logprobs=True, sample_uniforms=U, n=N_S)
    finally:
        del mm.llma.prefill_row
    assert len(calls) == len(PROMPTS), "one prefill per prompt, not per sample"
    assert mm.llma._kv8 is not None and "stage_k" not in mm.llma._kv8 and mm.llma._k_cache[0].shape[0] == 1
    rep = [p for p in PROMPTS for _ in range(N_S)]
    _, rid, rsc = mm.generate_many(rep, None, batch_rows=8, max_gen_len=[g for g in GEN for _ in range(N_S)], temperature=TEMP, top_p=TOP_P,
                                   return_ids=True, return_logprobs=True, sample_uniforms=U.reshape(len(rep), -1))
    assert [x for per in ids for x in per] == rid and [x for per in sc for x in per] == rsc
    assert any(len({tuple(x) for x in per}) > 1 for per in ids), "the samples of a prompt differ"
    assert all(len(per) == N_S and all(len(s["logprobs"]) == len(t) for s, t in zip(per, pid)) for per, pid in zip(sc, ids))


def test_share_prefix_and_rows_driven_by_hand(meta):
    """The model's own share_prefix (a3v_kv8_copy_span) and shared step, without generate_many around them: rows 1..3 made siblings
    of row 0 against rows that each prefilled the whole prompt, forward_inference_rows driven by hand on the same tokens."""
    mm = meta
    llma = mm.llma
    tok = torch.tensor([mm.tokenizer.encode(LONG, bos=True, eos=False)], device=DEV)
    P, lo, Rn = tok.shape[1], tok.shape[1] & ~63, 4
    assert lo == 64 and P > lo + 2
    llma.allocate_rows(Rn)
    for i in range(llma.n_layers):
        for k in KV8[:2]:
            llma._kv8[k][i].fill_(0x7F)
        for k in KV8[2:]:
            llma._kv8[k][i].fill_(float("inf"))
    first = llma.prefill_row(0, tok)
    assert llma.share_prefix(0, [1, 2, 3], P) == lo
    for i in range(llma.n_layers):
        for k in KV8:
            t = llma._kv8[k][i]
            sl = (lambda x: x[:, :, lo:P]) if k == "vt_q" else (lambda x: x[:, lo:P])
            dead = (lambda x: torch.cat((x[:, :, :lo], x[:, :, P:]), 2)) if k == "vt_q" else (lambda x: torch.cat((x[:, :lo], x[:, P:]), 1))
            for r in (1, 2, 3):
                assert torch.equal(sl(t[r]), sl(t[0])), (k, i, r)                   # the span behind the last 64 boundary is copied
                d = dead(t[r])
                assert bool((d == 0x7F).all() if d.dtype == torch.uint8 else torch.isinf(d).all()), (k, i, r)   # nothing else is written
    shared_state = _snapshot(llma)
    g = torch.Generator().manual_seed(3)
    steps = [torch.randint(3, mm.tokenizer.n_words, (Rn,), generator=g).to(DEV) for _ in range(4)]      # different tokens per row
    src, sh = i32([0, 0, 0, 0]), i32([0, lo, lo, lo])
    got = [llma.forward_inference_rows(t, i32([P + j] * Rn), P + j, src_row=src, shared=sh).clone() for j, t in enumerate(steps)]
    llma.allocate_rows(Rn)                                    # the same rows, each holding the whole prompt physically
    _restore(llma, shared_state)
    for r in range(Rn):
        assert torch.equal(llma.prefill_row(r, tok), first)
    for j, t in enumerate(steps):
        want = llma.forward_inference_rows(t, i32([P + j] * Rn), P + j)
        assert torch.isfinite(got[j]).all() and torch.equal(got[j], want), j


def test_generate_many_with_constraint_and_penalty(meta):
    mm = meta
    texts, ids = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=6, temperature=0, return_ids=True, constraint=r"\[\d\d?\]")
    assert len(texts) == len(PROMPTS) and all(len(t) > 0 for t in ids)
    for t in texts:
        assert re.fullmatch(r"\[\d\d?\]", t.strip()) or re.fullmatch(r"\[?\d?\d?", t.strip()), t       # a match, or a prefix cut by max_gen_len
    texts, ids, sc = mm.generate_many(PROMPTS, None, batch_rows=3, max_gen_len=5, temperature=0, return_ids=True, repetition_penalty=1.3,
                                      return_logprobs=True)
    V = mm.tokenizer.n_words
    assert all(0 < len(t) <= 5 and all(0 <= x < V for x in t) for t in ids)
    assert all(len(s["logprobs"]) == len(t) and all(lp <= 0 for lp in s["logprobs"]) for s, t in zip(sc, ids))


def test_refusals_raise_before_any_allocation(meta):
    mm = meta
    llma = mm.llma
    llma.quantize_kv_cache("fp8", rows=True)                  # drops any cache
    assert llma._cache_shape is None
    tok = torch.zeros(2, 2, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match=r"lookup=0"):
        mm.generate_many(["Lid?"], None, batch_rows=2, max_gen_len=2, temperature=0, lookup=2)
    with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
        llma.forward_verify_rows(tok, i32([0, 0]), i32([1, 1]), 0)
    with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
        mm.beam_search(["Lid?"], None, num_beams=2, batch_rows=2, max_gen_len=2)
    assert llma._cache_shape is None and llma._kv8 is None, "nothing was allocated"
    llma.quantize_kv_cache("fp8")                             # without rows: as before
    for call in (lambda: llma.allocate_rows(2), lambda: llma.forward_inference_rows(tok[0], i32([0, 0]), 0),
                 lambda: mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=2)):
        with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
            call()
    assert llma._cache_shape is None
    llma.quantize_kv_cache("fp8", rows=True)


def test_generate_still_allocates_its_own_cache(meta):
    """generate() / forward_inference on a rows model: the fp8 cache of 7b (full pair, staging pair), a different _cache_shape kind"""
    mm = meta
    llma = mm.llma
    llma.allocate_rows(2)
    rows_shape = llma._cache_shape
    _, ids = mm.generate(["Detect the lid"], None, max_gen_len=3, temperature=0, return_ids=True)
    assert llma._cache_shape != rows_shape and "stage_k" in llma._kv8 and llma._k_cache[0].shape[0] == 1 and len(ids[0]) > 0
    _, ids2 = mm.generate_many(["Detect the lid"], None, batch_rows=2, max_gen_len=3, temperature=0, return_ids=True)
    assert "stage_k" not in llma._kv8 and llma._kv8["k_q"][0].shape[0] == 2


# ------------------------------------------------------------------ 6. the eval entry
def test_eval_entry_continuous_rows_with_kv_quant(tmp_path):
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd import eval_affordance_v2 as ev
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({**DEC, **VIT}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, max_seq_len=512, **DEC), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(DEC["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    ckdir = ck.save_checkpoint(str(tmp_path / "ck"), types.SimpleNamespace(precision="tf32", only_save_trainable=False), mm, None, None, None, epoch=0)
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_v2", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2", "--num_workers", "0",
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "10", "--max_seq_len", "512",
           "--temperature", "0.7", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "bf16",
           "--continuous_rows", "2", "--kv_quant", "fp8"]
    for flag, extra in (("rows", []), ("two", ["--num_samples", "2"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = json.load(open(tmp_path / "logs" / "rows" / "demo.json"))
    assert len(recs) == 3
    for rec in recs:
        assert sorted(rec) == sorted(["answer", "format_answer", "annotation", "question", "image", "fail"])
    recs = json.load(open(tmp_path / "logs" / "two" / "demo.json"))
    assert len(recs) == 3
    for rec in recs:
        ss = rec["samples"]
        assert len(ss) == 2 and all(sorted(s) == ["answer", "fail", "format_answer", "logprob_sum"] for s in ss)
        b = ss[ev.select_sample(ss)]
        assert (rec["answer"], rec["format_answer"], rec["fail"]) == (b["answer"], b["format_answer"], b["fail"])
