"""The decode GEMV family on the GPU against tests/gemv_ref.py: for every table entry and input family the outputs (C, and for the fused
forms the KV-cache row / column at pos and the sums of squares) equal the fp64 product put through the rounding sequence bit for bit
(exact inputs) or lie inside the derived bound (bounded inputs; SwiGLU on exact inputs too).  Operands are views at a 16-byte offset
into NaN-filled buffers with padded strides (fp8 bytes / NF4 nibbles: 0x7F, scales NaN), outputs are views into sentinel-filled buffers
that must come back untouched around the written windows, the workspace has NaN partials, zero counters that must be zero again and a
guarded tail, and a second call must give the same bits.  tests/test_gemv_ref_cpu.py shows that a correct fp32 implementation passes
these checks on the same inputs.  Run with -s for the ratios."""
import pytest
import torch

import gemv_ref as R
from a3vlm_amd import lib as L
from a3vlm_amd import ops
from test_gemv_ref_cpu import plan_of
from test_gpu_gemm_parity import embedded, embedded1d, surroundings_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PARAMS = [(c.id, f) for c in R.TABLE for f in R.FAMILIES]
WS_HEAD = 65536 // 4          # floats of counters, attention counters and sums of squares in front of the partials
WS_TAIL = 256


def _bytes(t):
    """a uint8 matrix embedded with 0x7F around it and a row stride that is a multiple of 16 bytes"""
    return embedded(t, 0x7F, min_ld=t.shape[1] + 8)


def guarded(shape, dtype):
    """a contiguous tensor of ``shape`` as a view, at a 16-byte offset, into a sentinel-filled flat buffer -> (flat, view)"""
    n = 1
    for s in shape:
        n *= s
    off = 16 // torch.empty((), dtype=dtype).element_size()
    flat = torch.full((n + 2 * off,), R.SENT, dtype=dtype, device=DEV)
    return flat, flat[off:off + n].view(*shape)


def workspace(c):
    n = (ops.gemm_skinny_ws_bytes(c.M, c.N, c.K) + 3) // 4
    ws = torch.full((n + WS_TAIL,), NAN, dtype=torch.float32, device=DEV)
    ws[:WS_HEAD] = 0.0
    ws[n:] = R.SENT
    return ws, n


def operands(c, inp):
    """device views of the case's inputs -> dict"""
    d = {"A": embedded(inp["A"], NAN)[1]}
    if c.fmt == "bf16":
        d["W"], d["wscale"] = embedded(inp["W"], NAN)[1], None
    else:
        d["W"] = _bytes(inp["Wq"])[1]
        s = embedded1d(inp["wscale"].reshape(-1), NAN)[1]
        d["wscale"] = s.view(inp["wscale"].shape) if c.fmt == "nf4" else s
    if "pro" in c.fused:
        d["norm_w"] = embedded1d(inp["norm_w"], NAN)[1]
        d["ssq_in"] = embedded1d(inp["ssq_in"].reshape(-1), NAN)[1].view(c.K // 16, 16)
    if "rope" in c.fused:
        d["cos_sin"] = embedded1d(inp["cos_sin"].reshape(-1), NAN)[1].view(inp["cos_sin"].shape)
    return d


def run_case(c, inp, d):
    """one call on fresh outputs -> (output dict as gemv_ref.judge takes it, checks as a list of (name, bool))"""
    od = R.out_dtype(c)
    cflat, C = embedded(torch.zeros(c.M, R.out_cols(c), dtype=od), R.SENT)
    C.fill_(R.SENT)
    res = None
    if "res" in c.epi:
        if "ssq" in c.fused:                       # as the decode step calls it: C is the residual stream, updated in place
            C.copy_(inp["res"].to(DEV))
            res = C
        else:
            res = embedded(inp["res"], NAN)[1]
    ws, n = workspace(c)
    out, flats = {"C": C}, []
    with L.env(**c.env):
        if not c.fused:
            fn = {"bf16": ops.gemm_skinny, "fp8": ops.gemm_skinny_fp8, "nf4": ops.gemm_skinny_nf4}[c.fmt]
            args = (d["A"], d["W"]) + (() if c.fmt == "bf16" else (d["wscale"],)) + (C, ws)
            fn(*args, residual=res, epilogue=c.flags & ~R.EPI["res"])
        else:
            rope = None
            if "rope" in c.fused:
                Hh, Hkv, hd, pos = c.geom
                kflat, out["k_cache"] = guarded((c.M, Hkv, R.SMAX, hd), R.BF)
                vflat, out["vt_cache"] = guarded((c.M, Hkv, hd, R.SMAX), R.BF)
                flats += [(kflat, out["k_cache"]), (vflat, out["vt_cache"])]
                rope = (d["cos_sin"], out["k_cache"], out["vt_cache"], Hh, Hkv, hd, pos)
            if "ssq" in c.fused:
                sflat, out["ssq"] = guarded((c.N // 16, 16), torch.float32)
                flats.append((sflat, out["ssq"]))
            ops.gemv_fused(d["A"], d["W"], C, ws, wscale=d["wscale"], n4=c.fmt == "nf4", residual=res, epilogue=c.flags,
                           norm_w=d.get("norm_w"), ssq_in=d.get("ssq_in"), eps=inp.get("eps", 0.0), ssq_out=out.get("ssq"), rope=rope)
    torch.cuda.synchronize()
    checks = [("stores outside C", surroundings_intact(cflat, C)),
              ("workspace counters are zero again", bool((ws[:WS_HEAD] == 0).all())),
              ("workspace tail", bool((ws[n:] == R.SENT).all()))]
    for flat, view in flats:                      # the bytes around the caches and the table; inside the caches gemv_ref.judge looks
        off = view.storage_offset() - flat.storage_offset()
        checks.append(("stores outside a side output", bool((flat[:off] == R.SENT).all()) and bool((flat[off + view.numel():] == R.SENT).all())))
    return {k: v.cpu() for k, v in out.items()}, checks


@pytest.mark.parametrize("cid,family", PARAMS, ids=[f"{a}-{b}" for a, b in PARAMS])
def test_gemv_parity(cid, family):
    c = R.BY_ID[cid]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc, plan = plan_of(L, c, cus)
    assert rc == c.plan[0] and plan == tuple(c.plan), (cid, "the device's plan is not the table's", cus, rc, plan)
    inp = R.inputs(c, family)
    r = R.reference(c, inp, family)
    d = operands(c, inp)
    out, checks = run_case(c, inp, d)
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), (cid, family, name, "NaN / inf in an output: poison was read, or an element was not written")
    for name, ok in checks:
        assert ok, (cid, family, name)
    equal, ratio = R.judge(c, r, out)
    if family == "exact" and r["C"]["bits"] is not None:
        bad = int((out["C"] != r["C"]["bits"]).sum())
        print(f"{cid:48s} {family:5s} bit-exact: {equal} ({bad} of {out['C'].numel()} elements of C differ, ratio to the bound {ratio:.3f})")
        assert equal is True, (cid, family, bad, ratio)
    else:
        print(f"{cid:48s} {family:5s} worst ratio {ratio:.3f}")
        assert ratio <= 1.0, (cid, family, ratio)
    again, checks2 = run_case(c, inp, d)
    for name, ok in checks2:
        assert ok, (cid, family, "second call", name)
    for name in out:
        assert torch.equal(out[name], again[name]), (cid, family, name, "a second call gives other bits")


@pytest.mark.parametrize("i", range(len(R.REFUSALS)), ids=[c.id for c, _ in R.REFUSALS])
def test_fused_refusals(i):
    """what the fused entry point refuses, as return codes: nothing is launched and nothing written"""
    c, want = R.REFUSALS[i]
    inp = R.inputs(c, "same") if c.geom == () else R.inputs(c._replace(fused=("pro",)), "same")
    d = operands(c._replace(fused=("pro",)), inp)
    cflat, C = embedded(torch.zeros(c.M, c.N, dtype=R.BF), R.SENT)
    C.fill_(R.SENT)
    ws, n = workspace(c)
    rope = None
    if c.geom:
        Hh, Hkv, hd, pos = c.geom
        k = guarded((c.M, Hkv, R.SMAX, hd), R.BF)[1]
        v = guarded((c.M, Hkv, hd, R.SMAX), R.BF)[1]
        cs = torch.zeros(R.SMAX, hd // 2, 2, dtype=torch.float32, device=DEV)
        rope = (cs, k, v, Hh, Hkv, hd, pos)
    rc = ops.gemv_fused(d["A"], d["W"], C, ws, wscale=d["wscale"], n4=c.fmt == "nf4", epilogue=c.flags, norm_w=d["norm_w"],
                        ssq_in=d["ssq_in"], eps=1e-5, rope=rope, check=False)
    torch.cuda.synchronize()
    assert rc == want, (c.id, rc, want)
    assert bool((cflat == R.SENT).all()) and bool((ws[n:] == R.SENT).all()) and bool((ws[:WS_HEAD] == 0).all())
