"""The GEMM family on the GPU against tests/gemm_ref.py: for every table entry and input family the output equals the fp64 product put
through the epilogue's rounding sequence bit for bit (exact inputs) or lies inside the derived bound (bounded inputs; activation
epilogues on exact inputs too).  Operands are views at a 16-byte offset into NaN-filled buffers (beyond K, beyond the last row),
outputs views into sentinel-filled buffers that must come back untouched around them, split-K scratch is NaN-filled with a guarded tail.
tests/test_gemm_ref_cpu.py shows that a correct fp32 implementation passes these checks on the same inputs.  Run with -s for the ratios."""
import pytest
import torch

import gemm_ref as G
from a3vlm_amd import lib as L
from a3vlm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PARAMS = [(c.id, f) for c in G.TABLE for f in G.FAMILIES]


def _up8(n):
    return (n + 7) // 8 * 8


def embedded(t, fill, extra_rows=2, min_ld=0):
    """t [r, c] on the device as a view, at a 16-byte non-zero offset, into a flat buffer filled with ``fill``: row stride
    max(c rounded up to 8, min_ld) + 8, ``extra_rows`` more rows and 16 more bytes behind -> (flat buffer, view)"""
    r, c = t.shape
    ld = max(_up8(c), min_ld) + 8
    off = 16 // t.element_size()
    flat = torch.full((off + (r + extra_rows) * ld + off,), fill, dtype=t.dtype, device=DEV)
    view = flat[off:off + (r + extra_rows) * ld].view(r + extra_rows, ld)[:r, :c]
    view.copy_(t.to(DEV))
    return flat, view


def embedded1d(t, fill):
    off = 16 // t.element_size()
    flat = torch.full((t.numel() + 2 * off,), fill, dtype=t.dtype, device=DEV)
    flat[off:off + t.numel()] = t.to(DEV)
    return flat, flat[off:off + t.numel()]


def surroundings_intact(flat, view):
    """everything of ``flat`` outside ``view`` still holds the sentinel"""
    chk = flat.clone()
    off = view.storage_offset() - flat.storage_offset()
    r, c = view.shape
    chk[off:off + (r - 1) * view.stride(0) + c].as_strided((r, c), (view.stride(0), 1)).fill_(G.SENT)
    return bool((chk == G.SENT).all())


def poison_workspace():
    """the registered scratch of the hybrid dispatch, NaN in every plane before the call"""
    ops._ensure_gemm_workspace(DEV)
    for ws in ops._gemm_ws.values():
        ws.fill_(0xFF)


def run_case(c, inp):
    """-> (output view on the device, its flat buffer, extra checks as a list of (name, bool), sumsq slot sum or None)"""
    od = G.out_dtype(c)
    M, N = c.M, c.N
    checks, slots_sum = [], None
    cflat, C = embedded(torch.zeros(M, G.out_cols(c), dtype=od), G.SENT)
    C.fill_(G.SENT)
    res = None
    if inp.get("res") is not None:
        if "inplace" in c.epi or c.acc:
            C.copy_(inp["res"].to(DEV))
            res = C
        else:
            _, res = embedded(inp["res"], NAN)
    bias = embedded1d(inp["bias"], NAN)[1] if "bias" in c.epi else None
    if c.entry == "reduce":
        S = c.S
        sflat = torch.full((S * M * N + 256,), NAN, dtype=torch.float32, device=DEV)
        sflat[S * M * N:] = G.SENT
        sflat[:S * M * N] = inp["planes"].reshape(-1).to(DEV)
        L.check(L.load().a3v_splitk_reduce(sflat.data_ptr(), S, M, N, C.data_ptr(), C.stride(0), ops.dt(C), c.acc, ops._stream()), "a3v_splitk_reduce")
        checks.append(("scratch tail", bool((sflat[S * M * N:] == G.SENT).all())))
        return C, cflat, checks, slots_sum
    _, A = embedded(inp["A"], NAN, min_ld=64 if c.entry == "tn_strip" else 0)
    _, W = embedded(inp["W"], NAN)
    if c.entry in ("nt_splitk", "tn_splitk", "tn_strip"):
        S = c.S
        sflat = torch.full((S * M * N + 256,), NAN, dtype=torch.float32, device=DEV)
        sflat[S * M * N:] = G.SENT
        fn = {"nt_splitk": ops.gemm_nt_splitk, "tn_splitk": ops.gemm_tn_splitk, "tn_strip": ops.gemm_tn_strip}[c.entry]
        fn(A, W, C, sflat, S, accumulate=bool(c.acc))
        checks.append(("scratch tail", bool((sflat[S * M * N:] == G.SENT).all())))
        checks.append(("planes written", bool(torch.isfinite(sflat[:S * M * N]).all())))
        return C, cflat, checks, slots_sum
    poison_workspace()
    with L.env(**dict(c.env)):
        if c.entry in ("nt", "nt_f32"):
            ops.gemm_nt(A, W, C, bias=bias, residual=res, epilogue=c.flags)
        elif c.entry == "nn":
            ops.gemm_nn(A, W, C, residual=res, epilogue=c.flags)
        else:
            sumsq = None
            if c.entry == "tn_sumsq":
                slots = ops.gemm_tn_sumsq_slots(M, N)
                sumsq = torch.zeros(slots + 64, dtype=torch.float32, device=DEV)
                sumsq[slots:] = G.SENT
            ops.gemm_tn(A, W, C, residual=res, epilogue=c.flags, sumsq=sumsq)
            if sumsq is not None:
                checks.append(("sumsq tail", bool((sumsq[slots:] == G.SENT).all())))
                slots_sum = float(sumsq[:slots].double().sum())
    return C, cflat, checks, slots_sum


@pytest.mark.parametrize("cid,family", PARAMS, ids=[f"{a}-{b}" for a, b in PARAMS])
def test_gemm_parity(cid, family):
    c = G.BY_ID[cid]
    inp = G.inputs(c, family)
    rows = G.ref_rows(c) if c.subset else None
    r = G.reference(c, inp, rows)
    C, cflat, checks, slots_sum = run_case(c, inp)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(C).all()), (cid, family, "NaN / inf in the output: poison was read, or an element was not written")
    assert surroundings_intact(cflat, C), (cid, family, "stores outside C")
    for name, ok in checks:
        assert ok, (cid, family, name)
    got = C.cpu()
    got_rows = got if rows is None else got[rows]
    od = G.out_dtype(c)
    if family == "exact" and r["bits"] is not None:
        ratio = G.ratio(got_rows, r, od)
        bad = int((got_rows != r["bits"]).sum())
        print(f"{cid:64s} {family:5s} bit-exact: {bad} of {got_rows.numel()} differ (ratio to the bound {ratio:.3f})")
        assert torch.equal(got_rows, r["bits"]), (cid, family, bad, ratio)
    else:
        ratio = G.ratio(got_rows, r, od)
        print(f"{cid:64s} {family:5s} worst ratio {ratio:.3f}")
        assert ratio <= 1.0, (cid, family, ratio)
    if slots_sum is not None:
        sr = G.sumsq_ratio(slots_sum, got)
        print(f"{cid:64s} {family:5s} sumsq ratio {sr:.3g}")
        assert sr <= 1.0, (cid, family, sr)
