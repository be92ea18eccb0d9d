"""The W4A8 GEMM on MXFP4 images (include/a3vlm_hip.h "MXFP4 weights": a3v_quantize_rows_mxfp8, a3v_gemm_nt_mxfp4) restated in numpy.

Rows: ``quant_rows`` is mx4_ref.quant_act_mxfp8, optionally on the bf16 RMSNorm of the row (rounded where a3v_rmsnorm rounds:
bf16(bf16(x * rinv) * w), rinv in fp64 here -- the GPU test of the prologue compares against a3v_rmsnorm itself, bit for bit).
Product: fp64 over mx4_ref.dequantize of the image and 2^ea * a_q.  Epilogues: the rounding sequences the header states for
a3v_gemm_skinny_mxfp4 -- NONE bf16(acc); RESIDUAL bf16(bf16(acc) + residual); SWIGLU bf16(bf16(silu(bf16(gate))) * bf16(up)) on the
16-row interleaved gate | up rows; OUT_F32 float(bf16(acc)).

``bound``: every product a_q w_q 2^(ea + ew) is exact in fp32 (4 x 2 significant bits), so the only error of the accumulator is that of
adding K terms in fp32 in some order: |err| <= K 2^-24 sum |a| |w| =: E (mag = the summed |terms| in fp64).  E is pushed through the
epilogue as tests/gemm_ref.py ``reference`` does, with its constants (H = half a bf16 ulp, U24, LIP >= sup |silu'|, EVAL_F32 for the
device's silu); the element passes if |got - ref| <= rel |ref| + E' + TINY.  On exact inputs (every partial sum an integer number of
quanta below 2^24) E is zero in fact and ``bits`` is the expected output bit for bit; SwiGLU has no bits (silu is not correctly
rounded on the device) and keeps the bound.
"""
import numpy as np
import torch

import mx4_ref as R
from gemm_ref import EVAL_F32, HALF_ULP_BF16 as H, LIP, U24

EPI_RESIDUAL, EPI_SWIGLU, EPI_OUT_F32 = 8, 16, 32
TINY = 2.0 ** -134                      # half the bf16 / fp32-exponent subnormal spacing


def rbf(x):
    """fp64 values (exact in fp32 or not) -> the bf16 value a device conversion fp32 -> bf16 stores, as fp64."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def rmsnorm_bf16(x, w, eps):
    """bf16 RMSNorm of bf16 rows x (held in fp64) with a bf16 weight: (x * rsqrt(mean x^2 + eps)) -> bf16, * w -> bf16."""
    x = np.asarray(x, dtype=np.float64)
    rinv = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)
    return rbf(rbf(x * rinv) * np.asarray(w, dtype=np.float64)[None, :])


def quant_rows(x, norm_w=None, eps=0.0):
    """-> (e4m3 element values [M, K] fp64, block exponents [M, K/32] int64) of the rows, or of their bf16 RMSNorm."""
    y = np.asarray(x, dtype=np.float64) if norm_w is None else rmsnorm_bf16(x, norm_w, eps)
    return R.quant_act_mxfp8(y)


def e4m3_bytes(aq):
    """The e4m3fn byte of every element value of quant_rows (|v| <= 448, on the grid).  A negative element that rounds to zero keeps its
    sign (0x80, as v_cvt_pk_fp8_f32 writes it); an all-zero block is codes 0 whatever the signs of its zeros (the header's rule) -- a
    block with a nonzero element always has a nonzero code, its maximum lands in [256, 448]."""
    t = torch.from_numpy(np.ascontiguousarray(aq, dtype=np.float32)).to(torch.float8_e4m3fn)
    b = t.view(torch.uint8).numpy().copy()
    M, K = b.shape
    blk = b.reshape(M, K // 32, 32)
    blk[(np.asarray(aq).reshape(M, K // 32, 32) == 0).all(axis=-1)] = 0
    return b


def split_swiglu(p):
    """interleaved 16-row blocks of W -> (gate, up) columns of the product"""
    r, n = p.shape
    q = p.reshape(r, n // 32, 2, 16)
    return q[:, :, 0].reshape(r, n // 2), q[:, :, 1].reshape(r, n // 2)


def product64(aq, ea, q, s):
    """(acc, mag): the fp64 product of the dequantised operands and its summed |terms|."""
    A, W = R.dequant_act(aq, ea), R.dequantize(q, s)
    return A @ W.T, np.abs(A) @ np.abs(W).T


def reference(aq, ea, q, s, epi, res=None):
    """-> dict(ref fp64, E absolute allowance beyond the output rounding, rel the output rounding, bits: the output on an exact
    accumulator or None (SwiGLU))."""
    K = aq.shape[1]
    v, mag = product64(aq, ea, q, s)
    E = K * U24 * mag
    if epi & EPI_SWIGLU:
        g, u = split_swiglu(v)
        Eg, Eu = split_swiglu(E)
        Eg, Eu = Eg + H * (np.abs(g) + Eg), Eu + H * (np.abs(u) + Eu)
        sg = g / (1.0 + np.exp(-g))
        Es = LIP * Eg + EVAL_F32 * np.abs(g) + H * (np.abs(sg) + LIP * Eg)
        ref = sg * u
        Eo = (Es * (np.abs(u) + Eu) + np.abs(sg) * Eu) * (1.0 + U24) + U24 * np.abs(ref)
        return dict(ref=ref, E=Eo * (1.0 + H), rel=H, bits=None)
    bits = rbf(v)
    if epi & EPI_RESIDUAL:
        r = np.asarray(res, dtype=np.float64)
        E = E + H * (np.abs(v) + E)                     # rbf(acc)
        v = v + r
        E = E + U24 * (np.abs(v) + E)                   # the fp32 addition
        bits = bits + r                                 # exact inputs: one correctly rounded fp32 addition of two fp32 values
        bits = np.ascontiguousarray(bits, dtype=np.float32).astype(np.float64)
        if epi & EPI_OUT_F32:
            return dict(ref=v, E=E, rel=0.0, bits=bits)
        return dict(ref=v, E=E * (1.0 + H), rel=H, bits=rbf(bits))
    return dict(ref=v, E=E * (1.0 + H), rel=H, bits=bits)     # NONE and OUT_F32: the rounding of the accumulator is the output rounding


def ratio(got, r):
    """worst |got - ref| / bound over all elements (<= 1 passes; inf for a NaN / inf or a shape mismatch)"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != r["ref"].shape or not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - r["ref"]) / (r["rel"] * np.abs(r["ref"]) + r["E"] + TINY)).max())


def swiglu_on_exact(acc):
    """The SwiGLU sequence on an exact accumulator with a correctly rounded silu: the device result lies within two bf16 steps of it
    (its silu is v_exp / v_rcp, a few fp32 ulps: bf16(silu) may move one step, the rounding of the product one more)."""
    g, u = split_swiglu(rbf(acc))
    return rbf(rbf(g / (1.0 + np.exp(-g))) * u)
