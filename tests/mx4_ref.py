"""The MXFP4 weight format and the MXFP8 activation rule of include/a3vlm_hip.h ("MXFP4 weights"), restated in numpy.

Weights W [N, K] (bf16 values held in float32 / float64), K % 32 == 0, blocks of 32 consecutive k of one row:
  E = floor(log2(max|w|)) - 2 clamped to [-127, 127], scale byte s = E + 127 (e8m0, value 2^(s - 127)); zero block: s = 127, codes 0;
  w / 2^E rounded to the nearest e2m1 value (codes 0..7 = 0 .5 1 1.5 2 3 4 6, bit 3 the sign), ties to the even code, saturating at
  +-6, -0 written as +0; element 2j in the low nibble of byte j.
Activations: the same rule with e4m3fn elements: E = floor(log2(max|a|)) - 8, round to nearest even, saturating at +-448.
"""
import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# code c >= i + 1 iff |v| is beyond the midpoint of grid[i], grid[i + 1]; on the midpoint the even code wins
_MID = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
_UP_ON_TIE = np.array([False, True, False, True, False, True, False])     # the upper code i + 1 is even


def _block_exponent(x, bias):
    """floor(log2(max|x|)) - bias over the last axis, clamped to [-127, 127]; 0 for an all-zero block (with a zero mask)."""
    mx = np.abs(x).max(axis=-1)
    zero = mx == 0
    _, e = np.frexp(np.where(zero, 1.0, mx))
    E = np.clip(e.astype(np.int64) - 1 - bias, -127, 127)
    return np.where(zero, 0, E), zero


def quantize(w):
    """w [N, K] -> (q [N, K/2] uint8, s [N, K/32] uint8)."""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    assert K % 32 == 0
    blk = w.reshape(N, K // 32, 32)
    E, _ = _block_exponent(blk, 2)
    v = np.ldexp(blk, -E[..., None].astype(np.int64))
    a = np.abs(v)
    code = np.zeros(a.shape, dtype=np.int64)
    for mid, up in zip(_MID, _UP_ON_TIE):
        code += (a >= mid) if up else (a > mid)
    code = np.where((v < 0) & (code > 0), code | 8, code).reshape(N, K)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return q, (E + 127).astype(np.uint8)


def codes(q):
    """q [N, K/2] -> the e2m1 values [N, K] (unscaled)."""
    q = np.asarray(q, dtype=np.uint8)
    c = np.empty((q.shape[0], q.shape[1] * 2), dtype=np.int64)
    c[:, 0::2] = q & 15
    c[:, 1::2] = q >> 4
    return np.where(c & 8, -1.0, 1.0) * E2M1[c & 7]


def dequantize(q, s):
    """Wd [N, K] float64 = e2m1(q) * 2^(s - 127) (exact; exact in bf16 too)."""
    v = codes(q)
    N, K = v.shape
    e = np.asarray(s, dtype=np.int64).reshape(N, K // 32) - 127
    return np.ldexp(v.reshape(N, K // 32, 32), e[..., None]).reshape(N, K)


def _round_e4m3(x):
    """Round |x| <= 448 to the nearest e4m3fn value, ties to even (3 mantissa bits, minimum normal 2^-6, subnormal step 2^-9)."""
    a = np.abs(x)
    _, e = np.frexp(np.where(a == 0, 1.0, a))
    ex = np.maximum(e.astype(np.int64) - 1, -6)
    return np.ldexp(np.rint(np.ldexp(x, 3 - ex)), ex - 3)


def quant_act_mxfp8(a):
    """a [M, K] -> (aq [M, K] float64: the e4m3 element values, ea [M, K/32] int64: the block exponents; byte = ea + 127)."""
    a = np.asarray(a, dtype=np.float64)
    M, K = a.shape
    assert K % 32 == 0
    blk = a.reshape(M, K // 32, 32)
    E, _ = _block_exponent(blk, 8)
    v = np.clip(np.ldexp(blk, -E[..., None].astype(np.int64)), -448.0, 448.0)
    return _round_e4m3(v).reshape(M, K), E


def dequant_act(aq, ea):
    M, K = aq.shape
    return np.ldexp(aq.reshape(M, K // 32, 32), ea[..., None]).reshape(M, K)


def fake_quant_act(a):
    """The values the GEMV multiplies: a -> 2^ea * a_q."""
    return dequant_act(*quant_act_mxfp8(a))
