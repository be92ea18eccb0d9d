"""TEST INFRASTRUCTURE ONLY: the host restatement of the 8-bit AdamW moment format (include/a3vlm_hip.h, "8-bit AdamW moments") in
numpy -- blockwise e4m3 quantiser, its inverse, the code-0x01 rule of the second moment -- and of one AdamW step on that state in
float32.  The product quantises and steps with the HIP kernels of a3v_adam8.hip, never with this file."""
from __future__ import annotations

import numpy as np

BLOCK = 256
FLOOR = np.float32(1e-30)
F448 = np.float32(448.0)
ZERO_SCALE = FLOOR / F448            # the scale of an all-zero block


def e4m3_encode(t: np.ndarray) -> np.ndarray:
    """float32 t -> OCP e4m3fn codes (uint8): round to nearest even, saturating at +-448, the sign of a zero kept."""
    t = np.asarray(t, dtype=np.float32)
    sign = np.signbit(t).astype(np.uint8) << 7
    a = np.minimum(np.abs(t).astype(np.float64), 448.0)          # every step below is exact in float64
    sub = np.rint(a * 512.0)                                      # |t| < 2^-6: multiples of 2^-9 (rint: ties to even); 8 = the first normal
    mant, ex = np.frexp(np.maximum(a, 2.0 ** -6))                 # a = mant * 2^ex, mant in [0.5, 1)
    e = ex - 1
    n = np.rint(a / np.exp2((e - 3).astype(np.float64)))          # 8 .. 16 steps of 2^(e-3)
    e = np.where(n == 16, e + 1, e)
    n = np.where(n == 16, 8, n)
    norm = ((e + 7).astype(np.int64) << 3) | (n.astype(np.int64) - 8)
    mag = np.where(a < 2.0 ** -6, sub.astype(np.int64), norm)
    return (sign | mag.astype(np.uint8)).astype(np.uint8)


def e4m3_decode(q: np.ndarray) -> np.ndarray:
    """codes -> float32 (exact).  The two NaN codes never occur in quantised state."""
    q = np.asarray(q, dtype=np.uint8).astype(np.int64)
    e, f = (q >> 3) & 15, q & 7
    mag = np.where(e == 0, f * 2.0 ** -9, (8 + f) * np.exp2((e - 10).astype(np.float64)))
    return np.where(q & 0x80, -mag, mag).astype(np.float32)


def block_scale(x_abs: np.ndarray) -> np.ndarray:
    """|x| [n] -> one float32 scale per block of 256: max(max|x|, 1e-30) / 448."""
    amax = x_abs.reshape(-1, BLOCK).max(axis=1).astype(np.float32)
    return (np.maximum(amax, FLOOR) / F448).astype(np.float32)


def quantize_m(m: np.ndarray):
    m = np.asarray(m, dtype=np.float32).reshape(-1)
    s = block_scale(np.abs(m))
    t = (m.reshape(-1, BLOCK) / s[:, None]).astype(np.float32)    # a true float32 division
    return e4m3_encode(t).reshape(-1), s


def quantize_r(r: np.ndarray, keep_nonzero: bool = True):
    """r = sqrt(v) >= 0.  keep_nonzero: a non-zero r whose quotient rounds to code 0 is stored as code 0x01."""
    r = np.asarray(r, dtype=np.float32).reshape(-1)
    s = block_scale(r)
    q = e4m3_encode((r.reshape(-1, BLOCK) / s[:, None]).astype(np.float32)).reshape(-1)
    if keep_nonzero:
        q = np.where((r != 0) & ((q & 0x7F) == 0), q | 1, q).astype(np.uint8)
    return q, s


def quantize(m: np.ndarray, v: np.ndarray, keep_nonzero: bool = True):
    """(exp_avg, exp_avg_sq) float32 [n], n % 256 == 0 -> (m_q, m_scale, r_q, r_scale)."""
    mq, ms = quantize_m(m)
    rq, rs = quantize_r(np.sqrt(np.asarray(v, dtype=np.float32).reshape(-1)), keep_nonzero)
    return mq, ms, rq, rs


def dequantize_m(mq, ms) -> np.ndarray:
    return (e4m3_decode(mq).reshape(-1, BLOCK) * np.asarray(ms, dtype=np.float32)[:, None]).astype(np.float32).reshape(-1)


def dequantize_r(rq, rs) -> np.ndarray:
    return dequantize_m(rq, rs)


def dequantize(mq, ms, rq, rs):
    """-> (m^, v^) float32: m^ = float(q) * scale, v^ = (float(q) * scale)^2, every product rounded to float32."""
    r = dequantize_r(rq, rs)
    with np.errstate(under="ignore"):
        return dequantize_m(mq, ms), (r * r).astype(np.float32)


def e4m3_step(y: np.ndarray) -> np.ndarray:
    """Spacing of e4m3fn at |y| (code units, |y| <= 448): 2^(e-3), e = floor(log2|y|) >= -6 (subnormals: 2^-9)."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(y).astype(np.float64), 2.0 ** -6))) - 3)


def half_step_bound(x: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """|stored - x| allowed by round-to-nearest: half the e4m3 spacing at x / scale, times scale, plus the two float32 roundings on
    the way (x / scale, code * scale: 2^-23 of |x| each)."""
    s = np.repeat(np.asarray(scale, dtype=np.float64), BLOCK)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return 0.5 * e4m3_step(x / s) * s + 2.0 ** -22 * np.abs(x)


def adamw_step_fp32(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.AdamW's update in float32 (the statements of a3v_adamw_scaled, without its fma contraction)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    step_size = f(lr / (1.0 - b1 ** step))
    inv_bc2_sqrt = f(1.0 / np.sqrt(1.0 - b2 ** step))
    p = p * f(1.0 - lr * wd)
    m = m + (f(1) - f(b1)) * (g - m)
    v = f(b2) * v + (f(1) - f(b2)) * g * g
    p = p - step_size * m / (np.sqrt(v) * inv_bc2_sqrt + f(eps))
    return p.astype(f), m.astype(f), v.astype(f)


def adamw8_step(p, g, mq, ms, rq, rs, step, lr, b1, b2, eps, wd, keep_nonzero: bool = True):
    """One 8-bit step: dequantise, the float32 update, quantise.  -> (p, m_q, m_scale, r_q, r_scale)."""
    m, v = dequantize(mq, ms, rq, rs)
    p, m, v = adamw_step_fp32(p, g, m, v, step, lr, b1, b2, eps, wd)
    return (p,) + quantize(m, v, keep_nonzero)


def zero_state(n: int):
    return (np.zeros(n, np.uint8), np.full(n // BLOCK, ZERO_SCALE, np.float32), np.zeros(n, np.uint8), np.full(n // BLOCK, ZERO_SCALE, np.float32))
