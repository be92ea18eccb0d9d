"""TEST INFRASTRUCTURE ONLY: the reference, the inputs and the bounds of the optimizer-step parity tests (test_optim_ref_cpu.py,
test_gpu_optim_parity.py).  The product steps with the HIP kernels of a3v_train.hip / a3v_adam8.hip, never with this file.

* ``adamw_ref``        one AdamW step in float64, with the hyper-parameters as the float32 values the C ABI receives and the scaled
                       gradient g' = fp32(g * coef) (the kernels round that product with __fmul_rn: that rounding is contract).
* ``adamw_bounds``     per-element bounds of |device - reference| for m', v', p' (derivation below).
* ``exact_case``       inputs on which every operation of the step is exact in float32, with their closed-form results.
* ``bounded_inputs``   inputs on which the arithmetic variants differ.
* ``sumsq_ref`` / ``sumsq_bound`` / ``sumsq_exact_input``   the same for a3v_sumsq_partials, per slot.
* ``emu_*``            float32 emulations of the kernels (element arithmetic, ownership, layout), with the wrong variants of MUTATIONS.

Bounds (u = 2^-24, the unit round-off of float32; fl(x) = x (1 + d), |d| <= u, for +, -, *, /, sqrt, all correctly rounded on the
device: hipcc's default fp32 division and sqrtf are).  Every line is one float32 operation of ``adamw_update`` (a3v_common.h); a
term is dropped where the operation is exact FOR SURE (an operand is zero or a power of two), which is what makes the bounds tight
enough to see a single missing rounding.  A contracted form (fma) only removes roundings from this list, so the bounds hold for
every contraction the compiler may pick.  c1 = 1 - b1, c2 = 1 - b2 in exact arithmetic; e1, e2 = |fl(1.f - b) - (1 - b)| (zero
for every b in [0.5, 1] and for b = 0: Sterbenz).

  m' = m + c1 (g' - m):
      d  = fl(g' - m)            u |g' - m|            (0 where m = 0 or g' = 0)
      t  = fl(fl(c1) d)          e1 |g' - m| + u c1 |g' - m|      (the rounding: 0 where fl(c1) is a power of two)
      m' = fl(m + t)             u |m'|                (0 where m = 0)
    E_m = e1 |d| + u |d| [m, g' != 0] + u c1 |d| [c1 not 2^k] + u |m'| [m != 0]

  v' = b2 v + c2 g'^2            (every term is non-negative: no cancellation, E_v <= ~4 u v')
      t1 = fl(b2 v)              u b2 v                (0 where v = 0 or b2 is a power of two)
      t2 = fl(fl(c2) g')         (e2 + u c2) |g'|      -> times |g'| in t3       (the rounding: 0 where fl(c2) is a power of two)
      t3 = fl(t2 g')             u c2 g'^2             (0 where g' is a power of two)
      v' = fl(t1 + t3)           u v'                  (0 where v = 0 or g' = 0)
    E_v = e2 g'^2 + u b2 v [..] + u c2 g'^2 [..] + u c2 g'^2 [..] + u v' [..]

  p' = p decay - step_size m' / (sqrt(v') inv_bc2_sqrt + eps), with the host scalars decay = fl(1 - lr wd), step_size =
  fl(lr / (1 - b1^t)), inv_bc2_sqrt = fl(1 / sqrt(1 - b2^t)) rounded ONCE from float64 (errors ed, es, ei taken as they are):
      pd  = fl(p decay)          |p| ed + u |p decay|  (the rounding: 0 where decay is a power of two, i.e. wd = 0)
      s   = fl(sqrt(v'))         sqrt(v') (E_v / (2 v') + u)        (v' = 0: exact)
      q   = fl(s inv)            E_s inv + sqrt(v') |ei| + u q       (the rounding: 0 where inv is a power of two)
      den = fl(q + eps)          E_q + u den            (the rounding: 0 where eps = 0 or q = 0)
      num = fl(step_size m')     step_size E_m + |m'| |es| + u |num| (the rounding: 0 where step_size is a power of two)
      quo = fl(num / den)        E_num / den + |num| E_den / den^2 + u |quo|
      p'  = fl(pd - quo)         u |p'|                 (0 where quo = 0 or pd = 0)
    E_p = E_pd + E_quo + u |p'| [..]

Each E is multiplied by 1 + 2^-10 for the second-order terms dropped above (products of two relative errors of at most ~8 u each,
i.e. below 2^-20 of a first-order term).  The bf16 image is not bounded: it is the round-to-nearest-even of the DEVICE's own
float32 p', exactly.

sumsq: vector i (4 floats) belongs to slot (i // 256) % 1024 and, inside the slot, to thread i % 256; the n % 4 tail elements belong
to threads 0 .. of slot 0.  A thread adds its L squares with one fmaf each (one rounding of a partial sum that never exceeds the
thread's total), then six butterfly levels and two more additions reduce the block (each rounding at most u times a partial sum
of non-negative terms, i.e. at most u times the slot's total): |slot - reference| <= (L_max + 8) u slot, L_max = the longest
chain among the slot's threads = 4 ceil(vectors of the slot / 256) (+ 1 in slot 0 with a tail)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
F32, F64 = np.float32, np.float64
SLOTS = 1024
GRID_CAP = 4096                         # a3v_adamw_scaled: at most 4096 blocks of 256 threads, one 16-byte vector per thread and trip
CAP_N = GRID_CAP * 256 * 4              # 4 194 304 elements per trip

Hyper = namedtuple("Hyper", "lr b1 b2 eps wd step")

STEPS = (1, 2, 10, 1000, 100000)
BETAS = ((0.9, 0.95), (0.9, 0.999), (0.0, 0.5))
WDS = (0.0, 0.1)
COEFS = (None, 1.0, 0.37, 0.0)


def bounded_hypers(lr=3e-3, eps=1e-8):
    return [Hyper(lr, b1, b2, eps, wd, step) for (b1, b2) in BETAS for step in STEPS for wd in WDS]


def f32v(x) -> float:
    """The float32 value the C ABI receives, as a Python float."""
    return float(F32(x))


def scalars(h: Hyper, mut=None):
    """The host scalars of a3v_adamw_scaled: float64 values (the reference's) and their float32 roundings (the kernel's)."""
    lr, b1, b2, eps, wd = (f32v(x) for x in (h.lr, h.b1, h.b2, h.eps, h.wd))
    s1 = h.step - 1 if mut == "bc1_prev_step" else h.step
    s2 = h.step - 1 if mut == "bc2_prev_step" else h.step
    bc1, bc2 = 1.0 - b1 ** s1, 1.0 - b2 ** s2
    with np.errstate(divide="ignore"):
        step_size = float(np.divide(F64(lr), F64(bc1)))
        inv = 1.0 if mut == "bc2_missing" else float(np.divide(F64(1.0), np.sqrt(F64(bc2))))
    decay = 1.0 - lr * wd
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, decay=decay, step_size=step_size, inv=inv, c1=1.0 - b1, c2=1.0 - b2,
                decay32=f32v(decay), step_size32=f32v(step_size), inv32=f32v(inv), c1_32=float(F32(1) - F32(b1)),
                c2_32=float(F32(1) - F32(b2)))


def skipped(coef) -> bool:
    """A NaN coefficient or one with the sign bit set (negative, -0.0) makes the step a no-op."""
    return coef is not None and bool(np.isnan(F32(coef)) or np.signbit(F32(coef)))


def scaled_grad(g, coef):
    g = np.asarray(g, F32)
    return g if coef is None else (g.astype(F64) * F64(F32(coef))).astype(F32)


def bf16_bits(p) -> np.ndarray:
    """Round-to-nearest-even bf16 of finite float32 values, as uint16 bit patterns."""
    b = np.ascontiguousarray(np.asarray(p, F32)).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_torch(p: torch.Tensor) -> torch.Tensor:
    """The same on a torch float32 tensor (any device): int16 bit patterns, comparable with ``image.view(torch.int16)``."""
    b = p.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).to(torch.int16)        # int64 -> int16 keeps the low 16 bits


def adamw_ref(p, g, m, v, h: Hyper, coef=None):
    """One step in float64 -> dict(p, m, v (float64), image (uint16 bf16 bits of fp32(p)), and the intermediates the bounds use)."""
    p, m, v = (np.asarray(a, F32).astype(F64) for a in (p, m, v))
    if skipped(coef):
        return dict(p=p, m=m, v=v, skipped=True)
    s = scalars(h)
    g1 = scaled_grad(g, coef).astype(F64)
    pd = p * s["decay"]
    d = g1 - m
    m1 = m + s["c1"] * d
    v1 = s["b2"] * v + s["c2"] * g1 * g1
    root = np.sqrt(v1)
    den = root * s["inv"] + s["eps"]
    num = s["step_size"] * m1
    with np.errstate(invalid="ignore", divide="ignore"):
        quo = num / den
    p1 = pd - quo
    return dict(p=p1, m=m1, v=v1, g1=g1, d=d, pd=pd, root=root, den=den, num=num, quo=quo, p0=p, m0=m, v0=v, skipped=False)


def _pow2(x):
    """Element-wise (or scalar): x is zero or a power of two, so a float32 product with x is exact."""
    mant, _ = np.frexp(np.abs(np.asarray(x, F64)))
    return (mant == 0.5) | (mant == 0.0)


def adamw_bounds(r, h: Hyper):
    """(E_p, E_m, E_v) float64 per element for the reference ``r`` of ``adamw_ref`` (module docstring).  A skipped step: zeros."""
    if r["skipped"]:
        z = np.zeros_like(r["p"])
        return z, z, z
    s = scalars(h)
    g1, m0, v0, d, m1, v1 = r["g1"], r["m0"], r["v0"], r["d"], r["m"], r["v"]
    e1, e2 = abs(s["c1_32"] - s["c1"]), abs(s["c2_32"] - s["c2"])
    ad, g2 = np.abs(d), g1 * g1
    E_m = e1 * ad + U * ad * ((m0 != 0) & (g1 != 0)) + (0.0 if _pow2(s["c1_32"]) else U * s["c1"] * ad) + U * np.abs(m1) * (m0 != 0)
    E_v = (e2 * g2 + (0.0 if _pow2(s["b2"]) else U * s["b2"] * v0) + (0.0 if _pow2(s["c2_32"]) else U * s["c2"] * g2)
           + U * s["c2"] * g2 * ~_pow2(g1) + U * v1 * ((v0 != 0) & (g1 != 0)))
    E_m, E_v = E_m * SECOND_ORDER, E_v * SECOND_ORDER
    ed, es, ei = abs(s["decay32"] - s["decay"]), abs(s["step_size32"] - s["step_size"]), abs(s["inv32"] - s["inv"])
    p0, pd, root, den, num, quo, p1 = r["p0"], r["pd"], r["root"], r["den"], r["num"], r["quo"], r["p"]
    E_pd = np.abs(p0) * ed + (0.0 if _pow2(s["decay32"]) else U * np.abs(pd))
    with np.errstate(invalid="ignore", divide="ignore"):
        E_s = np.where(v1 > 0, root * (E_v / (2 * np.where(v1 > 0, v1, 1.0)) + U), 0.0)
        q = root * s["inv"]
        E_q = E_s * s["inv"] + root * ei + (0.0 if _pow2(s["inv32"]) else U * q)
        E_den = E_q + U * den * ((s["eps"] != 0) & (q != 0))
        E_num = s["step_size"] * E_m + np.abs(m1) * es + (0.0 if _pow2(s["step_size32"]) else U * np.abs(num))
        E_quo = E_num / den + np.abs(num) * E_den / (den * den) + U * np.abs(quo)
    E_p = (E_pd + E_quo + U * np.abs(p1) * ((quo != 0) & (pd != 0))) * SECOND_ORDER
    return E_p, E_m, E_v


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound over the elements (0/0 = 0: an exact match under a zero bound; x/0 = inf)."""
    err = np.abs(np.asarray(got).astype(F64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs

def _hash(idx: torch.Tensor, a: int, b: int, mod: int) -> torch.Tensor:
    """A multiplicative hash of the element index (int64, any device); a < 2^31 and idx < 2^31 keep the product inside int64."""
    return (((idx * a + b) & 0x7FFFFFFF) >> 7) % mod


EXACT_HYPER = dict(lr=2.0 ** -7, b1=0.5, b2=0.75, eps=0.0, step=1)


def exact_hyper(wd) -> Hyper:
    return Hyper(EXACT_HYPER["lr"], EXACT_HYPER["b1"], EXACT_HYPER["b2"], EXACT_HYPER["eps"], wd, EXACT_HYPER["step"])


def exact_case(n, wd, stationary, coef=None, device="cpu", offset=0):
    """Inputs on which every float32 operation of the step is exact, and their closed-form results (module docstring of the issue:
    b1 = 0.5, b2 = 0.75, step 1, lr = 2^-7, eps = 0, wd in {0, 0.5}; g' = +-2^k, p = j 2^-7, state zero or m = c g', v = g'^2).
    ``coef`` (a power of two, or None): the gradient handed to the kernel is g' / coef.  j, k, c and the sign come from different
    hashes of the element index (+ ``offset``).  -> dict of float32 torch tensors p, g, m, v (inputs) and p1, m1, v1 (results)."""
    assert wd in (0.0, 0.5) and (coef is None or coef in (0.5, 2.0, 0.25))
    idx = torch.arange(n, dtype=torch.int64, device=device) + offset
    k = _hash(idx, 2654435761 % (1 << 31), 12345, 41) - 20
    sg = _hash(idx, 1597334677, 977, 2)
    j = _hash(idx, 1103515245, 40503, 1 << 14)
    c = _hash(idx, 374761393, 668265263 % (1 << 20), 7) - 3
    sign = 1.0 - 2.0 * sg.to(torch.float64)
    g1 = ((k + 127) << 23).to(torch.int32).view(torch.float32).to(torch.float64) * sign              # 2^k from its bit pattern
    p = j.to(torch.float64) * 2.0 ** -7
    cf = c.to(torch.float64)
    if stationary:
        m, v = cf * g1, g1 * g1
        m1, v1, upd = (cf + 1) * g1 / 2 + 0.0, g1 * g1, (cf + 1) * 2.0 ** -8 * sign      # + 0.0: c = -1 gives +0, as x - x does
    else:
        m, v = torch.zeros_like(g1), torch.zeros_like(g1)
        m1, v1, upd = g1 / 2, g1 * g1 / 4, 2.0 ** -7 * sign
    p1 = p * (1.0 - 2.0 ** -7 * wd) - upd
    g = g1 if coef is None else g1 / coef
    out = dict(p=p, g=g, m=m, v=v, p1=p1, m1=m1, v1=v1)
    for name, t in out.items():
        t32 = t.to(torch.float32)
        assert torch.equal(t32.to(torch.float64), t), name            # every value is a float32
        out[name] = t32
    return out


def bounded_inputs(n, seed=0, eps=1e-8):
    """p, g, m, v (float32 numpy).  Element classes by (index + seed) % 8: 0: g = m = v = 0 (update 0, not NaN);  1: g = 0 with old
    state;  2: |g| near eps from a zero state (sqrt(v') ~ eps);  3: |g| near eps with old state of that size;  4, 5: |g| = 2^U(-30, 20)
    from a zero state;  6, 7: the same with old state (m of either sign, v around g^2)."""
    rs = np.random.RandomState(1000 + seed)
    cls = (np.arange(n) + seed) % 8
    mag = np.exp2(rs.uniform(-30, 20, n))
    mag = np.where((cls == 2) | (cls == 3), eps * np.exp2(rs.uniform(-3, 3, n)), mag)
    g = mag * rs.choice([-1.0, 1.0], n) * rs.uniform(1.0, 2.0, n)
    g = np.where(cls <= 1, 0.0, g)
    scale = np.where(cls == 1, np.exp2(rs.uniform(-20, 10, n)), mag)
    old = (cls == 1) | (cls == 3) | (cls >= 6)
    m = np.where(old, scale * rs.randn(n), 0.0)
    v = np.where(old, scale * scale * rs.uniform(0.25, 4.0, n), 0.0)
    p = rs.randn(n) * np.exp2(rs.uniform(-4, 4, n))
    return tuple(np.ascontiguousarray(a, dtype=F32) for a in (p, g, m, v))


# ------------------------------------------------------------------------------------------------ emulations of the update

MUTATIONS = {
    1: "eps_before_bc", 2: "bc2_missing", 3: "bc1_prev_step", 4: "l2_decay", 5: "decay_after_update", 6: "coef_m_only",
    7: "coef_twice_in_v", 8: "coef_unrounded", 9: "tail_skipped", 10: "trip_last_vector_skipped", 11: "lanes_rotated",
    12: "image_truncated", 13: "image_pre_update", 14: "t_rc_swapped", 15: "t_row_offset_dropped", 16: "neg_coef_abs",
    17: "sumsq_tail_dropped", 18: "sumsq_slot_to_neighbour",
}
MUTATION_2B = "bc2_prev_step"             # the second form of mutation 2


def _r(x):
    """Round a float64 array to float32 and back: +, -, *, /, sqrt of float32 operands done in float64 and rounded once more equal
    the float32 operation (53 >= 2 * 24 + 2 bits: the double rounding is innocuous)."""
    return np.asarray(x, F64).astype(F32).astype(F64)


def emu_update(p, g, m, v, h: Hyper, coef=None, form="plain", mut=None):
    """The statements of ``adamw_update`` in float32, element by element -> (p', m', v') float32.
    form: "plain" (every operation rounded), "fma_a" (m' = fma(c1, d, m), v' = fma(b2, v, (c2 g) g), den = fma(s, inv, eps)),
    "fma_b" (v' = fma(c2 g, g, b2 v) instead).  mut: one of the arithmetic MUTATIONS (1 - 8, 16)."""
    p, g, m, v = (np.asarray(a, F32).astype(F64) for a in (p, g, m, v))
    gs = None if coef is None else F32(coef)
    if mut == "neg_coef_abs" and gs is not None and gs < 0:
        gs = -gs
    if skipped(gs):
        return p.astype(F32), m.astype(F32), v.astype(F32)
    s = scalars(h, mut)
    gsd = 1.0 if gs is None else float(gs)
    gm = g * gsd if mut == "coef_unrounded" else _r(g * gsd)           # unrounded: the float64 product is exact
    gv = gm
    if mut == "coef_m_only":
        gv = g
    if mut == "coef_twice_in_v":
        gv = _r(gm * gsd)
    decay, b1, b2, ss, inv, eps, c1, c2 = (s[k] for k in ("decay32", "b1", "b2", "step_size32", "inv32", "eps", "c1_32", "c2_32"))
    fma = form != "plain"
    if mut == "l2_decay":
        gm = gv = _r(gm + _r(s["wd"] * p))
        pd = p
    elif mut == "decay_after_update":
        pd = p
    else:
        pd = _r(p * decay)
    d = _r(gm - m)
    m1 = _r(m + c1 * d) if fma else _r(m + _r(c1 * d))
    t2 = _r(c2 * gv)
    if form == "fma_a":
        v1 = _r(b2 * v + _r(t2 * gv))
    elif form == "fma_b":
        v1 = _r(t2 * gv + _r(b2 * v))
    else:
        v1 = _r(_r(b2 * v) + _r(t2 * gv))
    root = _r(np.sqrt(v1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mut == "eps_before_bc":
            den = _r(_r(root + eps) * inv)
        else:
            den = _r(root * inv + eps) if fma else _r(_r(root * inv) + eps)
        quo = _r(_r(ss * m1) / den)
        p1 = _r(pd - quo)
        if mut == "decay_after_update":
            p1 = _r(p1 * decay)
    return p1.astype(F32), m1.astype(F32), v1.astype(F32)


def adamw_blocks(n) -> int:
    return max(1, min(GRID_CAP, (n // 4 + 255) // 256))


def emu_adamw_flat(p, g, m, v, h, coef=None, form="plain", mut=None, sentinel=0xDEAD):
    """adamw_kernel on a flat tensor -> (p', m', v' float32, image uint16 bits).  Vector i of n // 4 is handled by thread i % stride on
    trip i // stride (stride = blocks * 256), the n % 4 tail by the scalar path; elements a mutation leaves out keep their old
    values and the image's ``sentinel``."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    n = p.size
    pn, mn, vn = emu_update(p, g, m, v, h, coef, form, mut)
    img_src = p if mut == "image_pre_update" else pn
    img = (np.ascontiguousarray(img_src).view(np.uint32) >> 16).astype(np.uint16) if mut == "image_truncated" else bf16_bits(img_src)
    n4 = n // 4
    if mut == "lanes_rotated" and n4:
        rot = np.arange(n4 * 4).reshape(n4, 4)[:, [1, 2, 3, 0]].reshape(-1)
        pn, mn, vn, img = (np.concatenate([a[rot], a[n4 * 4:]]) for a in (pn, mn, vn, img))
    done = np.ones(n, bool)
    if skipped(coef) and mut != "neg_coef_abs":
        done[:] = False
    if mut == "tail_skipped":
        done[n4 * 4:] = False
    if mut == "trip_last_vector_skipped" and n4:
        stride = adamw_blocks(n) * 256
        last = sorted(set(list(range(stride - 1, n4, stride)) + [n4 - 1]))
        for i in last:
            done[i * 4:i * 4 + 4] = False
    out = [np.where(done, a, b) for a, b in ((pn, p), (mn, m), (vn, v))]
    return out[0], out[1], out[2], np.where(done, img, np.uint16(sentinel))


def emu_image_t(img_bits, rows, cols, ldt, mut=None, sentinel=0xDEAD):
    """The transposed image [cols][ldt] adamw_tile_t_kernel writes from the forward image bits [rows * cols] (TR x 64 tiles, TR = 128
    where rows % 128 == 0, else 64): imgt[c][r] = img[r][c], columns r >= rows untouched."""
    a = np.asarray(img_bits, np.uint16).reshape(rows, cols)
    out = np.full((cols, ldt), sentinel, np.uint16)
    if mut == "t_rc_swapped":                      # inside every 64 x 64 block the patch is read back as it was written
        b = a.reshape(rows // 64, 64, cols // 64, 64).transpose(2, 1, 0, 3)         # [cb, r, rb, c]: block (rb, cb) un-transposed
        out[:, :rows] = b.reshape(cols, rows)
    elif mut == "t_row_offset_dropped":
        tr = 128 if rows % 128 == 0 else 64
        for r0 in range(0, rows, tr):
            out[:, :tr] = a[r0:r0 + tr].T
    else:
        out[:, :rows] = a.T
    return out


def emu_lora_refresh(wa, wb, r, in_f, nj, A, At, B, Bt, col0, row0):
    """a3v_lora_refresh on uint16 bf16-bit images (modified in place): A[col0 + i][t], At[t][col0 + i] <- lora_a[i][t];
    B[row0 + t][col0 + i], Bt[col0 + i][row0 + t] <- lora_b[t][i]."""
    a, b = bf16_bits(wa).reshape(r, in_f), bf16_bits(wb).reshape(nj, r)
    A[col0:col0 + r, :in_f] = a
    At[:in_f, col0:col0 + r] = a.T
    B[row0:row0 + nj, col0:col0 + r] = b
    Bt[col0:col0 + r, row0:row0 + nj] = b.T


# ------------------------------------------------------------------------------------------------ sum of squares

def _slot_of(n):
    """Slot of every element of an n-element range."""
    i = np.arange(n, dtype=np.int64)
    slot = ((i // 4) // 256) % SLOTS
    slot[(n // 4) * 4:] = 0
    return slot


def sumsq_ref(x):
    """float64 per-slot sums [1024] under the kernel's ownership rule."""
    x = np.asarray(x, F32).astype(F64)
    return np.bincount(_slot_of(x.size), weights=x * x, minlength=SLOTS).astype(F64)


def sumsq_bound(x, ref=None):
    """Per-slot bound (L_max + 8) u slot (module docstring); a slot without data must be exactly 0."""
    n = np.asarray(x).size
    n4, rem = n // 4, n % 4
    trips = np.zeros(SLOTS, np.int64)
    full, part = divmod(n4, SLOTS * 256)
    trips += full
    nblk = (part + 255) // 256                      # slots that get one more (maybe partial) run of vectors
    trips[:nblk] += 1
    L = 4 * trips
    L[0] += 1 if rem else 0
    ref = sumsq_ref(x) if ref is None else ref
    return (L + 8) * U * ref * SECOND_ORDER


def sumsq_exact_input(n, seed=0):
    """Integers |x| <= 15 (a few zeros), float32: every partial sum is an integer below 2^24 for n <= 74 000 * 1024."""
    assert n <= 74000 * SLOTS
    i = np.arange(n, dtype=np.int64) + seed
    return ((((i * 2654435761 + 97) & 0x7FFFFFFF) >> 9) % 31 - 15).astype(F32)


def emu_sumsq(x, mut=None):
    """sumsq_partials_kernel in float32, operation for operation -> [1024] float32."""
    x = np.asarray(x, F32).astype(F64)
    n = x.size
    n4, rem = n // 4, n % 4
    per = SLOTS * 256
    trips = max(1, (n4 + per - 1) // per)
    body = np.zeros(trips * per * 4, F64)
    body[:n4 * 4] = x[:n4 * 4]
    body = body.reshape(trips, SLOTS, 256, 4)
    a = np.zeros((SLOTS, 256), F64)
    for t in range(trips):
        for e in range(4):
            a = _r(a + body[t, :, :, e] * body[t, :, :, e])         # fmaf: the product is exact in float64
    if rem and mut != "sumsq_tail_dropped":
        tail = x[n4 * 4:]
        a[0, :rem] = _r(a[0, :rem] + tail * tail)
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        a = _r(a + a[:, lanes ^ o])
    red = a[:, ::64]
    out = _r(_r(red[:, 0] + red[:, 1]) + _r(red[:, 2] + red[:, 3]))
    if mut == "sumsq_slot_to_neighbour":
        s = 0 if n4 <= 256 else 1                   # a slot that has data
        out[(s + 1) % SLOTS] = _r(out[(s + 1) % SLOTS] + out[s])
        out[s] = 0.0
    return out.astype(F32)
