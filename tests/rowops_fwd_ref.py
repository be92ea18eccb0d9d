"""fp64 references, derived error bounds and input generators for the forward row kernels of a3vlm_amd/csrc/a3v_rowops.hip
(RMSNorm, LayerNorm, RoPE + KV-cache write, V^T pack, embedding / ViT assembly, patch im2col, view split, argmax, cross entropy,
generation step).  The scheme is that of tests/rowops_ref.py (whose ``within``, HALF_ULP_BF16, EVAL_F32 and TINY are used here):
every reference is closed-form fp64 math on exactly the bf16 / fp32 values the kernel is given and returns ``(ref, mag)``, ``mag`` =
the summed |terms| of the element.  The bound of an element is

    sum over the roundings to bf16 that the kernel's SPECIFIED semantic contains of HALF_ULP_BF16 |ref|   +   EVAL_F32 mag   +   TINY

n roundings compound: a value p rounded n times in a row is p (1 + d_1) .. (1 + d_n) with |d_i| <= 2^-8, so the relative term is
``rel_roundings(n)`` = (1 + 2^-8)^n - 1 (2^-8, 2^-7 + 2^-16, ..).  Where the specified result is a copy or ONE correctly rounded
operation the check is bit equality against torch on the CPU and no bound exists.

RMSNorm (a3vlm_hip.h: "fp32 normalise -> cast to x's dtype -> multiply by weight"): y = rnd_y(rnd_x(x r) w), r = rsqrt(mean(x^2) + eps).
  A bf16 x gives the rounding of x r, a bf16 y the rounding of the product: 2 terms for keys 0 and 2 (bf16 x, bf16 y), 1 for keys 4 and
  6 (fp32 x, bf16 y), none for key 7.  The element is one product (mag = |ref|); the sum under r has only positive terms, so its fp32
  error is relative and inside EVAL_F32 |ref|.  A zero row gives exact zeros.
  A bound against fp64 cannot see a MISSING intermediate rounding (one rounding is closer to fp64 than two), so for a bf16 x the
  order of the roundings is pinned by bits (``rmsnorm_exact``): where the fp64 value of x r lies further than EVAL_F32 |x r| from
  every midpoint of two neighbouring bf16 numbers, no admissible fp32 error of r can move its rounding, t = bf16(x r) is decided,
  and y = rnd_y(fl32(t w)) follows exactly (t w is one correctly rounded fp32 product).  Those elements -- all but ~2^-10 of them --
  must be bit-equal.
LayerNorm (torch.nn.LayerNorm): y = rnd_y((x - mean) rstd w + b), one rounding for a bf16 y.  The kernel centres before it squares, so the
  variance carries no E[x^2] - mean^2 cancellation; what is left is the fp32 error of mean -- a sum of dim terms, so relative to its
  summed |terms| mean(|x|), not to |mean| (on a centred row mean is ~0 and its error is not) -- and of the subtraction: the centred
  value is good to EVAL_F32 (|x| + mean(|x|)), hence mag = (|x| + mean(|x|)) rstd |w| + |b|.  On a row 64 standard deviations off
  zero this is 2^-13 of |w|: the honest cost of fp32 there, and far below what a variance formed from E[x^2] would lose.
RoPE (out0 = a cos - b sin, out1 = a sin + b cos on the pair (a, b), table row rope_pos0 + s): one rounding to the cache dtype,
  mag = |a cos| + |b sin| resp. |a sin| + |b cos|.  The V^T cache is a copy.
vit_embed: x = rnd(cls|patch + pos): ONE fp32 addition of two values (exact in fp32 for bf16 operands up to a final fp32 rounding, the
  same one torch's bf16 addition makes), rounded once: bit equality with (a.float() + p.float()).to(dtype).
Bicubic global view (split_views, view 0): r = (T)fp16(sum_dy sum_dx wt[dy] wt[dx] fp16(px)), wt = {-3/32, 19/32, 19/32, -3/32}, border
  indices clamped.  The kernel's own result rounding is to fp16: half an fp16 ulp = 2^-11 |ref| (compounded with 2^-8 for a bf16 out),
  plus EVAL_F32 mag, mag = sum |wt wt px|, plus half the fp16 subnormal spacing 2^-25.  The four quadrant views are copies.
Cross entropy (row_loss = lse - x_lab, dlogits = g (softmax - onehot), g = grad_scale / n_valid; fast __expf / __logf):
  with d_i = max - x_i >= 0, s = sum exp(-d_i).  The argument of each exponential carries an fp32 error relative to d_i, so term i
  of s is off by (a few ulps) d_i e^-d_i <= 1/e of an ulp of the LARGEST term (which is 1): s is good to a few fp32 ulps relative,
  log s to a few ulps absolute plus its own rounding, and the additions max + log s - x_lab to ulps of their operands:
      |row_loss - ref| <= EVAL_F32 (|max| + |log s| + |x_lab| + 1).
  p_i = exp(x_i - lse) inherits the absolute error of lse (EVAL_F32 (|max| + |log s| + 1) at most) and the argument error of its
  own exponential (relative to |x_i - lse|), both as RELATIVE errors of p_i; the label column subtracts 1 (an absolute ulp of 1):
      |dlogits_i - ref_i| <= [bf16: HALF_ULP_BF16 |ref_i|] + EVAL_F32 g (p_i (1 + |x_i - lse| + |max| + |log s|) + [i == lab]).
  Below 2^-126 an fp32 exponential is flushed: g 2^-126 absolute is added through ``underflow`` (as for SwiGLU in rowops_ref).
  A label outside (0, V) -- ignore_index 0, negative, >= V -- gives zero loss and an all-zero gradient row, exactly.
generate_step: integer bookkeeping; ``generate_step_ref`` transcribes the loop body of oracle/ref_cpu.py generate_greedy per row and
  adds the ``live`` counter; every comparison is equality.
"""
from __future__ import annotations

import torch

from rowops_ref import EVAL_F32, HALF_ULP_BF16, TINY, within, _randn  # noqa: F401  (re-exported for the two test files)

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
HALF_ULP_F16 = 2.0 ** -11
F16_HALF_SUBNORMAL = 2.0 ** -25
F32_MIN_NORMAL = 2.0 ** -126
SENT = -7.0


def rel_roundings(n_bf16: int, extra: float = 0.0) -> float:
    """relative bound of n successive roundings to bf16 (and one more of relative size ``extra``)"""
    return (1.0 + HALF_ULP_BF16) ** n_bf16 * (1.0 + extra) - 1.0


# ------------------------------------------------------------------ RMSNorm
RMS_EPS = 1e-5
RMS_KEYS = {0: (BF, BF, BF), 2: (BF, F32, BF), 4: (F32, BF, BF), 6: (F32, F32, BF), 7: (F32, F32, F32)}     # key -> (x, w, y) dtypes
RMS_DIMS = [8, 136, 2048, 2056, 4096, 5120, 8192]
RMS_ROWS = [1, 3, 37]
RMS_BAD_DIMS = [4, 12, 8200]
RMS_IDX_CASES = [(9, 136, [8, 8, 3, 2, 2, 0]), (40, 4096, [39, 17, 17, 16, 5, 5, 5, 0]), (5, 8192, [4, 4, 1])]   # (src rows, dim, row_idx)


def rmsnorm_inputs(rows, dim, xd, wd):
    """row 1 is zero, row 2 scaled by 2^10, row 3 by 2^-10 (as far as there are rows)"""
    s = 11000 * rows + dim
    x = 2.0 * _randn(rows, dim, seed=s + 1)
    if rows > 1:
        x[1] = 0.0
    if rows > 2:
        x[2] *= 2.0 ** 10
    if rows > 3:
        x[3] *= 2.0 ** -10
    return dict(x=x.to(xd), w=(1.0 + 0.1 * _randn(dim, seed=s + 2)).to(wd))


def rmsnorm_rel(xd, yd):
    return rel_roundings(int(xd == BF) + int(yd == BF))


def rmsnorm_ref(x, w, eps=RMS_EPS):
    x, w = x.to(F64), w.to(F64)
    ref = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w
    return ref, ref.abs()


def rmsnorm_exact(x, w, yd, eps=RMS_EPS):
    """bf16 x -> (y, decided): the bits the specified rounding order gives, and the elements where they do not depend on the fp32
    error of r (x r further than EVAL_F32 |x r| from the nearest bf16 rounding boundary)"""
    assert x.dtype == BF
    x64 = x.to(F64)
    p = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + eps)
    t = p.to(BF)
    _, e = torch.frexp(p)                                       # |p| in [2^(e-1), 2^e): bf16 spacing 2^(e-8)
    half_ulp = torch.ldexp(torch.ones_like(p), e - 9)
    decided = (p == 0) | (half_ulp - (p - t.to(F64)).abs() > EVAL_F32 * p.abs())
    return (t.float() * w.float()).to(yd), decided


def emu_rmsnorm(x, w, yd, eps=RMS_EPS):
    xf = x.float()
    inv = torch.rsqrt((xf * xf).sum(-1, keepdim=True) / x.shape[1] + eps)
    return ((xf * inv).to(x.dtype).float() * w.float()).to(yd)


# ------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
LN_KEYS = {0: (BF, BF, BF), 2: (BF, F32, BF), 3: (BF, F32, F32), 7: (F32, F32, F32)}          # key -> (x, w / b, y) dtypes
LN_DIMS = [8, 1024, 1032, 1664, 5120, 8192]
LN_OFFSETS = [0.0, 8.0, 64.0]
LN_ROWS = 6


def layernorm_inputs(rows, dim, offset_sd, xd, pd):
    """x has rows + 2 rows (the entry point is told ``rows``); row_map: a permutation prefix into 2 * rows destination rows"""
    s = 12000 + 10 * dim + int(offset_sd)
    x = 1.5 * _randn(rows + 2, dim, seed=s + 1)
    x = x - x.mean(-1, keepdim=True)
    if offset_sd:
        sign = torch.where(torch.arange(rows + 2) % 2 == 0, 1.0, -1.0)[:, None]
        x = x + sign * offset_sd * x.std(-1, keepdim=True)
    row_map = torch.randperm(2 * rows, generator=torch.Generator().manual_seed(s + 2))[:rows].to(torch.int32)
    return dict(x=x.to(xd), w=(1.0 + 0.1 * _randn(dim, seed=s + 3)).to(pd), b=(0.1 * _randn(dim, seed=s + 4)).to(pd), row_map=row_map)


def layernorm_ref(x, w, b, eps=LN_EPS):
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (x - mean) * rstd * w + b, (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd * w.abs() + b.abs()


def emu_layernorm(x, w, b, yd, eps=LN_EPS):
    xf = x.float()
    dim = x.shape[1]
    d = xf - xf.sum(-1, keepdim=True) / dim
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / dim + eps)
    return (d * rstd * w.float() + b.float()).to(yd)


# ------------------------------------------------------------------ RoPE + KV-cache write
ROPE_B, ROPE_H, ROPE_HKV = 2, 4, 2
ROPE_S = [1, 4, 5, 64, 65, 130]               # <= 4: the decode kernel; else the 64-token tile kernel (one tile, its edge, two tiles + 2)
ROPE_HD = [64, 128]
ROPE_POS = [(0, 0), (3, 3), (8, 0), (5, 40), (64, 7)]          # (start_pos, rope_pos0)
ROPE_SMAX = [256, 100]                        # 100 % 8 != 0: the scalar V^T path
ROPE_TABLE = 256


def rope_cases(S):
    """every (start_pos, rope_pos0, Smax) that fits the cache"""
    return [(sp, rp, Smax) for Smax in ROPE_SMAX for sp, rp in ROPE_POS if sp + S <= Smax]


def rope_inputs(S, hd, dtype):
    return _randn(ROPE_B * S, (ROPE_H + 2 * ROPE_HKV) * hd, seed=13000 + 10 * S + hd).to(dtype)


def rope_ref(qkv, cos_sin, S, hd, rope_pos0):
    """-> (qk [B, S, H + Hkv, hd] fp64, mag, v [B, S, Hkv, hd] in the input dtype)"""
    B, H, Hkv = ROPE_B, ROPE_H, ROPE_HKV
    t = qkv.view(B, S, H + 2 * Hkv, hd)
    qk = t[:, :, :H + Hkv].to(F64)
    a, b = qk[..., 0::2], qk[..., 1::2]
    cs = cos_sin[rope_pos0:rope_pos0 + S].to(F64)
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    ref = torch.stack([a * co - b * si, a * si + b * co], dim=-1).reshape(B, S, H + Hkv, hd)
    mag = torch.stack([(a * co).abs() + (b * si).abs(), (a * si).abs() + (b * co).abs()], dim=-1).reshape(B, S, H + Hkv, hd)
    return ref, mag, t[:, :, H + Hkv:]


def emu_rope(qkv, cos_sin, S, hd, rope_pos0):
    B, H, Hkv = ROPE_B, ROPE_H, ROPE_HKV
    qk = qkv.view(B, S, H + 2 * Hkv, hd)[:, :, :H + Hkv].float()
    a, b = qk[..., 0::2], qk[..., 1::2]
    cs = cos_sin[rope_pos0:rope_pos0 + S]
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    return torch.stack([a * co - b * si, a * si + b * co], dim=-1).reshape(B, S, H + Hkv, hd).to(qkv.dtype)


# ------------------------------------------------------------------ V^T pack
VT_N, VT_H = 2, 2
VT_HD = [64, 80, 128]
VT_L = [(64, 64), (65, 72), (77, 128), (257, 320), (257, 264), (50, 192)]         # (L, Lpad); 257 = the ViT's 16 x 16 patches + cls


def vt_pack_inputs(L, hd, dtype):
    """the packed in_proj output [N * L, 3 * H * hd]; v is its last third"""
    return _randn(VT_N * L, 3 * VT_H * hd, seed=14000 + 10 * L + hd).to(dtype)


def vt_pack_ref(qkv, L, hd, Lpad):
    W = VT_H * hd
    out = torch.zeros(VT_N, VT_H, hd, Lpad, dtype=qkv.dtype)
    out[..., :L] = qkv[:, 2 * W:].reshape(VT_N, L, VT_H, hd).permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------ embedding / ViT assembly
EMBED_B, EMBED_T, EMBED_V = 2, 5, 11
EMBED_DIMS = [8, 4096, 5120]
EMBED_W = [0, 7]
DTYPE_PAIRS = [(BF, BF), (BF, F32), (F32, BF), (F32, F32)]
FILL_DIM, FILL_ROWS, FILL_IDX = 5120, 16, [1, 4, 13]
VIT_WIDTHS = [64, 1024, 1664]
VIT_T = [16, 256]
VIT_N = 2


def embed_inputs(dim, table_dtype):
    """tokens [B, T] with -1 and V among them (clamped to rows 0 and V - 1)"""
    tok = torch.randint(0, EMBED_V, (EMBED_B, EMBED_T), generator=torch.Generator().manual_seed(15000 + dim))
    tok[0, 1] = -1
    tok[1, 3] = EMBED_V
    tok[1, 0] = EMBED_V - 1
    return dict(tokens=tok, table=_randn(EMBED_V, dim, seed=15001 + dim).to(table_dtype))


def embed_ref(tokens, table, W, h_dtype):
    """-> h [B, T + W, dim] in h_dtype with SENT in the image-word rows 1 .. W"""
    B, T = tokens.shape
    h = torch.full((B, T + W, table.shape[1]), SENT, dtype=h_dtype)
    rows = table[tokens.clamp(0, table.shape[0] - 1)].to(h_dtype)
    h[:, 0] = rows[:, 0]
    h[:, W + 1:] = rows[:, 1:]
    return h


def vit_embed_inputs(T, width, dtype):
    s = 16000 + 10 * T + width
    return dict(patch=_randn(VIT_N * T, width, seed=s).to(dtype), cls=_randn(width, seed=s + 1).to(dtype), pos=_randn(T + 1, width, seed=s + 2).to(dtype))


def vit_embed_ref(patch, cls, pos, T):
    width = patch.shape[1]
    a = torch.cat([cls.float().expand(VIT_N, 1, width), patch.float().view(VIT_N, T, width)], dim=1)
    return (a + pos.float()).to(patch.dtype)


# ------------------------------------------------------------------ patch im2col
IM2COL_KEYS = {0: (BF, BF), 2: (F32, BF), 3: (F32, F32)}
IM2COL_P = [14, 16]
IM2COL_GRIDS = [(2, 5), (16, 16)]             # (gh, g) patches
IM2COL_N = 2


def im2col_kpads(P):
    K = 3 * P * P
    return sorted({K, (K + 63) // 64 * 64, (K + 64) // 64 * 64})          # no pad; up to a multiple of 64; a pad in every case


def im2col_inputs(P, gh, g, in_dtype):
    return _randn(IM2COL_N, 3, gh * P, g * P, seed=17000 + 100 * P + 10 * gh + g).to(in_dtype)


def im2col_ref(img, P, Kpad, out_dtype):
    """row n gh g + gy g + gx, column c P P + py P + px; zeros in K .. Kpad"""
    N, _, Hi, Wi = img.shape
    gh, g = Hi // P, Wi // P
    out = torch.zeros(N * gh * g, Kpad, dtype=out_dtype)
    out[:, :3 * P * P] = img.view(N, 3, gh, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * g, 3 * P * P).to(out_dtype)
    return out


# ------------------------------------------------------------------ view split
SPLIT_KEYS = {0: (BF, BF), 2: (F32, BF), 3: (F32, F32)}
SPLIT_SHAPES = [(2, 7), (2, 28), (3, 224)]        # (B, c); the last: 5 * 3 * 3 * 224^2 > 8192 * 256 elements, the grid-stride loop runs
BICUBIC_WT = (-0.09375, 0.59375, 0.59375, -0.09375)


def split_inputs(B, c, in_dtype):
    return _randn(B, 3, 2 * c, 2 * c, seed=18000 + c).to(in_dtype)


def split_quadrants_ref(img, out_dtype):
    c = img.shape[-1] // 2
    return torch.cat([img[..., :c, :c], img[..., :c, c:], img[..., c:, :c], img[..., c:, c:]], dim=0).to(out_dtype)


def _bicubic_taps(img, dtype):
    """[4 (dy), 4 (dx), B, 3, c, c]: the fp16-rounded pixel under every tap, border-clamped"""
    S2 = img.shape[-1]
    c = S2 // 2
    px = img.half().to(dtype)
    base = 2 * torch.arange(c) - 1
    taps = []
    for dy in range(4):
        yy = (base + dy).clamp(0, S2 - 1)
        taps.append(torch.stack([px[..., yy, :][..., (base + dx).clamp(0, S2 - 1)] for dx in range(4)]))
    return torch.stack(taps)


def bicubic_ref(img):
    t = _bicubic_taps(img, F64)
    wt = torch.tensor(BICUBIC_WT, dtype=F64)
    w2 = (wt[:, None] * wt[None, :])[:, :, None, None, None, None]
    return (w2 * t).sum((0, 1)), (w2 * t).abs().sum((0, 1))


def bicubic_rel(out_dtype):
    return rel_roundings(int(out_dtype == BF), HALF_ULP_F16)


def bicubic_within(got, img, out_dtype):
    ref, mag = bicubic_ref(img)
    sub = torch.full_like(ref, F16_HALF_SUBNORMAL / F32_MIN_NORMAL)        # 2^-25 absolute, through within's 2^-126-scaled argument
    return within(got, ref, mag, out_dtype, rel=bicubic_rel(out_dtype), underflow=sub)


def emu_bicubic(img, out_dtype):
    t = _bicubic_taps(img, F32)
    wt = torch.tensor(BICUBIC_WT, dtype=F32)
    acc = torch.zeros_like(t[0, 0])
    for dy in range(4):
        row = torch.zeros_like(acc)
        for dx in range(4):
            row = row + wt[dx] * t[dy, dx]
        acc = acc + wt[dy] * row
    return acc.half().to(out_dtype)


# ------------------------------------------------------------------ argmax
ARGMAX_V = [1, 3, 5, 1023, 4096, 4100, 16385, 32000, 32003]


def argmax_inputs(V):
    """fp32 [R, V] and the expected ids (the lowest index of the maximum; 0 for a row of -inf).  Rows: the maximum at index 0, at V - 1,
    at the first index of the scalar tail (V // 4 * 4; V - 1 when there is none), inside the last full 4-vector; a two-way tie;
    an all-negative row; an all -inf row."""
    tail0 = V // 4 * 4 if V % 4 else V - 1
    last_vec = max(V // 4 * 4 - 2, 0)
    spots = [0, V - 1, tail0, last_vec]
    lg = _randn(len(spots) + 3, V, seed=19000 + V)
    for r, i in enumerate(spots):
        lg[r, i] = 50.0
    r = len(spots)
    lg[r, V // 3] = lg[r, V - 1] = 50.0                              # tie -> the lower index
    lg[r + 1] = -1.0 - lg[r + 1].abs()                               # all negative
    lg[r + 2] = float("-inf")
    want = torch.tensor([int((row == row.max()).nonzero()[0]) for row in lg])
    assert want[:len(spots)].tolist() == spots and int(want[r]) == V // 3 and int(want[r + 2]) == 0
    return lg, want


# ------------------------------------------------------------------ cross entropy
CE_SHAPES = [(7, 8), (5, 255), (5, 257), (9, 4100), (23, 32000), (3, 32003)]
CE_SCALES = [1.0, 0.25, 1.0 / 3.0]
CE_BAD_LABELS = [-100, -1, 0, None, None]                # None: V and V + 5 (filled in by ce_bad_label_inputs)


def ce_inputs(rows, V, dtype):
    """row 0: one logit 60 above the rest; row 1: flat; labels 1 and V - 1 in rows 0 and 1; row 2 ignored (label 0)"""
    s = 20000 + 10 * rows + V
    lg = 3.0 * _randn(rows, V, seed=s)
    lg[0, V // 2] = lg[0].max() + 60.0
    lg[1] = 1.5
    lab = torch.randint(1, V, (rows,), generator=torch.Generator().manual_seed(s + 1))
    lab[0], lab[1], lab[2] = 1, V - 1, 0
    if rows > 5:
        lab[5] = V // 2 if V // 2 > 0 else 1
    return dict(logits=lg.to(dtype), labels=lab)


def ce_bad_label_inputs(rows, V, dtype):
    """labels -100, -1, 0, V, V + 5 (zero loss, zero gradient, nothing read), then valid rows"""
    d = ce_inputs(rows, V, dtype)
    bad = [V if b is None else b for b in CE_BAD_LABELS]
    bad[4] = V + 5
    d["labels"][:5] = torch.tensor(bad)
    return d


def ce_one_valid_inputs(rows, V, dtype):
    d = ce_inputs(rows, V, dtype)
    d["labels"][:] = 0
    d["labels"][rows - 1] = V - 1
    return d


def ce_n_valid(labels):
    return int((labels != 0).sum())


def ce_ref(logits, labels, grad_scale, n_valid):
    """-> (row_loss, mag_loss, dlogits, mag_d, underflow sensitivity); g = fp32(grad_scale) / n_valid"""
    x = logits.to(F64)
    rows, V = x.shape
    valid = (labels > 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    mx = x.max(-1, keepdim=True).values
    logs = torch.log(torch.exp(x - mx).sum(-1, keepdim=True))
    lse = mx + logs
    xl = x.gather(1, lab[:, None])
    onehot = torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    g = float(torch.tensor(grad_scale, dtype=F32)) / max(n_valid, 1)
    p = torch.exp(x - lse)
    v = valid[:, None].to(F64)
    loss = ((lse - xl) * v).squeeze(1)
    mag_loss = ((mx.abs() + logs.abs() + xl.abs() + 1.0) * v).squeeze(1)
    d = g * (p - onehot) * v
    mag_d = g * (p * (1.0 + (x - lse).abs() + mx.abs() + logs.abs()) + onehot) * v
    return loss, mag_loss, d, mag_d, torch.full_like(x, g) * v


def emu_ce(logits, labels, grad_scale, n_valid):
    x = logits.float()
    rows, V = x.shape
    valid = (labels > 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    mx = x.max(-1, keepdim=True).values
    lse = mx + torch.log(torch.exp(x - mx).sum(-1, keepdim=True))
    loss = torch.where(valid, (lse - x.gather(1, lab[:, None])).squeeze(1), torch.zeros(rows))
    g = torch.tensor(grad_scale, dtype=F32) / torch.tensor(float(max(n_valid, 1)), dtype=F32)
    pr = torch.exp(x - lse) - torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    return loss, torch.where(valid[:, None], pr * g, torch.zeros_like(x)).to(logits.dtype)


# ------------------------------------------------------------------ generation step
GEN_V = 37
GEN_STEPS = 10
GEN_STOPS = [[2], [5, 6, 7], [6, 7], [9] * 12]        # EOS; two that can match at the same step; one longer than the sequence for 9 steps
GEN_PROMPTS = [[1, 3], [1, 8, 6, 7, 4, 4], [1, 5, 6], [1, 3], [1, 3, 3], [1, 6]]
# the id the logits favour at cur_pos = 2 .. 11 (ignored where the prompt is still running):
GEN_SCRIPT = [
    [4, 5, 6, 7, 3, 3, 3, 3, 3, 3],     # [5, 6, 7] and [6, 7] both match at cur 5: the FIRST in the list wins, stop_pos 3 (not 4)
    [2, 2, 2, 2, 4, 4, 2, 6, 7, 3],     # forced through cur 5: its prompt's 7 at cur 3 completes [6, 7] and the scripted EOS is overridden -- no stop; EOS at cur 8
    [2, 7, 3, 3, 3, 3, 3, 3, 3, 3],     # forced 6 at cur 2, then 7: [5, 6, 7] begins inside the prompt, stop_pos 1
    [9, 9, 9, 9, 9, 9, 9, 9, 9, 9],     # never stops; [9] * 12 becomes comparable at the last step only and does not match
    [2, 2, 6, 7, 2, 3, 3, 3, 3, 3],     # forced at cur 2, EOS at cur 3; [6, 7] and EOS after that must not move stop_pos
    [7, 3, 3, 2, 3, 3, 3, 3, 3, 3],     # [6, 7] spans the prompt's 6 and the first generated token: stop_pos 1
]
GEN_START = min(len(p) for p in GEN_PROMPTS)
GEN_TOTAL = GEN_START + GEN_STEPS


def gen_initial_state():
    """python-list state of MetaModel.generate before its loop"""
    B = len(GEN_PROMPTS)
    tokens = [[0] * GEN_TOTAL for _ in range(B)]
    mask = [[False] * GEN_TOTAL for _ in range(B)]
    for r, p in enumerate(GEN_PROMPTS):
        tokens[r][:len(p)] = p
        mask[r][:len(p)] = [True] * len(p)
    return dict(tokens=tokens, text_mask=mask, stopped=[False] * B, stop_pos=[GEN_START + 1] * B, live=B)


def gen_logits_table():
    """fp32 [GEN_TOTAL, B, V]: row cur_pos favours GEN_SCRIPT[b][cur_pos - GEN_START]"""
    B = len(GEN_PROMPTS)
    t = _randn(GEN_TOTAL, B, GEN_V, seed=21000)
    for b in range(B):
        for k in range(GEN_STEPS):
            t[GEN_START + k, b, GEN_SCRIPT[b][k]] = 10.0
    return t


def generate_step_ref(state, next_ids, cur, stops):
    """One step of oracle/ref_cpu.py generate_greedy's loop body on ``state`` (in place), row by row: the torch.where forcing, the
    token write, the stop_pos default, the ordered stop loop with c1 * c2 * ~stopped; ``live`` drops once when a row stops."""
    tokens, mask, stopped, stop_pos = state["tokens"], state["text_mask"], state["stopped"], state["stop_pos"]
    for r in range(len(tokens)):
        nxt = tokens[r][cur] if mask[r][cur] else int(next_ids[r])
        tokens[r][cur] = nxt
        if not stopped[r]:
            stop_pos[r] = cur + 1
        for st in stops:
            if cur + 1 - len(st) >= 0:
                c1 = tokens[r][cur + 1 - len(st):cur + 1] == list(st)
                c2 = not mask[r][cur]
                new = c1 and c2 and not stopped[r]
                if new:
                    stop_pos[r] = cur + 1 - len(st)
                    state["live"] -= 1
                stopped[r] = new or stopped[r]
    return state
