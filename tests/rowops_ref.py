"""fp64 references, derived error bounds and input generators for the row-op backward kernels of
a3vlm_amd/csrc/a3v_train.hip (RMSNorm / LayerNorm / SwiGLU / RoPE backward, embedding scatter, row sums).

Every reference is closed-form fp64 math on exactly the bf16 / fp32 values the kernel is given (tests/test_rowops_ref_cpu.py
checks each against torch fp64 autograd), and returns, next to the result, the per-element magnitude ``mag``: the sum of the
absolute values of the terms that are added to form the element.  ``within`` turns (ref, mag) into the bound

    bf16 output of fp32 arithmetic        |got - ref| <= 2^-8 |ref| + 2^-20 mag      (half a bf16 ulp + fp32 evaluation error)
    fp32 output (sums in no fixed order)  |got - ref| <= 2^-20 mag

``mag`` is not |ref|: where the terms cancel the bound stays as tight as the terms allow.  Two additions cover what the number
formats cannot represent at all (they are far below every bound above at ordinary magnitudes):
  * half the subnormal spacing of the output format (2^-134 bf16, 2^-150 fp32);
  * ``underflow``: for SwiGLU, sigmoid(g) of fp32 arithmetic is only good to 2^-126 absolute (exp(-g) overflows for g < -88.7 and
    the sigmoid becomes 0 where fp64 has 1e-39), so the result may be off by 2^-126 times its sensitivity to the sigmoid.

The ``emu_*`` functions are fp32 torch restatements of each kernel's formula rounded to the output dtype: a correct fp32
implementation.  The CPU test shows they stay inside the bounds for every input set the GPU test uses, so that a GPU failure
means the kernel is wrong and not the bound.  The ``*_inputs`` generators are shared by both test files.
"""
from __future__ import annotations

from typing import Optional

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

HALF_ULP_BF16 = 2.0 ** -8           # half a bf16 ulp relative to the value, at worst
EVAL_F32 = 2.0 ** -20               # fp32 evaluation error relative to the sum of |terms|
TINY = {BF: 2.0 ** -134, F32: 2.0 ** -150}      # half the subnormal spacing
F32_MIN_NORMAL = 2.0 ** -126
SWIGLU_FWD_REL = 2.0 ** -7 + 2.0 ** -15         # silu(g) rounded to bf16, then the product rounded to bf16


def within(got, ref, mag, out_dtype, rel: Optional[float] = None, underflow=None) -> float:
    """Worst |got - ref| / bound over all elements (<= 1 passes; inf for a NaN / inf or a shape mismatch).

    ``rel`` replaces the relative term of the output rounding (default: half a bf16 ulp for a bf16 output, none for fp32);
    ``mag`` may be None (no sum is evaluated); ``underflow`` is the sensitivity described in the module docstring."""
    got = got.detach().cpu().to(F64)
    ref = ref.to(F64)
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return float("inf")
    if rel is None:
        rel = HALF_ULP_BF16 if out_dtype == BF else 0.0
    bound = rel * ref.abs() + TINY[out_dtype]
    if mag is not None:
        bound = bound + EVAL_F32 * mag.to(F64)
    if underflow is not None:
        bound = bound + F32_MIN_NORMAL * underflow.to(F64)
    return float(((got - ref).abs() / bound).max())


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ RMSNorm backward
RMS_EPS = 1e-5
RMS_SHAPES = [(45, 512), (1, 4096), (17, 4096), (9, 4100), (19, 5120), (11, 8192), (8, 1028), (33, 130)]
RMS_SHAPES_F32_STREAM = [(9, 4100), (11, 8192)]


def rmsnorm_bwd_inputs(rows, dim, stream_dtype=BF):
    """x, dh0 in the stream dtype, dy bf16, w / dw0 fp32.  The last row (the ragged row of its 8-row block) has x30 outliers
    in every 7th column of x, row rows//2 has dy scaled by 1e-3, row rows//3 starts from dh0 = 0."""
    s = 1000 * rows + dim
    x = 2.0 * _randn(rows, dim, seed=s + 1)
    x[rows - 1, ::7] *= 30.0
    dy = _randn(rows, dim, seed=s + 2)
    dy[rows // 2] *= 1e-3
    dh0 = _randn(rows, dim, seed=s + 3)
    dh0[rows // 3] = 0.0
    return dict(x=x.to(stream_dtype), w=1.0 + 0.1 * _randn(dim, seed=s + 4), dy=dy.to(BF), dh0=dh0.to(stream_dtype),
                dw0=_randn(dim, seed=s + 5))


def rmsnorm_fwd64(x, w, eps):
    return w * x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)


def rmsnorm_bwd_ref(x, w, dy, dh0, dw0, eps=RMS_EPS):
    """-> (dh, mag_dh, dw, mag_dw): dh = dh0 + r dy w - x r^3 sum(dy w x) / dim,  dw = dw0 + sum_rows dy x r"""
    x, w, dy, dh0, dw0 = (t.to(F64) for t in (x, w, dy, dh0, dw0))
    dim = x.shape[1]
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    g = dy * w
    dh = dh0 + r * g - x * r ** 3 * (g * x).sum(-1, keepdim=True) / dim
    mag_dh = dh0.abs() + (r * g).abs() + x.abs() * r ** 3 * (g * x).abs().sum(-1, keepdim=True) / dim
    t = dy * x * r
    return dh, mag_dh, dw0 + t.sum(0), dw0.abs() + t.abs().sum(0)


def emu_rmsnorm_bwd(x, w, dy, dh0, dw0, eps=RMS_EPS):
    """fp32 restatement of the kernel -> (dh in the stream dtype, dw fp32)"""
    xf, dyf = x.float(), dy.float()
    dim = x.shape[1]
    r = torch.rsqrt((xf * xf).sum(-1, keepdim=True) / dim + eps)
    k2 = r * r * r * (dyf * w * xf).sum(-1, keepdim=True) / dim
    dh = (dh0.float() + (r * dyf * w - xf * k2)).to(dh0.dtype)
    return dh, dw0 + (dyf * xf * r).sum(0)


# ------------------------------------------------------------------ LayerNorm backward
LN_EPS = 1e-5
LN_SHAPES = [(37, 4096), (5, 5120), (18, 130), (17, 8192)]
LN_OFFSETS = [0.0, 8.0]             # row offset in standard deviations


def layernorm_bwd_inputs(rows, dim, offset_sd):
    """bf16 x / dy, fp32 w / dw0 / db0, and the int32 row_map (a permutation prefix) into a dy buffer of 2 * rows rows.
    offset_sd = 0: rows re-centred to zero mean before the bf16 rounding; else every row carries +-offset_sd standard deviations."""
    s = 2000 * rows + dim + int(offset_sd)
    x = 1.5 * _randn(rows, dim, seed=s + 1)
    x = x - x.mean(-1, keepdim=True)
    if offset_sd:
        sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
        x = x + sign * offset_sd * x.std(-1, keepdim=True)
    row_map = torch.randperm(2 * rows, generator=torch.Generator().manual_seed(s + 2))[:rows].to(torch.int32)
    dy_big = _randn(2 * rows, dim, seed=s + 3).to(BF)
    return dict(x=x.to(BF), w=1.0 + 0.1 * _randn(dim, seed=s + 4), dy_big=dy_big, row_map=row_map,
                dw0=_randn(dim, seed=s + 5), db0=_randn(dim, seed=s + 6))


def layernorm_bwd_ref(x, w, dy, dw0, db0, eps=LN_EPS):
    """dy: the gathered rows.  -> (dx, mag_dx, dw, mag_dw, db, mag_db).  kappa = E[x^2] / (var + eps) per row is the
    amplification of the fp32 error of a variance formed as E[x^2] - mean^2."""
    x, w, dy, dw0, db0 = (t.to(F64) for t in (x, w, dy, dw0, db0))
    dim = x.shape[1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    kappa = (x * x).mean(-1, keepdim=True) / (var + eps)
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    mag_dx = kappa * rstd * (g.abs() + g.abs().sum(-1, keepdim=True) / dim + xh.abs() * (g * xh).abs().sum(-1, keepdim=True) / dim)
    dw = dw0 + (dy * xh).sum(0)
    mag_dw = dw0.abs() + kappa.max() * (dy * xh).abs().sum(0)
    return dx, mag_dx, dw, mag_dw, db0 + dy.sum(0), db0.abs() + dy.abs().sum(0)


def emu_layernorm_bwd(x, w, dy, dw0, db0, eps=LN_EPS):
    """fp32 restatement of the kernel (variance as E[x^2] - mean^2) -> (dx bf16, dw, db)"""
    xf, dyf = x.float(), dy.float()
    dim = x.shape[1]
    mean = xf.sum(-1, keepdim=True) / dim
    rstd = torch.rsqrt(torch.clamp((xf * xf).sum(-1, keepdim=True) / dim - mean * mean, min=0.0) + eps)
    xh = (xf - mean) * rstd
    g = dyf * w
    a1, a2 = g.sum(-1, keepdim=True) / dim, (g * xh).sum(-1, keepdim=True) / dim
    return (rstd * (g - a1 - xh * a2)).to(x.dtype), dw0 + (dyf * xh).sum(0), db0 + dyf.sum(0)


# ------------------------------------------------------------------ embedding backward, row sums
EMBED_SHAPES = [(2, 5, 3, 320, 30), (1, 4, 0, 64, 7)]          # (B, T, W, dim, V)


def embed_bwd_inputs(B, T, W, dim, V):
    """tokens with a repeat, one below 0 and one >= V (the kernel clamps both); bf16 dh over [BOS | W image words | text]"""
    s = 3000 + 10 * dim + V
    tok = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(s))
    tok[0, 2] = tok[0, 0]
    tok[0, 1] = -2
    tok[B - 1, T - 1] = V + 2
    return dict(tokens=tok, dh=_randn(B * (T + W), dim, seed=s + 1).to(BF), dtable0=_randn(V, dim, seed=s + 2))


def embed_text_rows(B, T, W):
    """row of dh that token (b, t) owns: position 0 (BOS) or W + t"""
    b, t = torch.meshgrid(torch.arange(B), torch.arange(T), indexing="ij")
    return (b * (T + W) + torch.where(t == 0, t, t + W)).reshape(-1)


def embed_bwd_ref(tokens, dh, dtable0, W):
    """-> (dtable, mag): dtable[clamp(tok)] += dh[text rows]; image-word rows contribute nothing"""
    B, T = tokens.shape
    V = dtable0.shape[0]
    idx = tokens.clamp(0, V - 1).reshape(-1)
    src = dh.to(F64)[embed_text_rows(B, T, W)]
    d0 = dtable0.to(F64)
    return d0.index_add(0, idx, src), d0.abs().index_add(0, idx, src.abs())


def emu_embed_bwd(tokens, dh, dtable0, W):
    B, T = tokens.shape
    return dtable0.index_add(0, tokens.clamp(0, dtable0.shape[0] - 1).reshape(-1), dh.float()[embed_text_rows(B, T, W)])


ROWS_SUM_SHAPE = (130, 320, 140)          # n_rows (three 64-row chunks, the last ragged), dim, rows of the source


def rows_sum_inputs(with_idx: bool):
    n, dim, n_src = ROWS_SUM_SHAPE
    idx = None
    if with_idx:
        idx = torch.randint(0, n_src, (n,), generator=torch.Generator().manual_seed(41)).to(torch.int32)
        idx[5] = idx[70] = idx[129] = idx[0]          # repeats across chunks
    return dict(src=_randn(n_src, dim, seed=42).to(BF), row_idx=idx, out0=_randn(dim, seed=43))


def rows_sum_ref(src, row_idx, n_rows, out0):
    rows = src.to(F64)[row_idx.long() if row_idx is not None else slice(0, n_rows)]
    return out0.to(F64) + rows.sum(0), out0.to(F64).abs() + rows.abs().sum(0)


def emu_rows_sum(src, row_idx, n_rows, out0):
    return out0 + src.float()[row_idx.long() if row_idx is not None else slice(0, n_rows)].sum(0)


# ------------------------------------------------------------------ SwiGLU
SWIGLU_ROWS = 33
SWIGLU_F = [48, 176]
SWIGLU_GATES = [0.0, 30.0, -30.0, 90.0, -90.0]


def swiglu_inputs(F):
    """bf16 gate / up / dact [33, F]; the special gates sit at the start of row 0 and at the end of the last row"""
    s = 5000 + F
    g = 2.0 * _randn(SWIGLU_ROWS, F, seed=s + 1)
    n = len(SWIGLU_GATES)
    g[0, :n] = torch.tensor(SWIGLU_GATES)
    g[-1, -n:] = torch.tensor(SWIGLU_GATES)
    return dict(g=g.to(BF), u=_randn(SWIGLU_ROWS, F, seed=s + 2).to(BF), da=_randn(SWIGLU_ROWS, F, seed=s + 3).to(BF))


def swiglu_pack(g, u, interleaved: bool):
    """[rows, 2F]: gate | up halves, or 16-column blocks of gate and up alternating"""
    rows, F = g.shape
    if interleaved:
        return torch.stack([g.reshape(rows, F // 16, 16), u.reshape(rows, F // 16, 16)], dim=2).reshape(rows, 2 * F)
    return torch.cat([g, u], dim=1)


def swiglu_unpack(gu, interleaved: bool):
    rows, F2 = gu.shape
    if interleaved:
        d = gu.reshape(rows, F2 // 32, 2, 16)
        return d[:, :, 0].reshape(rows, F2 // 2), d[:, :, 1].reshape(rows, F2 // 2)
    return gu[:, :F2 // 2], gu[:, F2 // 2:]


def swiglu_fwd_ref(g, u):
    """-> (act, underflow sensitivity |g u|); bound: within(..., rel=SWIGLU_FWD_REL, underflow=...)"""
    g, u = g.to(F64), u.to(F64)
    return g * torch.sigmoid(g) * u, (g * u).abs()


def emu_swiglu_fwd(g, u):
    gf = g.float()
    return ((gf * (1.0 / (1.0 + torch.exp(-gf)))).to(g.dtype).float() * u.float()).to(g.dtype)


def swiglu_bwd_ref(g, u, da):
    """-> (dg, mag_dg, uf_dg, du, mag_du, uf_du);  dg = da u sig (1 + g (1 - sig)),  du = da g sig"""
    g, u, da = g.to(F64), u.to(F64), da.to(F64)
    sig, nsig = torch.sigmoid(g), torch.sigmoid(-g)            # 1 - sig without cancellation
    dg = da * u * sig * (1.0 + g * nsig)
    mag_dg = (da * u).abs() * sig * (1.0 + g.abs() * nsig)
    du = da * g * sig
    return dg, mag_dg, (da * u).abs() * (1.0 + g.abs()), du, du.abs(), (da * g).abs()


def emu_swiglu_bwd(g, u, da):
    gf, uf, daf = g.float(), u.float(), da.float()
    sig = 1.0 / (1.0 + torch.exp(-gf))
    return (daf * uf * (sig * (1.0 + gf * (1.0 - sig)))).to(g.dtype), (daf * (gf * sig)).to(g.dtype)


# ------------------------------------------------------------------ RoPE backward + pack
ROPE_SHAPES = [(2, 7, 4, 2, 64), (1, 5, 2, 2, 128)]           # (B, S, H, Hkv, hd)
ROPE_POS0 = 5


def rope_bwd_inputs(B, S, H, Hkv, hd):
    s = 6000 + hd
    return dict(dq=_randn(B, S, H, hd, seed=s + 1).to(BF), dk=_randn(B, Hkv, S, hd, seed=s + 2).to(BF),
                dv=_randn(B, Hkv, S, hd, seed=s + 3).to(BF))


def rope_bwd_pack_ref(dq, dk, dv, cos_sin, pos0):
    """dq [B,S,H,hd], dk / dv [B,Hkv,S,hd], cos_sin fp32 [end, hd/2, 2] -> (dqkv [B*S, (H+2Hkv) hd], mag): q and k slots rotated
    by -theta (out0 = a cos + b sin, out1 = -a sin + b cos, mag = |a cos| + |b sin| resp. |a sin| + |b cos|), v copied."""
    B, S, H, hd = dq.shape
    Hkv = dk.shape[1]
    qk = torch.cat([dq.to(F64), dk.to(F64).permute(0, 2, 1, 3)], dim=2)            # [B, S, H + Hkv, hd]
    a, b = qk[..., 0::2], qk[..., 1::2]
    cs = cos_sin[pos0:pos0 + S].to(F64)
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    out = torch.stack([a * co + b * si, -a * si + b * co], dim=-1).reshape(B, S, H + Hkv, hd)
    mag = torch.stack([(a * co).abs() + (b * si).abs(), (a * si).abs() + (b * co).abs()], dim=-1).reshape(B, S, H + Hkv, hd)
    v = dv.to(F64).permute(0, 2, 1, 3)
    return (torch.cat([out, v], dim=2).reshape(B * S, -1), torch.cat([mag, v.abs()], dim=2).reshape(B * S, -1))


def emu_rope_bwd_pack(dq, dk, dv, cos_sin, pos0):
    B, S, H, hd = dq.shape
    qk = torch.cat([dq.float(), dk.float().permute(0, 2, 1, 3)], dim=2)
    a, b = qk[..., 0::2], qk[..., 1::2]
    cs = cos_sin[pos0:pos0 + S]
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    out = torch.stack([a * co + b * si, -a * si + b * co], dim=-1).reshape(B, S, -1, hd).to(dq.dtype)
    return torch.cat([out, dv.permute(0, 2, 1, 3)], dim=2).reshape(B * S, -1)


# ------------------------------------------------------------------ bit-exact ops: shapes and inputs
ADD2D_SHAPE = (37, 68)
CAST_SHAPE = (37, 72)
SCALE_CAST_N = [1, 7, 8, 2055, 6149]
SCALE_CAST_SCALES = [1.0 / 8.0, 1.0 / 3.0]
LORA_SCATTER = [(16, (64, 32, 32)), (8, (40,)), (4, (16, 16, 16, 16))]         # (r, n_j of every module)
LORA_ROW0 = 8


def plain_inputs(rows, cols, dtype, seed):
    return _randn(rows, cols, seed=seed).to(dtype)


def scale_cast_ref(src, scale, dst_dtype):
    """(dst dtype)(fp32(src) * fp32(scale)): one fp32 multiply, one rounding"""
    return (src.float() * torch.tensor(scale, dtype=F32)).to(dst_dtype)


def lora_gb_scatter_inputs(r, njs):
    """gbt fp32 [n_mods * r, LORA_ROW0 + sum(n_j)] (module j's block: rows j r .., columns row0_j ..) and non-zero destinations"""
    s = 7000 + r + len(njs)
    row0s, c = [], LORA_ROW0
    for n in njs:
        row0s.append(c)
        c += n
    return dict(gbt=_randn(len(njs) * r, c, seed=s), row0s=row0s, dst0=[_randn(n, r, seed=s + 1 + j) for j, n in enumerate(njs)])


def lora_gb_scatter_ref(gbt, r, dst0, row0s):
    return [d + gbt[j * r:(j + 1) * r, row0s[j]:row0s[j] + d.shape[0]].t() for j, d in enumerate(dst0)]
