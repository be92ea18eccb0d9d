"""-m gpu: the row-op backward kernels of a3v_train.hip in the dtypes a bf16 training step launches them in, element by element
against the fp64 references of tests/rowops_ref.py.

Every bound is rowops_ref.within (half a bf16 ulp + 2^-20 of the summed |terms|; derived there, and shown on the CPU to hold for a
correct fp32 implementation on these very inputs by tests/test_rowops_ref_cpu.py) or bit equality.  Every output is a view into a
wider buffer pre-filled with a sentinel: row padding and the rows past the last one must come back untouched; every accumulating
output starts from non-zero values.  Each test prints its worst error-to-bound ratio."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_ref as R  # noqa: E402
from a3vlm_amd import ops  # noqa: E402
from a3vlm_amd.model.LLM.llama_ens5 import precompute_cos_sin  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENT = -7.0


def guarded(t, pad, extra_rows=2):
    """t on the device as the top-left view of a sentinel-filled buffer with ``pad`` more columns and ``extra_rows`` more rows"""
    r, c = t.shape
    wide = torch.full((r + extra_rows, c + pad), SENT, dtype=t.dtype, device=DEV)
    wide[:r, :c] = t.to(DEV)
    return wide, wide[:r, :c]


def guarded1d(t, pad=64):
    wide = torch.full((t.numel() + pad,), SENT, dtype=t.dtype, device=DEV)
    wide[:t.numel()] = t.to(DEV)
    return wide, wide[:t.numel()]


def intact(wide, view):
    """everything of ``wide`` outside ``view`` still holds the sentinel"""
    if wide.dim() == 1:
        return bool((wide[view.numel():] == SENT).all())
    r, c = view.shape
    return bool((wide[:r, c:] == SENT).all()) and bool((wide[r:] == SENT).all())


def strided(t, pad):
    """an input on the device with a padded row stride"""
    return guarded(t, pad, extra_rows=0)[1]


# ------------------------------------------------------------------ RMSNorm backward
@functools.lru_cache(maxsize=None)
def rms_case(rows, dim, stream):
    d = R.rmsnorm_bwd_inputs(rows, dim, stream)
    return d, R.rmsnorm_bwd_ref(d["x"], d["w"], d["dy"], d["dh0"], d["dw0"])


def run_rmsnorm(rows, dim, stream, with_dw, lowp=False):
    d, (dh_ref, mag_dh, dw_ref, mag_dw) = rms_case(rows, dim, stream)
    x, dy = strided(d["x"], 8), strided(d["dy"], 64)
    dh_wide, dh = guarded(d["dh0"], 8)
    dw_wide, dw = guarded1d(d["dw0"])
    lp_wide, lp = guarded(torch.zeros(rows, dim, dtype=BF), 64) if lowp else (None, None)
    ops.rmsnorm_bwd(x, d["w"].to(DEV), dy, dh, dw if with_dw else None, R.RMS_EPS, dh_lowp=lp)
    r_dh = R.within(dh, dh_ref, mag_dh, stream)
    r_dw = R.within(dw, dw_ref, mag_dw, F32) if with_dw else 0.0
    print(f"rmsnorm_bwd {stream} ({rows}, {dim}) dw={with_dw}: dh {r_dh:.3f} dw {r_dw:.3f}")
    assert r_dh <= 1.0 and r_dw <= 1.0
    assert intact(dh_wide, dh) and intact(dw_wide, dw)
    if not with_dw:
        assert torch.equal(dw.cpu(), d["dw0"])
    if lowp:
        assert torch.equal(lp, dh.to(BF)) and intact(lp_wide, lp)


@pytest.mark.parametrize("rows,dim", R.RMS_SHAPES)
def test_rmsnorm_bwd_bf16_stream(rows, dim):
    """x, dy, dh bf16: MAXV 4 (<= 4096), MAXV 8 with the next-row prefetch (> 4096; (9, 4100): slot 4 live for thread 0 only, one row
    in the last block), the scalar fallback (130); dw through the partial rows + column sum"""
    run_rmsnorm(rows, dim, BF, True)


@pytest.mark.parametrize("rows,dim", [(17, 4096), (9, 4100)])
def test_rmsnorm_bwd_bf16_stream_no_dw(rows, dim):
    run_rmsnorm(rows, dim, BF, False)


@pytest.mark.parametrize("rows,dim", R.RMS_SHAPES_F32_STREAM)
def test_rmsnorm_bwd_f32_stream_lowp_copy(rows, dim):
    """fp32 x / dh with bf16 dy and the bf16 copy of the updated dh, beyond dim 6144"""
    run_rmsnorm(rows, dim, F32, True, lowp=True)


def test_rmsnorm_bwd_refuses_dim_8196():
    d = R.rmsnorm_bwd_inputs(2, 8196)
    dh_wide, dh = guarded(d["dh0"], 8)
    dw_wide, dw = guarded1d(d["dw0"])
    before, before_w = dh_wide.clone(), dw_wide.clone()
    with pytest.raises(RuntimeError):
        ops.rmsnorm_bwd(strided(d["x"], 8), d["w"].to(DEV), strided(d["dy"], 8), dh, dw, R.RMS_EPS)
    torch.cuda.synchronize()
    assert torch.equal(dh_wide, before) and torch.equal(dw_wide, before_w)


# ------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("offset_sd", R.LN_OFFSETS)
@pytest.mark.parametrize("rows,dim", R.LN_SHAPES)
def test_layernorm_bwd_bf16(rows, dim, offset_sd):
    """bf16 x, dy (gathered through row_map from a buffer of twice the rows) and dx; zero-mean rows and rows offset by 8 sigma"""
    d = R.layernorm_bwd_inputs(rows, dim, offset_sd)
    dx_ref, mag_dx, dw_ref, mag_dw, db_ref, mag_db = R.layernorm_bwd_ref(d["x"], d["w"], d["dy_big"][d["row_map"].long()], d["dw0"], d["db0"])
    dx_wide, dx = guarded(torch.zeros(rows, dim, dtype=BF), 8)
    dw_wide, dw = guarded1d(d["dw0"])
    db_wide, db = guarded1d(d["db0"])
    ops.layernorm_bwd(strided(d["x"], 8), d["w"].to(DEV), strided(d["dy_big"], 64), d["row_map"].to(DEV), dx, dw, db, R.LN_EPS)
    rs = R.within(dx, dx_ref, mag_dx, BF), R.within(dw, dw_ref, mag_dw, F32), R.within(db, db_ref, mag_db, F32)
    print(f"layernorm_bwd offset {offset_sd} ({rows}, {dim}): dx {rs[0]:.3f} dw {rs[1]:.3f} db {rs[2]:.3f}")
    assert max(rs) <= 1.0
    assert intact(dx_wide, dx) and intact(dw_wide, dw) and intact(db_wide, db)


def test_layernorm_bwd_refuses_dim_8200():
    d = R.layernorm_bwd_inputs(2, 8200, 0.0)
    dx_wide, dx = guarded(torch.zeros(2, 8200, dtype=BF), 8)
    dw_wide, dw = guarded1d(d["dw0"])
    db_wide, db = guarded1d(d["db0"])
    before = [t.clone() for t in (dx_wide, dw_wide, db_wide)]
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(strided(d["x"], 8), d["w"].to(DEV), strided(d["dy_big"], 8), d["row_map"].to(DEV), dx, dw, db, R.LN_EPS)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((dx_wide, dw_wide, db_wide), before))


# ------------------------------------------------------------------ embedding backward, row sums
@pytest.mark.parametrize("B,T,W,dim,V", R.EMBED_SHAPES)
def test_embed_bwd_bf16(B, T, W, dim, V):
    """bf16 dh into a non-zero fp32 table: repeats accumulate, a token < 0 lands in row 0 and one >= V in row V - 1 (the kernel's
    clamp, pinned here), image-word rows add nothing, the rows behind the table stay"""
    d = R.embed_bwd_inputs(B, T, W, dim, V)
    ref, mag = R.embed_bwd_ref(d["tokens"], d["dh"], d["dtable0"], W)
    wide, _ = guarded(d["dtable0"], 0)
    dtable = wide[:V]
    ops.embed_bwd(strided(d["tokens"], 3), d["dh"].to(DEV), dtable, B, T, W, dim)
    r = R.within(dtable, ref, mag, F32)
    print(f"embed_bwd ({B}, {T}, {W}, {dim}, {V}): dtable {r:.3f}")
    assert r <= 1.0 and intact(wide, dtable)
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[d["tokens"].clamp(0, V - 1).reshape(-1)] = False
    assert torch.equal(dtable.cpu()[untouched], d["dtable0"][untouched])


@pytest.mark.parametrize("with_idx", [True, False])
def test_rows_sum_bf16(with_idx):
    d = R.rows_sum_inputs(with_idx)
    n = R.ROWS_SUM_SHAPE[0]
    ref, mag = R.rows_sum_ref(d["src"], d["row_idx"], n, d["out0"])
    wide, out = guarded1d(d["out0"])
    ops.rows_sum(strided(d["src"], 8), d["row_idx"].to(DEV) if with_idx else None, n, out)
    r = R.within(out, ref, mag, F32)
    print(f"rows_sum idx={with_idx}: out {r:.3f}")
    assert r <= 1.0 and intact(wide, out)


# ------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("Fd", R.SWIGLU_F)
def test_swiglu_fwd_bwd_bf16(Fd, inter):
    """the non-temporal bf16 kernels, both layouts, every leading dimension padded; gates 0, +-30, +-90 (exp overflows: the result
    is still the finite limit)"""
    d = R.swiglu_inputs(Fd)
    rows = R.SWIGLU_ROWS
    gu = strided(R.swiglu_pack(d["g"], d["u"], inter), 8)
    act_ref, uf = R.swiglu_fwd_ref(d["g"], d["u"])
    act_wide, act = guarded(torch.zeros(rows, Fd, dtype=BF), 64)
    ops.swiglu_fwd(gu, act, Fd, inter)
    r0 = R.within(act, act_ref, None, BF, rel=R.SWIGLU_FWD_REL, underflow=uf)
    dg_ref, mag_dg, uf_dg, du_ref, mag_du, uf_du = R.swiglu_bwd_ref(d["g"], d["u"], d["da"])
    dgu_wide, dgu = guarded(torch.zeros(rows, 2 * Fd, dtype=BF), 8)
    ops.swiglu_bwd(gu, strided(d["da"], 8), dgu, Fd, inter)
    dg, du = R.swiglu_unpack(dgu.cpu(), inter)
    r1, r2 = R.within(dg, dg_ref, mag_dg, BF, underflow=uf_dg), R.within(du, du_ref, mag_du, BF, underflow=uf_du)
    print(f"swiglu F {Fd} interleaved={inter}: fwd {r0:.3f} dg {r1:.3f} du {r2:.3f}")
    assert max(r0, r1, r2) <= 1.0
    assert intact(act_wide, act) and intact(dgu_wide, dgu)


# ------------------------------------------------------------------ RoPE backward + pack
@pytest.mark.parametrize("B,S,H,Hkv,hd", R.ROPE_SHAPES)
def test_rope_bwd_pack_bf16(B, S, H, Hkv, hd):
    d = R.rope_bwd_inputs(B, S, H, Hkv, hd)
    cos_sin = precompute_cos_sin(hd, 64, 10000.0, None)
    ref, mag = R.rope_bwd_pack_ref(d["dq"], d["dk"], d["dv"], cos_sin, R.ROPE_POS0)
    wide, dqkv = guarded(torch.zeros(B * S, (H + 2 * Hkv) * hd, dtype=BF), 8)
    ops.rope_bwd_pack(d["dq"].to(DEV), d["dk"].to(DEV), d["dv"].to(DEV), dqkv, cos_sin.to(DEV), B, S, H, Hkv, hd, R.ROPE_POS0)
    nqk = (H + Hkv) * hd
    r = R.within(dqkv[:, :nqk], ref[:, :nqk], mag[:, :nqk], BF)
    print(f"rope_bwd_pack ({B}, {S}, {H}, {Hkv}, {hd}): dq|dk {r:.3f}")
    assert r <= 1.0 and intact(wide, dqkv)
    assert torch.equal(dqkv[:, nqk:].cpu(), d["dv"].permute(0, 2, 1, 3).reshape(B * S, Hkv * hd))


# ------------------------------------------------------------------ bit-exact: add2d, cast, scale_cast, lora_gb_scatter
@pytest.mark.parametrize("dtype", [F32, BF])
def test_add2d(dtype):
    rows, cols = R.ADD2D_SHAPE
    a, b = R.plain_inputs(rows, cols, dtype, 31), R.plain_inputs(rows, cols, dtype, 32)
    wide, dst = guarded(a, 8)
    ops.add2d(dst, strided(b, 64))
    assert torch.equal(dst.cpu(), a + b) and intact(wide, dst)
    a, b = R.plain_inputs(rows, 70, dtype, 33), R.plain_inputs(rows, 70, dtype, 34)
    wide, dst = guarded(a, 8)
    before = wide.clone()
    with pytest.raises(RuntimeError):
        ops.add2d(dst, strided(b, 64))
    torch.cuda.synchronize()
    assert torch.equal(wide, before)


@pytest.mark.parametrize("src_dtype,dst_dtype", list(itertools.product([F32, BF], [F32, BF])))
def test_cast_all_pairs(src_dtype, dst_dtype):
    rows, cols = R.CAST_SHAPE
    a = R.plain_inputs(rows, cols, src_dtype, 35)
    wide, dst = guarded(torch.zeros(rows, cols, dtype=dst_dtype), 64)
    ops.cast(strided(a, 8), dst)
    assert torch.equal(dst.cpu(), a.to(dst_dtype)) and intact(wide, dst)
    a = R.plain_inputs(rows, 68, src_dtype, 36)
    wide, dst = guarded(torch.zeros(rows, 68, dtype=dst_dtype), 64)
    before = wide.clone()
    with pytest.raises(RuntimeError):
        ops.cast(strided(a, 8), dst)
    torch.cuda.synchronize()
    assert torch.equal(wide, before)


@pytest.mark.parametrize("src_dtype,dst_dtype", list(itertools.product([F32, BF], [F32, BF])))
def test_scale_cast_all_pairs(src_dtype, dst_dtype):
    """8-element vector body and the scalar tail (n = 1, 7: tail only; 8: body only; 2055, 6149: several blocks + tail)"""
    for n, scale in itertools.product(R.SCALE_CAST_N, R.SCALE_CAST_SCALES):
        src = R.plain_inputs(1, n, src_dtype, 50 + n).view(-1)
        wide, dst = guarded1d(torch.zeros(n, dtype=dst_dtype), 16)
        ops.scale_cast(src.to(DEV), dst, scale)
        assert torch.equal(dst.cpu(), R.scale_cast_ref(src, scale, dst_dtype)), (n, scale)
        assert intact(wide, dst), (n, scale)


def test_scale_cast_refuses_unaligned_source():
    n = 2055
    buf = R.plain_inputs(1, n + 1, F32, 60).view(-1).to(DEV)
    wide, dst = guarded1d(torch.zeros(n, dtype=BF), 16)
    before = wide.clone()
    with pytest.raises(RuntimeError):
        ops.scale_cast(buf[1:], dst, 0.125)             # 4 bytes past a 16-byte boundary
    torch.cuda.synchronize()
    assert torch.equal(wide, before)


def scatter_views(dst0, r):
    """module gradients [n_j, r] as contiguous pieces of one sentinel-filled buffer, 8 floats of sentinel after each"""
    flat = torch.full((sum(t.numel() + 8 for t in dst0),), SENT, dtype=F32, device=DEV)
    views, gaps, o = [], [], 0
    for t in dst0:
        v = flat[o:o + t.numel()].view(t.shape[0], r)
        v.copy_(t)
        views.append(v)
        gaps.append(flat[o + t.numel():o + t.numel() + 8])
        o += t.numel() + 8
    return flat, views, gaps


@pytest.mark.parametrize("r,njs", R.LORA_SCATTER)
def test_lora_gb_scatter(r, njs):
    d = R.lora_gb_scatter_inputs(r, njs)
    want = R.lora_gb_scatter_ref(d["gbt"], r, d["dst0"], d["row0s"])
    gbt = strided(d["gbt"], 8)
    _, views, gaps = scatter_views(d["dst0"], r)
    ops.lora_gb_scatter(gbt, r, views, d["row0s"])
    for v, w in zip(views, want):
        assert torch.equal(v.cpu(), w)
    assert all(bool((g == SENT).all()) for g in gaps)
    assert torch.equal(gbt.cpu(), d["gbt"])


def test_lora_gb_scatter_refuses_five_modules():
    d = R.lora_gb_scatter_inputs(4, (16,) * 5)
    flat, views, _ = scatter_views(d["dst0"], 4)
    before = flat.clone()
    with pytest.raises(RuntimeError):
        ops.lora_gb_scatter(strided(d["gbt"], 8), 4, views, d["row0s"])
    torch.cuda.synchronize()
    assert torch.equal(flat, before)
