"""CPU: the fp64 references of tests/rowops_ref.py against torch fp64 autograd (a), and every input set of
tests/test_gpu_rowops_bf16.py through an fp32 restatement of the kernel's formula (b): a correct fp32 implementation stays inside
the derived bounds on exactly these inputs, so a GPU failure there is the kernel's."""
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
from a3vlm_amd.model.LLM.llama_ens5 import precompute_cos_sin
from oracle import ref_cpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max())


def oracle_in_fp64():
    """ref_cpu.rmsnorm / apply_rotary_emb compute in ``x.float()``: inside this context that is fp64, so that their autograd is
    the 1e-12 reference the closed forms are held to."""
    return mock.patch.object(torch.Tensor, "float", lambda self: self.double())


# ------------------------------------------------------------------ (a) closed forms == fp64 autograd
def test_rmsnorm_bwd_ref_is_autograd():
    d = R.rmsnorm_bwd_inputs(9, 260)
    x, w = d["x"].to(F64).requires_grad_(True), d["w"].to(F64).requires_grad_(True)
    with oracle_in_fp64():
        y = ref_cpu.rmsnorm(x, w, R.RMS_EPS)
    assert y.dtype == F64 and rel(y, R.rmsnorm_fwd64(x.detach(), w.detach(), R.RMS_EPS)) < 1e-12
    y.backward(d["dy"].to(F64))
    dh, _, dw, _ = R.rmsnorm_bwd_ref(d["x"], d["w"], d["dy"], d["dh0"], d["dw0"])
    assert rel(dh - d["dh0"].to(F64), x.grad) < 1e-12 and rel(dw - d["dw0"].to(F64), w.grad) < 1e-12


@pytest.mark.parametrize("offset_sd", R.LN_OFFSETS)
def test_layernorm_bwd_ref_is_autograd(offset_sd):
    d = R.layernorm_bwd_inputs(7, 130, offset_sd)
    dy = d["dy_big"][d["row_map"].long()]
    x, w, b = d["x"].to(F64).requires_grad_(True), d["w"].to(F64).requires_grad_(True), torch.zeros(130, dtype=F64, requires_grad=True)
    F.layer_norm(x, (130,), w, b, R.LN_EPS).backward(dy.to(F64))
    dx, _, dw, _, db, _ = R.layernorm_bwd_ref(d["x"], d["w"], dy, d["dw0"], d["db0"])
    assert rel(dx, x.grad) < 1e-12 and rel(dw - d["dw0"].to(F64), w.grad) < 1e-12 and rel(db - d["db0"].to(F64), b.grad) < 1e-12


def test_swiglu_ref_is_autograd():
    d = R.swiglu_inputs(48)
    g, u = d["g"].to(F64).requires_grad_(True), d["u"].to(F64).requires_grad_(True)
    act = F.silu(g) * u
    assert rel(R.swiglu_fwd_ref(d["g"], d["u"])[0], act.detach()) < 1e-12
    act.backward(d["da"].to(F64))
    dg, _, _, du, _, _ = R.swiglu_bwd_ref(d["g"], d["u"], d["da"])
    assert rel(dg, g.grad) < 1e-12 and rel(du, u.grad) < 1e-12


@pytest.mark.parametrize("B,S,H,Hkv,hd", R.ROPE_SHAPES)
def test_rope_bwd_ref_is_autograd(B, S, H, Hkv, hd):
    d = R.rope_bwd_inputs(B, S, H, Hkv, hd)
    p0 = R.ROPE_POS0
    fc = ref_cpu.precompute_freqs_cis(hd, 64)
    cos_sin = precompute_cos_sin(hd, 64, 10000.0, None)
    assert torch.equal(cos_sin[..., 0], fc.real) and torch.equal(cos_sin[..., 1], fc.imag)
    q = torch.randn(B, S, H, hd, dtype=F64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    k = torch.randn(B, S, Hkv, hd, dtype=F64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    with oracle_in_fp64():
        oq, ok = ref_cpu.apply_rotary_emb(q, k, fc[p0:p0 + S])
    assert oq.dtype == F64
    ((oq * d["dq"].to(F64)).sum() + (ok * d["dk"].to(F64).permute(0, 2, 1, 3)).sum()).backward()
    ref, _ = R.rope_bwd_pack_ref(d["dq"], d["dk"], d["dv"], cos_sin, p0)
    ref = ref.view(B, S, H + 2 * Hkv, hd)
    assert rel(ref[:, :, :H], q.grad) < 1e-12 and rel(ref[:, :, H:H + Hkv], k.grad) < 1e-12
    assert torch.equal(ref[:, :, H + Hkv:], d["dv"].to(F64).permute(0, 2, 1, 3))


@pytest.mark.parametrize("B,T,W,dim,V", R.EMBED_SHAPES)
def test_embed_bwd_ref_is_autograd(B, T, W, dim, V):
    d = R.embed_bwd_inputs(B, T, W, dim, V)
    assert int(d["tokens"].min()) < 0 and int(d["tokens"].max()) >= V
    table = torch.zeros(V, dim, dtype=F64, requires_grad=True)
    dh = d["dh"].to(F64).view(B, T + W, dim)
    h = table[d["tokens"].clamp(0, V - 1)]                                 # [B, T, dim]
    text = torch.cat([dh[:, :1], dh[:, W + 1:]], dim=1)                     # BOS row, then the rows behind the image words
    (h * text).sum().backward()
    ref, mag = R.embed_bwd_ref(d["tokens"], d["dh"], d["dtable0"], W)
    assert rel(ref - d["dtable0"].to(F64), table.grad) < 1e-12
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_rows_sum_ref_is_index_select_sum():
    for with_idx in (True, False):
        d = R.rows_sum_inputs(with_idx)
        n = R.ROWS_SUM_SHAPE[0]
        src = d["src"].to(F64).requires_grad_(True)
        sel = src[d["row_idx"].long()] if with_idx else src[:n]
        want = d["out0"].to(F64) + sel.sum(0)
        ref, _ = R.rows_sum_ref(d["src"], d["row_idx"], n, d["out0"])
        assert rel(ref, want.detach()) < 1e-12


# ------------------------------------------------------------------ (b) a correct fp32 implementation is inside the bounds
def test_within_rejects_what_it_should():
    ref = torch.tensor([1.0, -3.0, 0.0], dtype=F64)
    mag = torch.tensor([1.0, 5.0, 2.0], dtype=F64)
    assert R.within(ref.to(BF), ref, mag, BF) == 0.0
    assert R.within((ref * (1 + 2.0 ** -9)).float(), ref, mag, BF) < 1.0
    assert R.within((ref * (1 + 2.0 ** -6)).float(), ref, mag, BF) > 1.0           # two bf16 ulps off
    assert R.within(torch.tensor([1.0, -3.0, 2.0 ** -18]), ref, mag, F32) > 1.0     # off where the terms cancel: mag, not |ref|
    assert R.within(torch.tensor([1.0, -3.0, 2.0 ** -20]), ref, mag, F32) <= 1.0
    assert R.within(torch.tensor([1.0, float("nan"), 0.0]), ref, mag, F32) == float("inf")
    assert R.within(ref[:2].float(), ref, mag, F32) == float("inf")


@pytest.mark.parametrize("stream", [BF, F32])
def test_rmsnorm_bwd_fp32_emulation_within_bounds(stream):
    for rows, dim in (R.RMS_SHAPES if stream == BF else R.RMS_SHAPES_F32_STREAM):
        d = R.rmsnorm_bwd_inputs(rows, dim, stream)
        dh, mag_dh, dw, mag_dw = R.rmsnorm_bwd_ref(d["x"], d["w"], d["dy"], d["dh0"], d["dw0"])
        e_dh, e_dw = R.emu_rmsnorm_bwd(d["x"], d["w"], d["dy"], d["dh0"], d["dw0"])
        r1, r2 = R.within(e_dh, dh, mag_dh, stream), R.within(e_dw, dw, mag_dw, F32)
        print(f"rmsnorm_bwd {stream} ({rows}, {dim}): dh {r1:.3f} dw {r2:.3f}")
        assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("offset_sd", R.LN_OFFSETS)
def test_layernorm_bwd_fp32_emulation_within_bounds(offset_sd):
    for rows, dim in R.LN_SHAPES:
        d = R.layernorm_bwd_inputs(rows, dim, offset_sd)
        dy = d["dy_big"][d["row_map"].long()]
        dx, mag_dx, dw, mag_dw, db, mag_db = R.layernorm_bwd_ref(d["x"], d["w"], dy, d["dw0"], d["db0"])
        e_dx, e_dw, e_db = R.emu_layernorm_bwd(d["x"], d["w"], dy, d["dw0"], d["db0"])
        rs = R.within(e_dx, dx, mag_dx, BF), R.within(e_dw, dw, mag_dw, F32), R.within(e_db, db, mag_db, F32)
        print(f"layernorm_bwd offset {offset_sd} ({rows}, {dim}): dx {rs[0]:.3f} dw {rs[1]:.3f} db {rs[2]:.3f}")
        assert max(rs) <= 1.0


def test_embed_and_rows_sum_fp32_emulation_within_bounds():
    for B, T, W, dim, V in R.EMBED_SHAPES:
        d = R.embed_bwd_inputs(B, T, W, dim, V)
        ref, mag = R.embed_bwd_ref(d["tokens"], d["dh"], d["dtable0"], W)
        assert R.within(R.emu_embed_bwd(d["tokens"], d["dh"], d["dtable0"], W), ref, mag, F32) <= 1.0
    for with_idx in (True, False):
        d = R.rows_sum_inputs(with_idx)
        n = R.ROWS_SUM_SHAPE[0]
        ref, mag = R.rows_sum_ref(d["src"], d["row_idx"], n, d["out0"])
        assert R.within(R.emu_rows_sum(d["src"], d["row_idx"], n, d["out0"]), ref, mag, F32) <= 1.0


@pytest.mark.parametrize("Fd", R.SWIGLU_F)
def test_swiglu_fp32_emulation_within_bounds(Fd):
    d = R.swiglu_inputs(Fd)
    for gate in R.SWIGLU_GATES:
        assert int((d["g"].float() == gate).sum()) >= 2
    act, uf = R.swiglu_fwd_ref(d["g"], d["u"])
    r0 = R.within(R.emu_swiglu_fwd(d["g"], d["u"]), act, None, BF, rel=R.SWIGLU_FWD_REL, underflow=uf)
    dg, mag_dg, uf_dg, du, mag_du, uf_du = R.swiglu_bwd_ref(d["g"], d["u"], d["da"])
    e_dg, e_du = R.emu_swiglu_bwd(d["g"], d["u"], d["da"])
    r1, r2 = R.within(e_dg, dg, mag_dg, BF, underflow=uf_dg), R.within(e_du, du, mag_du, BF, underflow=uf_du)
    print(f"swiglu F {Fd}: fwd {r0:.3f} dg {r1:.3f} du {r2:.3f}")
    assert max(r0, r1, r2) <= 1.0
    # the underflow allowance is what it says: nothing that an fp32 sigmoid represents is loosened by it
    assert float((R.F32_MIN_NORMAL * uf_dg).max()) < 1e-34 and float((R.F32_MIN_NORMAL * uf).max()) < 1e-34


@pytest.mark.parametrize("B,S,H,Hkv,hd", R.ROPE_SHAPES)
def test_rope_bwd_fp32_emulation_within_bounds(B, S, H, Hkv, hd):
    d = R.rope_bwd_inputs(B, S, H, Hkv, hd)
    cos_sin = precompute_cos_sin(hd, 64, 10000.0, None)
    ref, mag = R.rope_bwd_pack_ref(d["dq"], d["dk"], d["dv"], cos_sin, R.ROPE_POS0)
    emu = R.emu_rope_bwd_pack(d["dq"], d["dk"], d["dv"], cos_sin, R.ROPE_POS0)
    assert R.within(emu, ref, mag, BF) <= 1.0
    assert torch.equal(emu[:, (H + Hkv) * hd:].to(F64), ref[:, (H + Hkv) * hd:])


def test_bit_exact_references():
    """the torch expressions the copy / add / cast kernels must equal bit for bit, pinned against a second way to write them"""
    for n in R.SCALE_CAST_N:
        src = R.plain_inputs(1, n, F32, 50 + n).view(-1)
        for scale in R.SCALE_CAST_SCALES:
            want = R.scale_cast_ref(src, scale, BF)
            assert torch.equal(want, (src.double() * float(torch.tensor(scale, dtype=F32))).float().to(BF))     # fp32 product is one rounding of the exact one
    for r, njs in R.LORA_SCATTER:
        d = R.lora_gb_scatter_inputs(r, njs)
        assert d["row0s"][0] == R.LORA_ROW0 and d["gbt"].shape == (len(njs) * r, R.LORA_ROW0 + sum(njs))
        out = R.lora_gb_scatter_ref(d["gbt"], r, d["dst0"], d["row0s"])
        for j, o in enumerate(out):
            assert o.shape == (njs[j], r) and float(o[3, 1]) == float(d["dst0"][j][3, 1] + d["gbt"][j * r + 1, d["row0s"][j] + 3])
