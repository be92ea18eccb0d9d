"""CPU (-m "not gpu") checks of the 8-bit AdamW moments: the entry points exist in the header, the built library and the ctypes table;
the argument checks answer before any launch; the host restatement the GPU tests compare against (tests/adam8_ref.py) round-trips
within half an e4m3 step; FusedAdamW's state_dict / load_state_dict structure for both layouts (kernels patched out); the trainer's
parser; and the quality statement of DESIGN.md 5a on a seeded quadratic."""
import os
import re

import numpy as np
import pytest
import torch

import adam8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_adam8_quantize", "a3v_adam8_dequantize", "a3v_adamw8_scaled")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


def test_entries_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    assert "8-bit AdamW moments" in src and "1e-30" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = built.load()
    for name in ENTRIES:
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in include/a3vlm_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name


def test_arguments_are_refused_before_any_launch(built):
    """No device is needed to get these answers: a refused call never uses its pointers."""
    lib = built.load()
    p, odd, SHAPE, ARG = 4096, 4096 + 8, -1, -3      # p: non-NULL and 16-B aligned; odd: 8-B aligned only
    hp = (1e-3, 0.9, 0.95, 1e-8, 0.0)
    # n % 256
    assert lib.a3v_adam8_quantize(p, p, p, p, p, p, 300, None) == SHAPE
    assert lib.a3v_adam8_dequantize(p, p, p, p, p, p, 255, None) == SHAPE
    assert lib.a3v_adamw8_scaled(p, p, p, p, p, p, 257, *hp, 1, None, None, None) == SHAPE
    # alignment: 16 B for the arrays and the image, 4 B for the scales
    for i in (0, 1, 2, 4):
        a = [p] * 6
        a[i] = odd
        assert lib.a3v_adam8_quantize(*a, 256, None) == SHAPE, i
    for i in (3, 5):
        a = [p] * 6
        a[i] = p + 2
        assert lib.a3v_adam8_quantize(*a, 256, None) == SHAPE, i
        a[i] = p + 4                                   # 4-B aligned scales pass the check; so the next refusal is the size
        assert lib.a3v_adam8_quantize(*a, 100, None) == SHAPE, i
    for i in (0, 2, 4, 5):
        a = [p] * 6
        a[i] = odd
        assert lib.a3v_adam8_dequantize(*a, 256, None) == SHAPE, i
    for i in (0, 1, 2, 4):
        a = [p] * 6
        a[i] = odd
        assert lib.a3v_adamw8_scaled(*a, 256, *hp, 1, None, None, None) == SHAPE, i
    assert lib.a3v_adamw8_scaled(p, p, p, p + 2, p, p, 256, *hp, 1, None, None, None) == SHAPE        # m_scale
    assert lib.a3v_adamw8_scaled(p, p, p, p, p, p + 2, 256, *hp, 1, None, None, None) == SHAPE        # r_scale
    assert lib.a3v_adamw8_scaled(p, p, p, p, p, p, 256, *hp, 1, None, p + 2, None) == SHAPE           # grad_scale: 4 B
    assert lib.a3v_adam8_dequantize(p, p + 2, p, p, p, p, 256, None) == SHAPE                         # the scales of the inverse: 4 B
    assert lib.a3v_adam8_dequantize(p, p, p, p + 2, p, p, 256, None) == SHAPE
    assert lib.a3v_adamw8_scaled(p, p, p, p, p, p, 256, *hp, 1, odd, None, None) == SHAPE        # the bf16 image
    # NULL required pointers, n <= 0, step < 1
    for i in range(6):
        a = [p] * 6
        a[i] = None
        assert lib.a3v_adamw8_scaled(*a, 256, *hp, 1, None, None, None) == ARG, i
        assert lib.a3v_adam8_quantize(*a, 256, None) == ARG, i            # a triple is given whole or not at all
        assert lib.a3v_adam8_dequantize(*a, 256, None) == ARG, i
    assert lib.a3v_adam8_quantize(None, None, None, None, None, None, 256, None) == ARG
    assert lib.a3v_adam8_quantize(p, p, p, p, p, p, 0, None) == ARG
    assert lib.a3v_adamw8_scaled(p, p, p, p, p, p, 256, *hp, 0, None, None, None) == ARG


def _moments(seed, n=256 * 6):
    rs = np.random.RandomState(seed)
    g = (rs.randn(n) * np.exp2(rs.uniform(-8, 8, n))).astype(np.float32)
    m, v = (0.1 * g).astype(np.float32), (0.05 * g * g).astype(np.float32)
    m[256:512] = 0                                    # an all-zero block of each
    v[512:768] = 0
    v[768] = np.float32(2.0 ** 40) * v[769:1024].max()      # one element 2^20 times the rest in r: the rest rounds to code 0
    m[1300] = 0
    return m, v


def test_reference_round_trip_within_half_a_step():
    m, v = _moments(0)
    mq, ms, rq, rs = R.quantize(m, v)
    assert mq.dtype == rq.dtype == np.uint8 and mq.shape == rq.shape == m.shape and ms.shape == rs.shape == (m.size // 256,)
    assert ms.dtype == rs.dtype == np.float32
    r = np.sqrt(v)
    np.testing.assert_array_equal(ms, np.maximum(np.abs(m).reshape(-1, 256).max(1), np.float32(1e-30)) / np.float32(448))
    np.testing.assert_array_equal(rs, np.maximum(r.reshape(-1, 256).max(1), np.float32(1e-30)) / np.float32(448))
    md, rd = R.dequantize_m(mq, ms), R.dequantize_r(rq, rs)
    assert np.isfinite(md).all() and np.isfinite(rd).all()
    # all-zero blocks: codes 0, scale 1e-30 / 448, finite
    assert not mq[256:512].any() and ms[1] == R.ZERO_SCALE and not rq[512:768].any() and rs[2] == R.ZERO_SCALE
    # m: within half a step of its source (it may round to zero)
    assert (np.abs(md.astype(np.float64) - m) <= R.half_step_bound(m, ms)).all()
    # r: within half a step, or equal to 2^-9 * scale under the extra rule
    floor = (np.float32(2.0 ** -9) * np.repeat(rs, 256)).astype(np.float32)
    ok = np.abs(rd.astype(np.float64) - r) <= R.half_step_bound(r, rs)
    ruled = (r != 0) & (rd == floor) & ((rq & 0x7F) == 1)
    assert (ok | ruled).all()
    assert ruled[769:1024].all() and not ok[769:1024].all()       # the block with the outlier really needs the rule
    assert ((rq & 0x7F) != 0)[r != 0].all() and (rq[r == 0] == 0).all()       # non-zero r never gets code 0; zero stays zero
    no_rule = R.quantize_r(r, keep_nonzero=False)[0]
    assert (no_rule[769:1024] == 0).all() and (np.delete(no_rule, np.s_[769:1024]) == np.delete(rq, np.s_[769:1024])).sum() > 0
    # quantising a dequantised state gives the same codes (and scales)
    m2, v2 = R.dequantize(mq, ms, rq, rs)
    mq2, ms2, rq2, rs2 = R.quantize(m2, v2)
    np.testing.assert_array_equal(mq2, mq)
    np.testing.assert_array_equal(rq2, rq)
    np.testing.assert_array_equal(ms2, ms)
    np.testing.assert_array_equal(rs2, rs)


def test_reference_encoder_is_torchs_e4m3fn():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.randn(20000).astype(np.float32) * 100, np.linspace(-448, 448, 20001, dtype=np.float32),
                        (np.arange(-4096, 4097) / 4096 * 2.0 ** -5).astype(np.float32), np.float32([0.0, -0.0, 448, -448, 2.0 ** -10, 3 * 2.0 ** -11])])
    x = np.clip(x, -448, 448)
    q = R.e4m3_encode(x)
    np.testing.assert_array_equal(q, torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    np.testing.assert_array_equal(R.e4m3_decode(q), torch.from_numpy(q).view(torch.float8_e4m3fn).float().numpy())
    assert R.e4m3_encode(np.float32([1e9, -1e9])).tolist() == [0x7E, 0xFE]          # saturating, never the NaN code


# ---------------------------------------------------------------------------------------------------------------- host structure
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _patch_kernels(monkeypatch):
    """The two conversion kernels, replaced by the restatement (CPU tensors in, CPU tensors out)."""
    from a3vlm_amd import optim

    def quant(m, v):
        mq, ms, rq, rs = R.quantize(m.numpy().reshape(-1), v.numpy().reshape(-1))
        return _t(mq).view(m.shape), _t(ms), _t(rq).view(m.shape), _t(rs)

    def dequant(mq, ms, rq, rs):
        m, v = R.dequantize(mq.numpy().reshape(-1), ms.numpy(), rq.numpy().reshape(-1), rs.numpy())
        return _t(m).view(mq.shape), _t(v).view(mq.shape)
    monkeypatch.setattr(optim, "_quantize_state", quant)
    monkeypatch.setattr(optim, "_dequantize_state", dequant)
    monkeypatch.setenv("A3V_ADAMW_MULTI", "4096")
    return optim


def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(64, 128, generator=g)), torch.nn.Parameter(torch.randn(300, generator=g)),
            torch.nn.Parameter(torch.randn(64, 16, generator=g))]


def _stock_state(params):
    """A torch.optim.AdamW state_dict with fabricated moments."""
    opt = torch.optim.AdamW([{"params": params[:1], "weight_decay": 0.1}, {"params": params[1:], "weight_decay": 0.0}], lr=1e-3, betas=(0.9, 0.95))
    g = torch.Generator().manual_seed(4)
    for p in params:
        grad = torch.randn(p.shape, generator=g) * torch.exp2(torch.rand(p.shape, generator=g) * 12 - 6)
        opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": 0.1 * grad, "exp_avg_sq": 0.05 * grad * grad}
    return opt.state_dict()


def _same(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys(), i
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.dtype == y.dtype and x.shape == y.shape, (i, k)
            assert np.array_equal(x.numpy().reshape(-1).view(np.uint8), y.numpy().reshape(-1).view(np.uint8)), (i, k)       # bit for bit


def test_state_dict_layouts(monkeypatch):
    optim = _patch_kernels(monkeypatch)
    params = _params()
    stock = _stock_state(params)

    def make(moments):
        return optim.FusedAdamW([{"params": params[:1], "weight_decay": 0.1}, {"params": params[1:], "weight_decay": 0.0}], lr=1e-3,
                                betas=(0.9, 0.95), moments=moments)
    with pytest.raises(ValueError, match="moment format"):
        make("int8")
    o8 = make("e4m3")
    assert o8._is8(params[0]) and not o8._is8(params[1]) and not o8._is8(params[2])     # big and % 256 only: 300 is odd, 64 x 16 is small
    # the stock fp32 layout is accepted and quantised on load, tensor by tensor
    o8.load_state_dict(stock)
    st = o8.state[params[0]]
    assert sorted(st) == ["exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale", "step"] and float(st["step"]) == 7
    assert st["exp_avg_q"].dtype == torch.uint8 and st["exp_avg_q"].shape == params[0].shape and st["exp_avg_scale"].shape == (64 * 128 // 256,)
    want = R.quantize(stock["state"][0]["exp_avg"].numpy().reshape(-1), stock["state"][0]["exp_avg_sq"].numpy().reshape(-1))
    for k, w in zip(("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale"), want):
        np.testing.assert_array_equal(st[k].numpy().reshape(-1), w)
    for p, i in ((params[1], 1), (params[2], 2)):
        assert sorted(o8.state[p]) == ["exp_avg", "exp_avg_sq", "step"]
        assert torch.equal(o8.state[p]["exp_avg"], stock["state"][i]["exp_avg"]) and o8.state[p]["exp_avg"] is not stock["state"][i]["exp_avg"]
    # the marker, and native -> load -> save is identical
    native = o8.state_dict()
    assert all(g["moments"] == "e4m3x256" for g in native["param_groups"]) and len(native["param_groups"]) == 2
    assert "moments" not in o8.param_groups[0]
    o8b = make("e4m3")
    o8b.load_state_dict(native)
    _same(o8b.state_dict(), native)
    assert o8b.state[params[0]]["exp_avg_q"].data_ptr() != st["exp_avg_q"].data_ptr()       # copies, as torch's loader makes
    assert "moments" not in o8b.param_groups[0] and o8b.param_groups[0]["weight_decay"] == 0.1
    # an fp32 optimizer handed a native dict dequantises it; its own state_dict carries no marker
    o32 = make("fp32")
    o32.load_state_dict(native)
    assert sorted(o32.state[params[0]]) == ["exp_avg", "exp_avg_sq", "step"] and o32.state[params[0]]["exp_avg"].dtype == torch.float32
    m, v = R.dequantize(*want)
    np.testing.assert_array_equal(o32.state[params[0]]["exp_avg"].numpy().reshape(-1), m)
    np.testing.assert_array_equal(o32.state[params[0]]["exp_avg_sq"].numpy().reshape(-1), v)
    assert all("moments" not in g for g in o32.state_dict()["param_groups"])
    # ... and a stock dict loads into it the way it always did
    o32.load_state_dict(stock)
    assert torch.equal(o32.state[params[0]]["exp_avg"], stock["state"][0]["exp_avg"])
    # mismatches are explicit errors
    bad = {"state": native["state"], "param_groups": [{**g, "moments": "int8x64"} for g in native["param_groups"]]}
    with pytest.raises(ValueError, match="unknown moment format"):
        make("e4m3").load_state_dict(bad)
    short = {"state": {0: {**native["state"][0], "exp_avg_scale": native["state"][0]["exp_avg_scale"][:3]}, **{i: native["state"][i] for i in (1, 2)}},
             "param_groups": native["param_groups"]}
    with pytest.raises(ValueError, match="wrong sizes"):
        make("e4m3").load_state_dict(short)


def test_parser_takes_adam8bit_and_refuses_zero1(monkeypatch):
    from a3vlm_amd import main_finetune as mf
    a = mf.get_args_parser().parse_args(["--adam8bit"])
    assert a.adam8bit and not mf.get_args_parser().parse_args([]).adam8bit
    mf.check_args(a)
    bad = mf.get_args_parser().parse_args(["--adam8bit", "--zero1"])
    with pytest.raises(SystemExit, match="--zero1"):
        mf.check_args(bad)
    with pytest.raises(SystemExit, match="--zero1"):
        mf.main(bad)                                   # refused before the GPU is touched
    monkeypatch.setenv("A3V_TORCH_ADAMW", "1")
    with pytest.raises(SystemExit, match="A3V_TORCH_ADAMW"):
        mf.check_args(a)


# ---------------------------------------------------------------------------------------------------------------- quality statement
def quadratic_final_losses(keep_nonzero=True, steps=300, n=4096, rank=8, seed=0, lr0=0.1, span=10):
    """A seeded diagonal-plus-low-rank quadratic 0.5 z'(D + U U')z over n coordinates, z = c x, with per-coordinate GRADIENT scales c^2
    log-uniform over 2^+-span: one block of 256 coordinates really spans the format's range.  AdamW(0.9, 0.95), cosine learning rate
    from lr0 to 0 over ``steps`` steps, fp32 numpy AdamW against the restatement's 8-bit AdamW.  -> (fp32 loss, 8-bit loss, start loss)."""
    rs = np.random.RandomState(seed)
    c = np.exp2(rs.uniform(-span, span, n) / 2)
    d = rs.uniform(0.5, 2.0, n)
    U = rs.randn(n, rank) / np.sqrt(n)
    x0 = (1.0 + 0.5 * rs.randn(n)).astype(np.float32)

    def loss_grad(x):
        z = c * x.astype(np.float64)
        Az = d * z + U @ (U.T @ z)
        return 0.5 * float(z @ Az), (c * Az).astype(np.float32)
    hp = (0.9, 0.95, 1e-8, 0.0)
    x32, m, v = x0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    x8, st = x0.copy(), R.zero_state(n)
    with np.errstate(all="ignore"):
        for t in range(1, steps + 1):
            lr = lr0 * 0.5 * (1 + np.cos(np.pi * (t - 1) / steps))
            x32, m, v = R.adamw_step_fp32(x32, loss_grad(x32)[1], m, v, t, lr, *hp)
            out = R.adamw8_step(x8, loss_grad(x8)[1], *st, t, lr, *hp, keep_nonzero=keep_nonzero)
            x8, st = out[0], out[1:]
    return loss_grad(x32)[0], loss_grad(x8)[0], loss_grad(x0)[0]


# measured with this file (seed 0): fp32 1.44e-08, 8-bit 1.10e-07 from a start of 2.29e+05 -> ratio 7.62, excess 6.62; DESIGN.md 5a
MEASURED_RATIO = 7.62
RATIO_BOUND = 1.0 + 2.0 * (MEASURED_RATIO - 1.0)       # a margin of 2x over the measured excess


def test_quality_on_a_quadratic_that_spans_the_format():
    f32, f8, start = quadratic_final_losses()
    print(f"quadratic: start {start:.4g}  fp32 {f32:.4g}  8-bit {f8:.4g}  ratio {f8 / f32:.4g}  bound {RATIO_BOUND:.4g}")
    assert f32 < 1e-9 * start                          # the problem is solved: the comparison is between two converged runs
    assert f8 / f32 <= RATIO_BOUND
    # the code-0x01 rule is what holds this: without it an element whose r rounds to code 0 divides its m by eps alone
    _, f8_no, _ = quadratic_final_losses(keep_nonzero=False)
    print(f"quadratic without the 0x01 rule: 8-bit {f8_no:.4g}  ratio {f8_no / f32:.4g}")
    assert not f8_no / f32 <= 100 * RATIO_BOUND
