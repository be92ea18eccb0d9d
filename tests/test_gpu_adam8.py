"""-m gpu: the 8-bit AdamW moments on the device.  The quantiser and its inverse are bit-equal to the host restatement
(tests/adam8_ref.py); a3v_adamw8_scaled is bit for bit the sequence a3v_adam8_dequantize -> a3v_adamw_scaled -> a3v_adam8_quantize;
FusedAdamW(moments="e4m3") equals the per-tensor C calls, resumes bit for bit and takes a stock torch.optim.AdamW state; and
main_finetune --adam8bit trains, stays near the fp32 run, reloads its checkpoint byte for byte and logs the same losses after a resume."""
import argparse
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import adam8_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256, 768, 256 * 4099]           # one block / one wave; three blocks; more blocks than the widest grid (4096 waves), odd count
HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.02)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def quantize(L, m, v):
    n = m.numel()
    mq, rq = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ms, rs = torch.empty(n // 256, dtype=torch.float32, device="cuda"), torch.empty(n // 256, dtype=torch.float32, device="cuda")
    L.check(L.load().a3v_adam8_quantize(m.data_ptr(), v.data_ptr(), mq.data_ptr(), ms.data_ptr(), rq.data_ptr(), rs.data_ptr(), n, _stream()), "quantize")
    return mq, ms, rq, rs


def dequantize(L, mq, ms, rq, rs):
    m, v = torch.empty(mq.numel(), dtype=torch.float32, device="cuda"), torch.empty(mq.numel(), dtype=torch.float32, device="cuda")
    L.check(L.load().a3v_adam8_dequantize(mq.data_ptr(), ms.data_ptr(), rq.data_ptr(), rs.data_ptr(), m.data_ptr(), v.data_ptr(), mq.numel(), _stream()),
            "dequantize")
    return m, v


def bits(t):
    """A tensor's bytes on the host (bit-for-bit comparisons: -0.0 != 0.0, NaN == NaN)."""
    return t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy()


def _data(kind, n, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "normal":
        g = (rs.randn(n) * np.exp2(rs.uniform(-6, 6, n))).astype(np.float32)
        m, v = 0.1 * g, 0.05 * g * g
    elif kind == "zero_block":
        g = rs.randn(n).astype(np.float32)
        m, v = 0.1 * g, 0.05 * g * g
        m[:256] = 0
        v[:256] = 0
    elif kind == "outlier":                       # one element 2^20 times the rest: the rest of r rounds to code 0 -> the 0x01 rule
        g = (rs.randn(n) * 1e-3).astype(np.float32)
        g[np.abs(g) < 1e-5] = 1e-5
        g[::256] = np.float32(2.0 ** 20) * np.abs(g).reshape(-1, 256).max(1)
        m, v = g.copy(), g * g
    else:                                         # inf-free extremes near FLT_MIN (subnormals included)
        tiny = np.float32(np.finfo(np.float32).tiny)
        m = (rs.randn(n).astype(np.float32) * tiny * 4).astype(np.float32)
        v = (np.abs(rs.randn(n)).astype(np.float32) * tiny * 4).astype(np.float32)
        v[1::7] = 0
    return np.ascontiguousarray(m, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["normal", "zero_block", "outlier", "flt_min"])
def test_quantize_dequantize_are_the_restatement(lib, n, kind):
    m, v = _data(kind, n)
    want = R.quantize(m, v)
    got = quantize(lib, torch.from_numpy(m).cuda(), torch.from_numpy(v).cuda())
    for name, g, w in zip(("m_q", "m_scale", "r_q", "r_scale"), got, want):
        assert np.array_equal(bits(g), w.view(np.uint8)), (name, int((bits(g) != w.view(np.uint8)).sum()))
    if kind == "outlier":
        assert int(((want[2] & 0x7F) == 1).sum()) >= n - n // 256 - 8          # the case really is about the rule
    dm, dv = dequantize(lib, *got)
    wm, wv = R.dequantize(*want)
    assert np.array_equal(bits(dm), wm.view(np.uint8)) and np.array_equal(bits(dv), wv.view(np.uint8))
    assert bool(torch.isfinite(dm).all()) and bool(torch.isfinite(dv).all())
    # either pair alone: the other's outputs stay untouched
    L = lib.load()
    mq = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    ms = torch.full((n // 256,), 7.0, device="cuda")
    lib.check(L.a3v_adam8_quantize(None, torch.from_numpy(v).cuda().data_ptr(), None, None, mq.data_ptr(), ms.data_ptr(), n, _stream()), "quantize v")
    assert np.array_equal(bits(mq), want[2]) and np.array_equal(bits(ms), want[3].view(np.uint8))


def _zero_state(n):
    return [torch.from_numpy(a).cuda() for a in R.zero_state(n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("with_image", [False, True])
@pytest.mark.parametrize("gscale", [None, 0.37, -1.0, float("nan")])
def test_step_is_dequantize_adamw_quantize(lib, n, with_image, gscale):
    L = lib.load()
    gen = torch.Generator(device="cuda").manual_seed(n + 7)
    p0 = torch.randn(n, device="cuda", generator=gen)
    gs = torch.tensor([gscale], dtype=torch.float32, device="cuda") if gscale is not None else None
    # fused: param, image, codes, scales
    pf, sf = p0.clone(), _zero_state(n)
    imf = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda") if with_image else None
    # sequence
    ps, ss = p0.clone(), _zero_state(n)
    ims = imf.clone() if with_image else None
    hp = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"])
    for step in range(1, 6):
        g = torch.randn(n, device="cuda", generator=gen) * torch.exp2(torch.rand(n, device="cuda", generator=gen) * 16 - 8)
        before = [bits(t) for t in [pf] + sf + ([imf] if with_image else [])]
        lib.check(L.a3v_adamw8_scaled(pf.data_ptr(), g.data_ptr(), sf[0].data_ptr(), sf[1].data_ptr(), sf[2].data_ptr(), sf[3].data_ptr(), n, *hp,
                                      step, _ptr(imf), _ptr(gs), _stream()), "a3v_adamw8_scaled")
        m, v = dequantize(lib, *ss)
        lib.check(L.a3v_adamw_scaled(ps.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hp, step, _ptr(ims), _ptr(gs), _stream()),
                  "a3v_adamw_scaled")
        if gscale is None or gscale >= 0:
            ss = list(quantize(lib, m, v))
        names = ["param", "m_q", "m_scale", "r_q", "r_scale"] + (["image"] if with_image else [])
        for name, a, b in zip(names, [pf] + sf + ([imf] if with_image else []), [ps] + ss + ([ims] if with_image else [])):
            assert np.array_equal(bits(a), bits(b)), (name, step, int((bits(a) != bits(b)).sum()))
        if gscale is not None and not gscale >= 0:                        # negative / NaN: every output untouched
            for name, a, b in zip(names, [pf] + sf + ([imf] if with_image else []), before):
                assert np.array_equal(bits(a), b), (name, step)
    if gscale is None or gscale >= 0:
        assert not np.array_equal(bits(pf), bits(p0)) and bool(torch.isfinite(pf).all())
        assert int((sf[2] & 0x7F).eq(0).sum()) == 0                      # every element has seen a gradient: no r code is 0
        if with_image:
            assert np.array_equal(bits(imf), bits(pf.bfloat16()))


# ---------------------------------------------------------------------------------------------------------------- optimizer level
def _mix(seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(512, 512, device="cuda", generator=gen)), torch.nn.Parameter(torch.randn(300, device="cuda", generator=gen)),
            torch.nn.Parameter(torch.randn(64, 16, device="cuda", generator=gen))]


def _grads(params, step):
    gen = torch.Generator(device="cuda").manual_seed(1000 + step)
    return [torch.randn(p.shape, device="cuda", generator=gen) * torch.exp2(torch.rand(p.shape, device="cuda", generator=gen) * 12 - 6) for p in params]


def _make(params, images=None, **kw):
    from a3vlm_amd.optim import FusedAdamW
    image_of = (lambda p: images.get(id(p))) if images is not None else None
    return FusedAdamW([{"params": params[:1], "weight_decay": HP["wd"]}, {"params": params[1:], "weight_decay": 0.0}], lr=HP["lr"],
                      betas=(HP["b1"], HP["b2"]), eps=HP["eps"], image_of=image_of, **kw)


def _run(opt, params, steps):
    for s in steps:
        for p, g in zip(params, _grads(params, s)):
            p.grad = g
        opt.step()


def test_optimizer_mixes_8bit_and_fp32_state_and_resumes(lib, monkeypatch):
    monkeypatch.setenv("A3V_ADAMW_MULTI", "4096")
    L = lib.load()
    params = _mix()
    start = [p.detach().clone() for p in params]
    image = torch.zeros(512, 512, dtype=torch.bfloat16, device="cuda")
    opt = _make(params, {id(params[0]): image}, moments="e4m3")
    _run(opt, params, (1, 2, 3))
    st = opt.state[params[0]]
    assert sorted(st) == ["exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale", "step"]
    assert st["exp_avg_q"].dtype == torch.uint8 and st["exp_avg_q"].shape == (512, 512) and st["exp_avg_scale"].shape == (1024,)
    for p in params[1:]:
        assert sorted(opt.state[p]) == ["exp_avg", "exp_avg_sq", "step"] and opt.state[p]["exp_avg"].dtype == torch.float32
    # three steps equal the per-tensor C calls
    ref, img_ref = [t.clone() for t in start], torch.zeros_like(image)
    s8 = _zero_state(512 * 512)
    mv = [(torch.zeros_like(t), torch.zeros_like(t)) for t in ref[1:]]
    for s in (1, 2, 3):
        g = _grads(params, s)
        lib.check(L.a3v_adamw8_scaled(ref[0].data_ptr(), g[0].data_ptr(), s8[0].data_ptr(), s8[1].data_ptr(), s8[2].data_ptr(), s8[3].data_ptr(), 512 * 512,
                                      HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], s, img_ref.data_ptr(), None, _stream()), "a3v_adamw8_scaled")
        for t, gg, (m, v) in zip(ref[1:], g[1:], mv):
            lib.check(L.a3v_adamw_scaled(t.data_ptr(), gg.data_ptr(), m.data_ptr(), v.data_ptr(), t.numel(), HP["lr"], HP["b1"], HP["b2"], HP["eps"], 0.0, s,
                                         None, None, _stream()), "a3v_adamw_scaled")
    for p, t in zip(params, ref):
        assert np.array_equal(bits(p), bits(t))
    assert np.array_equal(bits(image), bits(img_ref))
    for k, t in zip(("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale"), s8):
        assert np.array_equal(bits(st[k]), bits(t)), k
    for p, (m, v) in zip(params[1:], mv):
        assert np.array_equal(bits(opt.state[p]["exp_avg"]), bits(m)) and np.array_equal(bits(opt.state[p]["exp_avg_sq"]), bits(v))
    # state_dict -> fresh optimizer -> load_state_dict -> a fourth step is bit-equal to the uninterrupted run
    sd = opt.state_dict()
    assert all(g["moments"] == "e4m3x256" for g in sd["param_groups"])
    params2 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    image2 = image.clone()
    opt2 = _make(params2, {id(params2[0]): image2}, moments="e4m3")
    opt2.load_state_dict(sd)
    _run(opt, params, (4,))
    _run(opt2, params2, (4,))
    for a, b in zip(params, params2):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(image), bits(image2))
    for a, b in zip(params, params2):
        assert opt.state[a].keys() == opt2.state[b].keys()
        for k in opt.state[a]:
            assert np.array_equal(bits(opt.state[a][k]), bits(opt2.state[b][k])), k
    # an fp32 FusedAdamW handed the native dict dequantises it
    opt32 = _make([torch.nn.Parameter(p.detach().clone()) for p in params], moments="fp32")
    opt32.load_state_dict(sd)
    p32 = opt32.param_groups[0]["params"][0]
    m, v = dequantize(lib, *[sd["state"][0][k].view(-1) for k in ("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale")])
    assert np.array_equal(bits(opt32.state[p32]["exp_avg"]), bits(m)) and np.array_equal(bits(opt32.state[p32]["exp_avg_sq"]), bits(v))


def test_optimizer_takes_a_stock_adamw_state(lib, monkeypatch):
    monkeypatch.setenv("A3V_ADAMW_MULTI", "4096")
    params = _mix(1)
    stock = torch.optim.AdamW([{"params": params[:1], "weight_decay": HP["wd"]}, {"params": params[1:], "weight_decay": 0.0}], lr=HP["lr"],
                              betas=(HP["b1"], HP["b2"]), eps=HP["eps"])
    _run(stock, params, (1, 2))
    sd = stock.state_dict()
    a = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = _make(a, moments="e4m3")
    opt.load_state_dict(sd)
    assert "exp_avg_q" in opt.state[a[0]] and "exp_avg" not in opt.state[a[0]] and float(opt.state[a[0]]["step"]) == 2
    assert "exp_avg" in opt.state[a[1]] and "exp_avg" in opt.state[a[2]]
    _run(opt, a, (3,))
    # "quantise, then step" with the C calls
    L = lib.load()
    ref = params[0].detach().clone()
    s8 = list(quantize(lib, sd["state"][0]["exp_avg"].reshape(-1).contiguous(), sd["state"][0]["exp_avg_sq"].reshape(-1).contiguous()))
    g = _grads(params, 3)[0]
    lib.check(L.a3v_adamw8_scaled(ref.data_ptr(), g.data_ptr(), s8[0].data_ptr(), s8[1].data_ptr(), s8[2].data_ptr(), s8[3].data_ptr(), ref.numel(),
                                  HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], 3, None, None, _stream()), "a3v_adamw8_scaled")
    assert np.array_equal(bits(a[0]), bits(ref))
    for k, t in zip(("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale"), s8):
        assert np.array_equal(bits(opt.state[a[0]][k]), bits(t)), k


class _EngineWithTransposedImages:
    """The optimizer hand-off surface of a TrainEngine that keeps W^T images current (full fine-tune, NT input gradients)."""

    def __init__(self, p):
        self.img, self.img_t = torch.zeros(p.shape, dtype=torch.bfloat16, device="cuda"), torch.zeros(p.shape[1], p.shape[0], dtype=torch.bfloat16, device="cuda")

    def sync_optimizer(self):
        pass

    def image_sink(self, p):
        return self.img

    def image_sink_t(self, p):
        return self.img_t, self.img_t.shape[1]

    def images_adopted(self, *a):
        pass


def test_transposed_image_sink_is_refused_with_the_way_out(lib, monkeypatch):
    from a3vlm_amd.optim import FusedAdamW
    monkeypatch.setenv("A3V_ADAMW_MULTI", "4096")
    p = torch.nn.Parameter(torch.randn(128, 128, device="cuda"))
    before = bits(p)
    opt = FusedAdamW([p], lr=1e-3, engine=_EngineWithTransposedImages(p), moments="e4m3")
    p.grad = torch.randn_like(p)
    with pytest.raises(RuntimeError, match="nn_dgrad"):
        opt.step()
    torch.cuda.synchronize()
    assert np.array_equal(bits(p), before)


# ---------------------------------------------------------------------------------------------------------------- trainer level
def _train(tmp_path, name, extra_args, capsys, interval=4):
    """main_finetune on the tiny synthetic configuration of test_gpu_trainer.py, full fine-tune, 8 optimizer steps, every step logged.
    --precision tf32: the checkpoint then holds the fp32 masters as they are (under bf16 save_checkpoint rounds them to bf16, as the
    reference does, and no resume of any optimizer can be bit for bit).
    -> ({step: loss string}, output dir)"""
    from a3vlm_amd import main_finetune as mf
    gd = os.path.join(ROOT, "tests", "golden")
    vit = tmp_path / "vit.json"
    vit.write_text(json.dumps(dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1)))
    out = tmp_path / name
    argv = ["--llama_type", "llama_ens5", "--llama_config", os.path.join(gd, "tiny_params.json"), str(vit),
            "--tokenizer_path", os.path.join(gd, "tokenizer.model"), "--batch_size", "2", "--accum_iter", "1", "--epochs", "1",
            "--warmup_epochs", "0.25", "--lr", "1e-3", "--min_lr", "0", "--clip_grad", "8", "--weight_decay", "0.02",
            "--max_words", "120", "--precision", "tf32", "--output_dir", str(out), "--synthetic", "16", "--num_workers", "0",
            "--dialog", "--model_parallel_size", "1", "--save_iteration_interval", str(interval)] + extra_args
    args = argparse.ArgumentParser(parents=[mf.get_args_parser()]).parse_args(argv)
    args.print_freq = 1
    args.loss_trace = []                                   # (step, loss as the trainer read it back), unrounded
    os.makedirs(out, exist_ok=True)
    capsys.readouterr()
    old = torch.get_default_dtype()
    try:
        mf.main(args)
    finally:
        torch.set_default_dtype(old)
    log = capsys.readouterr().out
    assert set(re.findall(r"\[\d+/(\d+)\] lr:", log)) == {"8"}, log[-2000:]               # 8 optimizer steps per epoch
    losses = {int(m.group(1)): m.group(2) for m in re.finditer(r"\[(\d+)/8\] lr: \S+ closs: (\S+)", log)}
    assert sorted(losses) == [s for s, _ in args.loss_trace]
    return losses, dict(args.loss_trace), out


def _same_tree(x, y, name):
    def walk(u, w, path):
        if torch.is_tensor(u):
            assert torch.is_tensor(w) and u.dtype == w.dtype and u.shape == w.shape and np.array_equal(bits(u), bits(w)), path
        elif isinstance(u, dict):
            assert u.keys() == w.keys(), path
            for k in u:
                walk(u[k], w[k], f"{path}/{k}")
        elif isinstance(u, (list, tuple)):
            assert len(u) == len(w), path
            for i, (p, q) in enumerate(zip(u, w)):
                walk(p, q, f"{path}/{i}")
        else:
            assert u == w or (isinstance(u, float) and math.isnan(u) and math.isnan(w)), path
    walk(x, y, name)


# |loss(step 8, --adam8bit) - loss(step 8, fp32 moments)| measured on an MI355X with this test, from the unrounded losses the trainer
# read back: fp32 moments 5.36740779876709, 8-bit moments 5.367241859436035 (step 1: 5.448187828063965 in both); DESIGN.md 5a.  The
# bound is the measured value with the margin of 2x of the CPU quadratic.
MEASURED_STEP8_DIFF = 1.6594e-4
STEP8_BOUND = 2.0 * MEASURED_STEP8_DIFF
LR = 1e-3                                 # --lr of _train: no step's learning rate is above it


def _checkpoint(out, it):
    d = out / f"epoch0-iter{it}"
    model = torch.load(d / "consolidated.00-of-01.model.pth", weights_only=False)["model"]
    opt = torch.load(d / "consolidated.00-of-01.optimizer.pth", weights_only=False)["optimizer"]
    # the optimizer's parameter order: util.add_weight_decay over the trainable parameters (the ViT is frozen)
    names = [k for k in model if ".clip." not in k]
    nodecay = [k for k in names if k.endswith(".bias") or k.endswith("norm.weight")]
    order = nodecay + [k for k in names if k not in nodecay]
    assert [len(g["params"]) for g in opt["param_groups"]] == [len(nodecay), len(names) - len(nodecay)]
    return model, opt, order


def test_trainer_adam8bit(tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("A3V_ADAMW_MULTI", "1024")          # the tiny model's matrices are far below the production threshold of 2^20 elements
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "A3V_TORCH_ADAMW", "A3V_ADAMW_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    _, t32, _ = _train(tmp_path, "fp32", [], capsys)
    _, t8, out8 = _train(tmp_path, "adam8", ["--adam8bit"], capsys, interval=1)          # a checkpoint after every step
    with capsys.disabled():
        print("\nfp32 moments:", t32)
        print("8-bit moments:", t8)
    for t in (t32, t8):
        assert sorted(t) == list(range(1, 9)) and all(math.isfinite(x) for x in t.values())
        assert t[8] < t[1]
    diff = abs(t8[8] - t32[8])
    with capsys.disabled():
        print(f"step-8 loss: fp32 {t32[8]!r}  8-bit {t8[8]!r}  |difference| {diff:.4e}  bound {STEP8_BOUND:.4e}")
    assert diff <= STEP8_BOUND
    # the checkpoints hold the native state
    model4, sd, order = _checkpoint(out8, 3)
    assert all(g["moments"] == "e4m3x256" for g in sd["param_groups"])
    kinds = {("exp_avg_q" in s) for s in sd["state"].values()}
    assert kinds == {True, False}                           # matrices in 8 bits, norms and other small tensors in fp32
    # the checkpoint resumes bit for bit: a fresh optimizer that loads the step-4 file holds, and writes, exactly that state
    from a3vlm_amd.optim import FusedAdamW
    shapes = {i: st["exp_avg_q"].shape if "exp_avg_q" in st else st["exp_avg"].shape for i, st in sd["state"].items()}
    fresh = FusedAdamW([{**{k: v for k, v in g.items() if k not in ("params", "moments")},
                         "params": [torch.nn.Parameter(torch.zeros(shapes[i], device="cuda")) for i in g["params"]]} for g in sd["param_groups"]],
                       moments="e4m3")
    fresh.load_state_dict(sd)
    _same_tree(fresh.state_dict(), sd, "optimizer")

    # The trainer resumed from the step-4 checkpoint, against the uninterrupted run.  What can be bit-equal is held bit-equal.  The
    # engine's backward sums SOME gradients with fp32 atomics (a3v_train.hip: norm and LayerNorm weights, the embedding table, the
    # start / end image rows, bias column sums), so two identical uninterrupted runs agree in those tensors only to the last bits, and
    # from the second step on in everything, because every gradient depends on every weight.  Hence:
    #  * step 5, the first after the resume, starts from byte-equal weights and state: its loss (a forward) is bit-equal, and so are
    #    the weights, codes and scales after it of every tensor whose gradient has one fixed summation order -- all 8-bit tensors
    #    but the embedding table -- and every step count;
    #  * the tensors with atomics after step 5: an fp32 sum of N addends taken in another order moves by at most N 2^-24 sum|a_i|;
    #    with N <= 512 rows and a cancellation sum|a_i| / |sum a_i| <= 2^8 (assumed) that is a relative 2^-7 of the gradient, and
    #    AdamW turns a relative change rho of this step's gradient into at most 3 lr rho of the weight ((1-b1) / bc1 / sqrt(1-b2) *
    #    sqrt(bc2) = 1.05 for the first moment, the same order for the second): 0.025 lr.  The embedding table has 8-bit state, where
    #    such a change may also flip one code of each moment, 1/8 of |m^| / r^ <= 1.35 each: 0.4 lr.  A lost or shifted moment or a
    #    step count off by one moves an element by the order of lr itself;
    #  * steps 6-8: the losses within 1e-5, twenty units in the last place of an fp32 loss of 5.4 (identical uninterrupted runs: one
    #    unit, measured) and a seventeenth of the smallest real effect known here, fp32 against 8-bit moments at step 8 (1.7e-4).
    _, tr, outr = _train(tmp_path, "resumed", ["--adam8bit", "--resume", str(out8 / "epoch0-iter3")], capsys, interval=1)
    with capsys.disabled():
        print("resumed:", tr)
    assert sorted(tr) == [5, 6, 7, 8]
    assert tr[5] == t8[5]
    (mu, ou, order), (mr, orr, _) = _checkpoint(out8, 4), _checkpoint(outr, 4)
    _same_tree(ou["param_groups"], orr["param_groups"], "param_groups")
    n_exact, worst = 0, {}
    for i, name in enumerate(order):
        su, sr = ou["state"][i], orr["state"][i]
        assert su.keys() == sr.keys() and float(su["step"]) == float(sr["step"]) == 5.0, name
        if "exp_avg_q" in su and "tok_embeddings" not in name:
            assert not np.array_equal(bits(mu[name]), bits(model4[name])), name             # step 5 did move it
            assert np.array_equal(bits(mu[name]), bits(mr[name])), name
            _same_tree(su, sr, name)
            n_exact += 1
        else:
            worst[name] = float((mu[name].float() - mr[name].float()).abs().max())
            assert worst[name] <= (0.4 if "exp_avg_q" in su else 0.025) * LR, (name, worst[name])
    with capsys.disabled():
        print(f"after step 5: {n_exact} tensors bit-equal (weights, codes, scales); the others' largest |difference|: {worst}")
    assert n_exact >= 16                                   # 14 decoder matrices, the head, the projector's linear
    for s in (6, 7, 8):
        assert abs(tr[s] - t8[s]) <= 1e-5, (s, tr[s], t8[s])
