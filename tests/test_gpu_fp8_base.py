"""-m gpu: the LoRA step on a frozen fp8 (e4m3, per-row scales) base -- ``quantize_base_weights("fp8")``, ``main_finetune --base_fp8``
(DESIGN.md 7c).  The reference has no fp8 path, so parity is stated against tests/fp8_base_ref.py: an fp64 step on the dequantised base
Wd = Wq * sw that fake-quantises exactly where the engine quantises."""
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import fp8_base_ref as R
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.LLM import llama_ens5_peft as peft
from a3vlm_amd.optim import FusedAdamW
from a3vlm_amd.train import TrainEngine
from a3vlm_amd.util import promote_trainable_params_to_fp32
from oracle import ref_cpu
from test_fp8_base_cpu import exact_problem
from test_gpu_qlora import BIG, NORM_REL, RANK

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
SENT = 0xA5            # sentinel byte of the quantiser's destinations
BASE = (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight")


def _is_base(k):
    return k.startswith("layers.") and k.endswith(BASE)


def _weights(cfg):
    oargs = ref_cpu.OracleArgs(**cfg)
    sd = ref_cpu.make_decoder_weights(oargs, seed=3, std=0.05)
    lsd = ref_cpu.make_lora_weights(oargs, RANK, seed=6, std_a=0.05, std_b=0.05)
    return oargs, sd, lsd


def _model(cfg, sd, lsd, mode="fp8"):
    """mode "fp8": quantised; None: the bf16 peft model on ``sd`` as given."""
    m = peft.Transformer(peft.ModelArgs(**cfg, lora_rank=RANK), with_visual=False)
    m.load_state_dict({**sd, **lsd}, strict=True)
    train = m.get_trainable_params()
    for n, p in m.named_parameters():
        p.requires_grad = n in train
    m.to(BF).to(DEV)
    if mode:
        m.quantize_base_weights(mode)
    return m


def _q8_cpu(m):
    return {k: (wq.cpu(), sw.cpu()) for k, (wq, sw, _) in m._q8base.items()}


def _batch(seed=13, B=3, T=47, V=320, lead=6):
    g = torch.Generator().manual_seed(seed)
    ex = torch.randint(3, V, (B, T), generator=g)
    ex[:, 0] = 1
    lab = ex.clone()
    lab[:, :lead] = 0
    return ex, lab


# ---------------------------------------------------------------------------------------------------------------- 1. the quantiser
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("cols,cols_pad", [(128, 128), (320, 384), (4096, 4096), (22016, 22016)])
@pytest.mark.parametrize("rows", [1, 17, 300])
def test_quantize_rows_fp8_cs(rows, cols, cols_pad, dtype):
    """scale = max|x cs| / 448 per row, q = fp8(x cs / scale), zero bytes up to cols_pad; nothing outside the window is touched.
    (22016 columns: the wide form of the kernel, rows beyond 16384 columns -- the fused w1|w3 gradient of the 7B model.)"""
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x = (torch.randn(rows, cols, generator=g) * torch.rand(rows, 1, generator=g) * 3).to(dtype)
    x[rows // 2] = 0
    cs = torch.rand(cols, generator=g) * 0.1 + 1e-3
    buf = torch.full((rows + 4, cols_pad + 64), SENT, dtype=torch.uint8, device=DEV)
    sb = torch.full((rows + 4,), -7.0, dtype=torch.float32, device=DEV)
    q, s = buf[2:2 + rows, :cols_pad], sb[2:2 + rows]
    ops.quantize_rows_fp8_cs(x.to(DEV), cs.to(DEV), q, s)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[2:2 + rows, :cols_pad] = False
    assert bool((buf[mask] == SENT).all()) and bool((sb[:2] == -7).all()) and bool((sb[2 + rows:] == -7).all())
    assert int(q[:, cols:].sum()) == 0
    y = x.float() * cs[None, :]
    amax = y.abs().amax(dim=1)
    want_s = amax.clamp_min(1e-12) / 448
    assert torch.allclose(s.cpu(), want_s, rtol=1e-6, atol=0)
    d = R.dequantize_rows(q[:, :cols].cpu(), s.cpu())
    assert torch.isfinite(d).all()
    step = torch.maximum(y.abs() * 2 ** -4, want_s[:, None] * 2 ** -10)     # half ulp of 3 mantissa bits / half a subnormal step
    assert bool(((d - y).abs() <= step * 1.001).all())
    nz = amax > 0
    assert torch.allclose(d.abs().amax(dim=1)[nz], amax[nz], rtol=1e-6, atol=0)
    # against the helper's bytes: equal except where y / scale sits on a rounding boundary of the two divisions (x * (1 / s) here)
    wq, ws = R.quantize_rows_cs(x, cs, cols_pad)
    assert float((wq != q.cpu()).float().mean()) < 1e-3


def test_quantize_rows_fp8_cs_refusals_leave_the_buffers_untouched():
    x = torch.ones(4, 320, dtype=BF, device=DEV)
    cs = torch.ones(320, device=DEV)
    q = torch.full((4, 384), SENT, dtype=torch.uint8, device=DEV)
    s = torch.full((4,), -7.0, device=DEV)
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    call = lambda xp, ldx, qp, ldq, cols, pad, dt: L.a3v_quantize_rows_fp8_cs(xp, ldx, cs.data_ptr(), qp, ldq, s.data_ptr(), 4, cols, pad, dt, st)
    assert call(x.data_ptr(), 320, q.data_ptr(), 384, 316, 384, 0) == -1          # cols % 8
    assert call(x.data_ptr(), 320, q.data_ptr(), 384, 320, 312, 0) == -1          # cols_pad < cols
    assert call(x.data_ptr(), 320, q.data_ptr(), 384, 320, 392, 0) == -1          # cols_pad % 16 / beyond ldq
    assert call(x.data_ptr(), 320, q.data_ptr() + 8, 384, 320, 368, 0) == -1      # q not 16-byte aligned
    assert call(x.data_ptr(), 320, q.data_ptr(), 384, 320, 384, 7) == -2          # dtype
    assert call(None, 320, q.data_ptr(), 384, 320, 384, 0) == -3
    big = torch.ones(1, 32776, dtype=BF, device=DEV)        # beyond the 32768 columns one pass holds
    assert L.a3v_quantize_rows_fp8_cs(big.data_ptr(), 32776, cs.data_ptr(), q.data_ptr(), 32784, s.data_ptr(), 1, 32776, 32784, 0, st) == -1
    torch.cuda.synchronize()
    assert bool((q == SENT).all()) and bool((s == -7).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the exact linear
class _OneGroup:
    """The least of a model the engine's base-product helpers read: one fp8 image group under the key ``wo.0``."""

    def __init__(self, w):
        N, K = w.shape
        wq = torch.empty(N, K, dtype=torch.uint8, device=DEV)
        sw = torch.empty(N, dtype=torch.float32, device=DEV)
        ops.quantize_rows_fp8(w.to(BF).to(DEV), wq, sw)
        wqt = torch.zeros(K, (N + 127) // 128 * 128, dtype=torch.uint8, device=DEV)
        wqt[:, :N] = wq.t()
        self._q8base = {"wo.0": (wq, sw, wqt)}
        self._device = torch.device(DEV)
        self.lora_rank = 0


@pytest.mark.parametrize("M", [3, 47])
def test_exact_linear_forward_and_input_gradient(M):
    """Engine-level base product and input gradient on inputs every quantisation represents exactly: bit-equal to bf16 of the fp64
    product (N = 320 is no multiple of 128: the pad of the byte transpose and of the gradient rows must be zero)."""
    N, K = 320, 256
    w, wcode, sw, x, dy, _ = exact_problem(M, N, K, seed=M)
    mdl = _OneGroup(w)
    assert torch.equal(mdl._q8base["wo.0"][1].cpu(), sw) and torch.equal(R.byte_values(mdl._q8base["wo.0"][0].cpu()), wcode.double())
    eng = TrainEngine(mdl, BF)
    assert eng._q8base() and eng._kext() == 0
    y = torch.empty(M, N, dtype=BF, device=DEV)
    eng._base_fwd_fp8("wo.0", x.to(BF).to(DEV), y)
    assert torch.equal(y.cpu(), (x.double() @ w.double().t()).to(BF))
    dx = torch.empty(M, K, dtype=BF, device=DEV)
    eng._dgrad_w(dy.to(BF).to(DEV), "wo.0", dx)
    assert torch.equal(dx.cpu(), (dy.double() @ w.double()).to(BF))


# ---------------------------------------------------------------------------------------------------------------- 3. the fused qkv form
@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
def test_gemm_qkv_rope_fp8_train_equals_the_unfused_sequence(hd, with_delta):
    B, S, H, Hkv, K, Smax = 2, 47, 4, 2, 256, 64
    N = (H + 2 * Hkv) * hd
    g = torch.Generator().manual_seed(hd + with_delta)
    x = torch.randn(B * S, K, generator=g).to(BF).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV)
    delta = (torch.randn(B * S, N, generator=g) * 0.1).to(BF).to(DEV)
    xq, sx = torch.empty(B * S, K, dtype=torch.uint8, device=DEV), torch.empty(B * S, device=DEV)
    wq, sw = torch.empty(N, K, dtype=torch.uint8, device=DEV), torch.empty(N, device=DEV)
    ops.quantize_rows_fp8(x, xq, sx)
    ops.quantize_rows_fp8(w, wq, sw)
    m = plugin.Transformer(plugin.ModelArgs(dim=H * hd, n_layers=1, n_heads=H, n_kv_heads=Hkv, vocab_size=64, multiple_of=64, max_seq_len=Smax))
    m.to(BF).to(DEV)
    cs = m._cos_sin_dev()
    fill = lambda *s: torch.full(s, -7.0, dtype=BF, device=DEV)
    # the unfused sequence
    qkv = torch.empty(B * S, N, dtype=BF, device=DEV)
    ops.gemm_nt_fp8(xq, sx, wq, sw, qkv)
    if with_delta:
        ops.add2d(qkv, delta)
    q0, k0, v0 = fill(B * S, H * hd), fill(B, Hkv, Smax, hd), fill(B, Hkv, hd, Smax)
    ops.rope_kvcache(qkv, q0, k0, v0, cs, B, S, H, Hkv, hd, 0, 0)
    vrows0 = qkv[:, (H + Hkv) * hd:].clone()
    # fused; delta lives in the buffer whose v columns receive v_rows, as in the engine
    buf = delta.clone() if with_delta else fill(B * S, N)
    q1, k1, v1 = fill(B * S, H * hd), fill(B, Hkv, Smax, hd), fill(B, Hkv, hd, Smax)
    ops.gemm_qkv_rope_fp8_train(xq, sx, wq, sw, q1, k1, v1, cs, B, S, H, Hkv, hd, 0, 0, v_rows=buf[:, (H + Hkv) * hd:],
                                delta=buf if with_delta else None)
    assert torch.equal(q1, q0) and torch.equal(k1, k0) and torch.equal(v1, v0)
    assert torch.equal(buf[:, (H + Hkv) * hd:], vrows0)
    assert bool((k1[:, :, S:] == -7).all()) and bool((v1[:, :, :, S:] == -7).all())      # cache positions >= S untouched


# ---------------------------------------------------------------------------------------------------------------- 4. the step
def _run_steps(m, batches, recompute):
    """two forward / backward steps with one FusedAdamW step on the ADAPTERS between them (tests/test_gpu_qlora.py::_run_steps and its
    reason), on each batch: {batch index: [(loss, {name: grad})] x 2}; the optimizer step is only taken on the first batch's run."""
    promote_trainable_params_to_fp32(m)
    train = m.get_trainable_params()
    eng = TrainEngine(m, BF, recompute=recompute)
    opt = FusedAdamW([p for n, p in m.named_parameters() if p.requires_grad and "lora_" in n], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.0,
                     engine=eng)
    out = []
    for step, (ex, lab) in enumerate(batches):
        loss = float(eng.forward_loss(ex.to(DEV), lab.to(DEV), None))
        eng.backward(1.0)
        out.append((loss, {n: p.grad.float().cpu().clone() for n, p in train.items()},
                    {n: p.detach().double().cpu().clone() for n, p in m.named_parameters()}))
        if step + 1 < len(batches):
            opt.step()
            m.zero_grad(set_to_none=True)
    return out, eng


@pytest.fixture(scope="module")
def step_reference():
    """(weights, the two batches, cache of fp64 references keyed by the adapter state they were computed for)."""
    oargs, sd, lsd = _weights(BIG)
    ex, lab = _batch()
    lab2 = torch.zeros_like(lab)
    lab2[0, 20], lab2[1, 33], lab2[2, 46] = ex[0, 20], ex[1, 33], ex[2, 46]      # three labelled rows: the <= 16-row tail
    return oargs, sd, lsd, [(ex, lab), (ex, lab2)], {}


def _reference(oargs, q8, params64, ex, lab, train):
    ps = {k: v.clone().requires_grad_(k in train) for k, v in params64.items()}
    loss = R.step_loss(oargs, ps, q8, ex, lab)
    loss.backward()
    return float(loss.detach()), {k: ps[k].grad for k in train}


@pytest.mark.parametrize("recompute", [True, False])
def test_fp8_base_step_against_the_fake_quant_reference(step_reference, recompute):
    """Loss within 2e-2 relative and gradient cosine > 0.98 for every trainable tensor (the project's bf16-step bounds) against the
    fp64 reference that models every quantisation on the same Wd -- what is left is bf16 rounding and the e4m3 rounding flips it
    causes.  Step 0: 3 x 47 with six ignored leading labels; step 1 (after one adapter step): three labelled rows only.  Two runs
    are bit-equal in step 0 (norm weight gradients within NORM_REL); the second step's loss differs from the first."""
    oargs, sd, lsd, batches, cache = step_reference
    runs = [_run_steps(_model(BIG, sd, lsd), batches, recompute) for _ in range(2)]
    (got, eng), (got2, _) = runs
    assert eng._q8base() and eng._kext() == 0 and eng.recompute == recompute
    q8 = _q8_cpu(eng.m)
    train = set(eng.m.get_trainable_params())
    cos = lambda x, y: float(torch.dot(x.flatten().double(), y.flatten().double()) / (x.double().norm() * y.double().norm() + 1e-300))
    for step, (ex, lab) in enumerate(batches):
        loss, grads, params = got[step]
        want_loss, want = _reference(oargs, q8, params, ex, lab, train)
        worst = min((cos(grads[n], want[n]), n) for n in train)
        print(f"\n[fp8 base step] recompute={recompute} step {step}: loss {loss!r} want {want_loss!r} "
              f"(rel {abs(loss - want_loss) / abs(want_loss):.3e}); worst gradient cosine {worst}")
        assert abs(loss - want_loss) < 2e-2 * abs(want_loss)
        for n in train:
            assert cos(grads[n], want[n]) > 0.98, (step, n, cos(grads[n], want[n]))
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-30))
    assert got[0][0] == got2[0][0]
    for n in train:
        if n.endswith("norm.weight"):
            assert rel(got[0][1][n], got2[0][1][n]) <= NORM_REL, n
        else:
            assert torch.equal(got[0][1][n], got2[0][1][n]), n
    # the optimizer's adapter sinks are found: the same batch after the step gives another loss
    loss_again = float(eng.forward_loss(batches[0][0].to(DEV), batches[0][1].to(DEV), None))
    assert loss_again != got[0][0]


# ---------------------------------------------------------------------------------------------------------------- 5. memory and state
def test_fp8_base_memory_and_state_dict():
    args = peft.ModelArgs(dim=1024, n_layers=2, n_heads=8, n_kv_heads=8, vocab_size=1024, multiple_of=256, max_seq_len=128, lora_rank=RANK)
    ex, lab = _batch(B=2, T=33, V=1024)
    m = peft.Transformer(args).to(BF).to(DEV)
    for n, p in m.named_parameters():
        p.requires_grad = n in m.get_trainable_params()
    promote_trainable_params_to_fp32(m)
    eng = TrainEngine(m, BF, recompute=True)
    eng.forward_loss(ex.to(DEV), lab.to(DEV), None)
    eng.backward(1.0)
    bf16_held = eng.weight_image_bytes(head=False)
    del eng
    names = [n for n in m.state_dict() if _is_base(n) and "lora_" not in n]
    assert len(names) == 2 * 7
    n_params = sum(m.state_dict()[n].numel() for n in names)
    n_rows = sum(m.state_dict()[n].shape[0] for n in names)
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    m.quantize_base_weights("fp8")
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    # 2 B per parameter of bf16 weights became 2 B per parameter of images plus the scales: the model did not grow (the caching
    # allocator hands out large blocks with up to 1 MiB of unsplit remainder each, 16 images here: bounded by a tenth of the weights)
    assert after - before <= 4 * n_rows + 0.1 * 2 * n_params, (before, after)
    for lyr in m.layers:
        for mod in (lyr.attention.wq, lyr.attention.wk, lyr.attention.wv, lyr.attention.wo, lyr.feed_forward.w1, lyr.feed_forward.w2,
                    lyr.feed_forward.w3):
            assert not hasattr(mod, "weight")                       # no bf16 decoder weight is alive
    sdq = m.state_dict()
    assert not any(n in sdq for n in names)
    assert {"layers.0.attention_norm.weight", "norm.weight", "tok_embeddings.weight", "output.weight", "layers.1.feed_forward.w2.lora_a.weight",
            "layers.0.attention.wq.lora_b.weight"} <= set(sdq)
    eng = TrainEngine(m, BF, recompute=True)
    assert eng.weight_image_bytes(head=False) == 2 * n_params + 4 * n_rows        # every N here is a multiple of 128: no pad bytes
    loss = float(eng.forward_loss(ex.to(DEV), lab.to(DEV), None))
    eng.backward(1.0)
    assert loss == loss
    assert eng.weight_image_bytes(head=False) == 2 * n_params + 4 * n_rows
    assert eng.weight_image_bytes(head=False) <= bf16_held // 2 + 4 * n_rows and bf16_held >= 4 * n_params
    assert eng.weight_image_bytes() > eng.weight_image_bytes(head=False)          # + the bf16 head's images


# ---------------------------------------------------------------------------------------------------------------- 6. inference and merge
def test_fp8_base_inference_and_merge_equal_the_bf16_model_on_wd():
    oargs, sd, lsd = _weights(BIG)
    mq = _model(BIG, sd, lsd)
    wd = R.wd_state(_q8_cpu(mq), sd)
    md = _model(BIG, {**sd, **wd}, lsd, mode=None)
    ex, _ = _batch(seed=21, B=3, T=32)
    with torch.no_grad():
        pq = mq.forward_inference(ex[:, :23].to(DEV), 0)
        pd = md.forward_inference(ex[:, :23].to(DEV), 0)
        assert torch.equal(pq, pd) and bool(torch.isfinite(pq).all())
        tq, td = ex[:, 23:24].to(DEV), ex[:, 23:24].to(DEV)
        for pos in range(23, 31):                                    # 8 greedy decode steps
            dq, dd = mq.forward_inference(tq, pos), md.forward_inference(td, pos)
            assert torch.equal(dq, dd)
            tq, td = dq.argmax(-1).view(3, 1), dd.argmax(-1).view(3, 1)
        assert torch.equal(mq(ex.to(DEV)), md(ex.to(DEV)))         # teacher-forced forward (all positions)
    mq.merge_adapters()
    md.merge_adapters()
    assert mq._q8base is None and not mq.is_peft
    sq, sdd = mq.state_dict(), md.state_dict()
    assert set(sq) == set(sdd) and not any("lora_" in k for k in sq)
    for k in sq:
        assert sq[k].dtype == sdd[k].dtype and torch.equal(sq[k], sdd[k]), k


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_fp8_base_refusals_leave_the_model_usable():
    oargs, sd, lsd = _weights(BIG)
    ex, lab = _batch(B=2, T=24)
    m = _model(BIG, sd, lsd)
    promote_trainable_params_to_fp32(m)
    with pytest.raises(ValueError, match="ZeRO-1"):
        TrainEngine(m, BF, zero1_world=2)
    with pytest.raises(ValueError, match="bf16 compute"):
        TrainEngine(m, torch.float32)
    with pytest.raises(RuntimeError, match="already fp8"):
        m.quantize_base_weights("nf4")
    with pytest.raises(RuntimeError, match="already fp8"):
        m.quantize_base_weights("fp8")
    loss = float(TrainEngine(m, BF).forward_loss(ex.to(DEV), lab.to(DEV), None))
    assert loss == loss
    m4 = _model(BIG, sd, lsd, mode="nf4")
    with pytest.raises(RuntimeError, match="already NF4"):
        m4.quantize_base_weights("fp8")
    assert m4._q8base is None and m4._q4 is not None
    assert not hasattr(plugin.Transformer, "quantize_base_weights")      # a non-peft model has no frozen base to quantise (--base_fp8 refuses it)
    cfg = dict(BIG, dim=320, n_heads=5, n_kv_heads=5, multiple_of=128)
    o2, sd2, lsd2 = _weights(cfg)
    m2 = _model(cfg, sd2, lsd2, mode=None)
    with pytest.raises(ValueError, match="K % 128"):
        m2.quantize_base_weights("fp8")
    assert m2._q8base is None and hasattr(m2.layers[1].feed_forward.w2, "weight")
    with torch.no_grad():
        assert bool(torch.isfinite(m2.forward_inference(ex[:, :8].to(DEV), 0)).all())


# ---------------------------------------------------------------------------------------------------------------- 8. trainer entry
@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    """a base checkpoint folder (decoder + zero adapters) written by checkpoint.save_checkpoint, and the config / tokenizer it needs"""
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    tmp = tmp_path_factory.mktemp("fp8base")
    cfg = {k: v for k, v in BIG.items() if k not in ("vocab_size", "max_seq_len")}
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps({**cfg, "lora_rank": RANK}))
    mm = MetaModel("llama_ens5_peft", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=64)
    V = mm.tokenizer.n_words
    oargs = ref_cpu.OracleArgs(vocab_size=V, max_seq_len=64, **cfg)
    sd = ref_cpu.make_decoder_weights(oargs, seed=3, std=0.05)
    mm.llma.load_state_dict(sd, strict=False)
    ckdir = ck.save_checkpoint(str(tmp / "base"), types.SimpleNamespace(precision="bf16", only_save_trainable=False), mm, None, None, None, epoch=0)
    return cfgp, ckdir, tmp


def _quantised_meta(cfgp, ckdir, adapters=None):
    from a3vlm_amd.checkpoint import load_tensor_parallel_model_list
    from a3vlm_amd.model.meta import MetaModel
    old = torch.get_default_dtype()
    torch.set_default_dtype(BF)
    try:
        with torch.device(DEV):
            mm = MetaModel("llama_ens5_peft", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=64)
    finally:
        torch.set_default_dtype(old)
    promote_trainable_params_to_fp32(mm)
    load_tensor_parallel_model_list(mm, [ckdir])
    mm.llma.quantize_base_weights("fp8")
    if adapters is not None:                      # resume: base, quantise, then the adapters by name
        res = load_tensor_parallel_model_list(mm, [adapters])
        assert res["unexpected_keys"] == [], res
    return mm


def test_main_finetune_base_fp8_trains_saves_adapters_and_resumes(base_ckpt):
    cfgp, ckdir, tmp = base_ckpt
    out = tmp / "out"
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.main_finetune", "--llama_type", "llama_ens5_peft", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--base_fp8", "--only_save_trainable",
           "--synthetic", "4", "--batch_size", "2", "--accum_iter", "1", "--epochs", "1", "--warmup_epochs", "0", "--lr", "1e-3",
           "--max_words", "48", "--no_visual", "--num_workers", "0", "--precision", "bf16", "--output_dir", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(x) for x in re.findall(r"closs: ([-+.\deE]+|nan|inf)", r.stdout)]
    assert losses and all(torch.isfinite(torch.tensor(losses))), r.stdout[-2000:]
    saved = torch.load(out / "epoch0" / "consolidated.00-of-01.model.pth", weights_only=False)["model"]
    assert "llma.layers.0.attention.wq.lora_a.weight" in saved and "llma.layers.1.ffn_norm.weight" in saved and "llma.norm.weight" in saved
    assert not any(_is_base(k[len("llma."):]) and "lora_" not in k for k in saved), sorted(saved)[:8]
    assert float(saved["llma.layers.0.attention.wq.lora_b.weight"].float().abs().max()) > 0     # lora_b started at zero: it trained
    # resume = base checkpoint, quantise, adapters by name: the same next-step loss as an in-process model holding the SAVED values
    mr = _quantised_meta(cfgp, ckdir, adapters=str(out / "epoch0"))
    mi = _quantised_meta(cfgp, ckdir)
    with torch.no_grad():
        own = dict(mi.named_parameters())
        for k, v in saved.items():
            own[k].copy_(v.to(own[k].dtype))
    V = mr.tokenizer.n_words
    ex, lab = _batch(seed=5, B=2, T=40, V=V)
    lr_ = float(mr.train_engine().forward_loss(ex.to(DEV), lab.to(DEV), None))
    li_ = float(mi.train_engine().forward_loss(ex.to(DEV), lab.to(DEV), None))
    assert lr_ == li_ and lr_ == lr_, (lr_, li_)
