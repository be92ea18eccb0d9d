"""-m gpu: QLoRA -- the LoRA step on an NF4 base (``llama_ens5_peft.Transformer.quantize_base_weights``), the streaming dequantiser that
feeds it (a3v_dequantize_nf4_images), inference on the quantised peft model, and ``main_finetune --quant``.

Model Q holds the NF4 base; model D is the same model with every quantised weight replaced by Wd = bf16(NF4[q] * s_b) from the CPU
restatement of the format (tests/nf4_ref.py).  Both run the same bf16 kernels on bit-identical images, so Q must equal D bit for bit
wherever the kernels are run-to-run deterministic."""
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import nf4_ref as R
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5_peft as peft
from a3vlm_amd.optim import FusedAdamW
from a3vlm_amd.train import TrainEngine
from a3vlm_amd.util import promote_trainable_params_to_fp32
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
BIG = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=320, multiple_of=256, max_seq_len=256)
RANK = 8
QUANT = (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight")
SENT = -7.0            # exactly representable in bf16; no dequantised weight of these tests reaches it


def _is_quant(k):
    return k == "output.weight" or (k.startswith("layers.") and k.endswith(QUANT))


def _weights(cfg):
    oargs = ref_cpu.OracleArgs(**cfg)
    sd = ref_cpu.make_decoder_weights(oargs, seed=3, std=0.05)
    lsd = ref_cpu.make_lora_weights(oargs, RANK, seed=6, std_a=0.05, std_b=0.05)
    return oargs, sd, lsd


def _wd_state(sd):
    """the state dict in bf16 with Wd in every quantised module (CPU restatement of the format)"""
    out = {}
    for k, v in sd.items():
        v = v.to(BF)
        if _is_quant(k):
            nib, sc, _ = R.quantize(v)
            v = R.dequantize(nib, sc)
        out[k] = v
    return out


def _model(cfg, sd, lsd, quant):
    m = peft.Transformer(peft.ModelArgs(**cfg, lora_rank=RANK), with_visual=False)
    m.load_state_dict({**(sd if quant else _wd_state(sd)), **lsd}, strict=True)
    train = m.get_trainable_params()
    for n, p in m.named_parameters():
        p.requires_grad = n in train
    m.to(BF).to(DEV)
    if quant:
        m.quantize_base_weights("nf4")
    return m


def _batch(seed=13, B=3, T=47, V=320):
    g = torch.Generator().manual_seed(seed)
    ex = torch.randint(3, V, (B, T), generator=g)
    ex[:, 0] = 1
    lab = ex.clone()
    lab[:, :6] = 0
    return ex, lab


# ---------------------------------------------------------------------------------------------------------------- 1. the dequantiser
def _windows(N, K):
    """sentinel-filled destinations with guard rows: Wd window [N, K] at ldd = K + 64, Wt window [K, N] at ldt = pad8(N) + 64"""
    ldd, ldt = K + 64, (N + 7) // 8 * 8 + 64
    bd = torch.full((N + 4, ldd), SENT, dtype=BF, device=DEV)
    bt = torch.full((K + 4, ldt), SENT, dtype=BF, device=DEV)
    return bd, bt, bd[2:2 + N, :K], bt[2:2 + K, :N]


def _outside_untouched(buf, rows, cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[2:2 + rows, :cols] = False
    return bool((buf[mask] == SENT).all())


@pytest.mark.parametrize("N,K", [(64, 64), (72, 64), (320, 256), (768, 256), (256, 768)])
def test_dequantize_images_bit_equal_in_both_orientations_inside_windows(N, K):
    g = torch.Generator().manual_seed(1000 * N + K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV)
    q, sc, _ = ops.quantize_nf4(w)
    want = ops.dequantize_nf4(q, sc, torch.empty(N, K, dtype=BF, device=DEV))
    assert torch.equal(want.cpu(), R.dequantize(q.cpu(), sc.cpu()))
    assert float(want.float().abs().max()) < -SENT
    for use_d, use_t in ((True, True), (True, False), (False, True)):
        bd, bt, wd, wt = _windows(N, K)
        ops.dequantize_nf4_images(q, sc, wd=wd if use_d else None, wt=wt if use_t else None)
        torch.cuda.synchronize()
        if use_d:
            assert torch.equal(wd, want), (N, K, use_d, use_t)
            assert torch.equal(wd.cpu(), R.dequantize(q.cpu(), sc.cpu()))
        else:
            assert bool((bd == SENT).all())
        if use_t:
            assert torch.equal(wt, want.t()), (N, K, use_d, use_t)
        else:
            assert bool((bt == SENT).all())
        assert _outside_untouched(bd, N, K) and _outside_untouched(bt, K, N), (N, K, use_d, use_t)


def test_dequantize_images_refusals_leave_the_buffers_untouched():
    N, K = 64, 128
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(1)) * 0.05).to(BF).to(DEV)
    q, sc, _ = ops.quantize_nf4(w)
    bd, bt, wd, wt = _windows(N, K)
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    call = lambda n, k, d, ldd, t, ldt: L.a3v_dequantize_nf4_images(q.data_ptr(), sc.data_ptr(), n, k, d, ldd, t, ldt, st)
    d, t = wd.data_ptr(), wt.data_ptr()
    assert call(N, K, None, 0, None, 0) == -3                                 # both outputs NULL: A3V_ERR_ARG
    assert call(N, 96, d, wd.stride(0), t, wt.stride(0)) == -1                # K % 64
    assert call(N, K, d, wd.stride(0) + 4, None, 0) == -1                     # ldd % 8
    assert call(N, K, None, 0, t, wt.stride(0) + 2) == -1                     # ldt % 8
    assert call(N, K, d + 2, wd.stride(0), None, 0) == -1                     # base not 16-B aligned
    assert call(N, K, None, 0, t + 8, wt.stride(0)) == -1
    assert call(N, K, d, K - 8, None, 0) == -1 and call(N, K, None, 0, t, N - 8) == -1     # windows narrower than the matrix
    torch.cuda.synchronize()
    assert bool((bd == SENT).all()) and bool((bt == SENT).all())
    with pytest.raises(lib.A3VError):
        ops.dequantize_nf4_images(q, sc, wd=bd[2:2 + N, 4:4 + K])              # 8-B aligned window through the Python wrapper
    assert bool((bd == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. the step
def _run_steps(m, ex, lab, recompute, kext=True, nt="all"):
    """two forward / backward steps with one FusedAdamW step between them: [(loss, {name: grad})] x 2.
    The optimizer holds the ADAPTERS only.  The RMSNorm weight gradients are not bit-reproducible (see below), and AdamW's first update
    is lr * g / (|g| + eps): an element of a norm gradient that is zero up to that noise would move its weight by +lr in one run and by
    -lr in the next, and the second step would then differ between two runs of the SAME model by far more than rounding (seen once:
    step-1 loss 4.68205 against 4.68192).  The adapter gradients of step 0 are bit-reproducible, so with the adapters alone in the
    optimizer the second step is a deterministic function of the first on either model -- and it still has to find the updated
    adapters, written by the optimizer's sinks, in the image tails."""
    promote_trainable_params_to_fp32(m)
    train = m.get_trainable_params()
    eng = TrainEngine(m, BF, recompute=recompute)
    eng.lora_kext = kext
    eng.lora_nt_dgrad = nt
    opt = FusedAdamW([p for n, p in m.named_parameters() if p.requires_grad and "lora_" in n], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.0,
                     engine=eng)
    out = []
    for step in range(2):
        loss = float(eng.forward_loss(ex.to(DEV), lab.to(DEV), None))
        eng.backward(1.0)
        out.append((loss, {n: p.grad.float().cpu().clone() for n, p in train.items()}))
        if step == 0:
            opt.step()
            m.zero_grad(set_to_none=True)
    return out, eng


# Run-to-run determinism of the bf16 LoRA step itself, measured as model D against model D on an MI355X (three pairs of runs for each
# of the four configurations below, both steps, max |a - b| / max |b| per tensor; that measurement still had every trainable in the
# optimizer): the RMSNorm weight gradients (a3v_rmsnorm_bwd adds with fp32 atomics; tests/test_gpu_lora.py says the same) differed in
# every pair, by 2.115e-7 at most.  The loss and every other gradient were bit-identical in 11 of the 12 pairs, both steps; the twelfth
# (lora_kext=False) differed in step 1 only after its optimizer step, the effect _run_steps describes and now excludes.
# Bound for the norm-weight gradients = twice their measured difference; the loss and every other tensor: bit-equal, in both steps
# and every configuration.
NORM_REL = 2 * 2.115e-7


@pytest.mark.parametrize("recompute,kext,nt", [(True, True, "all"), (False, True, "all"), (True, False, "all"), (True, True, "0")])
def test_qlora_step_equals_the_bf16_lora_step_on_the_dequantised_base(recompute, kext, nt):
    """Loss and every trainable gradient of two consecutive steps (an optimizer step between them: the second forward must find the
    updated adapters in the scratch tails; two layers with different weights: a stale scratch would serve layer 1's matrix to layer 0).
    Bit-equal wherever the bf16 LoRA step is itself reproducible; the measured exception and its bound are stated above."""
    oargs, sd, lsd = _weights(BIG)
    ex, lab = _batch()
    got_q, eng_q = _run_steps(_model(BIG, sd, lsd, True), ex, lab, recompute, kext, nt)
    got_d, _ = _run_steps(_model(BIG, sd, lsd, False), ex, lab, recompute, kext, nt)
    assert (eng_q._kext() > 0) == kext and eng_q.lora_nt_dgrad == nt and eng_q.recompute == recompute
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-30))
    for step in range(2):
        (lq, gq), (ld, gd) = got_q[step], got_d[step]
        worst = max((rel(gq[n], gd[n]), n) for n in gq)
        print(f"\n[qlora] recompute={recompute} kext={kext} nt={nt} step {step}: loss q={lq!r} d={ld!r} worst rel diff {worst}")
        assert set(gq) == set(gd)
        assert lq == ld, (step, lq, ld)
        for n in gq:
            if n.endswith("norm.weight"):
                assert rel(gq[n], gd[n]) <= NORM_REL, (step, n, rel(gq[n], gd[n]))
            else:
                assert torch.equal(gq[n], gd[n]), (step, n, rel(gq[n], gd[n]))
    assert got_q[0][0] != got_q[1][0]                      # the optimizer step moved the model


def test_qlora_step_against_the_oracle():
    """ref_cpu autograd on the Wd weights: the project's bf16-step bounds (loss 2e-2 relative, gradient cosine > 0.98 per tensor)."""
    oargs, sd, lsd = _weights(BIG)
    ex, lab = _batch()
    m = _model(BIG, sd, lsd, True)
    promote_trainable_params_to_fp32(m)
    train = m.get_trainable_params()
    eng = TrainEngine(m, BF)
    loss = float(eng.forward_loss(ex.to(DEV), lab.to(DEV), None))
    eng.backward(1.0)
    wd = {k: v.float() for k, v in _wd_state(sd).items() if _is_quant(k)}
    osd = {k: v.clone().requires_grad_(k in train) for k, v in {**sd, **wd, **lsd}.items()}
    want_loss = ref_cpu.meta_forward_loss(ref_cpu.OracleDecoder(oargs, osd), ex, lab, None)
    want_loss.backward()
    print(f"\n[qlora oracle] loss {loss} want {float(want_loss)}")
    assert abs(loss - float(want_loss)) < 2e-2 * abs(float(want_loss))
    cos = lambda x, y: float(torch.dot(x, y) / (x.norm() * y.norm() + 1e-20))
    for n, p in train.items():
        c = cos(p.grad.float().cpu().flatten(), osd[n].grad.flatten())
        assert c > 0.98, (n, c)


# ---------------------------------------------------------------------------------------------------------------- 4. memory
def test_qlora_memory_state_dict_and_one_layer_of_scratch():
    args = peft.ModelArgs(dim=1024, n_layers=2, n_heads=8, n_kv_heads=8, vocab_size=1024, multiple_of=256, max_seq_len=128, lora_rank=RANK)
    m = peft.Transformer(args).to(BF).to(DEV)
    names = [n for n in m.state_dict() if _is_quant(n) and "lora_" not in n]
    assert len(names) == 2 * 7 + 1
    bf16_bytes = sum(m.state_dict()[n].numel() * 2 for n in names)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    m.quantize_base_weights("nf4")
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    assert sum(q.numel() + s.numel() * 4 for q, s, _ in m._q4.values()) == bf16_bytes * 4.5 / 16
    assert before - after >= 0.7 * bf16_bytes, (before, after, bf16_bytes)
    sdq = m.state_dict()
    assert not any(n in sdq for n in names)
    assert {"layers.0.attention_norm.weight", "norm.weight", "tok_embeddings.weight", "layers.1.feed_forward.w2.lora_a.weight",
            "layers.0.attention.wq.lora_b.weight"} <= set(sdq)
    with pytest.raises(RuntimeError):
        m.quantize_base_weights("nf4")
    del m
    # the engine's weight-image scratch is one layer's worth whatever the depth; the bf16 engine's images grow with it
    held = {}
    ex, lab = _batch(B=2, T=33)
    for quant in (True, False):
        for nl in (2, 4):
            cfg = dict(BIG, n_layers=nl)
            oargs, sd, lsd = _weights(cfg)
            mm = _model(cfg, sd, lsd, quant)
            promote_trainable_params_to_fp32(mm)
            eng = TrainEngine(mm, BF, recompute=True)
            assert eng.weight_image_bytes() == 0
            eng.forward_loss(ex.to(DEV), lab.to(DEV), None)
            eng.backward(1.0)
            held[quant, nl] = (eng.weight_image_bytes(), eng.weight_image_bytes(head=False))
    assert held[True, 2] == held[True, 4] and held[True, 2][1] > 0
    assert held[False, 4][1] == 2 * held[False, 2][1]                  # per-layer images: twice the layers, twice the bytes
    assert held[False, 4][0] - held[False, 4][1] == held[False, 2][0] - held[False, 2][1] > 0      # (+ the head's, once)
    assert held[True, 2][1] == held[False, 2][1] // 2                  # exactly one of D's two layers


# ---------------------------------------------------------------------------------------------------------------- 5. inference
@pytest.mark.parametrize("fuse", [True, False])
def test_qlora_inference_prefill_and_decode_equal_the_bf16_model_on_wd(fuse):
    oargs, sd, lsd = _weights(BIG)
    mq, md = _model(BIG, sd, lsd, True), _model(BIG, sd, lsd, False)
    mq._fuse_qkv_rope = md._fuse_qkv_rope = fuse
    ex, _ = _batch(seed=21, B=3, T=24)
    with torch.no_grad():
        pq = mq.forward_inference(ex[:, :23].to(DEV), 0)          # 69 rows (> 16): head_dim 64 takes the fused qkv / RoPE GEMM when on
        pd = md.forward_inference(ex[:, :23].to(DEV), 0)
        assert torch.equal(pq, pd) and bool(torch.isfinite(pq).all())
        dq = mq.forward_inference(ex[:, 23:24].to(DEV), 23)       # the following decode step (S = 1, per-kernel peft path)
        dd = md.forward_inference(ex[:, 23:24].to(DEV), 23)
        assert torch.equal(dq, dd) and not torch.equal(dq, pq)
        assert torch.equal(mq(ex.to(DEV)), md(ex.to(DEV)))         # teacher-forced forward (all positions)


# ---------------------------------------------------------------------------------------------------------------- 6. trainer entry
@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    """a base checkpoint folder (decoder + zero adapters) written by checkpoint.save_checkpoint, and the config / tokenizer it needs"""
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    tmp = tmp_path_factory.mktemp("qlora")
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
    mm.llma.quantize_base_weights("nf4")
    if adapters is not None:                      # resume: base, quantise, then the adapters by name
        res = load_tensor_parallel_model_list(mm, [adapters])
        assert res["unexpected_keys"] == [], res
    return mm


def test_main_finetune_quant_trains_saves_adapters_and_resumes(base_ckpt):
    cfgp, ckdir, tmp = base_ckpt
    out = tmp / "out"
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.main_finetune", "--llama_type", "llama_ens5_peft", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--quant", "--only_save_trainable",
           "--synthetic", "8", "--batch_size", "2", "--accum_iter", "1", "--epochs", "1", "--warmup_epochs", "0", "--lr", "1e-3",
           "--max_words", "48", "--no_visual", "--num_workers", "0", "--precision", "bf16", "--output_dir", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(x) for x in re.findall(r"closs: ([-+.\deE]+|nan|inf)", r.stdout)]
    assert losses and all(torch.isfinite(torch.tensor(losses))), r.stdout[-2000:]
    saved = torch.load(out / "epoch0" / "consolidated.00-of-01.model.pth", weights_only=False)["model"]
    assert "llma.layers.0.attention.wq.lora_a.weight" in saved and "llma.layers.1.ffn_norm.weight" in saved and "llma.norm.weight" in saved
    assert not any(_is_quant(k[len("llma."):]) and "lora_" not in k for k in saved), sorted(saved)[:8]
    assert float(saved["llma.layers.0.attention.wq.lora_b.weight"].float().abs().max()) > 0     # lora_b started at zero: it trained
    # resume = base checkpoint, quantise, adapters by name.  The file holds the trainables in bf16 (--precision bf16 is the save dtype),
    # so the comparison is against an in-process model holding the SAVED values: its loss on a fixed batch, bit for bit.
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
