"""-m gpu: NF4 weight-only inference (the reference's 4-bit mode: bitsandbytes Linear4bit nf4, util/quant.py:95-163).

The format is restated on the CPU in tests/nf4_ref.py.  (1) the HIP quantiser reproduces it exactly, given its own module offset
(a reduction: only its rounding may differ); (2) the dequantiser is bit-equal to Wd; (3) the NF4 decode GEMV matches the fp32
product on NF4[q] * s_b and the bf16 GEMV on Wd; (4) an NF4 model's prefill is bit-identical to a bf16 model holding Wd (KV
caches), its decode follows the oracle on Wd; (5) the bf16 weights are freed."""
import pytest
import torch

import nf4_ref as R
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def weight(N, K, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * std
    w.view(-1)[64 * 5:64 * 6] = 0                     # a zero block
    w.view(-1)[64 * 9:64 * 10] *= 50                  # an outlier block
    return w.to(BF)


@pytest.mark.parametrize("N,K", [(256, 256), (1000, 1024), (4096, 11008), (12288, 4096)])
def test_quantiser_matches_the_cpu_restatement(N, K):
    w = weight(N, K, seed=N + K)
    q, s, off = ops.quantize_nf4(w.to(DEV))
    torch.cuda.synchronize()
    off = float(off)
    am = R.absmax_blocks(w)
    assert abs(off - float(am.mean())) <= 2e-6 * float(am.mean())
    want_q = R.pack_nibbles(R.quantize_codes(w, am))
    want_s, _ = R.double_quant_scales(am, offset=off)
    assert torch.equal(q.cpu(), want_q)
    assert torch.equal(s.cpu().view(-1), want_s)                      # bit-equal, given the kernel's offset
    assert float(s.view(-1)[5]) == 0.0 and bool((q.view(-1)[160:192] == 0x77).all())
    # (2) the dequantiser writes Wd exactly
    wd = torch.empty(N, K, dtype=BF, device=DEV)
    ops.dequantize_nf4(q, s, wd)
    assert torch.equal(wd.cpu(), R.dequantize(want_q, want_s.view(N, K // 64)))


def test_dequantiser_into_a_strided_destination():
    w = weight(64, 512, seed=3)
    q, s, _ = ops.quantize_nf4(w.to(DEV))
    big = torch.full((64, 640), 7.0, dtype=BF, device=DEV)
    ops.dequantize_nf4(q, s, big[:, :512])
    assert torch.equal(big[:, :512].cpu(), R.dequantize(q.cpu(), s.cpu()))
    assert bool((big[:, 512:] == 7.0).all())


GEMV_SHAPES = [(256, 256), (4096, 4096), (512, 11008), (32000, 4096), (22016, 4096)]


@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
@pytest.mark.parametrize("epi", ["none", "residual", "swiglu", "f32"])
def test_gemv_nf4(M, N, K, epi):
    w = weight(N, K, seed=N * 7 + K)
    q, s, _ = ops.quantize_nf4(w.to(DEV))
    if epi == "swiglu" and K < 512:        # the SwiGLU epilogue pairs tiles in the split-K fix-up: two K slices needed (as bf16 / fp8)
        out = torch.empty(M, N // 2, dtype=BF, device=DEV)
        with pytest.raises(RuntimeError, match="A3V_ERR_SHAPE"):
            ops.gemm_skinny_nf4(torch.zeros(M, K, dtype=BF, device=DEV), q, s, out, ops.gemm_skinny_workspace(M, N, K, DEV),
                                epilogue=ops.EPI_SWIGLU)
        return
    a = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 0.5).to(BF)
    wdec = R.decoded_f32(q.cpu(), s.cpu())                            # NF4[q] * s_b, fp32
    y = a.float() @ wdec.T
    ws = ops.gemm_skinny_workspace(M, N, K, DEV)
    kw, dt = {}, BF
    if epi == "residual":
        res = (torch.randn(M, N, generator=torch.Generator().manual_seed(9)) * 0.5).to(BF)
        kw["residual"] = res.to(DEV)
        want = y + res.float()
    elif epi == "swiglu":
        nb = N // 32
        g_, u_ = y.view(M, nb, 2, 16)[:, :, 0].reshape(M, -1), y.view(M, nb, 2, 16)[:, :, 1].reshape(M, -1)
        want = torch.nn.functional.silu(g_) * u_
        kw["epilogue"] = ops.EPI_SWIGLU
    elif epi == "f32":
        kw["epilogue"], dt = ops.EPI_OUT_F32, torch.float32
        want = y
    else:
        want = y
    out = torch.empty(M, want.shape[1], dtype=dt, device=DEV)
    if "residual" in kw:
        out.copy_(kw["residual"])
        kw["residual"] = out
    ops.gemm_skinny_nf4(a.to(DEV), q, s, out, ws, **kw)
    got = out.float().cpu()
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) < 2 ** -7 * scale
    # against the bf16 GEMV on Wd (differs by where the scale is rounded only)
    wd = torch.empty(N, K, dtype=BF, device=DEV)
    ops.dequantize_nf4(q, s, wd)
    out2 = torch.empty_like(out)
    kw2 = dict(kw)
    if "residual" in kw:
        out2.copy_(res.to(DEV))
        kw2["residual"] = out2
    ops.gemm_skinny(a.to(DEV), wd, out2, ops.gemm_skinny_workspace(M, N, K, DEV), **kw2)
    # Wd rounds every weight to bf16, the NF4 GEMV every code: both sides are within 2^-7 of the fp32 product, so 2^-6 apart
    assert float((got - out2.float().cpu()).abs().max()) < 2 ** -6 * scale


def _models(heads, kv, dim, B, seed=11, layers=2, vocab=640):
    args = dict(dim=dim, n_layers=layers, n_heads=heads, n_kv_heads=kv, vocab_size=vocab, multiple_of=256, max_seq_len=192)
    oargs = ref_cpu.OracleArgs(**args)
    sd = ref_cpu.make_decoder_weights(oargs, seed=seed, std=0.05)
    m = plugin.Transformer(plugin.ModelArgs(**args))
    m.load_state_dict(sd)
    m.to(BF).to(DEV)
    m.quantize_decode_weights("nf4")
    # the bf16 model on Wd: every quantised module replaced by its dequantised weight
    sdq = {k: v.to(BF) for k, v in sd.items()}
    for k in sd:
        if k == "output.weight" or (k.startswith("layers.") and k.endswith((".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight",
                                                                          ".w1.weight", ".w2.weight", ".w3.weight"))):
            nib, sc, _ = ops.quantize_nf4(sd[k].to(BF).to(DEV).contiguous())
            sdq[k] = R.dequantize(nib.cpu(), sc.cpu())
    mq = plugin.Transformer(plugin.ModelArgs(**args))
    mq.load_state_dict(sdq)
    mq.to(BF).to(DEV)
    return m, mq, oargs, sdq


@pytest.mark.parametrize("heads,kv,dim,B", [(4, 4, 512, 4), (8, 2, 1024, 8), (4, 4, 512, 20), (4, 4, 512, 40)])
def test_nf4_model_prefill_and_decode(heads, kv, dim, B):
    m, mq, oargs, sdq = _models(heads, kv, dim, B)
    g = torch.Generator().manual_seed(2)
    T0, steps = 33, 5
    ex = torch.randint(3, 640, (B, T0 + steps), generator=g).to(DEV)
    ex[:, 0] = 1
    lg = [m.forward_inference(ex[:, :T0], 0).float().clone()]
    lq0 = mq.forward_inference(ex[:, :T0], 0).float().clone()
    for i in range(oargs.n_layers):                               # prefill: the bf16 GEMMs on the dequantised scratch
        assert torch.equal(m._k_cache[i], mq._k_cache[i]) and torch.equal(m._vt_cache[i], mq._vt_cache[i]), i
    for t in range(T0, T0 + steps):
        lg.append(m.forward_inference(ex[:, t:t + 1], t).float().clone())
    dec = ref_cpu.OracleDecoder(oargs, sdq)
    want = [dec.forward_inference(ex[:, :T0].cpu(), 0).float()]
    for t in range(T0, T0 + steps):
        want.append(dec.forward_inference(ex[:, t:t + 1].cpu(), t).float())
    scale = max(float(w.abs().max()) for w in want)
    errs = [float((g_.cpu() - w).abs().max()) / scale for g_, w in zip(lg, want)]
    print(f"NF4 decode vs oracle on Wd, B={B}: max err / max|logit| = {max(errs):.3e}")
    assert max(errs) < 5e-2, errs
    assert float((lq0.cpu() - want[0]).abs().max()) / scale < 5e-2
    with pytest.raises(RuntimeError, match="NF4"):
        m.quantize_decode_weights(None)


def test_nf4_per_kernel_decode_matches_fused_step():
    m, _, _, _ = _models(4, 4, 512, 4)
    g = torch.Generator().manual_seed(3)
    ex = torch.randint(3, 640, (4, 20), generator=g).to(DEV)
    m.forward_inference(ex[:, :19], 0)
    fused = m.forward_inference(ex[:, 19:20], 19).clone()
    m.forward_inference(ex[:, :19], 0)
    m._per_kernel_decode = True
    per = m.forward_inference(ex[:, 19:20], 19).clone()
    scale = float(fused.abs().max())
    assert float((fused - per).abs().max()) / scale < 2e-2


def test_nf4_memory_and_state_dict():
    args = plugin.ModelArgs(dim=1024, n_layers=2, n_heads=8, n_kv_heads=8, vocab_size=1024, multiple_of=256, max_seq_len=128)
    m = plugin.Transformer(args).to(BF).to(DEV)
    names = [n for n in m.state_dict() if n == "output.weight" or n.endswith(
        (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight"))]
    bf16_bytes = sum(m.state_dict()[n].numel() * 2 for n in names)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    m.quantize_decode_weights("nf4")
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    n4_bytes = sum(q.numel() + s.numel() * 4 for q, s in m._weights.images.values())
    assert n4_bytes == bf16_bytes * 4.5 / 16
    assert before - after >= 0.7 * bf16_bytes, (before, after, bf16_bytes)
    sd = m.state_dict()
    assert not any(n in sd for n in names)
    assert "layers.0.attention_norm.weight" in sd and "tok_embeddings.weight" in sd


def test_nf4_refusals():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    args = plugin.ModelArgs(dim=512, n_layers=1, n_heads=4, vocab_size=256, multiple_of=256, max_seq_len=64)
    m = plugin.Transformer(args).to(DEV)                       # fp32 model: NF4 needs bf16
    with pytest.raises(ValueError):
        m.quantize_decode_weights("nf4")
    pm = peft.Transformer(peft.ModelArgs(dim=512, n_layers=1, n_heads=4, vocab_size=256, multiple_of=256, max_seq_len=64,
                                         lora_rank=8)).to(BF).to(DEV)
    with pytest.raises(NotImplementedError):
        pm.quantize_decode_weights("nf4")
