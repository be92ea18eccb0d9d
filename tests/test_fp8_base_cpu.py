"""CPU (-m "not gpu"): the host side of the fp8 frozen base -- the fp64 fake-quant reference of tests/fp8_base_ref.py is
exact where it must be, the size of the pure quantisation effect on the test model (printed, for the record), ``main_finetune
--base_fp8`` refuses what it cannot run before it touches a GPU, and the new entries are in the header, the ctypes table and the built
library alike."""
import argparse
import os
import re

import pytest
import torch

import fp8_base_ref as R
from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=320, multiple_of=256, max_seq_len=256)
RANK = 8


def exact_problem(M, N, K, seed):
    """W = e4m3-exact entries times a power-of-two row scale (different per row, the row maximum 448 so that the quantiser finds that
    scale); x and dY small integers whose rows hold 7 as their maximum, times a power of two per row: 448 / 7 = 64, so after the
    per-row scaling every entry is an integer multiple of 64 below 448 = e4m3-exact.  dY * sw stays of that kind only if sw is ONE
    power of two per ... column n -- it is not (a scale per n), so dY is built from g = dY * sw: g rows as x rows, dY = g / sw exact."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0., 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 64, 96, 128, 192, 256, 320, 384, 448])
    wcode = vals[torch.randint(0, len(vals), (N, K), generator=g)] * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1)
    wcode[:, 0] = 448.
    sw = torch.pow(2.0, torch.randint(-9, -3, (N,), generator=g).float())
    w = wcode * sw[:, None]

    def rows(m, n):
        t = torch.randint(-7, 8, (m, n), generator=g).float()
        t[:, 1] = 7.
        return t * torch.pow(2.0, torch.randint(-3, 3, (m, 1), generator=g).float())
    x = rows(M, K)
    gsc = rows(M, N)                                   # = dY * sw, exactly
    dy = gsc / sw[None, :]
    return w, wcode, sw, x, dy, gsc


@pytest.mark.parametrize("M", [3, 47])
def test_reference_linear_is_exact_on_exact_inputs(M):
    N, K = 320, 256
    w, wcode, sw, x, dy, gsc = exact_problem(M, N, K, seed=M)
    assert torch.equal(w.to(torch.bfloat16).float(), w) and torch.equal(dy.to(torch.bfloat16).float(), dy)
    wq, s = R.quantize_rows(w)
    assert torch.equal(s, sw) and torch.equal(R.byte_values(wq), wcode.double())
    xd = x.double().requires_grad_(True)
    y = R.base_linear(xd, wq, s)
    assert torch.equal(y, x.double() @ w.double().t())
    y.backward(dy.double())
    assert torch.equal(xd.grad, dy.double() @ w.double())
    gq, sg = R.quantize_rows_cs(dy, s, 384)
    assert gq.shape == (M, 384) and int(gq[:, N:].sum()) == 0
    assert torch.equal(R.dequantize_rows(gq[:, :N], sg), gsc)


def _weights():
    oargs = ref_cpu.OracleArgs(**BIG)
    sd = ref_cpu.make_decoder_weights(oargs, seed=3, std=0.05)
    lsd = ref_cpu.make_lora_weights(oargs, RANK, seed=6, std_a=0.05, std_b=0.05)
    return oargs, sd, lsd


def test_pure_quantisation_distance_of_the_step_is_printed():
    """fake-quant fp64 step against the unquantised fp64 step on the same Wd: what e4m3 activations and gradients alone do to the loss
    and the adapter / norm gradients of the test model (for the record in DESIGN.md 7c; the bound is only that they stay related)."""
    oargs, sd, lsd = _weights()
    q8 = R.quantize_state(sd, oargs.n_layers)
    g = torch.Generator().manual_seed(13)
    ex = torch.randint(3, 320, (3, 47), generator=g)
    ex[:, 0] = 1
    lab = ex.clone()
    lab[:, :6] = 0
    res = {}
    for quant in (True, False):
        params = {k: v.double().requires_grad_("lora_" in k or "norm" in k) for k, v in {**sd, **lsd}.items() if not k.endswith(tuple(
            nm.split(".")[1] + ".weight" for names in R.GROUPS.values() for nm in names))}
        loss = R.step_loss(oargs, params, q8, ex, lab, quant)
        loss.backward()
        res[quant] = (float(loss.detach()), {k: p.grad for k, p in params.items() if p.requires_grad})
    cos = lambda a, b: float(torch.dot(a.flatten(), b.flatten()) / (a.norm() * b.norm() + 1e-300))
    worst = min((cos(res[True][1][k], res[False][1][k]), k) for k in res[True][1])
    rel = abs(res[True][0] - res[False][0]) / abs(res[False][0])
    print(f"\n[fp8 base, pure quantisation] loss {res[True][0]:.6f} vs {res[False][0]:.6f} (rel {rel:.3e}); worst gradient cosine {worst}")
    assert rel < 2e-2 and worst[0] > 0.9


def _args(*extra):
    from a3vlm_amd import main_finetune as mf
    return argparse.ArgumentParser(parents=[mf.get_args_parser()]).parse_args(
        ["--llama_type", "llama_ens5_peft", "--base_fp8", "--only_save_trainable", "--precision", "bf16", "--synthetic", "8", *extra])


@pytest.mark.parametrize("change,message", [
    (dict(only_save_trainable=False), "--only_save_trainable"),
    (dict(llama_type="llama_ens5"), "peft"),
    (dict(precision="tf32"), "--precision bf16"),
    (dict(zero1=True), "--zero1"),
    (dict(quant=True), "--quant"),
])
def test_main_finetune_base_fp8_refusals(monkeypatch, change, message):
    from a3vlm_amd import main_finetune as mf

    def no_gpu(*a, **k):
        raise AssertionError("the refusal must come before the GPU is touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    a = _args()
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(SystemExit) as ei:
        mf.main(a)
    assert "--base_fp8" in str(ei.value) and message in str(ei.value), str(ei.value)


def test_new_entries_are_declared_alike_everywhere():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib, ops
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    fns = dict(re.findall(r"^\s*(?:int|int64_t)\s+(a3v_\w+)\s*\(([^;]*)\)\s*;", src, flags=re.M))
    for name, n in (("a3v_quantize_rows_fp8_cs", 11), ("a3v_gemm_qkv_rope_fp8_train", 25)):
        assert name in fns and name in lib.SIGNATURES
        params = [p.strip() for p in fns[name].split(",")]
        res, argtypes = lib.SIGNATURES[name]
        assert len(params) == len(argtypes) == n and res is lib.I
        kinds = [lib.P if "*" in p else lib.L if p.startswith("int64_t") else lib.I for p in params]
        assert kinds == list(argtypes), (name, params, argtypes)
        assert getattr(lib.load(), name).argtypes == argtypes
    L = lib.load()
    assert L.a3v_quantize_rows_fp8_cs(None, 0, None, None, 0, None, 1, 8, 16, 0, None) == -3        # A3V_ERR_ARG before any launch
    assert L.a3v_gemm_qkv_rope_fp8_train(None, 0, None, None, 0, None, 128, None, 0, None, None, None, 0, None, 0, None,
                                         1, 1, 1, 1, 64, 1, 0, 0, None) == -3
    assert callable(ops.quantize_rows_fp8_cs) and callable(ops.gemm_qkv_rope_fp8_train)
    # the existing fused fp8 entry keeps its signature
    assert len(lib.SIGNATURES["a3v_gemm_qkv_rope_fp8"][1]) == 21


def test_quantize_base_weights_fp8_refuses_cpu_models_and_unknown_modes():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    m = peft.Transformer(peft.ModelArgs(dim=128, n_layers=1, n_heads=2, vocab_size=64, multiple_of=64, max_seq_len=32, lora_rank=8)).to(torch.bfloat16)
    with pytest.raises(ValueError, match="bf16 model on the GPU"):
        m.quantize_base_weights("fp8")
    assert m._q8base is None and hasattr(m.layers[0].attention.wq, "weight")     # nothing was freed
    with pytest.raises(ValueError):
        m.quantize_base_weights("int8")


def test_hbm_budget_knows_the_fp8_base():
    from a3vlm_amd.train import hbm_budget
    kw = dict(dim=4096, n_layers=32, n_heads=32, ffn=11008, vocab=32000, batch=8, seq=1091, text=512, transposed_images=True)
    a, b = hbm_budget(**kw), hbm_budget(**kw, base_bytes=2)
    p_dec = 32 * (4096 * 3 * 4096 + 4096 * 4096 + 3 * 4096 * 11008)
    scales = 4 * 32 * (3 * 4096 + 2 * 4096 + 2 * 11008)
    assert a["images_bf16"] + a["images_t_bf16"] - (b["images_bf16"] + b["images_t_bf16"] + b["images_base"]) == 2 * p_dec - scales
    assert a["total"] - b["total"] == 2 * p_dec - scales
