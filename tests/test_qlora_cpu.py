"""CPU (-m "not gpu"): the host seams of QLoRA -- ``main_finetune --quant`` refuses what it cannot run before it touches a GPU, the new
dequantiser entry is declared alike in the header, the ctypes table and the built library, and ``quantize_base_weights`` refuses models
it cannot quantise."""
import argparse
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*extra):
    from a3vlm_amd import main_finetune as mf
    return argparse.ArgumentParser(parents=[mf.get_args_parser()]).parse_args(
        ["--llama_type", "llama_ens5_peft", "--quant", "--only_save_trainable", "--precision", "bf16", "--synthetic", "8", *extra])


@pytest.mark.parametrize("change,message", [
    (dict(only_save_trainable=False), "--only_save_trainable"),
    (dict(llama_type="llama_ens5"), "peft"),
    (dict(precision="tf32"), "--precision bf16"),
    (dict(zero1=True), "--zero1"),
])
def test_main_finetune_quant_refusals(monkeypatch, change, message):
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
    assert "--quant" in str(ei.value) and message in str(ei.value), str(ei.value)


def test_dequantize_images_entry_is_declared_alike_everywhere():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    fns = dict(re.findall(r"^\s*(?:int|int64_t)\s+(a3v_\w+)\s*\(([^;]*)\)\s*;", src, flags=re.M))
    name = "a3v_dequantize_nf4_images"
    assert name in fns and name in lib.SIGNATURES
    params = [p.strip() for p in fns[name].split(",")]
    res, argtypes = lib.SIGNATURES[name]
    assert len(params) == len(argtypes) == 9 and res is lib.I
    # pointers, ints and int64 strides in the header's order: (q, scales, N, K, Wd, ldd, Wt, ldt, stream)
    kinds = [lib.P if "*" in p else lib.L if p.startswith("int64_t") else lib.I for p in params]
    assert kinds == list(argtypes), (params, argtypes)
    fn = getattr(lib.load(), name)
    assert fn.argtypes == argtypes
    assert fn(None, None, 64, 64, None, 0, None, 0, None) == -3           # A3V_ERR_ARG before any launch (no GPU needed)
    from a3vlm_amd import ops
    assert callable(ops.dequantize_nf4_images)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_base_weights_refuses_cpu_and_fp32_models(dtype):
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    m = peft.Transformer(peft.ModelArgs(dim=128, n_layers=1, n_heads=2, vocab_size=64, multiple_of=64, max_seq_len=32, lora_rank=8)).to(dtype)
    with pytest.raises(ValueError, match="bf16 model on the GPU"):
        m.quantize_base_weights("nf4")
    assert m._q4 is None and hasattr(m.layers[0].attention.wq, "weight")     # nothing was freed
    with pytest.raises(ValueError):
        m.quantize_base_weights("int8")
