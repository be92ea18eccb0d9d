"""-m "not gpu": the host side of the LoRA merge -- the C-ABI declaration, the exactness of the test inputs the GPU tests rely on, the
``merge_lora`` command line, the config a merged model writes and the refusal of CPU models."""
import dataclasses
import json
import os
import re

import pytest
import torch

import lora_merge_ref as MR
from a3vlm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TK = dict(dim=128, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=64)


def test_entry_is_declared_in_header_and_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    m = re.search(r"\bint a3v_lora_merge\(([^;]*)\);", hdr)
    assert m, "a3v_lora_merge is not declared in include/a3vlm_hip.h"
    n_args = len(m.group(1).split(","))
    assert "a3v_lora_merge" in lib.SIGNATURES
    res, args = lib.SIGNATURES["a3v_lora_merge"]
    assert res is lib.I and len(args) == n_args == 15
    assert "a3v_merge.hip" in open(os.path.join(ROOT, "a3vlm_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("R", [8, 64, 256])
def test_exact_inputs_are_exact_in_fp32_in_any_order(R):
    base, B, A = MR.exact_inputs(40, 72, R, seed=R)
    ref = MR.merge_ref64(base, B, A)
    prod = B.float()[:, :, None] * A.float()[None, :, :]                 # [N, R, K] fp32 products
    assert torch.equal(prod.double(), B.double()[:, :, None] * A.double()[None, :, :])
    fwd = base.float().clone()
    for r in range(R):                                                   # base first, r ascending
        fwd += prod[:, r]
    bwd = torch.zeros_like(fwd)
    for r in reversed(range(R)):                                         # r descending, base last
        bwd += prod[:, r]
    bwd += base.float()
    assert torch.equal(fwd.double(), ref) and torch.equal(bwd.double(), ref)
    assert float(base.float().abs().max()) <= 4.0 and torch.equal(base.float() * 64, (base.float() * 64).round())


def test_exact_inputs_tell_double_rounding_apart():
    # the accumulator is a multiple of 2^-6: bf16 (8 bits) holds it exactly below 4 and loses its last bit from 4 on, which the sums
    # over R = 256 terms reach (R = 256 is one of the GPU test's ranks)
    base, B, A = MR.exact_inputs(40, 72, 256, seed=1)
    acc = B.double() @ A.double()
    once = (acc + base.double()).to(torch.bfloat16)                      # fp64 -> bf16: one rounding
    twice = (acc.to(torch.bfloat16).double() + base.double()).to(torch.bfloat16)
    assert int((once != twice).sum()) > 0


def test_merge_lora_argument_parser():
    from a3vlm_amd import merge_lora
    import argparse
    p = argparse.ArgumentParser(parents=[merge_lora.get_args_parser()])
    a = p.parse_args(["--pretrained_path", "base", "adapters", "--output_dir", "out"])
    assert a.pretrained_path == ["base", "adapters"] and a.output_dir == "out" and a.quant_base is False
    assert p.parse_args(["--pretrained_path", "x", "--output_dir", "o", "--quant_base"]).quant_base is True
    with pytest.raises(SystemExit):
        p.parse_args(["--output_dir", "o"])
    with pytest.raises(SystemExit):
        p.parse_args(["--pretrained_path", "x"])


def test_eval_entry_points_have_the_merge_flag():
    import argparse
    from a3vlm_amd import eval_affordance_v2
    p = argparse.ArgumentParser(parents=[eval_affordance_v2.get_args_parser()])
    assert p.parse_args([]).merge_lora is False and p.parse_args(["--merge_lora"]).merge_lora is True


def test_merged_config_drops_the_peft_only_fields():
    """what merge_adapters leaves in ``args`` (and save_checkpoint writes as config.json) is a base ModelArgs: the base plugin's
    MetaModel rejects unknown fields"""
    from a3vlm_amd.model.LLM import llama_ens5 as base, llama_ens5_peft as peft
    pa = peft.ModelArgs(**TK, lora_rank=8)
    extra = {f.name for f in dataclasses.fields(peft.ModelArgs)} - {f.name for f in dataclasses.fields(base.ModelArgs)}
    assert extra == {"lora_rank", "bias_tuning"}
    merged = peft.merged_args(pa)
    cfg = dataclasses.asdict(merged)
    assert type(merged) is base.ModelArgs and not extra & set(cfg)
    assert all(cfg[k] == v for k, v in dataclasses.asdict(pa).items() if k not in extra)
    base.ModelArgs(**json.loads(json.dumps(cfg)))                        # what MetaModel does with a config.json


def test_merge_adapters_refuses_a_cpu_model():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    m = peft.Transformer(peft.ModelArgs(**TK, lora_rank=8))
    with pytest.raises(ValueError, match="GPU"):
        m.merge_adapters()
    assert m.is_peft and hasattr(m.layers[0].attention.wq, "lora_a")      # untouched


def test_ops_lora_merge_refuses_cpu_tensors():
    from a3vlm_amd import ops
    base, B, A = MR.exact_inputs(16, 64, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.lora_merge(base, B, A)
