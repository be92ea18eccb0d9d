"""CPU (-m "not gpu") checks of the fp8 KV cache's boundary and host logic: the entry points exist in the header, the built library and
the ctypes table; quantize_kv_cache validates its argument; the LoRA plugin refuses it without touching a GPU; the eval parsers take
--kv_quant; and the host restatement the GPU tests compare against (tests/kv8_ref.py) round-trips within half an e4m3 step."""
import math
import os
import re

import pytest
import torch

import kv8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_kv_quantize_fp8", "a3v_kv_dequantize_fp8", "a3v_attention_decode_fp8kv", "a3v_llama_decode_step_kv8")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


def test_entries_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = built.load()
    for name in ENTRIES + ("a3v_attention_decode_fp8kv_splits",):
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in include/a3vlm_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert [n for n, _ in built.Kv8Layer._fields_] == re.findall(r"(\w+);", re.search(r"typedef struct a3v_kv8_layer \{(.*?)\}", src, flags=re.S).group(1))


def test_shapes_are_refused_before_any_launch(built):
    """hd outside {64, 128} is A3V_ERR_SHAPE from the argument check (no device is needed to get there: the pointers are never used)."""
    lib = built.load()
    p = 4096          # any non-NULL, 16-B aligned value: a refused call does not dereference it
    assert lib.a3v_kv_quantize_fp8(p, p, 64, 0, p, p, p, p, 1, 1, 96, 1, 64, 0, None) == -1
    assert lib.a3v_kv_quantize_fp8(p, p, 64, 0, p, p, p, p, 1, 1, 64, 1, 100, 0, None) == -1          # Smax % 64
    assert lib.a3v_kv_quantize_fp8(p, p, 64, 60, p, p, p, p, 1, 1, 64, 5, 64, 0, None) == -1          # source range past Smax_src
    assert lib.a3v_kv_quantize_fp8(p, p, 64, 0, p, p, p, p, 1, 1, 64, 5, 64, 60, None) == -1          # destination range past Smax
    assert lib.a3v_kv_dequantize_fp8(p, p, p, p, 64, p, p, 64, 1, 1, 32, 1, None) == -1
    assert lib.a3v_attention_decode_fp8kv(p, 256, p, p, p, p, p, 256, 1, 1, 1, 1, 256, 64, p, None, None) == -1
    assert lib.a3v_attention_decode_fp8kv(p, 64, p, p, p, p, p, 64, 1, 65, 1, 1, 64, 64, p, None, None) == -1   # Sk > Smax
    assert lib.a3v_kv_quantize_fp8(None, p, 64, 0, p, p, p, p, 1, 1, 64, 1, 64, 0, None) == -3
    assert lib.a3v_llama_decode_step_kv8(None, None, 1, p, p, p, p, p, p, p, p, p, p, 1, 256, 4, 4, 64, 512, 64, 0, 1e-5, None) == -3
    # the split rule is the fused bf16 entry's: one block per (batch, head) once those cover the CUs, else splits of >= 64 keys
    assert lib.a3v_attention_decode_fp8kv_splits(8, 32, 3500) == 1
    assert lib.a3v_attention_decode_fp8kv_splits(1, 2, 1500) > 1 and lib.a3v_attention_decode_fp8kv_splits(1, 2, 1) == 1


def _tiny(plugin, **kw):
    return plugin.Transformer(plugin.ModelArgs(dim=128, n_layers=1, n_heads=2, vocab_size=64, multiple_of=64, max_seq_len=64, **kw))


def test_quantize_kv_cache_rejects_unknown_names():
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    m = _tiny(plugin)
    assert m._kv_quant is None
    for bad in ("int8", "fp4", "FP8", "bf16", True):
        with pytest.raises(ValueError, match="KV-cache format"):
            m.quantize_kv_cache(bad)
    m.quantize_kv_cache("fp8")
    assert m._kv_quant == "fp8" and m._cache_shape is None and m._kv8 is None
    m.quantize_kv_cache(None)
    assert m._kv_quant is None
    odd = plugin.Transformer(plugin.ModelArgs(dim=96, n_layers=1, n_heads=2, vocab_size=64, multiple_of=32, max_seq_len=64))   # hd 48
    with pytest.raises(ValueError, match="head_dim"):
        odd.quantize_kv_cache("fp8")


def test_peft_refuses_before_any_gpu_use():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    m = _tiny(peft, lora_rank=8)                      # a CPU model: nothing below may need a device
    with pytest.raises(NotImplementedError, match=r"merge_adapters\(\)"):
        m.quantize_kv_cache("fp8")
    assert m._kv_quant is None
    m.quantize_kv_cache(None)                         # restoring the bf16 cache is always fine


def test_eval_parsers_accept_kv_quant():
    from a3vlm_amd import eval_affordance_v2, eval_affordance_with_quant
    a = eval_affordance_v2.get_args_parser().parse_args(["--kv_quant", "fp8"])
    assert a.kv_quant == "fp8" and eval_affordance_v2.get_args_parser().parse_args([]).kv_quant is None
    src = open(eval_affordance_with_quant.__file__).read()
    assert "get_args_parser" in src                   # the --quant script builds on the v2 parser, so it takes the flag too
    with pytest.raises(SystemExit):
        eval_affordance_v2.get_args_parser().parse_args(["--kv_quant", "int8"])


def test_from_pretrained_has_kv_quant():
    import inspect
    from a3vlm_amd.model.meta import MetaModel
    assert inspect.signature(MetaModel.from_pretrained).parameters["kv_quant"].default is None


@pytest.mark.parametrize("hd", [64, 128])
def test_reference_round_trip_within_half_a_step(hd):
    g = torch.Generator().manual_seed(hd)
    x = (torch.randn(3, 2, 19, hd, generator=g) * torch.rand(3, 2, 19, 1, generator=g) * 4).bfloat16().float()
    x[1, 0, 5] = 0                                   # an all-zero row stays finite
    x[2, 1, 7, 3] = 0
    q, s = R.quantize_rows(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.shape == x.shape[:-1]
    amax = x.abs().amax(-1)
    torch.testing.assert_close(s, amax.clamp_min(1e-12) / 448, rtol=1e-6, atol=0)
    dq = R.dequantize_rows(q, s)
    assert torch.isfinite(dq).all() and float(dq[1, 0, 5].abs().max()) == 0
    assert bool(((dq - x).abs().double() <= R.half_step_bound(x, s)).all())
    code = q.view(torch.float8_e4m3fn).float()
    nz = amax > 0
    assert bool((code.abs().amax(-1)[nz] == 448).all())                       # the row maximum maps to +-448
    assert float(R.e4m3_step(torch.tensor(448.0))) == 32 and float(R.e4m3_step(torch.tensor(1.0))) == 0.125
    # cache layouts + the fp64 attention over them: equal to a plain fp64 softmax attention on the dequantised rows
    B, Hkv, S = 3, 2, 19
    k, v = x, x.flip(2)
    kq, vtq, ks, vs = R.quantize_kv(k, v)
    assert kq.shape == (B, Hkv, S, hd) and vtq.shape == (B, Hkv, hd, S) and ks.shape == vs.shape == (B, Hkv, S)
    qv = torch.randn(B, 4, hd, generator=g)
    got = R.decode_attention_fp64(qv, kq, vtq, ks, vs, S)
    f8 = torch.float8_e4m3fn                         # (the products code * scale are exact in fp64, as the attention takes them)
    kd, vd = kq.view(f8).double() * ks[..., None].double(), vtq.transpose(2, 3).contiguous().view(f8).double() * vs[..., None].double()
    for b in range(B):
        for h in range(4):
            p = torch.softmax(kd[b, h // 2] @ qv[b, h].double() / math.sqrt(hd), 0)
            assert float((p @ vd[b, h // 2] - got[b, h]).abs().max()) < 1e-12
