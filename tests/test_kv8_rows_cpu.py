"""CPU (-m "not gpu") checks of the fp8 KV cache on the ragged decode path: the reference module of the GPU test judges a plain fp32
restatement of the rows walk correct in every family and each of its mutants wrong; the restated quantising write; the host
interface (quantize_kv_cache(rows=), from_pretrained(kv_rows=), the eval entries' argument checks) without a device; and the new
entry points in the header, the built library and the ctypes table."""
import inspect
import os
import re

import pytest
import torch

import kv8_ref
import kv8_rows_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_rope_kvquant_rows", "a3v_attention_decode_rows_fp8kv", "a3v_attention_decode_rows_fp8kv_shared",
           "a3v_attention_decode_rows_fp8kv_splits", "a3v_kv8_copy_span", "a3v_llama_decode_step_rows_kv8",
           "a3v_llama_decode_step_rows_kv8_form")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


@pytest.fixture(scope="module")
def cases(built):
    from a3vlm_amd import ops
    return R.cpu_cases(lambda B, H, Sk: ops.attention_decode_plan(B, H, Sk))


def test_entries_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = built.load()
    for name in ENTRIES:
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in include/a3vlm_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name


def test_shapes_are_refused_before_any_launch(built):
    lib = built.load()
    p = 4096          # any non-NULL, 16-B aligned value: a refused call does not dereference it
    assert lib.a3v_rope_kvquant_rows(p, 384, p, 384, p, p, p, p, p, p, 1, 2, 2, 96, 64, None) == -1            # hd
    assert lib.a3v_rope_kvquant_rows(p, 256, p, 256, p, p, p, p, p, p, 1, 2, 1, 64, 100, None) == -1           # Smax % 64
    assert lib.a3v_rope_kvquant_rows(p, 256, p, 256, None, p, p, p, p, p, 1, 2, 1, 64, 64, None) == -3
    assert lib.a3v_attention_decode_rows_fp8kv(p, 256, p, p, p, p, p, 256, p, 1, 1, 1, 1, 256, 64, p, p, None) == -1     # hd
    assert lib.a3v_attention_decode_rows_fp8kv(p, 64, p, p, p, p, p, 64, p, 65, 1, 1, 1, 64, 64, p, p, None) == -1       # sk_max > Smax
    assert lib.a3v_attention_decode_rows_fp8kv(p, 64, p, p, p, p, p, 64, p, 64, 1, 1, 1, 64, 64, p, None, None) == -3    # no counters
    assert lib.a3v_attention_decode_rows_fp8kv_shared(p, 64, p, p, p, p, p, 64, p, p, None, 64, 1, 1, 1, 64, 64, p, p, None) == -3
    assert lib.a3v_kv8_copy_span(p, p, p, p, 1, 0, p, 1, 2, 0, 64, 1, 64, 128, None) == -1                     # span of 64
    assert lib.a3v_kv8_copy_span(p, p, p, p, 1, 0, p, 1, 2, 0, 8, 1, 96, 128, None) == -1                      # hd
    assert lib.a3v_kv8_copy_span(p, p, p, p, 1, 0, p, 1, 2, 8, 8, 1, 64, 128, None) == 0                       # empty span: nothing launched
    assert lib.a3v_kv8_copy_span(p, p, p, p, 1, 0, None, 0, 2, 0, 8, 1, 64, 128, None) == 0                    # no destination
    assert lib.a3v_kv8_copy_span(p, p, p, p, 1, 2, p, 1, 2, 0, 8, 1, 64, 128, None) == -3                      # src_row outside
    # one of src_row / shared alone is an error; a geometry without the fused form is refused by the form query
    assert lib.a3v_llama_decode_step_rows_kv8(None, None, 1, p, p, p, p, p, p, p, p, p, p, None, 0, 1, 256, 4, 4, 64, 512, 64, 1e-5, None) == -3
    assert lib.a3v_llama_decode_step_rows_kv8_form(3, 100, 2, 2, 50, 128, 0) == 0
    for B, H, Sk in ((8, 32, 3500), (1, 2, 1500), (1, 2, 1), (4, 8, 1100)):                                     # a3v_decode_wave_plan's values
        assert lib.a3v_attention_decode_rows_fp8kv_splits(B, H, Sk) == lib.a3v_attention_decode_fp8kv_splits(B, H, Sk)


# ----------------------------------------------------------------------------------------------------------------- the reference
def test_case_table_covers_the_edges(cases):
    sks = {s for c in cases for s in c.sk}
    assert {1, 15, 16, 17, 63, 64, 65, 127, 128, 129} <= sks
    assert any(s <= 0 for s in sks) and any(s > c.sk_max for c in cases for s in c.sk)
    assert {(c.H, c.Hkv, c.hd) for c in cases} == {(4, 2, 64), (8, 2, 128)} and {c.B for c in cases} == {2, 3, 4}
    assert any(c.nsplit > 1 for c in cases) and any(c.nsplit == 1 for c in cases)
    lens = {(c.shared_len(b)[1], c.keys()[b]) for c in cases for b in range(c.B) if c.src}
    assert any(S == 0 for S, _ in lens) and any(S == 64 for S, _ in lens) and any(S > 64 and S == n & ~63 for S, n in lens)
    for m in R.MUTANTS:
        assert any(R.mutant_applies(c, m) for c in cases), m


def test_rows_differ_in_scale_and_dead_positions_are_poisoned(cases):
    c = cases[0]
    inp = R.inputs(c, "bounded")
    valid = c.valid()
    both = valid[0] & valid[1]
    assert bool(both.any()) and bool((inp["ks"][0][:, both] != inp["ks"][1][:, both]).all()) and bool((inp["vs"][0][:, both] != inp["vs"][1][:, both]).all())
    for b in range(c.B):
        dead = ~valid[b]
        assert bool((inp["kq"][b][:, dead] == kv8_ref.NAN_BYTE).all()) and bool((inp["vtq"][b][:, :, dead] == kv8_ref.NAN_BYTE).all())
        assert bool(torch.isinf(inp["ks"][b][:, dead]).all()) and bool(torch.isinf(inp["vs"][b][:, dead]).all())
    S = c.shared_len(1)[1]
    assert S == 64 and not bool(valid[1, :S].any())          # a sibling's own [0, S_b) is dead


@pytest.mark.parametrize("family", R.FAMILIES)
def test_restatement_passes_in_every_family(cases, family):
    for c in cases:
        ref = R.reference(c, family)
        out, part = R.emu(c, ref["inp"])
        ok, ratio, why = R.judge(c, family, ref, out, part if c.nsplit > 1 else None)
        assert ok, (c.id, family, ratio, why)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails(cases, mutant):
    hit = 0
    for c in cases:
        if not R.mutant_applies(c, mutant):
            continue
        ref = R.reference(c, "exact")
        out, part = R.emu(c, ref["inp"], mutant)
        ok, ratio, why = R.judge(c, "exact", ref, out, part if c.nsplit > 1 else None)
        assert not ok, (c.id, mutant, "the exact family accepts the mutant")
        hit += 1
    assert hit


@pytest.mark.parametrize("hd", [64, 128])
def test_restated_quantising_write(hd):
    H, Hkv, Smax, B = 4, 2, 128, 4
    g = torch.Generator().manual_seed(hd)
    qkv = (torch.randn(B, (H + 2 * Hkv) * hd, generator=g) * 3).bfloat16()
    qkv[1, (H + Hkv) * hd:(H + Hkv + 1) * hd] = 0             # an all-zero v row stays finite
    ang = torch.rand(Smax, hd // 2, generator=g) * 6.28
    cos_sin = torch.stack((ang.cos(), ang.sin()), -1)
    pos = [0, 63, -1, Smax]
    q_out, writes = R.rope_kvquant_rows_ref(qkv, cos_sin, pos, H, Hkv, hd, Smax)
    assert writes[2] is None and writes[3] is None and float(q_out[2:].float().abs().sum()) == 0
    x = qkv.float().view(B, H + 2 * Hkv, hd)
    for b in (0, 1):
        p, kq, ks, vq, vs = writes[b]
        assert p == pos[b] and kq.dtype == vq.dtype == torch.uint8 and kq.shape == vq.shape == (Hkv, hd) and ks.shape == vs.shape == (Hkv,)
        # a rotation keeps the norm of a pair: the bf16 k row is the rotated one to half a bf16 ulp, and the codes are those of
        # kv8_ref.quantize_rows on it, so they dequantise within half an e4m3 step
        pair = x[b, H:H + Hkv].view(Hkv, hd // 2, 2)
        kd = kv8_ref.dequantize_rows(kq, ks).view(Hkv, hd // 2, 2)
        n0, n1 = pair.norm(dim=-1), kd.norm(dim=-1)
        assert bool(((n0 - n1).abs() <= 2.0 ** -7 * n0 + 0.75 * ks[:, None] * 32).all())
        v = x[b, H + Hkv:]
        assert bool(((kv8_ref.dequantize_rows(vq, vs) - v).abs().double() <= kv8_ref.half_step_bound(v, vs)).all())
        assert torch.equal(vs, v.abs().amax(-1).clamp_min(1e-12) / 448)
    assert float(kv8_ref.dequantize_rows(writes[1][3], writes[1][4])[0].abs().max()) == 0 and bool(torch.isfinite(writes[1][4]).all())
    if pos[0] == 0:                                           # position 0 of a table with angle 0 would be the identity; here: q moves
        assert not torch.equal(q_out[0], qkv[0, :H * hd])


# ----------------------------------------------------------------------------------------------------------------- host interface
def _tiny(plugin, **kw):
    return plugin.Transformer(plugin.ModelArgs(dim=128, n_layers=1, n_heads=2, vocab_size=64, multiple_of=64, max_seq_len=64, **kw))


def test_quantize_kv_cache_takes_rows():
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    m = _tiny(plugin)
    assert inspect.signature(m.quantize_kv_cache).parameters["rows"].default is False
    m.quantize_kv_cache("fp8", rows=True)
    assert m._kv_quant == "fp8" and m._kv_rows is True and m._cache_shape is None and m._kv8 is None
    m._ragged_check()                                         # the ragged path is open ...
    for what in ("lookup decoding", "forward_verify_rows", "beam_search"):
        with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
            m._ragged_check(what)                             # ... but for what has no fp8 form
    m.quantize_kv_cache("fp8")
    assert m._kv_rows is False
    with pytest.raises(RuntimeError, match=r"quantize_kv_cache\(None\)"):
        m._ragged_check()                                     # without rows: today's refusal
    with pytest.raises(ValueError, match="rows=True"):
        m.quantize_kv_cache(None, rows=True)
    assert m._kv_quant == "fp8"                               # a refused call changes nothing
    m.quantize_kv_cache(None)
    assert m._kv_quant is None and m._kv_rows is False
    m._ragged_check("beam_search")                            # the bf16 cache refuses nothing


def test_peft_and_from_pretrained_take_the_keyword():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    from a3vlm_amd.model.meta import MetaModel
    m = _tiny(peft, lora_rank=8)
    with pytest.raises(NotImplementedError, match=r"merge_adapters\(\)"):
        m.quantize_kv_cache("fp8", rows=True)
    assert inspect.signature(MetaModel.from_pretrained).parameters["kv_rows"].default is False
    with pytest.raises(ValueError, match="kv_quant='fp8'"):
        MetaModel.from_pretrained("/nonexistent-checkpoint-folder", kv_rows=True)


def test_eval_argument_checks():
    from a3vlm_amd import eval_affordance_v2 as ev
    parse = ev.get_args_parser().parse_args
    assert ev.check_kv_quant(parse([])) is False
    assert ev.check_kv_quant(parse(["--kv_quant", "fp8"])) is False                       # generate(): the cache as it was
    assert ev.check_kv_quant(parse(["--kv_quant", "fp8", "--continuous_rows", "8"])) is True
    assert ev.check_kv_quant(parse(["--continuous_rows", "8", "--lookup_decoding", "3", "--temperature", "0"])) is False
    with pytest.raises(SystemExit, match="--lookup_decoding"):
        ev.check_kv_quant(parse(["--kv_quant", "fp8", "--continuous_rows", "4", "--lookup_decoding", "3", "--temperature", "0"]))
    with pytest.raises(SystemExit, match="--num_beams"):
        ev.check_kv_quant(parse(["--kv_quant", "fp8", "--continuous_rows", "4", "--num_beams", "2", "--temperature", "0"]))
    assert "Not with --kv_quant" not in ev.get_args_parser().format_help()
    src = inspect.getsource(ev.main)
    assert src.index("check_kv_quant(args)") < src.index("MetaModel(")                    # before the model is built
