"""Parallel sampling without a GPU: the three entries exist in header, library and ctypes table and refuse bad arguments before any
launch; --num_samples parses and is checked before the model is built; the best-of-n record rule; generate_many's refusals."""
import argparse
import ctypes
import inspect
import os
import re

import pytest

from a3vlm_amd import eval_affordance_v2 as ev
from a3vlm_amd import eval_affordance_with_quant as evq
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_attention_decode_rows_shared", "a3v_kv_copy_span", "a3v_llama_decode_step_rows_shared")
OK, SHAPE, DTYPE, ARG = 0, -1, -2, -3
P = 4096            # a dummy, 16-B aligned, never dereferenced: every refusal comes before any launch


def test_entries_in_header_library_and_table():
    header = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    assert "Shared prompt keys" in header and "BIT-EQUALITY CONTRACT" in header
    L = lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES and getattr(L, name) is not None
    n_plain, n_shared = (len(lib.SIGNATURES[k][1]) for k in ("a3v_attention_decode_rows", "a3v_attention_decode_rows_shared"))
    assert n_shared == n_plain + 2
    n_plain, n_shared = (len(lib.SIGNATURES[k][1]) for k in ("a3v_llama_decode_step_rows", "a3v_llama_decode_step_rows_shared"))
    assert n_shared == n_plain + 2
    assert callable(ops.attention_decode_rows_shared) and callable(ops.kv_copy_span)


def test_kv_copy_span_refusals_before_any_launch():
    f = lib.load().a3v_kv_copy_span
    #            k  vt layers src dst n_dst B  lo  hi  Hkv hd  Smax dtype stream
    assert f(None, P, 2, 0, P, 1, 4, 64, 70, 2, 64, 128, 0, None) == ARG
    assert f(P, None, 2, 0, P, 1, 4, 64, 70, 2, 64, 128, 0, None) == ARG
    assert f(P, P, 2, 0, None, 1, 4, 64, 70, 2, 64, 128, 0, None) == ARG
    assert f(P, P, 2, 4, P, 1, 4, 64, 70, 2, 64, 128, 0, None) == ARG          # the source row is a host value: out of range is an error
    assert f(P, P, 2, -1, P, 1, 4, 64, 70, 2, 64, 128, 0, None) == ARG
    assert f(P, P, 2, 0, P, 1, 4, 64, 128, 2, 64, 128, 0, None) == SHAPE       # hi - lo = 64
    assert f(P, P, 2, 0, P, 1, 4, 70, 64, 2, 64, 128, 0, None) == SHAPE        # hi < lo
    assert f(P, P, 2, 0, P, 1, 4, 100, 130, 2, 64, 128, 0, None) == SHAPE      # hi > Smax
    assert f(P, P, 2, 0, P, 1, 4, 64, 70, 2, 60, 128, 0, None) == SHAPE        # hd % 8
    assert f(P, P, 2, 0, P, 1, 4, 64, 70, 2, 64, 124, 0, None) == SHAPE        # Smax % 8
    assert f(P, P, 2, 0, P, 1, 4, 64, 70, 2, 64, 128, 7, None) == DTYPE
    assert f(P, P, 2, 0, P, 1, 4, 64, 64, 2, 64, 128, 0, None) == OK           # an empty span launches nothing
    assert f(P, P, 2, 0, None, 0, 4, 64, 70, 2, 64, 128, 0, None) == OK        # no destination either


def test_shared_entries_refuse_half_a_pair():
    L = lib.load()
    strides = (ctypes.c_int64 * 12)(512, 512, 64, 2 * 128 * 64, 128 * 64, 64, 2 * 64 * 128, 64 * 128, 128, 512, 512, 64)
    # src_row without shared
    assert L.a3v_attention_decode_rows_shared(P, P, P, P, P, P, None, 100, 2, 8, 2, 64, strides, P, P, 0, None) == ARG
    tab = (lib.LlamaLayer * 1)()
    assert L.a3v_llama_decode_step_rows_shared(tab, 1, P, P, P, P, P, P, P, P, P, P, None, 5, 2, 256, 4, 2, 64, 768, 128, 1e-5, None) == ARG
    assert L.a3v_llama_decode_step_rows_shared(tab, 1, P, P, P, P, P, P, P, P, P, None, P, 5, 2, 256, 4, 2, 64, 768, 128, 1e-5, None) == ARG


def test_python_signatures():
    sig = inspect.signature(plugin.Transformer.forward_inference_rows)
    assert [sig.parameters[k].kind for k in ("src_row", "shared")] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert sig.parameters["src_row"].default is None and sig.parameters["shared"].default is None
    assert list(inspect.signature(plugin.Transformer.share_prefix).parameters) == ["self", "src_row", "dst_rows", "P"]
    assert inspect.signature(MetaModel.generate_many).parameters["n"].default == 1


def test_num_samples_parses():
    for mod in (ev, evq):
        src = inspect.getsource(mod)
        assert "get_args_parser" in src
    p = argparse.ArgumentParser(parents=[ev.get_args_parser()])
    assert p.parse_args([]).num_samples == 1
    a = p.parse_args(["--num_samples", "4", "--continuous_rows", "8"])
    assert a.num_samples == 4 and a.continuous_rows == 8 and ev.check_num_samples(a) == 4
    assert ev.check_num_samples(p.parse_args([])) == 1
    with pytest.raises(SystemExit, match="--continuous_rows"):
        ev.check_num_samples(p.parse_args(["--num_samples", "4", "--continuous_rows", "3"]))
    with pytest.raises(SystemExit, match="--continuous_rows"):
        ev.check_num_samples(p.parse_args(["--num_samples", "2"]))
    with pytest.raises(SystemExit, match="--temperature"):
        ev.check_num_samples(p.parse_args(["--num_samples", "2", "--continuous_rows", "2", "--temperature", "0"]))
    with pytest.raises(SystemExit):
        ev.check_num_samples(p.parse_args(["--num_samples", "0"]))


def _s(fail, lp):
    return {"answer": "", "format_answer": [], "fail": fail, "logprob_sum": lp}


def test_record_selection_rule():
    assert ev.select_sample([_s(True, -1.0), _s(True, -0.5), _s(True, -3.0)]) == 1, "all failed: the largest sum overall"
    assert ev.select_sample([_s(True, -0.1), _s(False, -9.0), _s(True, -0.2)]) == 1, "one passes: it wins whatever its sum"
    assert ev.select_sample([_s(False, -2.0), _s(True, -0.1), _s(False, -1.0)]) == 2, "the most confident well-formed one"
    assert ev.select_sample([_s(False, -1.0), _s(False, -1.0), _s(True, 0.0)]) == 0, "ties go to the first"
    assert ev.select_sample([_s(True, -1.0), _s(True, -1.0)]) == 0
    assert ev.select_sample([_s(False, -4.0)]) == 0


def test_make_record_is_the_eval_loop_rule():
    r = ev.make_record("[0.1, 0.2, 0.5, 0.6]", {"sum": -1.5, "logprobs": [-1.0, -0.5]})
    assert r["fail"] is False and len(r["format_answer"]) == 4 and r["logprob_sum"] == -1.5 and "logprobs" not in r
    r = ev.make_record("no box here")
    assert r["fail"] is True and "logprob_sum" not in r


def test_generate_many_refuses_before_any_device_use():
    nothing = object()                       # not a model: the refusals come before anything of it is touched
    with pytest.raises(ValueError, match="temperature > 0"):
        MetaModel.generate_many(nothing, ["a"], None, batch_rows=4, n=2, temperature=0.0)
    with pytest.raises(ValueError, match="batch_rows"):
        MetaModel.generate_many(nothing, ["a"], None, batch_rows=2, n=3, temperature=0.5)
    with pytest.raises(ValueError):
        MetaModel.generate_many(nothing, ["a"], None, batch_rows=2, n=0, temperature=0.5)
