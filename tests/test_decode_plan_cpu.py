"""CPU (-m "not gpu") check that the decode step's host decisions are the ones of the commit before the split plan and the fused
layer loop were given one definition each (a3v_decode_wave_plan in a3v_attn.hip, a3v_decode_fused_layers in a3v_decode.hip).

tests/golden/decode_split_plan.json was recorded from the library of that commit (its hash is the file's "parent" field): built
from a clean checkout with `make -C a3vlm_amd/csrc`, loaded without a GPU through A3V_LIB_PATH, and written by

    import json, test_decode_plan_cpu as t
    from a3vlm_amd import lib
    json.dump({"parent": "<hash>", **t.evaluate(lib.load())}, open(t.FIXTURE, "w"), separators=(",", ":"))

evaluate() below is all there is to it: every exported plan / scratch-size / form entry over the grids, flattened in loop order."""
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_split_plan.json")

PLAN_B = (1, 2, 3, 4, 8, 16, 17, 32)
PLAN_H = (1, 2, 4, 8, 32, 40)
PLAN_SK = (1, 63, 64, 65, 127, 128, 129, 300, 1091, 1500, 3500, 4096, 8192)
VERIFY_Q = (1, 4, 8)
FORM_B = (1, 16, 17, 32, 33)
FORM_Q = (1, 2, 4, 5, 8)
FORM_GEOM = ((256, 4, 4, 64, 512), (512, 4, 2, 128, 1536), (4096, 32, 32, 128, 11008), (5120, 40, 40, 128, 13824), (200, 4, 4, 50, 512))
FORM_W8 = (0, 1, 2)


def evaluate(L):
    plan = list(itertools.product(PLAN_B, PLAN_H, PLAN_SK))
    form = list(itertools.product(FORM_B, FORM_GEOM, FORM_W8))
    out = {
        "scratch_floats_hd64": [L.a3v_attention_scratch_floats(B, H, 64, Sk) for B, H, Sk in plan],
        "scratch_floats_hd128": [L.a3v_attention_scratch_floats(B, H, 128, Sk) for B, H, Sk in plan],
        "fp8kv_splits": [L.a3v_attention_decode_fp8kv_splits(B, H, Sk) for B, H, Sk in plan],
        "rows_splits": [L.a3v_attention_decode_rows_splits(B, H, Sk) for B, H, Sk in plan],
        "verify_splits": [L.a3v_attention_verify_rows_splits(B, H, Sk) for B, H, Sk in plan],
        "step_form": [L.a3v_llama_decode_step_form(B, *g, w8) for B, g, w8 in form],
        "rows_form": [L.a3v_llama_decode_step_rows_form(B, *g, w8) for B, g, w8 in form],
        "verify_form": [L.a3v_llama_decode_step_verify_form(B, Q, *g, w8) for B, g, w8 in form for Q in FORM_Q],
    }
    for Q in VERIFY_Q:
        for hd in (64, 128):
            out[f"verify_scratch_floats_q{Q}_hd{hd}"] = [L.a3v_attention_verify_rows_scratch_floats(B, Q, H, hd, Sk) for B, H, Sk in plan]
    return out


@pytest.fixture(scope="module")
def got():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return evaluate(lib.load())


def test_every_plan_and_form_is_the_recorded_one(got):
    want = json.load(open(FIXTURE))
    assert len(want.pop("parent")) == 40
    assert sorted(want) == sorted(got)
    n_plan = len(PLAN_B) * len(PLAN_H) * len(PLAN_SK)
    for name, values in got.items():
        assert len(values) == len(want[name]) and len(values) >= len(FORM_B) * len(FORM_GEOM) * len(FORM_W8), name
        if "form" not in name:
            assert len(values) == n_plan, name
        bad = [i for i, (a, b) in enumerate(zip(values, want[name])) if a != b]
        assert not bad, (name, bad[:5], [values[i] for i in bad[:5]], [want[name][i] for i in bad[:5]])
    # the grid does reach both forms and the refusals, and more than one split
    assert {0, 1, 2} == set(got["step_form"]) and {0, 2} == set(got["rows_form"]) == set(got["verify_form"])
    assert min(got["rows_splits"]) == 1 and max(got["rows_splits"]) > 1


def test_the_three_split_entries_agree(got):
    assert got["fp8kv_splits"] == got["rows_splits"] == got["verify_splits"]
