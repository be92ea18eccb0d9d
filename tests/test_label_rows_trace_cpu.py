"""The host side of the step with ``TrainEngine.label_rows`` on against its recorded call trace (tools/train_step_trace.py --cases
label_rows, no GPU): as tests/test_train_trace_cpu.py, for the second table -- the engines whose last block, final norm, head and loss
run on the labelled rows only, and the engines that fall back to every row."""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("train_step_trace", os.path.join(ROOT, "tools", "train_step_trace.py"))
tst = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tst)

TABLES = sorted(glob.glob(os.path.join(ROOT, "profiles", "label_rows_trace_*.tsv")))
CASES = tst.label_rows_cases()
FALL_BACK = {"lora.recompute": "lora.recompute", "lora.stream_f32": "lora.stream_f32", "zero1": "zero1"}     # -> case of the first table


@pytest.fixture(scope="module")
def table():
    assert len(TABLES) == 1, TABLES
    return tst.read_table(TABLES[0])


def test_case_list_is_the_tables(table):
    assert [name for name, _ in CASES] == list(table)
    assert all(len(rows) > 20 for rows in table.values())


@pytest.mark.parametrize("name,spec", CASES, ids=[name for name, _ in CASES])
def test_step_trace_matches_table(table, name, spec):
    rows = tst.trace(spec)
    j = tst.first_difference(rows, table[name])
    assert j is None, f"{name}: row {j} of {len(rows)} (table: {len(table[name])}): {rows[j] if j < len(rows) else '-'}"
    ops_used = {r.split("\t")[0] for r in rows}
    assert ("gather_rows" in ops_used) == ("scatter_rows" in ops_used) == (name not in FALL_BACK)


@pytest.mark.parametrize("name", sorted(FALL_BACK))
def test_fall_back_engines_run_the_first_tables_rows(name):
    """Recompute, fp32 stream and ZeRO-1 engines make the calls of the every-row step with the switch on, too."""
    first = tst.read_table(sorted(glob.glob(os.path.join(ROOT, "profiles", "train_trace_*.tsv")))[0])[FALL_BACK[name]]
    rows = tst.trace(dict(CASES)[name])
    assert tst.first_difference(rows, first) is None
