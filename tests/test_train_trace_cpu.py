"""The host side of the training step against its recorded call trace (tools/train_step_trace.py, no GPU): every ``a3vlm_amd.ops`` call
of two steps -- op, operand dtypes / shapes / strides / storage identities, scalars -- and every request to the weight images, for each
engine configuration of the table, row for row (the table keeps a digest of each row).  The table was made from the commit in its file name; a change of ``TrainEngine`` that
is meant to leave the launch sequence alone leaves every row alone."""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("train_step_trace", os.path.join(ROOT, "tools", "train_step_trace.py"))
tst = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tst)

TABLES = sorted(glob.glob(os.path.join(ROOT, "profiles", "train_trace_*.tsv")))
CASES = tst.cases()


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
