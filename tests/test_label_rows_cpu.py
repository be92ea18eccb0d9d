"""No GPU: the torch reference of the labelled-row list (``a3vlm_amd.train.label_rows_ref``: what a3v_label_rows computes, in both
coordinate systems) against hand-written cases, and ``TrainEngine``'s decisions to run every row instead."""
import types

import torch

from a3vlm_amd.train import TrainEngine, label_rows_ref

BF, F32 = torch.bfloat16, torch.float32


def _lab(rows):
    return torch.tensor(rows, dtype=torch.int64)


def test_row_list_one_answer_per_sample():
    # B = 2, T = 5, W = 3 image words: S = 8; shifted labels
    srows, hrows, labs = label_rows_ref(_lab([[0, 0, 7, 9, 0], [0, 5, 6, 0, 0]]), 3, 8)
    assert srows.tolist() == [5, 6, 12, 13] and hrows.tolist() == [2, 3, 6, 7] and labs.tolist() == [7, 9, 5, 6]
    assert srows.dtype == torch.int32 and hrows.dtype == torch.int32


def test_row_list_segments_empty_sample_and_no_image():
    srows, hrows, labs = label_rows_ref(_lab([[4, 0, 0, 2, 2, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]]), 0, 6)
    assert srows.tolist() == hrows.tolist() == [0, 3, 4, 17] and labs.tolist() == [4, 2, 2, 1]
    srows, hrows, _ = label_rows_ref(_lab([[4, 0, 0, 2, 2, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]]), 10, 16)
    assert srows.tolist() == [10, 13, 14, 47] and hrows.tolist() == [0, 3, 4, 17]


def test_row_list_none_and_all():
    srows, hrows, labs = label_rows_ref(_lab([[0, 0, 0], [0, 0, 0]]), 2, 5)
    assert srows.numel() == hrows.numel() == labs.numel() == 0
    srows, hrows, labs = label_rows_ref(_lab([[3, 4, -1], [5, 6, 7]]), 2, 5)          # (any non-zero label counts, as in a3v_count_valid)
    assert srows.tolist() == [2, 3, 4, 7, 8, 9] and hrows.tolist() == [0, 1, 2, 3, 4, 5]


def _stub(**kw):
    base = dict(label_rows=True, recompute=False, zero1_world=0, stream=BF, act=BF)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_engines_that_run_every_row():
    ok = TrainEngine._label_rows_engine
    assert ok(_stub())
    assert not ok(_stub(label_rows=False))            # A3V_LABEL_ROWS=0
    assert not ok(_stub(recompute=True))              # blocks recomputed in backward
    assert not ok(_stub(stream=F32))                  # fp32 stream
    assert not ok(_stub(stream=F32, act=F32))
    assert not ok(_stub(zero1_world=2))               # ZeRO-1


def test_row_counts_that_run_every_row():
    take = TrainEngine._label_rows_take
    assert not take(0, 100)                           # no labelled row: nothing of zero size is launched
    assert not take(100, 100)                         # nothing to leave out
    assert take(1, 100) and take(99, 100)


def test_count_zero_falls_back_and_a_count_gives_the_row_views(monkeypatch):
    """_label_rows returns None for n = 0; for n > 0 the first n entries of the row buffers and the capacity B T of the compact buffers."""
    from a3vlm_amd import ops
    eng = _stub(_label_rows_take=TrainEngine._label_rows_take)
    eng._buf = lambda name, shape, dtype=None, zero=False: torch.zeros(*shape, dtype=dtype)
    for n, want in ((0, False), (7, True)):
        monkeypatch.setattr(ops, "label_rows", lambda *a, _n=n: _n)
        got = TrainEngine._label_rows(eng, torch.zeros(2, 6, dtype=torch.int64), 3, 9)
        assert (got is not None) == want
    assert got["n"] == 7 and got["cap"] == 12 and got["rows"].numel() == 7 and got["head"].numel() == 7 and got["lab"].numel() == 7


def test_labelled_row_buffers_keep_one_set_whatever_n_does():
    """_sel_buf: a buffer of n rows is a view of ONE buffer of cap rows; anything else is a view of one flat scratch that only grows."""
    eng = _stub(_ws={}, m=types.SimpleNamespace(_device="cpu"), _sel_rows=None)
    eng._sel_buf = types.MethodType(TrainEngine._sel_buf, eng)
    seen = set()
    for n in (5, 9, 3):
        eng._sel_rows = (n, 12)
        t = TrainEngine._buf(eng, "gu", (n, 16), BF)
        s1 = TrainEngine._buf(eng, "splitk", (4 * n * 8,), F32, zero=True)
        assert tuple(t.shape) == (n, 16) and t.is_contiguous() and s1.numel() == 32 * n and not bool(s1.any())
        seen.add((t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()))
    assert len(seen) == 1 and len(eng._ws) == 2 and all(".sel" in k[0] for k in eng._ws)
    assert eng._ws[("splitk.sel", "flat", F32)].numel() == 32 * 9
    eng._sel_rows = None
    assert TrainEngine._buf(eng, "gu", (5, 16), BF).untyped_storage().data_ptr() not in {p for p, _ in seen}
