"""Arena and job-table planning of the one-launch gradient finish (a3vlm_amd.grad_finish), without a GPU: slice offsets and sizes,
no overlap, the budget decision, the a3v_finish_job rows the kernel reads, and that a step shape builds its table once."""
import pytest
import torch

from a3vlm_amd import grad_finish as gf
from a3vlm_amd.lib import SIGNATURES


def _plan(budget=1 << 30):
    p = gf.FinishPlan(budget)
    p.add_planes(("L0", "gA"), 48, 4096, 16, dst=0x10000, ldo=4096)
    p.add_scatter(("L0", "gB"), 48, 12288, 6, 16, dsts=(0x20000, 0x30000, 0x40000), row0s=(0, 4096, 8192), njs=(4096, 4096, 4096))
    p.add_colsum(("L0", "norm"), 137, 4100, dst=0x50000)
    p.add_planes(("L1", "gA"), 20, 260, 3, dst=0x60000, ldo=264, accumulate=False)
    return p


def test_slices_are_aligned_sized_and_disjoint():
    p = _plan()
    assert p.close() and p.fits
    spans = sorted((s.offset, s.offset + s.floats) for s in p.slots.values())
    assert spans[0][0] == 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0                                   # no two slices share a float
    for s in p.slots.values():
        assert s.offset % gf.SLICE_ALIGN == 0
    sizes = {k: s.floats for k, s in p.slots.items()}
    assert sizes == {("L0", "gA"): 16 * 48 * 4096, ("L0", "gB"): 6 * 48 * 12288, ("L0", "norm"): 137 * 4100, ("L1", "gA"): 3 * 20 * 260}
    assert p.total_floats >= spans[-1][1] and p.bytes == 4 * p.total_floats
    with pytest.raises(RuntimeError):
        p.add_colsum("late", 8, 256, dst=0x70000)         # the arena's size is final once closed


def test_budget_decides_and_an_empty_plan_never_fits():
    p = _plan()
    need = 4 * p.total_floats
    assert gf.FinishPlan(need).budget_bytes == need
    q = _plan(budget=need)
    assert q.close()
    q = _plan(budget=need - 1)
    assert not q.close() and not q.fits
    assert not gf.FinishPlan(1 << 30).close()


def test_unit_counts_follow_the_kernel():
    assert gf.job_units(gf.PLANES, 48, 4096) == 48 * 1024 // 256
    assert gf.job_units(gf.PLANES, 20, 260) == -(-20 * 65 // 256) == 6
    assert gf.job_units(gf.SCATTER, 64, 384, (200, 120, 64)) == 4 + 2 + 1
    assert gf.job_units(gf.COLSUM, 0, 4100) == 16 * 5
    assert gf.job_units(gf.COLSUM, 0, 256) == 16


def test_rows_carry_pointers_counts_and_running_units():
    p = _plan()
    p.close()
    base = 0x7000000
    rows, units = p.rows({("L0", "norm"): 100, ("L0", "gA"): 9, ("L1", "gA"): 1, ("L0", "gB"): 6}, base)
    assert [len(r) for r in rows] == [gf.JOB_FIELDS] * 4
    s = p.slots
    ga, gb, nm, g1 = rows                                 # plan order, whatever order the counts came in
    assert ga[:9] == [gf.PLANES, base, 9, 48, 4096, 4096, 1, 0, 0] and ga[9:13] == [0x10000, 0, 0, 0] and ga[21] == 0
    assert gb[:9] == [gf.SCATTER, base + 4 * s[("L0", "gB")].offset, 6, 48, 12288, 0, 1, 16, 3]
    assert gb[9:13] == [0x20000, 0x30000, 0x40000, 0] and gb[13:17] == [0, 4096, 8192, 0] and gb[17:21] == [4096, 4096, 4096, 0]
    assert gb[21] == 192
    assert nm[:5] == [gf.COLSUM, base + 4 * s[("L0", "norm")].offset, 1, 100, 4100] and nm[21] == 192 + 192
    assert g1[:7] == [gf.PLANES, base + 4 * s[("L1", "gA")].offset, 1, 20, 260, 264, 0] and g1[21] == 192 + 192 + 80
    assert units == 192 + 192 + 80 + 6
    sub, u = p.rows({("L0", "gB"): 2}, base)              # a step that ran only some producers
    assert len(sub) == 1 and sub[0][21] == 0 and u == 192
    with pytest.raises(ValueError):
        p.rows({("L0", "gA"): 17}, base)                  # more planes than the slice holds
    with pytest.raises(KeyError):
        p.rows({"unknown": 1}, base)
    with pytest.raises(ValueError):
        p.rows({("L0", "gA"): 1}, base + 4)               # arena not 16-byte aligned


@pytest.mark.parametrize("bad", [
    dict(kind="planes", R=16, N=258, dst=0x100, ldo=260),                 # N no multiple of 4
    dict(kind="planes", R=16, N=256, dst=0x104, ldo=256),                 # destination not 16-byte aligned
    dict(kind="planes", R=16, N=256, dst=0x100, ldo=128),                 # rows of the destination overlap
    dict(kind="scatter", r=6, njs=(128, 128), row0s=(0, 128)),            # rank no multiple of 4
    dict(kind="scatter", r=16, njs=(130, 126), row0s=(0, 130)),           # a block's width no multiple of 4
    dict(kind="scatter", r=16, njs=(128, 192), row0s=(0, 128)),           # a block past the plane's columns
    dict(kind="scatter", r=32, njs=(64, 64, 128), row0s=(0, 64, 128)),    # more adapter rows than plane rows
])
def test_shapes_the_kernel_does_not_take_are_refused(bad):
    p = gf.FinishPlan(1 << 30)
    with pytest.raises(ValueError):
        if bad["kind"] == "planes":
            p.add_planes("k", bad["R"], bad["N"], 4, bad["dst"], bad["ldo"])
        else:
            p.add_scatter("k", 64, 256, 4, bad["r"], [0x100 * (j + 1) for j in range(len(bad["njs"]))], bad["row0s"], bad["njs"])
    assert not p.slots and p.total_floats == 0
    p.add_colsum("k", 4, 256, 0x100)
    with pytest.raises(ValueError):
        p.add_colsum("k", 4, 256, 0x100)                  # one slice per producer call


def test_table_is_built_once_per_step_shape():
    fin = gf.GradFinisher(1 << 30, flat_ptr=0)
    fin.plan.add_planes("a", 16, 256, 4, dst=0x100, ldo=256)
    fin.plan.add_colsum("n", 32, 256, dst=0x4000)
    assert fin.commit("cpu") and fin.arena.numel() == fin.plan.total_floats and fin.arena.dtype == torch.float32
    t1 = fin.table({"a": 4, "n": 30})
    t2 = fin.table({"n": 30, "a": 4})
    assert t1[0] is t2[0] and fin.tables_built == 1 and t1[1:] == (2, 4 + 16)
    assert t1[0].dtype == torch.int64 and tuple(t1[0].shape) == (2, gf.JOB_FIELDS)
    assert t1[0][0, 1].item() == fin.arena.data_ptr() and t1[0][1, 1].item() == fin.arena.data_ptr() + 4 * fin.plan.slots["n"].offset
    fin.table({"a": 3, "n": 30})                          # another row count: another table, the first one is kept
    assert fin.tables_built == 2 and fin.table({"a": 4, "n": 30})[0] is t1[0] and fin.tables_built == 2
    small = gf.GradFinisher(64, flat_ptr=0)               # over budget: no arena, the engine keeps its per-call reduces
    small.plan.add_colsum("n", 32, 256, dst=0x4000)
    assert not small.commit("cpu") and small.arena is None


def test_signatures_name_the_new_exports():
    assert len(SIGNATURES["a3v_grad_finish_multi"][1]) == 5 and len(SIGNATURES["a3v_rmsnorm_bwd_parts_bf16"][1]) == 13
