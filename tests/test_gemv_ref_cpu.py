"""tests/gemv_ref.py without a GPU: the exact inputs are exact, correct fp32 restatements of the decode GEMV arithmetic stay inside the
derived bound on the very inputs tests/test_gpu_gemv_parity.py uses and equal the reference's bits on the exact sets, eleven wrong kernels
are caught, at most 1 % of a prologue input is fragile, and every table entry gets the plan it names from a3v_gemv_plan (256 CUs).
Run with -s for the ratios."""
import ctypes

import pytest
import torch

import gemv_ref as R

IDS = [c.id for c in R.TABLE]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


@pytest.mark.parametrize("cid", IDS)
def test_exact_inputs_are_exact_and_the_bound_is_honest(cid):
    """Per table entry: (exact set) the budget holds and every restatement gives the reference's bits, every mutant that applies changes
    them; (bounded sets) every restatement has ratio <= 1, every mutant that applies has ratio > 1; the fragile share is below its cap."""
    c = R.BY_ID[cid]
    for family in R.FAMILIES:
        inp = R.inputs(c, family)
        r = R.reference(c, inp, family)
        has_bits = r["C"]["bits"] is not None
        if family == "exact":
            assert R.exact_budget_ok(c, inp), (cid, "the exact budget of the module docstring does not hold")
            assert has_bits == ("swiglu" not in c.epi), cid
        elif "pro" in c.fused:
            _, fragile = R.prologue64(c, inp)
            share = float(fragile.double().mean())
            assert share <= R.FRAGILE_CAP, (cid, family, share)
        good = {m: R.judge(c, r, R.emu(c, inp, m)) for m in R.RESTATEMENTS}
        assert max(v[1] for v in good.values()) <= 1.0, (cid, family, good)
        if has_bits:
            assert all(v[0] is True for v in good.values()), (cid, "a restatement is not bit-exact on exact data", good)
        mut = {}
        for m in R.MUTANTS:
            if not R.mutant_applies(c, m, family):
                continue
            eq, ratio = R.judge(c, r, R.emu(c, inp, m))
            mut[m] = (float("inf") if not eq else 0.0) if has_bits else ratio
            assert mut[m] > 1.0, (cid, family, m, mut[m])
        print(f"{cid:48s} {family:5s} worst ratio {max(v[1] for v in good.values()):.3f}   mutants " + " ".join(f"{m}={v:.3g}" for m, v in mut.items()))


def test_every_mutant_is_exercised():
    for m in R.MUTANTS:
        fams = [f for f in R.FAMILIES if any(R.mutant_applies(c, m, f) for c in R.TABLE)]
        assert fams, m
        for f in fams:
            assert sum(R.mutant_applies(c, m, f) for c in R.TABLE) >= 4, (m, f)
    assert len(R.MUTANTS) == 11 and len(R.RESTATEMENTS) == 3


def plan_of(lib, c, cus=256):
    plan = (ctypes.c_int32 * 13)()
    with lib.env(**c.env):
        rc = lib.load().a3v_gemv_plan(c.M, c.N, c.K, c.flags, R.FMT[c.fmt], int("pro" in c.fused), int("rope" in c.fused),
                                      int("ssq" in c.fused), 1, cus, plan)
    return rc, (plan[0], plan[1], plan[7], plan[11])


def test_the_table_agrees_with_the_plan(built):
    for c in R.TABLE:
        rc, got = plan_of(built, c)
        assert rc == c.plan[0] and got == tuple(c.plan), (c.id, rc, got, c.plan)
        assert not (c.fused and rc in (R.DIRECT1, R.DIRECT2)), (c.id, "the fused forms have no direct kernel")
    for c, want in R.REFUSALS:
        if want == R.ERR_SHAPE:                   # no LDS-DMA kernel can run it: the plan names a direct kernel, which the fused entry refuses
            rc, _ = plan_of(built, c)
            assert rc in (R.ERR_SHAPE, R.DIRECT1, R.DIRECT2), (c.id, rc)


def test_table_covers_what_the_family_can_do():
    T = R.TABLE
    pub = [c for c in T if not c.fused]
    assert {c.M for c in pub} >= {1, 7, 8, 9, 15, 16}
    assert {c.N for c in pub if "swiglu" not in c.epi} >= {4, 20, 60, 64, 68, 132}
    assert all(c.N % 32 == 0 for c in T if "swiglu" in c.epi) and any(c.N == 96 for c in T if "swiglu" in c.epi)
    forms = {(c.fmt, c.plan[0], c.plan[1], "pro" in c.fused) for c in T}
    for fmt in ("bf16", "fp8", "nf4"):                       # the twelve template forms of the across-blocks kernel
        for arows in (8, 16):
            for pro in (False, True):
                assert (fmt, R.DMA, arows, pro) in forms, (fmt, arows, pro)
        f = [c for c in T if c.fmt == fmt]
        assert {frozenset(c.epi) for c in f if not c.fused} >= {frozenset(), frozenset({"res"}), frozenset({"out_f32"}),
                                                                 frozenset({"res", "out_f32"}), frozenset({"swiglu"})}
        assert {frozenset(c.fused) for c in f if c.plan[0] == R.DMA} >= {frozenset({"pro", "rope"}), frozenset({"pro"}), frozenset({"ssq"})}
        assert {c.geom[:3] for c in f if c.geom} == {(2, 1, 16), (1, 1, 128)} and {c.geom[3] for c in f if c.geom} == {0, 5, 23}
        assert any(c.N == 68 for c in f)
    assert ("bf16", R.KQ, 8, False) in forms and ("bf16", R.KQ, 8, True) in forms
    assert {c.plan[0] for c in T} == {R.DMA, R.KQ, R.DIRECT1, R.DIRECT2}
    dma = [c for c in T if c.fmt == "bf16" and c.plan[0] == R.DMA]
    assert {c.K for c in dma} >= {128, 256, 384, 640, 1408, 3200} and {c.plan[2] for c in dma} == {1, 2, 4, 8}
    kq = [c for c in T if c.plan[0] == R.KQ]
    assert any(c.kq is None and c.N == 4096 for c in kq) and any(c.plan[3] < c.plan[2] for c in kq) and any(c.M == 1 for c in kq)
    assert any("swiglu" in c.epi and c.plan[3] == 6 for c in kq) and {frozenset(c.fused) for c in kq} >= {frozenset({"pro", "rope"}), frozenset({"ssq"})}
    assert {c.K for c in T if c.plan[0] == R.DIRECT1} >= {32, 96, 160, 2080, 245760} and any(c.K == 128 for c in T if c.plan[0] == R.DIRECT2)
    assert {c.K for c in T if c.fmt == "fp8"} >= {256, 512, 768, 6400} and {c.K for c in T if c.fmt == "nf4"} >= {256, 512, 768, 10496}
    assert any("ssq" in c.fused and "res" in c.epi for c in T)
    assert {rc for _, rc in R.REFUSALS} == {R.ERR_SHAPE, R.ERR_ARG}


def test_cost_cap():
    assert len(R.TABLE) <= R.MAX_ENTRIES
    for c in R.TABLE:
        assert c.macs <= R.MAX_MACS, c.id


def test_the_code_book_is_the_bf16_rounding_of_nf4():
    from nf4_ref import NF4
    assert torch.equal(R.CODES.float(), NF4.to(torch.bfloat16).float())
    assert bool((R.CODES * 2 ** 11 == (R.CODES * 2 ** 11).round()).all()) and float(R.CODES.abs().max()) == 1.0
