"""tests/gemm_ref.py without a GPU: the exact inputs are exact, correct fp32 restatements of the GEMM arithmetic stay inside the derived
bound on the very inputs tests/test_gpu_gemm_parity.py uses, five wrong kernels leave it, and the shape table reaches every bf16 / fp32
kernel and dispatch outcome of a3v_gemm_plan.  Run with -s for the ratios."""
import ctypes

import pytest
import torch

import gemm_ref as G
from test_gemm_plan_cpu import FAMILY, OUTCOMES, kernel_names, outcome

IDS = [c.id for c in G.TABLE]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


@pytest.mark.parametrize("cid", IDS)
def test_exact_inputs_are_exact_and_the_bound_is_honest(cid):
    """Per table entry: (exact set) the magnitude condition holds, fp32 matmul and every fp32 restatement give the fp64 reference's bits,
    every mutant changes bits; (bounded sets) every restatement has ratio <= 1, every mutant that applies has ratio > 1."""
    c = G.BY_ID[cid]
    rows = None
    if c.subset or c.M * c.N > 2 ** 22:          # the proof needs the inputs, not every row: rows 0..15 and a third of the GPU test's rows
        r = G.ref_rows(c, force=True)
        rows = torch.cat([r[:16], r[16::3]])
    od = G.out_dtype(c)
    for family in G.FAMILIES:
        inp = G.inputs(c, family)
        r = G.reference(c, inp, rows)
        exact = family == "exact" and r["bits"] is not None
        if family == "exact":
            assert G.exact_budget_ok(c, inp), (cid, "K max|A| max|W| + max|bias| + max|res| >= 2^24")
            prod64, _ = G.product64(c, inp, rows)
            assert torch.equal(G.accumulate(c, inp, rows, "matmul").double(), prod64), (cid, "fp32 matmul != fp64 product")
            if exact:
                want = G.epilogue_f32(c, inp, prod64.float(), rows)
                assert want.dtype == r["bits"].dtype and torch.equal(want, r["bits"]), (cid, "fp64 chain != fp32 chain on exact data")
                frac = float((prod64.float().to(torch.bfloat16).double() != prod64).double().mean())
                assert c.entry == "nt_f32" or frac > 0.5, (cid, "too few results need rounding", frac)
        good = {m: G.emu(c, inp, m, rows) for m in G.RESTATEMENTS}
        ratios = {m: G.ratio(o, r, od) for m, o in good.items()}
        assert max(ratios.values()) <= 1.0, (cid, family, ratios)
        if exact:
            assert all(torch.equal(o, r["bits"]) for o in good.values()), (cid, "a restatement is not bit-exact on exact data")
        mut = {}
        for m in G.MUTANTS:
            if not G.mutant_applies(c, m, family):
                continue
            o = G.emu(c, inp, m, rows)
            if exact:
                mut[m] = float("inf") if not torch.equal(o, r["bits"]) else 0.0
            else:
                mut[m] = G.ratio(o, r, od)
            assert mut[m] > 1.0, (cid, family, m, mut[m])
        print(f"{cid:64s} {family:5s} worst ratio {max(ratios.values()):.3f}   mutants " + " ".join(f"{m}={v:.3g}" for m, v in mut.items()))


def test_every_mutant_is_exercised():
    for m in G.MUTANTS:
        for family in G.FAMILIES:
            if family != "exact" and m == "res_before_rounding":
                continue
            assert sum(G.mutant_applies(c, m, family) for c in G.TABLE) >= 8, (m, family)


def plan_of(lib, names, c):
    fam = "nt_f32" if c.entry == "nt_f32" else c.entry if c.entry in ("tn", "nn") else "tn_sumsq" if c.entry == "tn_sumsq" else "nt"
    family = FAMILY[fam]
    M, N, K = c.M, c.N, c.K
    lda, ldw = (M, N) if family == 2 else (K, N) if family == 3 else (K, K)
    steps = (ctypes.c_int32 * 24)()
    with lib.env(**dict(c.env)):
        n = lib.load().a3v_gemm_plan(family, M, N, K, lda, ldw, c.flags, int(fam == "nt_f32"), 0, 1, int(fam == "tn_sumsq"), 96 << 20, 256, steps)
    assert n > 0, (c.id, n)
    st = [(names[steps[8 * i]], *steps[8 * i + 1:8 * i + 5]) for i in range(n)]
    return outcome(fam, c.flags, st), st


def coverage(lib, table):
    names = kernel_names()
    kernels, outcomes, lines = set(), set(), []
    for c in table:
        if c.entry not in ("nt", "nt_f32", "tn", "tn_sumsq", "nn"):
            continue
        o, st = plan_of(lib, names, c)
        kernels |= {s[0] for s in st}
        outcomes.add(o)
        lines.append(f"{c.id:64s} {o:28s} " + " + ".join(s[0] for s in st))
    return kernels, outcomes, lines


def test_table_reaches_every_kernel_and_outcome(built):
    want_k = {k for k in kernel_names() if "F8" not in k and "FP8" not in k and k != "RING_ROPE"}
    want_o = {o for o in OUTCOMES if o.startswith(("nt_", "tn_", "nn_"))}
    kernels, outcomes, lines = coverage(built, G.TABLE)
    print("\n".join(lines))
    print("kernels:", sorted(kernels))
    print("outcomes:", sorted(outcomes))
    assert kernels == want_k, (sorted(want_k - kernels), sorted(kernels - want_k))
    assert outcomes == want_o, (sorted(want_o - outcomes), sorted(outcomes - want_o))
    # a sole reacher is load-bearing: without it the coverage is no longer complete
    names = kernel_names()
    reach = {}
    for c in G.TABLE:
        if c.entry in ("nt", "nt_f32", "tn", "tn_sumsq", "nn"):
            o, st = plan_of(built, names, c)
            for key in {o} | {s[0] for s in st}:
                reach.setdefault(key, []).append(c)
    for key, cs in reach.items():
        if len(cs) == 1:
            k2, o2, _ = coverage(built, [c for c in G.TABLE if c is not cs[0]])
            assert k2 != want_k or o2 != want_o, key


def test_table_covers_the_entry_points_the_edges_and_the_split_forms():
    T = G.TABLE
    assert {c.entry for c in T} == {"nt", "nt_f32", "tn", "tn_sumsq", "nn", "nt_splitk", "tn_splitk", "tn_strip", "reduce"}
    nt_epi = set().union(*(set(c.epi) for c in T if c.entry == "nt"))
    assert nt_epi >= {"bias", "gelu", "quickgelu", "res", "inplace", "swiglu", "out_f32", "res_f32", "swiglu_bwd"}
    assert any("swiglu_bwd" in c.epi for c in T if c.entry == "nn")
    for tile, t in G.TILE_ROWS.items():
        f = [c for c in T if c.tile == tile and c.macs < 2 ** 26]
        assert {c.M for c in f} >= {1, t - 1, t, t + 1} and {c.N for c in f} >= {4, 124, 132, 252, 260} and {c.K for c in f} >= {64, 128, 192, 320}
        assert any(c.M % t and c.N % 128 for c in f)
        big = [c for c in T if c.tile == tile and c.tile in ("256pp", "192pp") and (c.M + t - 1) // t * ((c.N + 255) // 256) > 256]
        assert tile in ("128", "256") or ({c.K for c in big} >= {64, 192} and {("bias" in c.epi) for c in big} == {True, False})
    assert {c.K for c in T if c.entry == "tn"} >= {8, 63, 64, 65, 130} and all(c.M % 8 == 0 for c in T if c.entry.startswith("tn"))
    assert all(c.N % 8 == 0 for c in T if c.entry == "nn")
    for e in ("nt_splitk", "tn_splitk", "tn_strip"):
        f = [c for c in T if c.entry == e]
        assert any(c.S == 1 for c in f) and any(c.S == G.ktiles(c) for c in f) and any(c.S == 3 and G.ktiles(c) == 7 for c in f)
        assert any(c.S == 7 and G.ktiles(c) == 7 for c in f) and {c.acc for c in f} == {0, 1} and {c.out for c in f} == {"bf16", "f32"}
    sk = [c for c in T if c.entry == "nt_splitk" and c.M >= 512 and c.N <= 64]
    blocks = [c.S * ((c.M + 255) // 256) for c in sk]
    assert any(128 < b <= 256 for b in blocks) and any(b <= 128 for b in blocks)
    assert {c.M for c in T if c.entry == "tn_strip"} == {8, 16, 48, 64}
    red = [c for c in T if c.entry == "reduce"]
    assert {(c.acc, c.out) for c in red} == {(0, "bf16"), (1, "bf16"), (0, "f32"), (1, "f32")}
    multi = [c for c in T if c.subset or (c.entry == "nt" and c.env)]
    assert all(G.has_res(c) for c in multi)


def test_cost_cap():
    assert len(G.TABLE) <= G.MAX_ENTRIES
    for c in G.TABLE:
        assert c.macs <= G.MAX_MACS, c.id
        assert c.subset == (c.macs > G.SUBSET_MACS), (c.id, "entries above 2^33 multiply-adds are marked: reference on a row subset")
        if c.subset:
            rows = G.ref_rows(c)
            assert len(rows) < c.M // 4 and {0, c.M - 1} <= set(rows.tolist())
