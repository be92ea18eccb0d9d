"""The GEMM dispatch, without a GPU: a3v_gemm_plan (the plan the a3v_gemm_nt / _nt_fp8 / _tn / _nn entry points execute) against
profiles/gemm_dispatch_cf018f4.tsv, the launch sequences commit cf018f4 -- the last one whose dispatchers decided and launched in one
piece -- produced for the same rows at 256 CUs (kernel, grid x, grid y, block and xmap per launch)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSV = os.path.join(ROOT, "profiles", "gemm_dispatch_cf018f4.tsv")
FAMILY = {"nt": 0, "nt_ub": 0, "nt_f32": 0, "nt_rope": 0, "fp8": 1, "fp8_rope": 1, "tn": 2, "tn_sumsq": 2, "nn": 3}   # nt_ub: bias not 8-byte aligned
BIAS, TILES = 1, {1 << 16: "128", 1 << 17: "256", 1 << 18: "256pp", 1 << 23: "192pp"}

# every outcome of the dispatch the table has to reach ("no_ws": the same shapes without a registered workspace)
OUTCOMES = {"nt_small", "nt_ring_256", "nt_ring_192", "nt_ring_split", "nt_hybrid_ring_tail", "nt_hybrid_small_split_tail",
            "nt_hybrid_plain_tail", "nt_forced_128", "nt_forced_256", "nt_forced_256pp", "nt_forced_192pp", "nt_f32",
            "tn_one", "tn_tail", "nn_one", "nn_tail", "fp8_one", "fp8_tail", "fp8_192", "fp8_two_stage_bias", "no_ws"}
# kernel ids the table need not contain, each with its reason
NOT_IN_TABLE = {}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


def kernel_names():
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src[src.index("A3V_GEMM_K_NT_128 = 0"):src.index("A3V_GEMM_K_COUNT")], flags=re.S)
    return re.findall(r"A3V_GEMM_K_(\w+)", body)


def table():
    rows = []
    for line in open(TSV):
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\n").split("\t")
        env = dict(kv.split("=") for kv in f[7].split(",")) if f[7] != "-" else {}
        steps = [(s.split()[0], *map(int, s.split()[1:])) for s in f[8:]]
        rows.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), env, steps))
    return rows


def outcome(fam, epi, steps):
    k = [s[0] for s in steps]
    split = k[-1] == "REDUCE"
    if fam == "nt_f32":
        return "nt_f32"
    if fam in ("nt", "nt_ub", "nt_rope"):
        forced = [name for bit, name in TILES.items() if epi & bit]
        if forced:
            return "nt_forced_" + forced[0]
        if len(k) == 1:
            return "nt_small" if k[0] == "NT_128" else "nt_ring_192" if "192" in k[0] else "nt_ring_256"
        if len(k) == 2 and split:
            return "nt_ring_split"
        return "nt_hybrid_plain_tail" if not split else "nt_hybrid_ring_tail" if k[1] == "RING" else "nt_hybrid_small_split_tail"
    if fam in ("fp8", "fp8_rope"):
        if epi & BIAS:
            assert k == ["FP8_PP"]
            return "fp8_two_stage_bias"
        return "fp8_192" if "192" in k[0] else "fp8_tail" if split else "fp8_one"
    return fam[:2] + ("_tail" if split else "_one")


def test_plan_equals_the_recorded_dispatch(built):
    lib = built.load()
    names = kernel_names()
    rows = table()
    steps = (ctypes.c_int32 * 24)()
    for fam, M, N, K, epi, rope, ws, env, want in rows:
        family = FAMILY[fam]
        lda, ldw = (M, N) if family == 2 else (K, N) if family == 3 else (K, K)
        with built.env(**env):
            n = lib.a3v_gemm_plan(family, M, N, K, lda, ldw, epi, int(fam == "nt_f32"), rope, int(fam != "nt_ub"), int(fam == "tn_sumsq"), ws, 256,
                                      steps)
        assert n == len(want), (fam, M, N, K, epi, ws, env, n)
        got = [(names[steps[8 * i]], *steps[8 * i + 1:8 * i + 5]) for i in range(n)]
        assert got == want, (fam, M, N, K, epi, ws, env)
        # the fields the trace cannot see: rows covered (whole problem, or big rows + tail) and the slices = the split launch's grid y
        body = [steps[8 * i:8 * i + 8] for i in range(n) if names[steps[8 * i]] != "REDUCE"]
        assert body[0][5] == 0 and sum(s[6] for s in body) == M and all(s[7] == s[2] for s in body if names[s[0]] != "F32")


def test_the_table_is_not_thin():
    rows = table()
    assert len(rows) >= 150
    seen = {s[0] for r in rows for s in r[8]}
    assert set(NOT_IN_TABLE) <= set(kernel_names())
    assert seen | set(NOT_IN_TABLE) == set(kernel_names()), sorted(set(kernel_names()) - seen)
    got = {outcome(r[0], r[4], r[8]) for r in rows} | ({"no_ws"} if any(r[6] == 0 for r in rows) else set())
    assert OUTCOMES <= got, sorted(OUTCOMES - got)
    # xmap values other than the default, and an unaligned bias that turns the whole-problem split down
    assert {s[4] for r in rows for s in r[8]} >= {0, 1, 5}
    ub = {r[0]: r[8] for r in rows if r[1:5] == (2056, 1024, 4096, 9) and r[6] > (1 << 20)}
    assert ub["nt"][-1][0] == "REDUCE" and ub["nt_ub"][-1][0] != "REDUCE"
    # the same shape with and without a workspace, where the workspace changes the outcome
    with_ws = {r[:5]: r[8] for r in rows if r[6] > (1 << 20) and not r[7]}
    assert any(r[6] == 0 and not r[7] and r[:5] in with_ws and with_ws[r[:5]] != r[8] for r in rows)


def test_plan_refuses_what_it_cannot_plan(built):
    lib = built.load()
    steps = (ctypes.c_int32 * 24)()
    assert lib.a3v_gemm_plan(0, 0, 64, 64, 64, 64, 0, 0, 0, 1, 0, 0, 256, steps) == -3
    assert lib.a3v_gemm_plan(7, 64, 64, 64, 64, 64, 0, 0, 0, 1, 0, 0, 256, steps) == -3
    assert lib.a3v_gemm_plan(0, 64, 64, 64, 64, 64, 0, 2, 0, 1, 0, 0, 256, steps) == -2
    assert lib.a3v_gemm_plan(0, 70000, 1024, 16384, 16384, 16384, 1 << 18, 0, 0, 1, 0, 0, 256, steps) == -1      # A beyond 2 GiB on a ring tile


def test_the_table_has_the_rows_of_the_trace_driver():
    """tools/gemm_dispatch_trace.py (the GPU run whose kernel trace the table can be checked against) lists the same rows in the same order."""
    import sys
    sys.path.insert(0, ROOT)
    from tools.gemm_dispatch_trace import rows
    assert [(r[0], *r[1:5], r[6], {k: str(v) for k, v in r[7].items()}) for r in table()] == \
           [(f, M, N, K, epi, ws, {k: str(v) for k, v in env.items()}) for f, M, N, K, epi, ws, env in rows()]
