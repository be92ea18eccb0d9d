"""The decode GEMV dispatch, without a GPU: a3v_gemv_plan (the plan a3v_gemm_skinny / _fp8 / _nf4 and the decode step's fused GEMVs execute)
against profiles/gemv_dispatch_de04e97.tsv, the launch commit de04e97 -- the last one whose GEMV entry points decided and launched in one
piece -- made for the same rows: kernel with template arguments, grid, block, dynamic LDS bytes, size of the argument struct, the split
values in it (S, nkb, tgs, maxkb; kslice of the direct kernels) and a hash of its bytes as the recorder filled it, or the error code."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TSV = os.path.join(ROOT, "profiles", "gemv_dispatch_de04e97.tsv")
SWIGLU = 16
DMA, KQ, DIRECT1, DIRECT2 = range(4)
ERR_SHAPE, ERR_ARG = -1, -3

# every outcome of the dispatch the table has to reach
OUTCOMES = {"kq_taken", "kq_uneven_tiles", "kq_forced", "kq_forbidden", "kq_swiglu_cap_6", "kq_fewer_slices_short_k", "kq_unaligned_a",
            "kq_prologue", "kq_16_rows_never", "kq_quantised_never", "dma_8_rows", "dma_16_rows", "direct_k_96", "direct_swiglu_one_slice",
            "direct_lds_limit", "direct_pair", "none_fp8", "none_nf4", "none_fused", "second_cu_count"}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


def kernel_ids():
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src[src.index("A3V_GEMV_K_DMA = 0"):src.index("A3V_GEMV_K_COUNT")], flags=re.S)
    return re.findall(r"A3V_GEMV_K_(\w+)", body)


def table():
    """[(row as tools/gemv_dispatch_trace.rows() spells it, launch)]; launch: (kernel, grid, block, lds, argsize, S, nkb, tgs, maxkb, kslice) or ("ERR", rc)"""
    out = []
    for line in open(TSV):
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\n").split("\t")
        env = dict(kv.split("=") for kv in f[8].split(",")) if f[8] != "-" else {}
        launch = f[9].split()
        out.append(((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], int(f[6]), int(f[7]), env), (launch[0], *map(int, launch[1:10]))))
    return out


def plan_of(built, row):
    from tools.gemv_dispatch_trace import plan_args
    plan = (ctypes.c_int32 * 13)()
    with built.env(**row[8]):
        rc = built.load().a3v_gemv_plan(*plan_args(row), plan)
    return rc, list(plan)


def test_plan_equals_the_recorded_dispatch(built):
    from tools.gemv_dispatch_trace import kernel_name
    for row, want in table():
        rc, p = plan_of(built, row)
        fused = row[5] != "-"
        if want[0] == "ERR":
            # no kernel, or (the fused forms have no fallback) only a direct kernel
            assert want[1] == ERR_SHAPE and (rc == ERR_SHAPE or (rc in (DIRECT1, DIRECT2) and fused)), (row, rc)
            continue
        assert rc == p[0] and 0 <= rc < 4, (row, rc)
        kernel, arows, pro, fmt, grid, block, lds, S, nkb, tgs, maxkb, slices, kslice = p
        direct = rc in (DIRECT1, DIRECT2)
        assert not (direct and (fused or row[0] != "bf16")), row
        got = (kernel_name(p), grid, block, lds, 88 if direct else 200, S, nkb, tgs, maxkb, kslice)
        assert got == want, (row, got, want)
        # the slice count as launched: the waves of a KQ block (two per slice with SwiGLU), else the across-blocks split
        assert slices == (block // 64 // (2 if row[4] & SWIGLU else 1) if rc == KQ else S), (row, p)


def outcomes(rows):
    got = set()
    by_shape = {}
    for row, launch in rows:
        by_shape.setdefault(row[:6], []).append((row, launch))
    for row, launch in rows:
        fmt, M, N, K, epi, form, cus, aligned, env = row
        k = launch[0]
        kq_env = env.get("A3V_GEMV_KQ")
        if cus != 256:
            got.add("second_cu_count")
        if k == "ERR":
            got.add("none_fused" if form != "-" else "none_" + fmt)
        elif k.startswith("gemv_kq"):
            if kq_env is None and aligned and (N // 16) % cus == 0:
                got.add("kq_taken")
            if kq_env == "2":
                got.add("kq_forced")
            if "true" in k:
                got.add("kq_prologue")
            if epi & SWIGLU and launch[5] == 8 and launch[2] == 12 * 64:
                got.add("kq_swiglu_cap_6")
            if launch[2] // 64 < launch[5] and not epi & SWIGLU:
                got.add("kq_fewer_slices_short_k")
        elif k.startswith("gemv_dma"):
            got.add("dma_8_rows" if k.startswith("gemv_dma_bf16_kernel<8,") else "dma_16_rows")
            bf16_8 = fmt == "bf16" and M <= 8 and form in ("-", "ssq") and not epi & SWIGLU
            if bf16_8 and kq_env is None and aligned and (N // 16) % cus:
                got.add("kq_uneven_tiles")
            if bf16_8 and kq_env == "0" and (N // 16) % cus == 0:
                got.add("kq_forbidden")
            if bf16_8 and not aligned and any(l[0].startswith("gemv_kq") for r, l in by_shape[row[:6]] if r[7] == 1 and r[6] == cus):
                got.add("kq_unaligned_a")
            if kq_env == "2" and fmt == "bf16" and M > 8:
                got.add("kq_16_rows_never")
            if kq_env == "2" and fmt != "bf16" and M <= 8:
                got.add("kq_quantised_never")
        else:
            assert fmt == "bf16" and form == "-", row
            if k.endswith("<2>"):
                got.add("direct_pair")
            got.add("direct_k_96" if K % 128 else "direct_swiglu_one_slice" if epi & SWIGLU else "direct_lds_limit" if N <= 65536 else "direct_many_tiles")
    return got


def test_the_table_is_not_thin():
    rows = table()
    assert len(rows) >= 180
    names = {l[0] for _, l in rows}
    b = ("false", "true")
    every = {f"gemv_dma_bf16_kernel<{a},{p},{b[f == 1]},{b[f == 2]}>" for a in (8, 16) for p in b for f in (0, 1, 2)} | \
            {"gemv_kq_bf16_kernel<false>", "gemv_kq_bf16_kernel<true>", "gemm_skinny1_bf16_kernel<1>", "gemm_skinny1_bf16_kernel<2>", "ERR"}
    assert names == every, sorted(every ^ names)
    assert kernel_ids() == ["DMA", "KQ", "DIRECT1", "DIRECT2"]
    got = outcomes(rows)
    assert OUTCOMES <= got, sorted(OUTCOMES - got)
    # the decode linears of both geometries at M = 1, 8, 16 in all three formats, as public calls and in their fused forms
    have = {r[:6] for r, _ in rows}
    for d, ffn in ((4096, 11008), (5120, 13824)):
        for M in (1, 8, 16):
            for fmt in ("bf16", "fp8", "nf4"):
                for N, K, epi, form in ((3 * d, d, 0, "qkv"), (d, d, 8, "ssq"), (2 * ffn, d, 16, "pro"), (d, ffn, 8, "ssq"), (32000, d, 32, "-")):
                    assert (fmt, M, N, K, epi, "-") in have and (fmt, M, N, K, epi, form) in have
    # (16, 49152, 4096): 32 blocks of A x 16 rows x 256 B + the rings = 163840 bytes > 150 KiB
    lds = {r[0]: l for r, l in rows if r[1:6] == (16, 49152, 4096, 0, "-")}
    assert lds["bf16"][0] == "gemm_skinny1_bf16_kernel<1>" and lds["fp8"][0] == "ERR" and lds["nf4"][0] == "ERR"
    assert 32 * 16 * 256 + 4 * 2 * 4096 == 163840 > 150 * 1024


def test_plan_refuses_what_it_cannot_plan(built):
    lib = built.load()
    plan = (ctypes.c_int32 * 13)()
    ok = (8, 4096, 4096, 0, 0, 0, 0, 0, 1, 256)
    assert lib.a3v_gemv_plan(*ok, plan) == KQ
    for i, bad in ((0, 0), (0, 17), (1, 0), (2, 0), (4, 3), (4, -1), (9, 0)):      # M, N, K, format, cus
        args = list(ok)
        args[i] = bad
        assert lib.a3v_gemv_plan(*args, plan) == ERR_ARG, (i, bad)
    assert lib.a3v_gemv_plan(*ok, None) == ERR_ARG
    assert lib.a3v_gemv_plan(3, 48, 96, 0, 0, 0, 0, 0, 1, 256, plan) == DIRECT1
    assert lib.a3v_gemv_plan(3, 48, 80, 0, 0, 0, 0, 0, 1, 256, plan) == ERR_SHAPE          # K % 32: no kernel at all
    for fmt in (1, 2):
        assert lib.a3v_gemv_plan(3, 48, 96, 0, fmt, 0, 0, 0, 1, 256, plan) == ERR_SHAPE
        assert lib.a3v_gemv_plan(3, 48, 128, 0, fmt, 0, 0, 0, 1, 256, plan) == ERR_SHAPE   # K % 256
        assert lib.a3v_gemv_plan(8, 64, 256, SWIGLU, fmt, 0, 0, 0, 1, 256, plan) == ERR_SHAPE
        assert lib.a3v_gemv_plan(16, 49152, 4096, 0, fmt, 0, 0, 0, 1, 256, plan) == ERR_SHAPE
    for pro, rope, ssq in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):                                # the direct kernels have no fused form
        assert lib.a3v_gemv_plan(16, 49152, 4096, 0, 0, pro, rope, ssq, 1, 256, plan) == ERR_SHAPE


def test_the_public_queries_follow_the_plan(built):
    """a3v_gemm_skinny_split is the plan's across-blocks slice count wherever an LDS-DMA kernel runs, and 1 for the direct kernels."""
    lib = built.load()
    for row, launch in table():
        if row[0] == "bf16" and launch[0] != "ERR":
            S = lib.a3v_gemm_skinny_split(row[1], row[2], row[3])
            if launch[0].startswith("gemm_skinny1"):
                assert launch[5] == 0 and (S == 1 or row[3] % 128 == 0), row
            else:
                assert S == launch[5], (row, S)
                assert lib.a3v_gemm_skinny_ws_bytes(row[1], row[2], row[3]) >= 65536 + launch[7] * S * 4 * 1024, row


def test_the_table_has_the_rows_of_the_trace_driver():
    """tools/gemv_dispatch_trace.py (the GPU run whose kernel trace the table can be checked against) lists the same rows in the same order."""
    from tools.gemv_dispatch_trace import rows
    assert [(*r[:8], {k: str(v) for k, v in r[8].items()}) for r, _ in table()] == [(*r[:8], {k: str(v) for k, v in r[8].items()}) for r in rows()]
