"""The shape list of profiles/gemv_dispatch_*.tsv, and a driver that runs every row of it the C-ABI can reach once on the GPU.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemv_dispatch_trace.py --hashes OUT.tsv
                                                                 (kernel trace only: no counters in that run)
    python tools/gemv_dispatch_trace.py --from-trace DIR/.../*_kernel_trace.csv --tsv NEW.tsv        (kernel, grid, block per launch;
                                                                 compare with the first three values of each launch of the tsv)
    A3V_LIB_PATH=<another build> python tools/gemv_dispatch_trace.py --hashes OUT.tsv    (the same calls through another build)

Each row is one decode linear: weight format, M, N, K, epilogue, the decode step's fused form ("-": a public call of a3v_gemm_skinny /
_fp8 / _nf4; "qkv": RMSNorm prologue + RoPE / KV-cache epilogue; "pro": prologue; "ssq": sums of squares on the way out), the CU
count, whether A is 16-byte aligned, and the row's A3V_* switches.  The driver runs the public rows planned for the device's CU count
and an aligned A with seeded inputs and a zeroed workspace; --hashes writes the SHA-256 of every output and of the arrival counters per row (the split-K
sums are ordered: two builds that dispatch alike produce equal hashes).  The fused forms have no C-ABI entry of their own -- they run
inside a3v_llama_decode_step and its tests -- so those rows exist for the table and for a3v_gemv_plan, which
tests/test_gemv_plan_cpu.py compares with the table without a GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES, SWIGLU, OUT_F32 = 8, 16, 32
FORMAT = {"bf16": 0, "fp8": 1, "nf4": 2}                                    # -> A3V_GEMV_*
FORMS = {"-": (0, 0, 0), "qkv": (1, 1, 0), "pro": (1, 0, 0), "ssq": (0, 0, 1)}      # -> prologue, rope, ssq


def rows():
    """(format, M, N, K, epilogue, fused form, CUs, A aligned, {switch: value})"""
    out = []

    def add(fmt, M, N, K, epi=0, form="-", cus=256, aligned=1, **env):
        out.append((fmt, M, N, K, epi, form, cus, aligned, env))

    for d, ffn in ((4096, 11008), (5120, 13824)):            # 7B / 13B decode linears, as public calls and as the fused step issues them
        for M in (1, 8, 16):
            for fmt in FORMAT:
                for N, K, epi, form in ((3 * d, d, 0, "qkv"), (d, d, RES, "ssq"), (2 * ffn, d, SWIGLU, "pro"), (d, ffn, RES, "ssq")):
                    add(fmt, M, N, K, epi)
                    add(fmt, M, N, K, epi, form)
                add(fmt, M, 32000, d, OUT_F32)               # LM head
    # in-block K split (KQ): forbidden, forced (uneven tiles, SwiGLU with the cap at 6 slices, the prologue forms), fewer slices than the
    # across-blocks plan because K is short, an A that the in-block form cannot address
    add("bf16", 8, 4096, 4096, RES, A3V_GEMV_KQ=0)
    add("bf16", 8, 5120, 5120, RES, A3V_GEMV_KQ=2)
    add("bf16", 8, 8192, 4096, SWIGLU, A3V_GEMV_KQ=2)
    add("bf16", 8, 22016, 4096, SWIGLU, A3V_GEMV_KQ=2)
    add("bf16", 8, 22016, 4096, SWIGLU, "pro", A3V_GEMV_KQ=2)
    add("bf16", 8, 12288, 4096, 0, "qkv", A3V_GEMV_KQ=2)
    add("bf16", 16, 4096, 4096, RES, A3V_GEMV_KQ=2)          # 16 activation rows: never
    add("fp8", 8, 4096, 4096, RES, A3V_GEMV_KQ=2)            # bf16 weights only
    add("nf4", 8, 4096, 4096, RES, A3V_GEMV_KQ=2)
    add("bf16", 8, 4096, 512)
    add("bf16", 8, 4096, 512, A3V_GEMV_KQ=0)
    add("bf16", 8, 4096, 4096, RES, aligned=0)
    add("bf16", 8, 4096, 4096, RES, aligned=0, A3V_GEMV_KQ=2)
    add("bf16", 9, 4096, 4096, RES)                          # 16-row form from 9 rows on
    add("bf16", 12, 256, 512)
    add("fp8", 12, 256, 512)
    add("nf4", 12, 256, 512)
    # the direct-to-VGPR kernels (bf16 public calls only), and the same problems where nothing can run them
    for fmt in FORMAT:
        add(fmt, 3, 48, 96)                                  # K % 128
        add(fmt, 4, 4096, 160, RES)
        add(fmt, 8, 64, 128, SWIGLU)                         # SwiGLU without a split
        add(fmt, 8, 64, 256, SWIGLU)
        add(fmt, 16, 49152, 4096)                            # 163840 bytes of LDS
        add(fmt, 8, 65600, 4096)                             # more tiles than arrival counters
    add("bf16", 16, 49152, 4096, 0, "qkv")
    add("bf16", 8, 64, 128, SWIGLU, "pro")
    # a second CU count: the even-tiles rule of KQ follows it
    add("bf16", 8, 4096, 4096, RES, cus=304)
    add("bf16", 8, 4864, 4096, RES, cus=304)
    add("bf16", 8, 9728, 4096, 0, "ssq", cus=304)
    add("bf16", 8, 14592, 4096, cus=304)
    return out


def plan_args(row):
    """The a3v_gemv_plan arguments (all but `plan`) of a row."""
    fmt, M, N, K, epi, form, cus, aligned, _ = row
    pro, rope, ssq = FORMS[form]
    return (M, N, K, epi, FORMAT[fmt], pro, rope, ssq, aligned, cus)


def kernel_name(plan):
    """The kernel with its template arguments, as the tsv spells it, of the A3V_GEMV_PLAN_INTS values of a plan."""
    b = ("false", "true")
    k, arows, pro, fmt = plan[:4]
    return (f"gemv_dma_bf16_kernel<{arows},{b[pro]},{b[fmt == 1]},{b[fmt == 2]}>", f"gemv_kq_bf16_kernel<{b[pro]}>",
            "gemm_skinny1_bf16_kernel<1>", "gemm_skinny1_bf16_kernel<2>")[k]


def tsv_line(row, launch):
    """One line of profiles/gemv_dispatch_*.tsv; launch: the fields after the row's own, e.g. (kernel, grid, block) or ("ERR", -1)."""
    return "\t".join([*map(str, row[:8]), ",".join(f"{k}={v}" for k, v in row[8].items()) or "-", " ".join(map(str, launch))])


def run_row(L, torch, row, st):
    """One public call on the GPU; returns (return code, output tensors)."""
    fmt, M, N, K, epi, form, cus, aligned, _ = row
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 31 + N * 7 + K)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device=dev) * sc).to(torch.bfloat16)      # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)      # noqa: E731
    A = rnd(M * K + 8)[(0 if aligned else 4):][:M * K].view(M, K)
    Wd = rnd(N, K, sc=0.05)
    ncol = N // 2 if epi & SWIGLU else N
    C = torch.zeros(M, ncol, device=dev, dtype=torch.float32 if epi & OUT_F32 else torch.bfloat16)
    res = rnd(M, ncol) if epi & RES else None
    ws = torch.zeros(int(L.a3v_gemm_skinny_ws_bytes(M, N, K)) // 4, device=dev, dtype=torch.int32)
    if fmt == "bf16":
        rc = L.a3v_gemm_skinny(P(A), K, P(Wd), K, P(C), ncol, M, N, K, P(res), ncol, epi, P(ws), st)
    elif fmt == "fp8":
        Wq, sc = Wd.to(torch.float8_e4m3fn), torch.rand(N, generator=g, device=dev) + 0.5
        rc = L.a3v_gemm_skinny_fp8(P(A), K, P(Wq), K, P(sc), P(C), ncol, M, N, K, P(res), ncol, epi, P(ws), st)
    else:
        Wq = torch.randint(0, 256, (N, K // 2), generator=g, device=dev, dtype=torch.uint8)
        sc = torch.rand(N, max(K // 64, 1), generator=g, device=dev) * 0.1
        rc = L.a3v_gemm_skinny_nf4(P(A), K, P(Wq), K // 2, P(sc), P(C), ncol, M, N, K, P(res), ncol, epi, P(ws), st)
    torch.cuda.synchronize()
    return rc, [C, ws[:4096]]


def kernel_id(name):
    """The tsv spelling of a demangled kernel name of the trace, or None for any other kernel."""
    m = re.search(r"(gemv_dma_bf16_kernel|gemv_kq_bf16_kernel|gemm_skinny1_bf16_kernel)<([^>]*)>", name)
    if not m:
        return None
    targs = [{"0": "false", "1": "true"}.get(t, t) if i or m.group(1) == "gemv_kq_bf16_kernel" else t
             for i, t in enumerate(re.sub(r"\(\w+\)|\s", "", m.group(2)).split(","))]
    if m.group(1) == "gemv_dma_bf16_kernel":
        targs += ["false"] * (4 - len(targs))
    return f"{m.group(1)}<{','.join(targs)}>"


def trace_to_tsv(csv_path, out_path, cus=256):
    """A `rocprofv3 --kernel-trace --output-format csv` kernel trace of this driver -> the tsv form (kernel, grid, block, dynamic LDS).
    Every row the driver runs makes exactly one launch of the family, or none where the entry point refuses the problem."""
    import csv
    recs = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    got = [(k, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"]))
           for r in recs for k in [kernel_id(r["Kernel_Name"])] if k]
    with open(out_path, "w") as f:
        for row in driven_rows(cus):
            launch = got.pop(0) if runs(row) else ("ERR", -1)
            f.write(tsv_line(row, launch) + "\n")
    assert not got, len(got)


def driven_rows(cus):
    """The rows the driver runs: public calls planned for this CU count with an aligned A (the unaligned rows are for the planner)."""
    return [r for r in rows() if r[5] == "-" and r[6] == cus and r[7] == 1]


def runs(row):
    """Does a public row launch anything: bf16 always (the direct kernels take what the LDS-DMA kernels cannot), fp8 / NF4 unless the plan is none."""
    from a3vlm_amd import lib
    plan = (ctypes.c_int32 * 13)()
    return lib.load().a3v_gemv_plan(*plan_args(row), plan) >= 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", help="run every public row on the GPU; tsv to write: row, return code, SHA-256 of each output")
    ap.add_argument("--from-trace", metavar="CSV", help="convert the kernel trace of such a run to the tsv form (no GPU)")
    ap.add_argument("--tsv", help="with --from-trace: the file to write")
    ap.add_argument("--list", action="store_true", help="print the rows in the tsv's form (no GPU)")
    a = ap.parse_args()
    if a.list:
        for row in rows():
            print(tsv_line(row, ())[:-1])
        return
    if a.from_trace:
        return trace_to_tsv(a.from_trace, a.tsv)
    import torch
    from a3vlm_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)       # not lib.load(): an older build (A3V_LIB_PATH) may lack the newest entry points
    for name, (r, args) in lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = r, args
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cus = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    with open(a.hashes, "w") as f:
        for row in driven_rows(cus):
            old = {k: os.environ.get(k) for k in row[8]}
            os.environ.update({k: str(v) for k, v in row[8].items()})
            L.a3v_reload_env()
            try:
                rc, outs = run_row(L, torch, row, st)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
                L.a3v_reload_env()
            hs = [hashlib.sha256(o.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for o in outs]
            f.write(tsv_line(row, (rc, *hs)) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
