"""The shape list of profiles/gemm_dispatch_*.tsv, and a driver that runs every row of it once on the GPU.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_dispatch_trace.py --hashes OUT.tsv
                                                                 (kernel trace only: no counters in that run)
    python tools/gemm_dispatch_trace.py --from-trace DIR/.../*_kernel_trace.csv --tsv NEW.tsv        (kernel, grid x, grid y, block per
                                                                 launch; compare with the first four values of each launch of the tsv)
    A3V_LIB_PATH=<another build> python tools/gemm_dispatch_trace.py --hashes OUT.tsv    (the same calls through another build)

Each row is one call of a3v_gemm_nt / _qkv_rope / _nt_fp8 / _qkv_rope_fp8 / _tn / _tn_sumsq / _nn with seeded inputs, the row's
workspace registered for the stream and the row's A3V_* switches set; --hashes writes the SHA-256 of every output tensor per row (the
split-K reduce is ordered: two builds that dispatch alike produce equal hashes).  The kernel trace of the run, row by row, is the
launch sequence the tsv records; tests/test_gemm_plan_cpu.py compares a3v_gemm_plan against the same tsv without a GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES, SWIGLU, GELU, BIAS, OUT_F32, RES_F32, SWIGLU_BWD = 8, 16, 2, 1, 32, 64, 128
T128, T256, T256PP, T192PP = 1 << 16, 1 << 17, 1 << 18, 1 << 23
WS = 256 << 20          # the registered workspace of the "yes" rows; 1 MiB: registered, too small for any split
FAMILY = {"nt": 0, "nt_ub": 0, "nt_f32": 0, "nt_rope": 0, "fp8": 1, "fp8_rope": 1, "tn": 2, "tn_sumsq": 2, "nn": 3}      # -> A3V_GEMM_*


def rows():
    """(family, M, N, K, epilogue, workspace bytes, {switch: value})"""
    out = []

    def add(fam, M, N, K, epi=0, ws=(WS, 0), **env):
        for w in (ws if isinstance(ws, tuple) else (ws,)):
            out.append((fam, M, N, K, epi, w, env))

    for d, ffn in ((4096, 11008), (5120, 13824)):           # 7B / 13B decoder linears at the step's 8 x 1091 rows
        M = 8728
        for fam in ("nt", "fp8"):
            add(fam, M, 3 * d, d)
            add(fam, M, d, d, RES)
            add(fam, M, 2 * ffn, d, SWIGLU)
            add(fam, M, d, ffn, RES)
        add("nt_rope", M, 3 * d, d)
        add("fp8_rope", M, 3 * d, d)
        add("nt", M, 32000, d, OUT_F32, ws=WS)              # LM head
        for (N, K) in ((3 * d, d), (d, d), (2 * ffn, d), (d, ffn)):
            add("nn", M, K, N)                              # dX = dY . W
            add("nt", M, K, N, 0, ws=WS)                    # the same on the transposed image (full step since round 5: nt_dgrad_ft)
            add("nt", M, K, N + 64, 0, ws=WS)               # the LoRA step's form: [dy | dt] . [W^T | A^T]^T, 64 adapter columns (nt_dgrad)
            add("tn", N, K, M, OUT_F32)                     # dW = dY^T . X
            add("tn_sumsq", N, K, M, OUT_F32, ws=WS)
        add("nn", M, d, ffn, SWIGLU_BWD, ws=WS)
        add("nt", M, ffn, d, SWIGLU_BWD, ws=WS)
    vr, w = 8 * 577, 1024                                   # ViT-L/14 @ 336: 8 x 577 tokens
    for epi in (0, BIAS):                                   # as the roofline leg times them, and with the biases the model has
        add("nt", vr, 3 * w, w, epi)
        add("nt", vr, w, w, epi | RES)
        add("nt", vr, 4 * w, w, epi | GELU)
        add("nt", vr, w, 4 * w, epi | RES)
    add("nt", vr, 4096, w)
    add("nt", 8 * 576, w, 640)
    add("fp8", vr, 4 * w, w, BIAS | GELU)                   # fp8 with a bias: the two-stage kernel
    # the issue's checked shapes and every remaining outcome
    add("nt", 8728, 4096, 4096)
    add("nt", 2056, 1024, 4096, RES)
    add("nt", 2056, 1024, 4096, BIAS | RES, ws=WS)
    add("nt_ub", 2056, 1024, 4096, BIAS | RES, ws=WS)       # the same with a bias that is not 8-byte aligned: no whole-problem split
    add("nt", 1024, 1024, 2048)
    add("nt", 2056, 1024, 1024)
    add("nt", 300, 4096, 512)
    add("nt", 8728, 4096, 11008, RES, ws=1 << 20)           # priced as a ring tail, launched as the plain 128 x 128 tail
    add("nt", 8728, 4096, 11008, RES, ws=WS, A3V_GEMM_RING_TAIL=0)      # the 128 x 128 split-K tail
    add("nt", 8728, 4096, 11008, RES, ws=WS, A3V_GEMM_TAIL_SLICES=6)
    add("nt", 8728, 4096, 4096, RES, ws=WS, A3V_GEMM_RING_192=0)
    add("nt", 8728, 4096, 4096, RES, ws=WS, A3V_GEMM_RING_192=0, A3V_GEMM_RING_TAIL=0)
    add("nt", 2056, 1024, 4096, RES, ws=WS, A3V_GEMM_RING_SPLIT=0)
    add("nt", 8728, 4096, 4096, 0, ws=WS, A3V_GEMM_PERSISTENT=0)
    for t in (T128, T256, T256PP, T192PP):
        add("nt", 2056, 1024, 1024, t, ws=WS)
        add("nt", 1000, 1000, 512, t | BIAS | GELU, ws=WS)
    add("nt_f32", 300, 1000, 512, BIAS, ws=WS)
    add("nt_f32", 300, 1024, 512, SWIGLU, ws=WS)
    for fam in ("tn", "nn"):
        add(fam, 4352, 4096, 2048)
        add(fam, 4608, 4096, 1024)
        add(fam, 8728, 4096, 4096, RES)
    add("tn", 8728, 4096, 4096, 0, ws=WS, A3V_TN_TAIL=0)
    add("tn", 4096, 4096, 4096, 0, ws=WS, A3V_GEMM_XMAP_TN=5)
    add("fp8", 8728, 4096, 4096, RES, ws=WS, A3V_GEMM_FP8_192=0)
    add("fp8", 8728, 4096, 4096, RES, ws=WS, A3V_GEMM_FP8_RING=0)
    add("fp8", 8728, 4096, 4096, RES, ws=WS, A3V_GEMM_FP8_192=0, A3V_GEMM_FP8_RING=0)
    add("fp8", 8728, 4096, 11008, RES, ws=WS, A3V_GEMM_FP8_192=2)
    add("fp8", 4096, 4096, 4096)
    return out


def plan_args(row, cus=256):
    """The a3v_gemm_plan arguments (all but `steps`) of a row."""
    fam, M, N, K, epi, ws, _ = row
    family = FAMILY[fam]
    lda, ldw = (M, N) if family == 2 else (K, N) if family == 3 else (K, K)
    return (family, M, N, K, lda, ldw, epi, 1 if fam == "nt_f32" else 0, int(fam.endswith("_rope")), int(fam != "nt_ub"), int(fam == "tn_sumsq"), ws, cus)


def run_row(L, torch, row, wsbuf, st):
    """One call on the GPU; returns its output tensors."""
    fam, M, N, K, epi, ws, _ = row
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 31 + N * 7 + K)
    rnd = lambda *s, dt=torch.bfloat16, sc=1.0: (torch.randn(*s, generator=g, device=dev) * sc).to(dt)      # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)      # noqa: E731
    L.a3v_gemm_set_workspace_for(st, P(wsbuf) if ws else None, ws)
    f32 = bool(epi & (OUT_F32 | RES_F32))
    if fam in ("nt", "nt_ub", "nt_f32", "fp8"):
        dt = torch.float32 if fam == "nt_f32" else torch.bfloat16
        ncol = N // 2 if epi & SWIGLU else 2 * N if epi & SWIGLU_BWD else N
        C = torch.zeros(M, ncol, device=dev, dtype=torch.float32 if f32 or fam == "nt_f32" else torch.bfloat16)
        res = rnd(M, ncol, dt=C.dtype if fam == "nt_f32" else torch.bfloat16) if epi & (RES | SWIGLU_BWD) else None
        bias = rnd(N + 1, dt=dt)[1:] if fam == "nt_ub" else rnd(N, dt=dt) if epi & BIAS else None
        if fam == "fp8":
            A, W = rnd(M, K).to(torch.float8_e4m3fn), rnd(N, K, sc=0.05).to(torch.float8_e4m3fn)
            sa, sw = torch.rand(M, generator=g, device=dev) + 0.5, torch.rand(N, generator=g, device=dev) + 0.5
            rc = L.a3v_gemm_nt_fp8(P(A), K, P(sa), P(W), K, P(sw), P(C), ncol, M, N, K, P(bias), P(res), ncol, epi, st)
        else:
            A, W = rnd(M, K, dt=dt), rnd(N, K, dt=dt, sc=0.05)
            rc = L.a3v_gemm_nt(P(A), K, P(W), K, P(C), ncol, M, N, K, P(bias), P(res), ncol, epi, 1 if fam == "nt_f32" else 0, st)
        outs = [C]
    elif fam in ("nt_rope", "fp8_rope"):
        hd = 128
        H = N // (3 * hd)
        B, S = 8, M // 8
        q, kc, vt = (torch.zeros(M, N, device=dev, dtype=torch.bfloat16), torch.zeros(B, H, S, hd, device=dev, dtype=torch.bfloat16),
                     torch.zeros(B, H, hd, S, device=dev, dtype=torch.bfloat16))
        cs = torch.rand(S, hd // 2, 2, generator=g, device=dev)
        if fam == "fp8_rope":
            A, W = rnd(M, K).to(torch.float8_e4m3fn), rnd(N, K, sc=0.05).to(torch.float8_e4m3fn)
            sa, sw = torch.rand(M, generator=g, device=dev) + 0.5, torch.rand(N, generator=g, device=dev) + 0.5
            rc = L.a3v_gemm_qkv_rope_fp8(P(A), K, P(sa), P(W), K, P(sw), K, P(q), N, P(kc), P(vt), P(cs), B, S, H, H, hd, S, 0, 0, st)
        else:
            A, W = rnd(M, K), rnd(N, K, sc=0.05)
            rc = L.a3v_gemm_qkv_rope(P(A), K, P(W), K, K, P(q), N, P(kc), P(vt), None, 0, None, 0, P(cs), B, S, H, H, hd, S, 0, 0, st)
        outs = [q, kc, vt]
    else:
        C = torch.zeros(M, 2 * N if epi & SWIGLU_BWD else N, device=dev, dtype=torch.float32 if f32 else torch.bfloat16)
        res = rnd(M, C.shape[1]) if epi & (RES | SWIGLU_BWD) else None
        if fam == "nn":
            A, W = rnd(M, K), rnd(K, N, sc=0.05)
            rc = L.a3v_gemm_nn(P(A), K, P(W), N, P(C), C.shape[1], M, N, K, P(res), C.shape[1], epi, st)
            outs = [C]
        else:
            A, W = rnd(K, M), rnd(K, N, sc=0.05)
            if fam == "tn_sumsq":
                slots = int(L.a3v_gemm_tn_sumsq_slots(M, N))
                ss = torch.zeros(slots, device=dev)
                rc = L.a3v_gemm_tn_sumsq(P(A), M, P(W), N, P(C), N, M, N, K, P(res), N, epi, P(ss), slots, st)
                outs = [C, ss]
            else:
                rc = L.a3v_gemm_tn(P(A), M, P(W), N, P(C), N, M, N, K, P(res), N, epi, st)
                outs = [C]
    assert rc == 0, (row, rc)
    torch.cuda.synchronize()
    return outs


def tsv_line(row, launches):
    """One line of profiles/gemm_dispatch_*.tsv; a launch is (kernel id name, grid x, grid y, block[, xmap])."""
    fam, M, N, K, epi, ws, env = row
    return "\t".join([fam, str(M), str(N), str(K), str(epi), str(int(fam.endswith("_rope"))), str(ws),
                      ",".join(f"{k}={v}" for k, v in env.items()) or "-"] + [" ".join(map(str, x)) for x in launches])


RING = {"1,256,false": "RING", "3,256,false": "RING_PRE", "4,256,false": "RING_ROPE", "1,192,false": "RING_192", "3,192,false": "RING_PRE_192",
        "1,256,true": "RING_F8", "4,256,true": "RING_ROPE_F8", "1,192,true": "RING_192_F8"}      # <EPI_SET_*, rows, fp8>


def kernel_id(name):
    """The A3V_GEMM_K_* name of a demangled kernel name of the trace, or None for any other kernel."""
    m = re.search(r"(gemm_nt_bf16_ring_kernel|gemm_nt_bf16_kernel|gemm_tn_bf16_pp_kernel|gemm_nt_fp8_pp_kernel|gemm_nt_f32_kernel|"
                  r"splitk_epilogue_kernel)(<[^>]*>)?", name)
    if not m:
        return None
    targs = re.sub(r"\(\w+\)|\s", "", (m.group(2) or "")).strip("<>")
    if m.group(1) == "gemm_nt_bf16_ring_kernel":
        full = targs.split(",") + ["256", "false"][len(targs.split(",")) - 1:]
        full[2] = {"0": "false", "1": "true"}.get(full[2], full[2])
        return RING[",".join(full)]
    if m.group(1) == "gemm_nt_bf16_kernel":
        return {"128,128,2,2": "NT_128", "256,256,2,4": "NT_256"}.get(targs)     # the skinny forms are not this dispatch's
    return {"gemm_tn_bf16_pp_kernel": "NN" if targs in ("true", "1") else "TN", "gemm_nt_fp8_pp_kernel": "FP8_PP", "gemm_nt_f32_kernel": "F32",
            "splitk_epilogue_kernel": "REDUCE"}[m.group(1)]


def trace_to_tsv(csv_path, out_path):
    """A `rocprofv3 --kernel-trace --output-format csv` kernel trace of this driver -> the tsv form.  Every row of rows() fills its
    inputs with torch kernels right before its one library call, so a run of consecutive dispatch kernels is one row."""
    import csv
    recs = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], []
    for r in recs:
        k = kernel_id(r["Kernel_Name"])
        if k is None:
            if cur:
                groups.append(cur)
            cur = []
        else:
            b = int(r["Workgroup_Size_X"])
            cur.append((k, int(r["Grid_Size_X"]) // b, int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]), b))
    if cur:
        groups.append(cur)
    R = rows()
    assert len(groups) == len(R), (len(groups), len(R))
    with open(out_path, "w") as f:
        for row, g in zip(R, groups):
            f.write(tsv_line(row, g) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", help="run every row on the GPU; tsv to write: row index, row, SHA-256 of each output")
    ap.add_argument("--from-trace", metavar="CSV", help="convert the kernel trace of such a run to the tsv form (no GPU)")
    ap.add_argument("--tsv", help="with --from-trace: the file to write")
    a = ap.parse_args()
    if a.from_trace:
        return trace_to_tsv(a.from_trace, a.tsv)
    import torch
    from a3vlm_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)       # not lib.load(): an older build (A3V_LIB_PATH) may lack the newest entry points
    for name, (r, args) in lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = r, args
    wsbuf = torch.empty(WS // 4, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with open(a.hashes, "w") as f:
        for i, row in enumerate(rows()):
            old = {k: os.environ.get(k) for k in row[6]}
            os.environ.update({k: str(v) for k, v in row[6].items()})
            L.a3v_reload_env()
            try:
                outs = run_row(L, torch, row, wsbuf, st)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
                L.a3v_reload_env()
            hs = [hashlib.sha256(o.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for o in outs]
            f.write("\t".join([str(i), *map(str, row[:6]), ",".join(f"{k}={v}" for k, v in row[6].items()) or "-", *hs]) + "\n")
            f.flush()
    L.a3v_gemm_set_workspace_for(st, None, 0)


if __name__ == "__main__":
    main()
