#!/usr/bin/env python3
"""MXFP4 decode measurement: the 7B decode GEMV shapes (qkv, wo, w13, w2, LM head) at M 8 in bf16, fp8, NF4 and MXFP4, the four formats
alternating round by round in one run (device events; every format's images rotate through >= 1.5 GB of its own bytes, so each call
streams its weights from HBM), median [min .. max] over the rounds; then the 7B B-8 decode step and the allocated memory for the four
formats at bench.py's decode geometry.  Writes profiles/mx4_decode_bench.json and prints it.
usage: tools/mx4_decode_bench.py [--skip-model] [--rounds R]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from a3vlm_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES_7B = {"qkv": (12288, 4096), "wo": (4096, 4096), "w13": (22016, 4096), "w2": (4096, 11008), "lm_head": (32000, 4096)}
M = 8


def _time(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def _copies(nbytes):
    return max(2, min(64, int(1.5e9 // nbytes) + 1))


def _stat(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 2), "min_us": round(min(xs) * 1e6, 2), "max_us": round(max(xs) * 1e6, 2)}


def gemv_shapes(rounds):
    out = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, (N, K) in SHAPES_7B.items():
        nbytes = {"bf16": N * K * 2, "fp8": N * K, "nf4": N * K // 2 + N * K // 64 * 4, "mxfp4": N * K // 2 + N * K // 32}
        img = {
            "bf16": [torch.randn(N, K, device=DEV, generator=g).mul_(0.02).to(torch.bfloat16) for _ in range(_copies(nbytes["bf16"]))],
            "fp8": [(torch.randint(0, 120, (N, K), device=DEV, dtype=torch.uint8, generator=g), torch.rand(N, device=DEV, generator=g))
                    for _ in range(_copies(nbytes["fp8"]))],
            "nf4": [(torch.randint(0, 256, (N, K // 2), device=DEV, dtype=torch.uint8, generator=g), torch.rand(N, K // 64, device=DEV, generator=g))
                    for _ in range(_copies(nbytes["nf4"]))],
            "mxfp4": [(torch.randint(0, 256, (N, K // 2), device=DEV, dtype=torch.uint8, generator=g),
                       torch.randint(110, 130, (N, K // 32), device=DEV, dtype=torch.uint8, generator=g)) for _ in range(_copies(nbytes["mxfp4"]))],
        }
        a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
        o = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        wsp = torch.zeros((max(ops.gemm_skinny_ws_bytes(M, N, K), ops.gemm_skinny_mxfp4_ws_bytes(M, N, K)) + 3) // 4, dtype=torch.float32, device=DEV)
        it = {"i": 0}

        def nxt(c):
            it["i"] += 1
            return c[it["i"] % len(c)]
        run = {"bf16": lambda: ops.gemm_skinny(a, nxt(img["bf16"]), o, wsp), "fp8": lambda: ops.gemm_skinny_fp8(a, *nxt(img["fp8"]), o, wsp),
               "nf4": lambda: ops.gemm_skinny_nf4(a, *nxt(img["nf4"]), o, wsp), "mxfp4": lambda: ops.gemm_skinny_mxfp4(a, *nxt(img["mxfp4"]), o, wsp)}
        times = {f: [] for f in run}
        for _ in range(rounds):
            for f, fn in run.items():
                times[f].append(_time(fn))
        out[f"{name}_M{M}"] = {"N": N, "K": K, "K_slices_mxfp4": ops.mx4_gemv_plan(M, N, K)[1][2],
                               **{f: {**_stat(ts), "bytes": nbytes[f], "TBps": round(nbytes[f] / statistics.median(ts) / 1e12, 3),
                                      "copies": len(img[f])} for f, ts in times.items()}}
        del img
        torch.cuda.empty_cache()
    return out


def decode_7b():
    B, T = 8, 512
    res = {}
    for mode in ("bf16", "fp8", "nf4", "mxfp4"):          # NF4 and MXFP4 free the bf16 weights: each starts from a fresh model
        m, args = bench.build_model("7b", DEV, 2048)
        timer = bench.Timer(None, DEV)
        g = torch.Generator(device=DEV).manual_seed(0)
        img = torch.randn(B, 3, 336, 336, device=DEV, generator=g).to(torch.bfloat16)
        tokens = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=g)
        if mode != "bf16":
            m.quantize_decode_weights(mode)
        torch.cuda.synchronize()
        sec = bench.decode_leg(m, lambda: m.forward_inference(tokens, 0, img), B, T, 16, timer, DEV)
        res[mode] = {"ms_per_step": round(sec * 1e3, 3), "tok_s": round(B / sec, 1), "allocated_GB": round(torch.cuda.memory_allocated() / 1e9, 2)}
        geometry = f"7B, B={B}, {T}-token prompt + {m.image_words} image words, 16 timed decode steps"
        del m, img, tokens
        torch.cuda.empty_cache()
    return geometry, res


if __name__ == "__main__":
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    out = {"rounds": rounds, "calls_per_round": 20, "M": M, "gemv": gemv_shapes(rounds)}
    if "--skip-model" in sys.argv:
        out["decode"] = "NOT MEASURED (--skip-model)"
    else:
        out["decode_geometry"], out["decode"] = decode_7b()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "mx4_decode_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
