#!/usr/bin/env python3
"""NF4 decode measurement: per-shape NF4 GEMV time (vs the bf16 and fp8 GEMVs on the same shape) and the 7B decode step with bf16,
fp8 and NF4 weights at bench.py's decode geometry (B 8, 512-token prompt + 579 image words, 16 timed steps).  One JSON object on
stdout.  Reuses bench.py's model builder, decode_leg and byte model.   usage: tools/nf4_decode_bench.py [--skip-model]
(--skip-model: the per-shape GEMV times only)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from a3vlm_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES_7B = {"qkv": (12288, 4096), "wo": (4096, 4096), "w13": (22016, 4096), "w2": (4096, 11008), "lm_head": (32000, 4096)}


def _time(fn, reps=50, warm=5):
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
    """images of one format to rotate through: >= 1.5 GB of that format's bytes (6x the 256-MB last-level cache), so every call
    streams its weights from HBM"""
    return max(2, min(64, int(1.5e9 // nbytes) + 1))


def gemv_shapes():
    out = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, (N, K) in SHAPES_7B.items():
        # timing does not depend on the values: random images of each format, the copy count sized from that format's bytes
        nb_bf, nb_f8, nb_n4 = N * K * 2, N * K, N * K // 2 + N * K // 64 * 4
        ws = [torch.randn(N, K, device=DEV, generator=g).mul_(0.02).to(torch.bfloat16) for _ in range(_copies(nb_bf))]
        f8 = [(torch.randint(0, 120, (N, K), device=DEV, dtype=torch.uint8, generator=g), torch.rand(N, device=DEV, generator=g))
              for _ in range(_copies(nb_f8))]
        n4 = [(torch.randint(0, 256, (N, K // 2), device=DEV, dtype=torch.uint8, generator=g), torch.rand(N, K // 64, device=DEV, generator=g))
              for _ in range(_copies(nb_n4))]
        for M in (1, 8):
            a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
            o = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            wsp = ops.gemm_skinny_workspace(M, N, K, DEV)
            it = {"i": 0}

            def nxt(c):
                it["i"] += 1
                return c[it["i"] % len(c)]
            t_bf = _time(lambda: ops.gemm_skinny(a, nxt(ws), o, wsp))
            t_f8 = _time(lambda: ops.gemm_skinny_fp8(a, *nxt(f8), o, wsp))
            t_n4 = _time(lambda: ops.gemm_skinny_nf4(a, *nxt(n4), o, wsp))
            out[f"{name}_M{M}"] = {"N": N, "K": K, "us_bf16": round(t_bf * 1e6, 2), "us_fp8": round(t_f8 * 1e6, 2), "us_nf4": round(t_n4 * 1e6, 2),
                                   "nf4_TBps": round(nb_n4 / t_n4 / 1e12, 3), "fp8_TBps": round(nb_f8 / t_f8 / 1e12, 3),
                                   "bf16_TBps": round(nb_bf / t_bf / 1e12, 3), "nf4_bytes": nb_n4,
                                   "copies": [len(ws), len(f8), len(n4)]}
        del ws, n4, f8
        torch.cuda.empty_cache()
    return out


def decode_7b():
    B, T = 8, 512
    m, args = bench.build_model("7b", DEV, 2048)
    timer = bench.Timer(None, DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    img = torch.randn(B, 3, 336, 336, device=DEV, generator=g).to(torch.bfloat16)
    tokens = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=g)
    fwd = lambda: m.forward_inference(tokens, 0, img)  # noqa: E731
    S = T + m.image_words
    res = {"geometry": f"7B, B={B}, {T}-token prompt + {m.image_words} image words, 16 timed decode steps"}
    for mode in ("bf16", "fp8", "nf4"):
        if mode != "bf16":
            m.quantize_decode_weights(mode)
        torch.cuda.synchronize()
        sec = bench.decode_leg(m, fwd, B, T, 16, timer, DEV)
        res[mode] = {"ms_per_step": round(sec * 1e3, 3), "tok_s": round(B / sec, 1),
                     "allocated_GB": round(torch.cuda.memory_allocated() / 1e9, 2)}
        if mode == "fp8":
            m.quantize_decode_weights(None)
    ctx = S + 2 + 8
    db = bench.bytes_decode_step(args, B, ctx)
    n4b = db - 2 * (bench.p_decoder(args) + args.dim * args.vocab_size) * (1 - 4.5 / 16)
    res["nf4"]["bytes_per_step"] = int(n4b)
    res["nf4"]["hbm_frac"] = round(n4b / (res["nf4"]["ms_per_step"] * 1e-3) / bench.HBM_PEAK, 4)
    res["bf16"]["bytes_per_step"] = db
    return res


if __name__ == "__main__":
    out = {"gemv": gemv_shapes()}
    if "--skip-model" not in sys.argv:
        out["decode"] = decode_7b()
    print(json.dumps(out, indent=1))
