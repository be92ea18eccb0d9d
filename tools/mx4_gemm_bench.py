#!/usr/bin/env python3
"""W4A8 GEMM measurement: the five 7B decoder products (qkv, wo, w13, w2, LM head) at M 33, 64, 128, 512, 2048 on two paths that
alternate round by round in one run -- ``dequant``: what quantize_decode_weights("mxfp4") runs above 32 rows, a3v_dequantize_mxfp4 into
a bf16 scratch plus the bf16 GEMM on it; ``w4a8``: quantize_rows_mxfp8 plus gemm_nt_mxfp4 on the image (prefill=True).  Device events;
the images rotate through >= 1.5 GB, so every call streams its weights from HBM; median [min .. max] over the rounds.  Then the 7B
decode step at B = 64 and a 1100-token prefill, each in both modes, alternating as well.  Writes profiles/mx4_gemm_bench.json and
prints it.
usage: tools/mx4_gemm_bench.py [--skip-model] [--skip-shapes] [--rounds R]"""
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
SHAPES_7B = {"qkv": (12288, 4096, 0), "wo": (4096, 4096, ops.EPI_RESIDUAL), "w13": (22016, 4096, ops.EPI_SWIGLU),
             "w2": (4096, 11008, ops.EPI_RESIDUAL), "lm_head": (32000, 4096, ops.EPI_OUT_F32)}
MS = (33, 64, 128, 512, 2048)
BF = torch.bfloat16


def _time(fn, reps, warm=2):
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


def _stat(xs, unit=1e6, key="us"):
    return {f"median_{key}": round(statistics.median(xs) * unit, 2), f"min_{key}": round(min(xs) * unit, 2), f"max_{key}": round(max(xs) * unit, 2)}


def _faster(new, old, key):
    """new is faster than old: the gap between the medians exceeds both spreads (max - min)."""
    gap = old[f"median_{key}"] - new[f"median_{key}"]
    return bool(gap > max(new[f"max_{key}"] - new[f"min_{key}"], old[f"max_{key}"] - old[f"min_{key}"]))


def gemm_shapes(rounds):
    out = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, (N, K, epi) in SHAPES_7B.items():
        nbytes = N * K // 2 + N * K // 32
        ncopy = max(2, min(64, int(1.5e9 // nbytes) + 1))
        img = [(torch.randint(0, 256, (N, K // 2), device=DEV, dtype=torch.uint8, generator=g),
                torch.randint(110, 130, (N, K // 32), device=DEV, dtype=torch.uint8, generator=g)) for _ in range(ncopy)]
        scratch = torch.empty(N, K, dtype=BF, device=DEV)
        ncol = N // 2 if epi == ops.EPI_SWIGLU else N
        for M in MS:
            a = torch.randn(M, K, device=DEV, generator=g).to(BF)
            o = torch.zeros(M, ncol, device=DEV, dtype=torch.float32 if epi == ops.EPI_OUT_F32 else BF)
            res = torch.zeros(M, N, device=DEV, dtype=BF) if epi == ops.EPI_RESIDUAL else None
            xq, xe = torch.empty(M, K, dtype=torch.uint8, device=DEV), torch.empty(M, K // 32, dtype=torch.uint8, device=DEV)
            e0 = epi & ~ops.EPI_RESIDUAL
            it = {"i": 0}

            def nxt():
                it["i"] += 1
                return img[it["i"] % ncopy]

            def dequant():
                ops.dequantize_mxfp4(*nxt(), scratch)
                ops.gemm_nt(a, scratch, o, residual=res, epilogue=e0)

            def w4a8():
                ops.quantize_rows_mxfp8(a, xq, xe)
                ops.gemm_nt_mxfp4(xq, xe, *nxt(), o, residual=res, epilogue=e0)
            run = {"dequant": dequant, "w4a8": w4a8}
            times = {f: [] for f in run}
            reps = 10 if M <= 512 else 5
            for _ in range(rounds):
                for f, fn in run.items():
                    times[f].append(_time(fn, reps))
            st = {f: _stat(ts) for f, ts in times.items()}
            rc, plan = ops.mx4_gemm_plan(M, N, K, e0)
            out[f"{name}_M{M}"] = {"N": N, "K": K, "M": M, "image_bytes": nbytes, "copies": ncopy, "calls_per_round": reps,
                                   "plan": dict(zip(("tile_rows", "tile_cols", "k_stage", "grid", "block", "lds", "k_slices", "k_stages"), plan)),
                                   **st, "w4a8_image_TBps": round(nbytes / (st["w4a8"]["median_us"] * 1e-6) / 1e12, 3),
                                   "w4a8_TFLOPs": round(2.0 * M * N * K / (st["w4a8"]["median_us"] * 1e-6) / 1e12, 1),
                                   "w4a8_faster": _faster(st["w4a8"], st["dequant"], "us"), "dequant_faster": _faster(st["dequant"], st["w4a8"], "us")}
            print(f"{name} M {M}: dequant {st['dequant']['median_us']} us, w4a8 {st['w4a8']['median_us']} us", file=sys.stderr, flush=True)
        del img, scratch
        torch.cuda.empty_cache()
    return out


def model_7b(rounds):
    """The 7B decoder in both modes side by side (two sets of images, ~4 GB each): a 1100-token prefill at B = 1, then the decode step at
    B = 64 after a 64-token prompt, the two modes alternating round by round."""
    ms = {}
    for mode, flag in (("dequant", False), ("w4a8", True)):
        m, args = bench.build_model("7b", DEV, 1280)
        m.quantize_decode_weights("mxfp4", prefill=flag)
        ms[mode] = m
    torch.cuda.synchronize()
    g = torch.Generator(device=DEV).manual_seed(0)
    res = {"allocated_GB_both_models": round(torch.cuda.memory_allocated() / 1e9, 2)}
    tok = torch.randint(3, args.vocab_size, (1, 1100), device=DEV, generator=g)
    times = {f: [] for f in ms}
    for _ in range(rounds):
        for f, m in ms.items():
            times[f].append(_time(lambda: m.forward_inference(tok, 0), 2, warm=1))
    st = {f: _stat(ts, 1e3, "ms") for f, ts in times.items()}
    print(f"prefill: {st}", file=sys.stderr, flush=True)
    res["prefill_1100_tokens_B1"] = {**st, "w4a8_faster": _faster(st["w4a8"], st["dequant"], "ms"), "dequant_faster": _faster(st["dequant"], st["w4a8"], "ms")}
    B, T = 64, 64
    tok = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=g)
    cur = torch.randint(3, args.vocab_size, (B, 1), device=DEV, generator=g)
    for m in ms.values():
        m.forward_inference(tok, 0)
    times = {f: [] for f in ms}
    for _ in range(rounds):
        for f, m in ms.items():
            times[f].append(_time(lambda: m.forward_inference(cur, T), 4, warm=1))
    st = {f: _stat(ts, 1e3, "ms") for f, ts in times.items()}
    res["decode_step_B64"] = {**st, "tok_s_w4a8": round(B / (st["w4a8"]["median_ms"] * 1e-3), 1), "tok_s_dequant": round(B / (st["dequant"]["median_ms"] * 1e-3), 1),
                              "w4a8_faster": _faster(st["w4a8"], st["dequant"], "ms")}
    res["scratch_allocated"] = {f: "nf4_scratch" in m._ws for f, m in ms.items()}
    return res


if __name__ == "__main__":
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    out = {"rounds": rounds, "faster_means": "gap between the medians larger than both spreads (max - min)"}
    out["gemm"] = "NOT MEASURED (--skip-shapes)" if "--skip-shapes" in sys.argv else gemm_shapes(rounds)
    out["model_7b"] = "NOT MEASURED (--skip-model)" if "--skip-model" in sys.argv else model_7b(rounds)
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "mx4_gemm_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
