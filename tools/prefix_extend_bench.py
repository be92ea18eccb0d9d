#!/usr/bin/env python3
"""Prefix sharing on the ragged path: measurement (writes profiles/prefix_extend_bench.json, or --out FILE; one JSON object on stdout).

7B geometry, bf16 weights, prompts of 1100 cache positions ([BOS | image words | text]), runs of g = 1 / 2 / 4 / 8 questions about
one image whose prompts differ in their last --suffix tokens.  Timed per run, the PROMPT PHASE of generate_many's two paths,
alternating run by run in one process:
  refill   g x prefill_row of the whole prompt with its image (the plain path);
  sharing  one prefill_row of the first P = (1100 - 1) & ~63 positions with the image + one extend_rows over the g suffixes
           (g == 1: the plain path, as generate_many takes it for a run of one).
Method (tools/kv8_rows_bench.py): device events around every repetition, warm-up repetitions first, median [min .. max] over the
timed ones; both forms run on the same model and cache.  The decode phase is not timed here: the shared step is
tools/parallel_sampling_bench.py's.  DESIGN 7j holds the expectation that was written before this tool ran.
usage: tools/prefix_extend_bench.py [--groups 1,2,4,8] [--positions 1100] [--suffix 12] [--reps 10] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DEV = "cuda"


def timed(fns, reps, warmup):
    """fns alternate repetition by repetition; per fn {"median", "min", "max"} in seconds"""
    out = [[] for _ in fns]
    for it in range(warmup + reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                out[k].append(a.elapsed_time(b) * 1e-3)
    return [{"median": statistics.median(x), "min": min(x), "max": max(x)} for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2,4,8")
    ap.add_argument("--positions", type=int, default=1100)
    ap.add_argument("--suffix", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_extend_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"status": "NOT MEASURED", "reason": "no GPU in this run"}))
        return
    m, args = bench.build_model("7b", DEV, 2048)
    m.eval()
    W = m.image_words
    T = a.positions - W
    P = (a.positions - 1) & ~63
    assert T > a.suffix + 1 and P >= W + 1, (T, P, W)
    g0 = torch.Generator(device=DEV).manual_seed(0)
    crop = args.vit_crop
    image = torch.randn(1, 3, crop, crop, device=DEV, generator=g0)
    stem = torch.randint(3, args.vocab_size, (T - a.suffix,), device=DEV, generator=g0)
    stem[0] = 1
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B bf16, {a.positions} cache positions per prompt ({W} image words), suffix {a.suffix} tokens, P = {P}, "
                       f"{a.reps} timed repetitions per cell after {a.warmup} warm-up, forms alternating", "cells": []}
    for g in [int(x) for x in a.groups.split(",")]:
        m._destroy_kv_cache()
        m.allocate_rows(max(g, 1))
        prompts = [torch.cat([stem, torch.randint(3, args.vocab_size, (a.suffix,), device=DEV, generator=g0)]) for _ in range(g)]

        def refill():
            for r, t in enumerate(prompts):
                m.prefill_row(r, t[None], image)

        def sharing():
            if g == 1:
                return refill()
            m.prefill_row(0, prompts[0][None, :P - W], image)
            m.extend_rows(list(range(g)), [t[P - W:] for t in prompts], [P] * g, src_row=[0] * g, shared=[P] * g)

        tr, ts = timed([refill, sharing], a.reps, a.warmup)
        cell = {"group": g, "refill_ms": round(tr["median"] * 1e3, 3), "refill_min_max_ms": [round(tr["min"] * 1e3, 3), round(tr["max"] * 1e3, 3)],
                "sharing_ms": round(ts["median"] * 1e3, 3), "sharing_min_max_ms": [round(ts["min"] * 1e3, 3), round(ts["max"] * 1e3, 3)],
                "ratio": round(tr["median"] / ts["median"], 3)}
        print(json.dumps(cell), flush=True)
        res["cells"].append(cell)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
