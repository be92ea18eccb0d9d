"""Launch-level cost of the sampler's filters: a3v_sample_top_p (the path without them) and a3v_sample_top_k_p with the filters off,
top_k 50, min_p 0.05 and both, the five configurations alternating launch by launch in one run, device events around each launch,
median [min .. max] of N launches each after warm-up -> profiles/sampler_controls_bench.json.
usage (GPU box): PYTHONPATH=. python tools/sampler_controls_bench.py [--n 40] [--out FILE]"""
import argparse
import json
import os
import statistics

import torch

from a3vlm_amd import ops

DEV = "cuda"
T, TOP_P = 0.1, 0.75          # the eval recipe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_controls_bench.json"))
    a = ap.parse_args()
    res = {"temperature": T, "top_p": TOP_P, "batch": 8, "n": a.n, "logits": "randn * 2.5 rounded to bf16", "shapes": {}}
    for V in (32000, 50000):
        g = torch.Generator(device=DEV).manual_seed(0)
        B = 8
        logits = (torch.randn(B, V, device=DEV, generator=g) * 2.5).bfloat16().float()
        u = torch.rand(B, device=DEV, generator=g)
        out = torch.empty(B, dtype=torch.long, device=DEV)
        cfgs = {
            "sample_top_p": lambda: ops.sample_top_p(logits, T, TOP_P, u, out),
            "top_k_p_filters_off": lambda: ops.sample_top_k_p(logits, T, 0, TOP_P, 0.0, u, out),
            "top_k_50": lambda: ops.sample_top_k_p(logits, T, 50, TOP_P, 0.0, u, out),
            "min_p_0.05": lambda: ops.sample_top_k_p(logits, T, 0, TOP_P, 0.05, u, out),
            "top_k_50_min_p_0.05": lambda: ops.sample_top_k_p(logits, T, 50, TOP_P, 0.05, u, out),
        }
        for _ in range(5):
            for fn in cfgs.values():
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in cfgs}
        for _ in range(a.n):
            for k, fn in cfgs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                ev[k].append((t0, t1))
        torch.cuda.synchronize()
        shape = {}
        for k, pairs in ev.items():
            us = [p[0].elapsed_time(p[1]) * 1e3 for p in pairs]
            shape[k] = {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}
            print(f"B={B} V={V} {k}: {shape[k]['median_us']} [{shape[k]['min_us']} .. {shape[k]['max_us']}] us", flush=True)
        res["shapes"][f"V{V}"] = shape
    res["note"] = ("one run, the five configurations alternating launch by launch; device events around one launch each, so every figure "
                   "includes the launch itself; sample_top_p is the path generation takes without top_k / min_p")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
