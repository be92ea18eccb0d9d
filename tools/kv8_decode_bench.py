#!/usr/bin/env python3
"""fp8 KV cache measurement (writes profiles/kv8_decode_bench.json, or --out FILE; one JSON object on stdout as well).

7B geometry, B = 8, one decode step (forward_inference of one token: embedding, the single-call layer stack, final norm, LM head)
at contexts 1100, 2500 and 3500, for bf16 / fp8 / NF4 weights, each with the bf16 and with the fp8 KV cache.  The bf16-KV cell of a
row is the code path that exists without the fp8 cache; the fp8-KV cell is compared against it and nothing else.

Method (tools/merge_bench.py): device events around every step, the two KV variants of a row alternate step by step in one run
(same clocks, same thermal state), warm-up steps first, median [min .. max] over the timed steps.  The two variants are two plugin
objects around the SAME parameter tensors, each with its own cache; the caches are filled with N(0, 1) rows (bf16) and their
quantised form (fp8) instead of being prefilled -- a decode step reads every byte of positions 0 .. context-1 whatever they hold.
Every step decodes at the same position, so each one reads the same number of bytes; the working set of a step (weights + cache,
>= 8 GB) is far beyond the 256-MB last-level cache.

Per cell: ms/step, tok/s, bytes per step derived from the layouts (weight images + cache bytes + scales; activations are noise), that
byte count over the time as a fraction of the 8 TB/s peak, and the memory torch holds allocated.
usage: tools/kv8_decode_bench.py [--contexts 1100,2500,3500] [--steps 30] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from a3vlm_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
B = 8
PEAK = 8e12


def weight_bytes(m, fmt):
    """bytes of the decoder matrices + LM head a step streams, in the format it streams them"""
    a = m.args
    H, Hkv, hd, dim, ffn = m.n_heads, m.n_kv_heads, m.head_dim, a.dim, m.ffn
    per_layer = (H + 2 * Hkv) * hd * dim + dim * H * hd + 3 * ffn * dim
    rows = (H + 2 * Hkv) * hd + dim + 2 * ffn + dim
    head = a.vocab_size * dim
    if fmt == "bf16":
        return (per_layer * a.n_layers + head) * 2
    if fmt == "fp8":                       # e4m3 images + one fp32 scale per row; the LM head stays bf16
        return (per_layer + rows * 4) * a.n_layers + head * 2
    return (per_layer * a.n_layers + head) // 2 + (per_layer * a.n_layers + head) // 64 * 4      # nibbles + one fp32 scale per 64


def kv_bytes(m, ctx, kv):
    per_pos = 2 * m.n_layers * m.n_kv_heads * m.head_dim            # K and V elements of one position of one batch row
    if kv == "bf16":
        return per_pos * 2 * ctx * B
    return (per_pos + 2 * m.n_layers * m.n_kv_heads * 4) * ctx * B  # e4m3 bytes + the two fp32 scales per (layer, kv-head, position)


def fill_cache(m, ctx, g):
    """positions 0 .. ctx-1 of every layer: N(0, 1) rows; an fp8 cache gets their quantised form through the shared pair"""
    m._allocate_kv_cache(B)
    m._pack(check=True)
    m.cache_image_words = 0
    if m._kv8 is None:
        for k, v in zip(m._k_cache, m._vt_cache):
            k[:, :, :ctx].normal_(generator=g)
            v[:, :, :, :ctx].normal_(generator=g)
        return
    pk, pv = m._k_cache[0], m._vt_cache[0]
    for i in range(m.n_layers):
        pk[:, :, :ctx].normal_(generator=g)
        pv[:, :, :, :ctx].normal_(generator=g)
        ops.kv_quantize_fp8(pk, pv, 0, m._kv8["k_q"][i], m._kv8["vt_q"][i], m._kv8["k_scale"][i], m._kv8["v_scale"][i], ctx, 0)


def time_alternating(fns, reps, warm):
    for _ in range(warm):
        for f in fns:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    torch.cuda.synchronize()
    for i in range(reps):
        for j, f in enumerate(fns):
            s, e = ev[j][i]
            s.record()
            f()
            e.record()
    torch.cuda.synchronize()
    out = []
    for j in range(len(fns)):
        ts = sorted(s.elapsed_time(e) * 1e-3 for s, e in ev[j])
        out.append({"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1100,2500,3500")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_decode_bench.json"))
    a = ap.parse_args()
    contexts = [int(c) for c in a.contexts.split(",")]
    if not torch.cuda.is_available():
        res = {"status": "NOT MEASURED", "reason": "no GPU in this run"}
        print(json.dumps(res))
        return
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    m16, args = bench.build_model("7b", DEV, 4096)
    m8 = bench.share_into(plugin.Transformer, args, m16, DEV)          # the same parameter tensors, its own (fp8) cache
    m16.eval(), m8.eval()
    m8.quantize_kv_cache("fp8")
    g = torch.Generator(device=DEV).manual_seed(0)
    tok = torch.randint(3, args.vocab_size, (B, 1), device=DEV, generator=g)
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B, B={B}, Smax 4096, one decode step at the context, {a.steps} timed steps per cell after {a.warmup} warm-up, "
                       "KV variants alternating", "cells": []}
    for fmt in ("bf16", "fp8", "nf4"):
        if fmt != "bf16":
            for m in (m16, m8):
                m._destroy_kv_cache()
                m.quantize_decode_weights(fmt)
            torch.cuda.empty_cache()
        for ctx in contexts:
            mem = {}
            for name, m in (("bf16", m16), ("fp8", m8)):
                m._pack(check=True)              # the packed weight images exist before the cache is measured
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                fill_cache(m, ctx, g)
                torch.cuda.synchronize()
                mem[name] = (torch.cuda.memory_allocated() - before, torch.cuda.memory_allocated())
            t = time_alternating([lambda: m16.forward_inference(tok, ctx), lambda: m8.forward_inference(tok, ctx)], a.steps, a.warmup)
            for (name, m), tt in zip((("bf16", m16), ("fp8", m8)), t):
                nbytes = weight_bytes(m, fmt) + kv_bytes(m, ctx, name)
                res["cells"].append({
                    "weights": fmt, "kv": name, "context": ctx,
                    "ms_per_step": round(tt["median"] * 1e3, 3), "ms_min": round(tt["min"] * 1e3, 3), "ms_max": round(tt["max"] * 1e3, 3),
                    "tok_s": round(B / tt["median"], 1), "bytes_per_step": nbytes, "kv_bytes_per_step": kv_bytes(m, ctx, name),
                    "fraction_of_8TBps": round(nbytes / tt["median"] / PEAK, 3),
                    "cache_alloc_GB": round(mem[name][0] / 1e9, 3), "allocated_GB_with_both_caches": round(mem[name][1] / 1e9, 3)})
                print(json.dumps(res["cells"][-1]), flush=True)
            for m in (m16, m8):
                m._destroy_kv_cache()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
