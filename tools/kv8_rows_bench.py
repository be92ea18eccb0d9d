#!/usr/bin/env python3
"""fp8 KV cache on the ragged decode path: measurement (writes profiles/kv8_rows_bench.json, or --out FILE; one JSON object on stdout).

7B geometry, bf16 weights, B = 8 cache rows, one ragged decode step (forward_inference_rows of one token per row: embedding, the
single-call layer stack, final norm, LM head) at contexts 1100 and 2500, three forms alternating step by step in one run:
  bf16-rows     the bf16 ragged step (the path that exists without this feature), every row at the context;
  fp8-rows      the fp8 ragged step at equal positions (a3v_llama_decode_step_rows_kv8);
  fp8-shared    the fp8 ragged step with shared prompt keys as 2 groups of 4: rows 1..3 read rows 0's keys below context & ~63,
                rows 5..7 row 4's.
Method (tools/ragged_decode_bench.py, tools/kv8_decode_bench.py): device events around every step, warm-up steps first, median
[min .. max] over the timed steps; the models are plugin objects around the SAME parameter tensors, each with its own cache; the
caches are filled with N(0, 1) rows (bf16) and their quantised form (fp8) instead of being prefilled.  Every step decodes at the
same positions, so each one reads the same bytes.
--parent_lib FILE: the bf16-rows form is timed twice more, each time alone in a child process: with this build of the library and
with that build (the parent commit's), to show the existing step did not move.
usage: tools/kv8_rows_bench.py [--contexts 1100,2500] [--steps 30] [--warmup 4] [--parent_lib FILE] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from kv8_decode_bench import time_alternating  # noqa: E402
from a3vlm_amd import ops  # noqa: E402

DEV = "cuda"
B = 8


def fill_rows(m, ctx, g):
    """positions 0 .. ctx-1 of every layer and row: N(0, 1); an fp8 rows cache gets their quantised form through a scratch pair"""
    m.allocate_rows(B)
    m.cache_image_words = 0
    if m._kv8 is None:
        for k, v in zip(m._k_cache, m._vt_cache):
            k[:, :, :ctx].normal_(generator=g)
            v[:, :, :, :ctx].normal_(generator=g)
        return
    Hkv, hd, smax = m.n_kv_heads, m.head_dim, m._k_cache[0].shape[2]
    pk = torch.zeros(B, Hkv, smax, hd, dtype=torch.bfloat16, device=DEV)
    pv = torch.zeros(B, Hkv, hd, smax, dtype=torch.bfloat16, device=DEV)
    for i in range(m.n_layers):
        pk[:, :, :ctx].normal_(generator=g)
        pv[:, :, :, :ctx].normal_(generator=g)
        ops.kv_quantize_fp8(pk, pv, 0, m._kv8["k_q"][i], m._kv8["vt_q"][i], m._kv8["k_scale"][i], m._kv8["v_scale"][i], ctx, 0)
    del pk, pv
    torch.cuda.empty_cache()


def cell(form, ctx, tt, lib=None):
    c = {"form": form, "context": ctx, "ms_per_step": round(tt["median"] * 1e3, 3), "ms_min": round(tt["min"] * 1e3, 3),
         "ms_max": round(tt["max"] * 1e3, 3), "tok_s": round(B / tt["median"], 1)}
    if lib:
        c["library"] = lib
    print(json.dumps(c), flush=True)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1100,2500")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--only_bf16", action="store_true", help="(the child of --parent_lib) the bf16-rows form alone; cells on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_rows_bench.json"))
    a = ap.parse_args()
    contexts = [int(c) for c in a.contexts.split(",")]
    if not torch.cuda.is_available():
        print(json.dumps({"status": "NOT MEASURED", "reason": "no GPU in this run"}))
        return
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    if a.only_bf16:
        # an older build of the same library lacks the entries added since; the bf16 rows step calls none of them, so the loader's
        # table is cut to what that build exports (this process measures nothing else)
        import ctypes
        from a3vlm_amd import lib as _lib
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:
            del _lib.SIGNATURES[name]
    m16, args = bench.build_model("7b", DEV, 4096)
    m16.eval()
    g = torch.Generator(device=DEV).manual_seed(0)
    tok = torch.randint(3, args.vocab_size, (B,), device=DEV, generator=g)
    if a.only_bf16:
        for ctx in contexts:
            m16._destroy_kv_cache()
            m16._layer_tab_key = None
            fill_rows(m16, ctx, g)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
            t = time_alternating([lambda: m16.forward_inference_rows(tok, pos, ctx)], a.steps, a.warmup)
            cell("bf16-rows", ctx, t[0], lib="parent")
        return
    m8 = bench.share_into(plugin.Transformer, args, m16, DEV)          # the same parameter tensors, its own fp8 rows cache
    m8.eval()
    m8.quantize_kv_cache("fp8", rows=True)
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B bf16 weights, B={B}, Smax 4096, one ragged decode step at the context, {a.steps} timed steps per cell after "
                       f"{a.warmup} warm-up, forms alternating", "cells": [], "cache_alloc_GB": {}}
    for ctx in contexts:
        for name, m in (("bf16-rows", m16), ("fp8-rows", m8)):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            fill_rows(m, ctx, g)
            torch.cuda.synchronize()
            res["cache_alloc_GB"][name] = round((torch.cuda.memory_allocated() - before) / 1e9, 3)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        src = torch.tensor([0, 0, 0, 0, 4, 4, 4, 4], dtype=torch.int32, device=DEV)
        shared = torch.tensor([0 if b % 4 == 0 else ctx & ~63 for b in range(B)], dtype=torch.int32, device=DEV)
        t = time_alternating([lambda: m16.forward_inference_rows(tok, pos, ctx), lambda: m8.forward_inference_rows(tok, pos, ctx),
                              lambda: m8.forward_inference_rows(tok, pos, ctx, src_row=src, shared=shared)], a.steps, a.warmup)
        res["cells"] += [cell(f, ctx, tt) for f, tt in zip(("bf16-rows", "fp8-rows", "fp8-shared"), t)]
        for m in (m16, m8):
            m._destroy_kv_cache()
            m._layer_tab_key = None            # the step's pointer tables follow the allocation, not only its shape
        torch.cuda.empty_cache()
    if a.parent_lib:
        del m16, m8
        torch.cuda.empty_cache()
        # like for like: the bf16 rows step alone in a process of its own, once with this build and once with the parent's
        for label, path in (("this build, alone", None), ("parent, alone", os.path.abspath(a.parent_lib))):
            env = dict(os.environ)
            if path:
                env["A3V_LIB_PATH"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_bf16", "--contexts", a.contexts, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                res["alone_error"] = r.stderr[-2000:]
            for line in r.stdout.splitlines():
                if line.startswith('{"form"'):
                    res["cells"].append({**json.loads(line), "library": label})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
