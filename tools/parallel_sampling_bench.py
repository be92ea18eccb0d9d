#!/usr/bin/env python3
"""Parallel sampling measurement (writes profiles/parallel_sampling_bench.json, or --out FILE; one JSON object on stdout as well).

1. Step cost.  7B geometry bf16, B = 8, contexts 1100 / 2500: forward_inference_rows plain against the shared form with the 8 rows
   as 2 groups of 4 (rows 1..3 read row 0's keys below ctx & ~63, rows 5..7 row 4's).  Same process, model object and cache, the
   forms alternating step by step, device events around every step, median [min .. max] (tools/kv8_decode_bench.py's method).
   With --parent_lib FILE (a liba3vlm_hip.so built from the parent commit) the parent's a3v_llama_decode_step_rows joins the
   alternation: the plain step must not have moved by more than the parent's own min-to-max spread.
2. End to end.  16 prompts with image, 4 samples each, 8 rows, temperature 0.7: generate_many(n=4) against the same prompts
   repeated 4 times (n = 1, which the parent runs too).  Per leg: wall seconds, prefills (counted by wrapping prefill_row), kept
   tokens per second, the largest number of cache positions in use (sum over rows of the positions a row holds itself: a sibling
   does not hold the shared part) and the bytes they take.
usage: tools/parallel_sampling_bench.py [--contexts 1100,2500] [--steps 30] [--prompts 16] [--gen 128] [--parent_lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from a3vlm_amd import lib as _lib, ops  # noqa: E402
from tools.kv8_decode_bench import time_alternating  # noqa: E402

DEV = "cuda"
B = 8
GROUP = 4


def parent_step_fn(path):
    """the parent library's a3v_llama_decode_step_rows with this library's signature table"""
    L = ctypes.CDLL(path)
    f = L.a3v_llama_decode_step_rows
    f.restype, f.argtypes = _lib.SIGNATURES["a3v_llama_decode_step_rows"]
    return f


def step_cost(m, args, contexts, steps, warmup, parent):
    g = torch.Generator(device=DEV).manual_seed(0)
    tok = torch.randint(3, args.vocab_size, (B,), device=DEV, generator=g)
    out = torch.empty(B, args.vocab_size, dtype=torch.float32, device=DEV)
    src = torch.tensor([b - b % GROUP for b in range(B)], dtype=torch.int32, device=DEV)
    cells = []
    for ctx in contexts:
        m.allocate_rows(B)
        m.cache_image_words = 0
        for k, v in zip(m._k_cache, m._vt_cache):
            k[:, :, :ctx].normal_(generator=g)
            v[:, :, :, :ctx].normal_(generator=g)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        shared = torch.full((B,), ctx & ~63, dtype=torch.int32, device=DEV)

        def parent_step():            # forward_inference_rows with the layer stack from the parent's library
            a = m.args
            h = m._buf("h", (B, a.dim))
            ops.embed_assemble(tok.view(B, 1), m.tok_embeddings.weight, h, B, 1, 0, a.dim)
            tab = m._llama_layer_table()
            xn, qkv, att, act, scratch, sws = m._decode_step_buffers(B)
            rc = parent(tab, m.n_layers, h.data_ptr(), xn.data_ptr(), qkv.data_ptr(), att.data_ptr(), act.data_ptr(), scratch.data_ptr(),
                        sws.data_ptr(), m._cos_sin_dev().data_ptr(), pos.data_ptr(), ctx, B, a.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn,
                        m._k_cache[0].shape[2], a.norm_eps, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
            xl = m._buf("xn_last", (B, a.dim))
            ops.rmsnorm(h, m.norm.weight, xl, a.norm_eps)
            m._lm_head_last(xl, out, True)

        names = ["plain", "shared"] + (["parent_plain"] if parent else [])
        fns = [lambda: m.forward_inference_rows(tok, pos, ctx, out=out),
               lambda: m.forward_inference_rows(tok, pos, ctx, out=out, src_row=src, shared=shared)] + ([parent_step] if parent else [])
        t = time_alternating(fns, steps, warmup)
        cell = {"context": ctx, "shared_positions": ctx & ~63}
        for name, tt in zip(names, t):
            cell[name] = {"ms_per_step": round(tt["median"] * 1e3, 3), "ms_min": round(tt["min"] * 1e3, 3), "ms_max": round(tt["max"] * 1e3, 3)}
        cell["shared_minus_plain_ms"] = round((t[1]["median"] - t[0]["median"]) * 1e3, 3)
        if parent:
            cell["plain_minus_parent_ms"] = round((t[0]["median"] - t[2]["median"]) * 1e3, 3)
            cell["parent_spread_ms"] = round((t[2]["max"] - t[2]["min"]) * 1e3, 3)
        cells.append(cell)
        print(json.dumps(cell), flush=True)
    return cells


def end_to_end(m, args, n_prompts, n, gen, prompt_len):
    from a3vlm_amd.model.meta import MetaModel
    mm = MetaModel.__new__(MetaModel)
    torch.nn.Module.__init__(mm)
    mm.llma, mm.tokenizer, mm.llama_type = m, bench._SynthTokenizer(prompt_len), "llama_ens5"
    prompts = [f"synthetic prompt {i}" for i in range(n_prompts)]
    g = torch.Generator(device=DEV).manual_seed(1)
    crop = args.vit_crop
    images = torch.randn(n_prompts, 3, crop, crop, device=DEV, generator=g)
    P = m.image_words + prompt_len
    a = m.args
    pos_bytes = 2 * a.n_layers * m.n_kv_heads * m.head_dim * 2            # K and V^T, bf16, all layers, per cache position
    calls = []
    orig = m.prefill_row

    def counted(row, *aa, **kw):
        calls.append(row)
        return orig(row, *aa, **kw)
    m.prefill_row = counted
    res = {"prompts": n_prompts, "samples": n, "rows": B, "prompt_positions": P, "max_gen_len": gen, "temperature": 0.7,
           "allocated_cache_bytes": B * m.args.max_seq_len * pos_bytes}
    kw = dict(batch_rows=B, max_gen_len=gen, temperature=0.7, top_p=0.9, return_ids=True)
    try:
        for name, call in (("repeated_n1", lambda: mm.generate_many([p for p in prompts for _ in range(n)], images.repeat_interleave(n, dim=0), **kw)),
                           ("shared_n%d" % n, lambda: mm.generate_many(prompts, images, n=n, **kw))):
            torch.manual_seed(3)
            mm.generate_many(prompts[:2], images[:2], batch_rows=B, max_gen_len=4, temperature=0.7, n=1 if name.startswith("rep") else n)   # warm
            calls.clear()
            torch.manual_seed(4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ids = call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            flat = ids if name.startswith("rep") else [t for per in ids for t in per]
            kept = sum(len(t) for t in flat)
            # positions a full house of rows holds itself: every row its prompt (repeated) / one prompt per group + the tails (shared)
            own = P if name.startswith("rep") else (P + (n - 1) * (P - (P & ~63))) / n
            res[name] = {"seconds": round(dt, 3), "prefills": len(calls), "kept_tokens": kept, "kept_tok_s": round(kept / dt, 1),
                         "prompt_positions_held_per_row": round(own, 1), "prompt_cache_bytes_in_use_8_rows": int(B * own * pos_bytes)}
        res["speedup"] = round(res["repeated_n1"]["seconds"] / res["shared_n%d" % n]["seconds"], 3)
    finally:
        del m.prefill_row
        mm.llma = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1100,2500")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prompts", type=int, default=16)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--prompt_len", type=int, default=64)
    ap.add_argument("--parent_lib", default=None, help="liba3vlm_hip.so of the parent commit: its plain ragged step joins the alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parallel_sampling_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"status": "NOT MEASURED", "reason": "no GPU in this run"}))
        return
    m, args = bench.build_model("7b", DEV, 4096)
    m.eval()
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B bf16, B={B} as {B // GROUP} groups of {GROUP}, Smax 4096; step cost: {a.steps} timed steps per cell after {a.warmup} "
                       "warm-up, the step forms alternating"}
    res["step_cost"] = step_cost(m, args, [int(c) for c in a.contexts.split(",")], a.steps, a.warmup,
                                 parent_step_fn(a.parent_lib) if a.parent_lib else None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:                     # the first half is kept even if the second does not finish
        json.dump(res, f, indent=1)
    res["end_to_end"] = end_to_end(m, args, a.prompts, a.samples, a.gen, a.prompt_len)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
