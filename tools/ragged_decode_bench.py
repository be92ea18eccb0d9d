#!/usr/bin/env python3
"""Ragged decode measurement (writes profiles/ragged_decode_bench.json, or --out FILE; one JSON object on stdout as well).

1. Step cost.  7B geometry, B = 8, contexts 1100 / 2500: one decode step through a3v_llama_decode_step_rows with every row at the
   same position against a3v_llama_decode_step at that position (forward_inference_rows against forward_inference: embedding, the
   single-call layer stack, final norm, LM head).  Same process, same model object and cache, the two alternating step by step,
   device events around every step, median [min .. max] (the method of tools/kv8_decode_bench.py).  The caches hold N(0, 1) rows.
   Expected from the project's own figures (5-7 us per small launch, one more launch per layer): 0.15-0.25 ms on ~3.8 ms.
2. End to end.  64 text prompts of 64 tokens, per-prompt max_gen_len from a fixed seeded list in [32, 1024] (random weights do not
   emit EOS, so the list IS the answer-length mix), greedy: MetaModel.generate in batches of 8 -- every batch runs to its longest
   answer and the ids behind a prompt's own length are dropped -- against MetaModel.generate_many(batch_rows=8).  Reported: wall
   seconds (host included), kept tokens, kept tokens per second, decode steps by arithmetic (sum over batches of the longest row
   against sum of lengths / 8).
usage: tools/ragged_decode_bench.py [--contexts 1100,2500] [--steps 30] [--prompts 64] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.kv8_decode_bench import time_alternating  # noqa: E402

DEV = "cuda"
B = 8


def step_cost(m, args, contexts, steps, warmup):
    g = torch.Generator(device=DEV).manual_seed(0)
    tok = torch.randint(3, args.vocab_size, (B, 1), device=DEV, generator=g)
    flat = tok.view(B).contiguous()
    out = torch.empty(B, args.vocab_size, dtype=torch.float32, device=DEV)
    cells = []
    for ctx in contexts:
        m.allocate_rows(B)
        m.cache_image_words = 0
        for k, v in zip(m._k_cache, m._vt_cache):
            k[:, :, :ctx].normal_(generator=g)
            v[:, :, :, :ctx].normal_(generator=g)
        pos = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        t = time_alternating([lambda: m.forward_inference(tok, ctx), lambda: m.forward_inference_rows(flat, pos, ctx, out=out)], steps, warmup)
        cell = {"context": ctx}
        for name, tt in zip(("uniform", "rows"), t):
            cell[name] = {"ms_per_step": round(tt["median"] * 1e3, 3), "ms_min": round(tt["min"] * 1e3, 3), "ms_max": round(tt["max"] * 1e3, 3)}
        cell["rows_minus_uniform_ms"] = round((t[1]["median"] - t[0]["median"]) * 1e3, 3)
        cell["per_layer_us"] = round((t[1]["median"] - t[0]["median"]) * 1e6 / args.n_layers, 2)
        cells.append(cell)
        print(json.dumps(cell), flush=True)
    return cells


def end_to_end(m, n_prompts, prompt_len):
    from a3vlm_amd.model.meta import MetaModel
    mm = MetaModel.__new__(MetaModel)
    torch.nn.Module.__init__(mm)
    mm.llma, mm.tokenizer, mm.llama_type = m, bench._SynthTokenizer(prompt_len), "llama_ens5"
    prompts = [f"synthetic prompt {i}" for i in range(n_prompts)]
    lens = [random.Random(1234 + i).randint(32, 1024) for i in range(n_prompts)]
    res = {"prompts": n_prompts, "prompt_tokens": prompt_len, "gen_len_list_seed": "random.Random(1234 + i).randint(32, 1024)",
           "sum_of_lengths": sum(lens), "steps_generate": sum(max(lens[i:i + B]) for i in range(0, n_prompts, B)),
           "steps_generate_many_ideal": -(-sum(lens) // B)}
    # warm both paths (weight images, workspaces, first-launch costs)
    mm.generate(prompts[:B], None, max_gen_len=8, temperature=0.0)
    mm.generate_many(prompts[:B], None, batch_rows=B, max_gen_len=8, temperature=0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kept_a, short_a = 0, []
    for i in range(0, n_prompts, B):
        _, ids = mm.generate(prompts[i:i + B], None, max_gen_len=max(lens[i:i + B]), temperature=0.0, return_ids=True)
        kept_a += sum(min(len(t), n) for t, n in zip(ids, lens[i:i + B]))
        short_a += [(i + j, lens[i + j], len(t)) for j, t in enumerate(ids) if len(t) < lens[i + j]]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _, ids = mm.generate_many(prompts, None, batch_rows=B, max_gen_len=lens, temperature=0.0, return_ids=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    kept_b = sum(len(t) for t in ids)
    # answers that ended before their length limit (the random weights emitted EOS): (prompt, limit, ids kept)
    res["ended_early"] = {"generate": short_a, "generate_many": [(i, n, len(t)) for i, (t, n) in enumerate(zip(ids, lens)) if len(t) < n]}
    res["generate_batches_of_8"] = {"seconds": round(t1 - t0, 3), "kept_tokens": kept_a, "kept_tok_s": round(kept_a / (t1 - t0), 1)}
    res["generate_many_rows_8"] = {"seconds": round(t2 - t1, 3), "kept_tokens": kept_b, "kept_tok_s": round(kept_b / (t2 - t1), 1)}
    res["speedup"] = round((t1 - t0) / (t2 - t1), 3)
    mm.llma = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1100,2500")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--prompt_len", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"status": "NOT MEASURED", "reason": "no GPU in this run"}))
        return
    m, args = bench.build_model("7b", DEV, 4096)
    m.eval()
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B bf16, B={B}, Smax 4096; step cost: {a.steps} timed steps per cell after {a.warmup} warm-up, the two step forms alternating"}
    res["step_cost"] = step_cost(m, args, [int(c) for c in a.contexts.split(",")], a.steps, a.warmup)
    res["end_to_end"] = end_to_end(m, a.prompts, a.prompt_len)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
