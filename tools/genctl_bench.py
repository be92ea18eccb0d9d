"""What the generation controls cost per decode step: 7B bf16, B 8, context about 1100, the step of MetaModel.generate (model step +
a3v_generate_step) with the options off and on (a3v_logits_prepare with penalty and lse in front, a3v_generate_record behind),
alternating step by step in ONE run, device events around every step.  Median [min .. max] of 30 steps each after warm-up.
usage (GPU box): PYTHONPATH=. python tools/genctl_bench.py [--out profiles/genctl_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from a3vlm_amd import ops  # noqa: E402
from a3vlm_amd.model.genctl import GenControls  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/genctl_bench.json")
    ap.add_argument("--model", default="7b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--context", type=int, default=1100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    B, T, n = a.batch, a.context, 2 * (a.steps + a.warmup)
    m, args = bench.build_model(a.model, DEV, T + n + 8)
    m.eval()
    V = args.vocab_size
    g = torch.Generator(device=DEV).manual_seed(1)
    tokens = torch.zeros(B, T + n, dtype=torch.long, device=DEV)
    tokens[:, :T] = torch.randint(3, V, (B, T), device=DEV, generator=g)
    tokens[:, 0] = 1
    text_mask = torch.zeros(B, T + n, dtype=torch.bool, device=DEV)
    text_mask[:, :T] = True
    stopped = torch.zeros(B, dtype=torch.bool, device=DEV)
    stop_pos = torch.full((B,), T + 1, dtype=torch.long, device=DEV)
    live = torch.full((1,), B, dtype=torch.int32, device=DEV)
    stop_seq = torch.tensor([2], dtype=torch.long, device=DEV)
    stop_off = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    gc = GenControls(B, V, n, 1.3, True, DEV)
    gc.prompt_len.fill_(T)
    gc.mark_prompts(tokens)
    with torch.no_grad():
        m.forward_inference(tokens[:, :T - 1], 0)
        times = {False: [], True: []}
        for k in range(n):
            cur, on = T + k, bool(k & 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            logits = m.forward_inference(tokens[:, cur - 1:cur], cur - 1)
            z = gc.prepare(logits) if on else logits
            ops.generate_step(z, None, tokens, text_mask, cur, stop_seq, stop_off, 1, stopped, stop_pos, live)
            if on:
                gc.record(logits, tokens, col=cur)
            e1.record()
            e1.synchronize()
            if k >= 2 * a.warmup:
                times[on].append(e0.elapsed_time(e1) * 1e3)
            stopped.zero_()                       # a random model may emit EOS: keep every row running, the work per step the same
    def stat(x):
        return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1), "max_us": round(max(x), 1), "n": len(x)}
    off, on = stat(times[False]), stat(times[True])
    res = {"model": a.model, "dtype": "bf16", "batch": B, "context": T, "vocab": V, "penalty": 1.3, "logprobs": True,
           "step_options_off": off, "step_options_on": on, "difference_us": round(on["median_us"] - off["median_us"], 1),
           "note": "one run, off / on alternating step by step, device events around model step + bookkeeping launches; the context grows "
                   "by one key per step, so the on steps see on average half a key more than the off steps"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
