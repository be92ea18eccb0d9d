"""What constrained decoding costs, two measurements in ONE run:
 1. the mask pass a3v_constrain_logits at B 8, V 32000 (out of place, and in place) beside a3v_logits_prepare at the same shape (penalty +
    lse, and penalty alone: the existing pass over the same logits), alternating launch by launch, device events around one launch each;
 2. the step of MetaModel.generate on the 7B bf16 model, B 8, context about 1100 (model step + a3v_generate_step), without and with a
    constraint (a3v_constrain_logits in front, a3v_constrain_advance behind), alternating step by step.
The table is random (64 states, about 30 % of the tokens allowed per state): the work does not depend on its values.
Median [min .. max] after warm-up.  usage (GPU box): PYTHONPATH=. python tools/constrain_bench.py [--out profiles/constrain_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from a3vlm_amd import ops  # noqa: E402

DEV = "cuda"


def stat(x):
    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1), "max_us": round(max(x), 1), "n": len(x)}


def random_table(S, V, g):
    t = torch.randint(0, S, (S, V), generator=g, device=DEV, dtype=torch.int32).to(torch.int16)
    t[torch.rand(S, V, generator=g, device=DEV) >= 0.3] = -1
    t[:, 5] = 0                                            # every state allows something
    return t.contiguous()


def kernels(B, V, n, warmup, g):
    logits = torch.randn(B, V, device=DEV, generator=g) * 2.5
    S = 64
    trans = random_table(S, V, g)
    state = torch.randint(0, S, (B,), generator=g, device=DEV, dtype=torch.int32)
    out = torch.empty_like(logits)
    work = logits.clone()
    seen = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, (V + 31) // 32), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    lse = torch.empty(B, device=DEV)
    runs = {
        "constrain_logits": lambda: ops.constrain_logits(logits, trans, state, out),
        "constrain_logits_in_place": lambda: ops.constrain_logits(work, trans, state, work),
        "logits_prepare_penalty_lse": lambda: ops.logits_prepare(logits, seen, 1.3, out, lse),
        "logits_prepare_penalty": lambda: ops.logits_prepare(logits, seen, 1.3, out, None),
        "logits_prepare_lse": lambda: ops.logits_prepare(logits, None, 1.0, None, lse),
    }
    times = {k: [] for k in runs}
    for it in range(n + warmup):
        for name, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {k: stat(v) for k, v in times.items()}
    res["bytes_constrain_logits"] = B * V * (4 + 4 + 2)
    return res


def step(a, g):
    B, T, n = a.batch, a.context, 2 * (a.steps + a.warmup)
    m, args = bench.build_model(a.model, DEV, T + n + 8)
    m.eval()
    V = args.vocab_size
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
    S = 64
    trans = random_table(S, V, g)
    state = torch.randint(0, S, (B,), generator=g, device=DEV, dtype=torch.int32)
    first = torch.full((B,), T, dtype=torch.int32, device=DEV)
    out = torch.empty((B, V), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        m.forward_inference(tokens[:, :T - 1], 0)
        times = {False: [], True: []}
        for k in range(n):
            cur, on = T + k, bool(k & 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            logits = m.forward_inference(tokens[:, cur - 1:cur], cur - 1)
            z = ops.constrain_logits(logits, trans, state, out) if on else logits
            ops.generate_step(z, None, tokens, text_mask, cur, stop_seq, stop_off, 1, stopped, stop_pos, live)
            if on:
                ops.constrain_advance(tokens, trans, state, first, col=cur)
            e1.record()
            e1.synchronize()
            if k >= 2 * a.warmup:
                times[on].append(e0.elapsed_time(e1) * 1e3)
            stopped.zero_()                       # a random model may emit EOS: keep every row running, the work per step the same
        assert bool(((state >= 0) & (state < S)).all()), "every constrained step chose an allowed token"
    off, on = stat(times[False]), stat(times[True])
    return {"model": a.model, "dtype": "bf16", "batch": B, "context": T, "vocab": V, "step_unconstrained": off, "step_constrained": on,
            "difference_us": round(on["median_us"] - off["median_us"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/constrain_bench.json")
    ap.add_argument("--model", default="7b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--context", type=int, default=1100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    res = {"kernels": {"batch": a.batch, "vocab": a.vocab, "states": 64, **kernels(a.batch, a.vocab, a.launches, 20, g)}}
    if not a.no_step:
        res["step"] = step(a, g)
    res["note"] = ("one run; kernels: the five launches alternating launch by launch, device events around ONE launch each, so every figure "
                   "includes the launch itself; step: off / on alternating step by step, device events around model step + bookkeeping "
                   "launches, the context grows by one key per step")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
