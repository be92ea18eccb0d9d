"""What sample-and-match lookup decoding adds to a lookup step ("Sample and match"), two measurements in ONE run:
 1. a3v_verify_prepare (penalty + constraint + lse) at V 32000 for (B, Q) in {(1, 4), (4, 4), (4, 8)} beside the pair it replaces,
    a3v_logits_prepare + a3v_constrain_logits over the same B * Q rows, alternating launch by launch, device events around each form;
 2. the step of generate_many(lookup=D) on the 7B bf16 model at context 1100 and the same (B, Q): `argmax` = forward_verify_rows +
    a3v_accept_rows (the parent commit's step) against `choice` = forward_verify_rows + a3v_verify_prepare + a3v_argmax +
    a3v_accept_rows_chosen (penalty, constraint and log-probs on), alternating step by step.  Every query is live; the rows are reset
    after every step, so the work per step is the same.
The table is random (64 states, about 30 % of the tokens allowed per state): the work does not depend on its values.
Median [min .. max] after warm-up.  usage (GPU box): PYTHONPATH=. python tools/lookup_ctl_bench.py [--out profiles/lookup_ctl_bench.json]"""
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
SHAPES = ((1, 4), (4, 4), (4, 8))


def stat(x):
    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1), "max_us": round(max(x), 1), "n": len(x)}


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def random_table(S, V, g):
    t = torch.randint(0, S, (S, V), generator=g, device=DEV, dtype=torch.int32).to(torch.int16)
    t[torch.rand(S, V, generator=g, device=DEV) >= 0.3] = -1
    t[:, 5] = 0                                            # every state allows something
    return t.contiguous()


def controls(B, Q, V, g, S=64):
    trans = random_table(S, V, g)
    return dict(trans=trans, state=torch.zeros(B, dtype=torch.int32, device=DEV),
                seen=torch.randint(-2 ** 31, 2 ** 31 - 1, (B, (V + 31) // 32), generator=g, device=DEV, dtype=torch.int64).to(torch.int32),
                x=torch.full((B, Q), 5, dtype=torch.long, device=DEV),       # token 5 is allowed everywhere and leads to state 0: no dead query
                nq=torch.full((B,), Q, dtype=torch.int32, device=DEV))


def kernels(V, n, warmup, g):
    cells = []
    for B, Q in SHAPES:
        c = controls(B, Q, V, g)
        logits = torch.randn(B * Q, V, device=DEV, generator=g) * 2.5
        out, lse = torch.empty_like(logits), torch.empty(B * Q, device=DEV)
        pos = torch.full((B,), 100, dtype=torch.int32, device=DEV)
        vseen, vstate = c["seen"].repeat_interleave(Q, 0).contiguous(), c["state"].repeat_interleave(Q).contiguous()

        def pair():
            ops.logits_prepare(logits, vseen, 1.3, out, lse)
            ops.constrain_logits(out, c["trans"], vstate, out)
        runs = {"verify_prepare": lambda: ops.verify_prepare(logits, c["x"], c["nq"], pos, out, seen=c["seen"], penalty=1.3, trans=c["trans"],
                                                             state=c["state"], lse=lse),
                "logits_prepare_plus_constrain_logits": pair}
        times = {k: [] for k in runs}
        for it in range(n + warmup):
            for name, f in runs.items():
                t = timed(f)
                if it >= warmup:
                    times[name].append(t)
        cell = {"rows": B, "Q": Q, "vocab": V, **{k: stat(v) for k, v in times.items()}, "bytes_streamed": B * Q * V * (4 + 4 + 2)}
        cells.append(cell)
        print(json.dumps(cell), flush=True)
    return cells


def steps(a, g):
    m, args = bench.build_model(a.model, DEV, a.context + 64)
    m.eval()
    V, ctx = args.vocab_size, a.context
    cells = []
    for B, Q in SHAPES:
        m.allocate_rows(B)
        m.cache_image_words = 0
        for k, v in zip(m._k_cache, m._vt_cache):
            k[:, :, :ctx + 8].normal_(generator=g)
            v[:, :, :, :ctx + 8].normal_(generator=g)
        c = controls(B, Q, V, g)
        W = ctx + 16
        tokens = torch.zeros(B, W, dtype=torch.long, device=DEV)
        cur = torch.zeros(B, dtype=torch.int32, device=DEV)
        limit = torch.full((B,), W, dtype=torch.int32, device=DEV)
        stopped, stop_pos = torch.zeros(B, dtype=torch.bool, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV)
        next_tok, pos = torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        stop_seq, stop_off = torch.tensor([2], dtype=torch.long, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV)
        vlogits = torch.empty(B * Q, V, dtype=torch.float32, device=DEV)
        out, lse, chosen = torch.empty_like(vlogits), torch.empty(B * Q, device=DEV), torch.zeros(B * Q, dtype=torch.long, device=DEV)
        lp, plen = torch.zeros(B, 64, device=DEV), torch.full((B,), ctx - 8, dtype=torch.int32, device=DEV)

        def reset():
            cur.fill_(ctx)
            pos.fill_(ctx)
            stopped.zero_()
            c["state"].zero_()

        def argmax_step():
            m.forward_verify_rows(c["x"], pos, c["nq"], ctx, out=vlogits)
            ops.accept_rows(vlogits, c["x"], c["nq"], tokens, cur, limit, 0, stop_seq, stop_off, 1, stopped, stop_pos, next_tok, pos, stats)

        def choice_step():
            m.forward_verify_rows(c["x"], pos, c["nq"], ctx, out=vlogits)
            ops.verify_prepare(vlogits, c["x"], c["nq"], pos, out, seen=c["seen"], penalty=1.3, trans=c["trans"], state=c["state"], lse=lse)
            ops.argmax(out, chosen)
            ops.accept_rows_chosen(chosen, c["x"], c["nq"], tokens, cur, limit, 0, stop_seq, stop_off, 1, stopped, stop_pos, next_tok, pos, stats,
                                   V=V, logits=vlogits, lse=lse, logprob=lp, prompt_len=plen, seen=c["seen"], trans=c["trans"], state=c["state"])
        times = {"argmax": [], "choice": []}
        with torch.no_grad():
            for it in range(a.steps + a.warmup):
                for name, f in (("argmax", argmax_step), ("choice", choice_step)):
                    reset()
                    t = timed(f)
                    if it >= a.warmup:
                        times[name].append(t)
        s0, s1 = stat(times["argmax"]), stat(times["choice"])
        cell = {"rows": B, "Q": Q, "context": ctx, "step_argmax": s0, "step_choice": s1, "difference_us": round(s1["median_us"] - s0["median_us"], 1),
                "ratio": round(s1["median_us"] / s0["median_us"], 4)}
        cells.append(cell)
        print(json.dumps(cell), flush=True)
    return {"model": a.model, "dtype": "bf16", "vocab": V, "cells": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lookup_ctl_bench.json")
    ap.add_argument("--model", default="7b")
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--context", type=int, default=1100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    res = {"kernels": kernels(a.vocab, a.launches, 20, g)}
    if not a.no_step:
        res["step"] = steps(a, g)
    res["note"] = ("one run; kernels: the two forms alternating launch by launch, device events around each form (the pair is two launches), so "
                   "every figure includes the launches themselves; step: argmax / choice alternating step by step, device events around the "
                   "verify step + bookkeeping launches, rows reset to the same position before every step")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
