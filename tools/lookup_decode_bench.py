#!/usr/bin/env python3
"""Lookup decoding measurement (writes profiles/lookup_decode_bench.json, or --out FILE; one JSON object on stdout as well).

1. Step cost.  7B geometry bf16, contexts 1100 / 2500, B in {1, 2, 4} cache rows: the verify step (forward_verify_rows, every one of
   the Q queries live) at Q in {1, 2, 4, 8} against the plain ragged step at the same B -- with --parent_lib FILE (a
   liba3vlm_hip.so built from the parent commit) the PARENT's a3v_llama_decode_step_rows, else this library's.  Same process, model
   object and cache, the forms alternating step by step, device events around every step, median [min .. max]
   (tools/kv8_decode_bench.py's method).  c(B, Q) = verify / plain; a step that accepts a drafts emits 1 + a tokens, so lookup
   decoding pays when a > c - 1: "break_even_accepted".
2. End to end.  Text prompts, batch_rows 1 and 4: generate_many without lookup against lookup=D with a SCRIPTED drafter that drafts
   the known greedy continuation with probability p (0, 0.5, 0.9) and ids the model does not pick otherwise.  Random weights say
   nothing about the acceptance of real prompt lookup on real answers: the legs show what a given acceptance is worth.
usage: tools/lookup_decode_bench.py [--contexts 1100,2500] [--steps 30] [--prompts 4] [--gen 96] [--parent_lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from a3vlm_amd import lib as _lib, ops  # noqa: E402
from tools.kv8_decode_bench import time_alternating  # noqa: E402

DEV = "cuda"
ROWS = (1, 2, 4)
QS = (1, 2, 4, 8)


def rows_step_fn(path):
    """a3v_llama_decode_step_rows of the library at ``path`` (the parent commit's) with this library's signature table"""
    L = ctypes.CDLL(path) if path else _lib.load()
    f = L.a3v_llama_decode_step_rows
    f.restype, f.argtypes = _lib.SIGNATURES["a3v_llama_decode_step_rows"]
    return f


def step_cost(m, args, contexts, steps, warmup, rows_step):
    g = torch.Generator(device=DEV).manual_seed(0)
    cells = []
    for ctx in contexts:
        for B in ROWS:
            m.allocate_rows(B)
            m.cache_image_words = 0
            for k, v in zip(m._k_cache, m._vt_cache):
                k[:, :, :ctx + 8].normal_(generator=g)
                v[:, :, :, :ctx + 8].normal_(generator=g)
            tok = torch.randint(3, args.vocab_size, (B, 8), device=DEV, generator=g)
            pos = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
            out1 = torch.empty(B, args.vocab_size, dtype=torch.float32, device=DEV)

            def plain_step():             # forward_inference_rows with the layer stack from the given library
                a = m.args
                h = m._buf("h", (B, a.dim))
                ops.embed_assemble(tok[:, :1].contiguous(), m.tok_embeddings.weight, h, B, 1, 0, a.dim)
                tab = m._llama_layer_table()
                xn, qkv, att, act, scratch, sws = m._decode_step_buffers(B)
                rc = rows_step(tab, m.n_layers, h.data_ptr(), xn.data_ptr(), qkv.data_ptr(), att.data_ptr(), act.data_ptr(), scratch.data_ptr(),
                               sws.data_ptr(), m._cos_sin_dev().data_ptr(), pos.data_ptr(), ctx, B, a.dim, m.n_heads, m.n_kv_heads, m.head_dim,
                               m.ffn, m._k_cache[0].shape[2], a.norm_eps, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
                xl = m._buf("xn_last", (B, a.dim))
                ops.rmsnorm(h, m.norm.weight, xl, a.norm_eps)
                m._lm_head_last(xl, out1, True)

            def verify(Q):
                x = tok[:, :Q].contiguous()
                nq = torch.full((B,), Q, dtype=torch.int32, device=DEV)
                out = torch.empty(B * Q, args.vocab_size, dtype=torch.float32, device=DEV)
                return lambda: m.forward_verify_rows(x, pos, nq, ctx, out=out)
            t = time_alternating([plain_step] + [verify(Q) for Q in QS], steps, warmup)
            cell = {"context": ctx, "rows": B,
                    "plain": {"ms_per_step": round(t[0]["median"] * 1e3, 3), "ms_min": round(t[0]["min"] * 1e3, 3), "ms_max": round(t[0]["max"] * 1e3, 3)}}
            for Q, tt in zip(QS, t[1:]):
                c = tt["median"] / t[0]["median"]
                cell[f"Q{Q}"] = {"ms_per_step": round(tt["median"] * 1e3, 3), "ms_min": round(tt["min"] * 1e3, 3), "ms_max": round(tt["max"] * 1e3, 3),
                                 "c": round(c, 3), "break_even_accepted": round(max(c - 1, 0), 3)}
            cells.append(cell)
            print(json.dumps(cell), flush=True)
    return cells


def end_to_end(m, args, n_prompts, gen, prompt_len, D):
    from a3vlm_amd.model.meta import MetaModel
    mm = MetaModel.__new__(MetaModel)
    torch.nn.Module.__init__(mm)
    mm.llma, mm.tokenizer, mm.llama_type = m, bench._SynthTokenizer(prompt_len), "llama_ens5"
    prompts = [f"synthetic prompt {i}" for i in range(n_prompts)]
    order = []
    orig = m.prefill_row

    def counted(row, *aa, **kw):
        order.append(row)
        return orig(row, *aa, **kw)
    m.prefill_row = counted
    res = {"prompts": n_prompts, "prompt_tokens": prompt_len, "max_gen_len": gen, "lookup": D}
    try:
        for rows in (1, 4):
            kw = dict(batch_rows=rows, max_gen_len=gen, return_ids=True)
            mm.generate_many(prompts[:1], None, batch_rows=rows, max_gen_len=4)                      # warm
            mm.generate_many(prompts[:1], None, batch_rows=rows, max_gen_len=4, lookup=D)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, want = mm.generate_many(prompts, None, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            kept = sum(len(t) for t in want)
            leg = {"plain": {"seconds": round(dt, 3), "kept_tokens": kept, "tok_s": round(kept / dt, 1)}}
            for p in (0.0, 0.5, 0.9):
                rng = random.Random(7)
                order.clear()
                in_row = {}

                def drafter(tokens, cur, limit, pos, stopped, next_tok, x, nq):
                    for k, r in enumerate(order):          # the k-th prefill of the call is prompt k
                        in_row[r] = k
                    cu, li, st, nt = cur.tolist(), limit.tolist(), stopped.tolist(), next_tok.tolist()
                    xs, ns = [], []
                    for r in range(len(cu)):
                        row, nd = [nt[r]] + [0] * D, 0
                        if not st[r] and r in in_row:
                            ids = want[in_row[r]]
                            g0 = cu[r] - prompt_len                       # generated so far
                            nd = max(min(D, li[r] - 1 - cu[r]), 0)
                            right = rng.random() < p
                            for e in range(nd):
                                t = ids[g0 + e] if g0 + e < len(ids) else 0
                                row[1 + e] = t if right else (t + 1) % args.vocab_size
                        xs.append(row)
                        ns.append(1 + nd)
                    x.copy_(torch.tensor(xs, device=DEV))
                    nq.copy_(torch.tensor(ns, dtype=torch.int32, device=DEV))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, ids = mm.generate_many(prompts, None, lookup=D, lookup_drafter=drafter, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                kept = sum(len(t) for t in ids)
                st = mm.last_lookup_stats
                leg[f"scripted_p{p}"] = {"seconds": round(dt, 3), "kept_tokens": kept, "tok_s": round(kept / dt, 1), "stats": st,
                                         "accepted_per_step": round(st["accepted"] / max(st["steps"], 1), 3), "same_ids_as_plain": ids == want,
                                         "note": "the scripted drafter reads the row state on the host every step: a real drafter does not"}
            res[f"rows{rows}"] = leg
    finally:
        del m.prefill_row
        mm.llma = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", default="1100,2500")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--gen", type=int, default=96)
    ap.add_argument("--prompt_len", type=int, default=64)
    ap.add_argument("--lookup", type=int, default=3)
    ap.add_argument("--parent_lib", default=None, help="liba3vlm_hip.so of the parent commit: its plain ragged step is the yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"status": "NOT MEASURED", "reason": "no GPU in this run"}))
        return
    m, args = bench.build_model("7b", DEV, 4096)
    m.eval()
    res = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "geometry": f"7B bf16, Smax 4096; step cost: {a.steps} timed steps per cell after {a.warmup} warm-up, the forms alternating; "
                       f"plain = a3v_llama_decode_step_rows of {'the parent library' if a.parent_lib else 'this library'}"}
    res["step_cost"] = step_cost(m, args, [int(c) for c in a.contexts.split(",")], a.steps, a.warmup, rows_step_fn(a.parent_lib))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:                     # the first half is kept even if the second does not finish
        json.dump(res, f, indent=1)
    res["end_to_end"] = end_to_end(m, args, a.prompts, a.gen, a.prompt_len, a.lookup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
