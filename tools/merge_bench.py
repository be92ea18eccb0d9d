#!/usr/bin/env python3
"""LoRA merge measurement (writes profiles/lora_merge_bench.json, or --out FILE; one JSON object on stdout as well).

(a) per-module merge on the 7B decoder shapes, r = 16: a3v_lora_merge over a bf16 base (in place) and over an NF4 base (into a bf16
    matrix), beside the route that existed before it, timed in the same run with the calls alternating: a3v_gemm_nt with the residual
    epilogue on the adapters padded to the GEMM's 64-wide K granule (bf16(acc) + W: two roundings), preceded by a3v_dequantize_nf4
    where the base is NF4.  Bytes moved are the bytes the algorithm needs (base read once, result written once; the adapters are
    noise), divided by the event time per call.  Every call works on another copy of the matrix (> 1.5 GB in rotation), so the base
    streams from HBM and not from the 256-MB last-level cache.
(b) 7B decode ms/step at B = 8 (bench.py's decode geometry and decode_leg): the adapter model (per-kernel path with adapter GEMMs), the
    same object after merge_adapters() in bf16, the base bf16 model (the expectation: equal to the merged one, it is the same code),
    and the merged model after quantize_decode_weights("nf4").
usage: tools/merge_bench.py [--skip-model] [--out FILE]"""
import dataclasses
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
R = 16
SHAPES_7B = {"wq_wk_wv_wo": (4096, 4096), "w1_w3": (11008, 4096), "w2": (4096, 11008)}


def _time_alternating(fns, reps=40, warm=4):
    """seconds per call of each fn: rounds of one call each, alternating, each call between its own pair of events"""
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


def merge_shapes():
    res = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, (N, K) in SHAPES_7B.items():
        ncopy = max(2, int(1.5e9 // (N * K * 2)) + 1)
        ws = [torch.randn(N, K, device=DEV, generator=g).mul_(0.02).to(BF) for _ in range(ncopy)]
        q4 = [ops.quantize_nf4(w)[:2] for w in ws]
        out = [torch.empty(N, K, device=DEV, dtype=BF) for _ in range(ncopy)]
        lb = torch.randn(N, R, device=DEV, generator=g).mul_(0.02).to(BF)
        la = torch.randn(R, K, device=DEV, generator=g).mul_(0.02).to(BF)
        lb64 = torch.zeros(N, 64, device=DEV, dtype=BF)              # the GEMM route: contraction padded to its 64 granule
        lb64[:, :R] = lb
        lat64 = torch.zeros(K, 64, device=DEV, dtype=BF)
        lat64[:, :R] = la.t()
        it = {"i": 0}

        def nxt():
            it["i"] = (it["i"] + 1) % ncopy
            return it["i"]

        def merge_bf16():
            ops.lora_merge(ws[nxt()], lb, la)

        def gemm_bf16():
            w = ws[nxt()]
            ops.gemm_nt(lb64, lat64, w, residual=w, epilogue=ops.EPI_RESIDUAL)

        def merge_nf4():
            i = nxt()
            ops.lora_merge(q4[i], lb, la, out=out[i])

        def route_nf4():
            i = nxt()
            ops.dequantize_nf4(*q4[i], out[i])
            ops.gemm_nt(lb64, lat64, out[i], residual=out[i], epilogue=ops.EPI_RESIDUAL)

        t = _time_alternating([merge_bf16, gemm_bf16, merge_nf4, route_nf4])
        b_bf = 2 * N * K * 2                                         # read + write of the bf16 matrix
        b_n4 = N * K // 2 + N * K // 64 * 4 + N * K * 2              # codes + scales read, bf16 written
        b_n4_route = b_n4 + 2 * N * K * 2                            # dequantise (codes in, bf16 out), then read + write again
        rows = (("merge_bf16", b_bf), ("gemm_residual_bf16", b_bf), ("merge_nf4", b_n4), ("dequant_then_gemm_residual_nf4", b_n4_route))
        res[name] = {"N": N, "K": K, "R": R, "copies": ncopy}
        for (key, nbytes), tt in zip(rows, t):
            res[name][key] = {"us_median": round(tt["median"] * 1e6, 1), "us_min": round(tt["min"] * 1e6, 1), "us_max": round(tt["max"] * 1e6, 1),
                              "bytes": nbytes, "TBps_at_median": round(nbytes / tt["median"] / 1e12, 3)}
        del ws, q4, out
        torch.cuda.empty_cache()
    return res


def decode_7b():
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    B, T = 8, 512
    m, args = bench.build_model("7b", DEV, 2048)
    timer = bench.Timer(None, DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    img = torch.randn(B, 3, 336, 336, device=DEV, generator=g).to(BF)
    tokens = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=g)
    res = {"geometry": f"7B, B={B}, {T}-token prompt + {m.image_words} image words, 16 timed decode steps, lora_rank {R}"}

    def leg(model):
        torch.cuda.synchronize()
        sec = bench.decode_leg(model, lambda: model.forward_inference(tokens, 0, img), B, T, 16, timer, DEV)
        return {"ms_per_step": round(sec * 1e3, 3), "tok_s": round(B / sec, 1)}

    res["base_bf16"] = leg(m)
    pm = bench.share_into(peft.Transformer, peft.ModelArgs(**dataclasses.asdict(args), lora_rank=R), m, DEV)     # shares the base matrices
    pm.eval()
    res["adapter_model_per_kernel"] = leg(pm)
    m._destroy_kv_cache()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    pm.merge_adapters()                                              # in place: m's shared matrices are the merged ones from here on
    e.record()
    torch.cuda.synchronize()
    res["merge_adapters_ms"] = round(s.elapsed_time(e), 1)
    res["merged_bf16"] = leg(pm)
    res["base_bf16_again"] = leg(m)                                  # spread of the same code on the same weights
    m._destroy_kv_cache()
    pm.quantize_decode_weights("nf4")
    res["merged_nf4"] = leg(pm)
    return res


if __name__ == "__main__":
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lora_merge_bench.json")
    out = {"merge": merge_shapes()}
    if "--skip-model" not in sys.argv:
        out["decode"] = decode_7b()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)
