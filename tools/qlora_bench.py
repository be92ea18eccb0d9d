#!/usr/bin/env python3
"""QLoRA measurement (run on an MI355X from the repository root; writes profiles/qlora_bench.json and prints it).

(a) a3v_dequantize_nf4_images at the 7B module shapes -- Wd only, Wt only, both -- against the composition the library offered before
    it (a3v_dequantize_nf4, then a3v_transpose), alternating the two in one process; achieved bytes/s from the bytes the algorithm
    needs (0.5 B codes + 4/64 B scales + 2 B per image written, per weight) beside this box's own device-copy rate.
    GATE: for every shape the fused kernel (both images) is not slower than the composition (2.56 against 6.56 B per weight).
(b) one QLoRA step against the bf16 LoRA step on the same weights (Wd) at the headline geometry of BASELINE.json configs[2]
    (bench.py's lora leg: 7B, B 8, 512 text tokens + one 336^2 image, rank 16): seconds per step and torch.cuda.max_memory_allocated.

usage: tools/qlora_bench.py [--skip-step] [--steps K] [--warmup W] [--model 7b]"""
import argparse
import dataclasses
import gc
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
SHAPES_7B = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096)]


def _time(fns, reps=30, warm=3):
    """seconds per call of each fn, the candidates alternating inside one timed loop (same box, same moment)"""
    for fn in fns:
        for _ in range(warm):
            fn()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)] for _ in fns]
    torch.cuda.synchronize()
    for r in range(reps):
        for j, fn in enumerate(fns):
            ev[j][2 * r].record()
            fn()
            ev[j][2 * r + 1].record()
    torch.cuda.synchronize()
    out = []
    for j in range(len(fns)):
        ts = sorted(ev[j][2 * r].elapsed_time(ev[j][2 * r + 1]) for r in range(reps))
        out.append(ts[len(ts) // 2] * 1e-3)            # median
    return out


def copy_rate():
    """bytes/s (read + write) of a 1-GiB device-to-device copy on this box"""
    a = torch.empty(2 ** 30, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    (t,) = _time([lambda: b.copy_(a)], reps=10)
    return 2 * a.numel() / t


def dequantiser():
    res = []
    for N, K in SHAPES_7B:
        # rotate through enough modules that the codes come from HBM (>= 1.5 GB of images written per round)
        n = max(2, int(1.5e9 // (4 * N * K)) + 1)
        g = torch.Generator(device=DEV).manual_seed(N + K)
        mods = [ops.quantize_nf4((torch.randn(N, K, device=DEV, generator=g) * 0.02).to(BF))[:2] for _ in range(n)]
        Np = (N + 63) // 64 * 64
        wd = torch.empty(N, K + 64, dtype=BF, device=DEV)[:, :K]         # windows inside wider images, as the engine's
        wt = torch.empty(K, Np + 64, dtype=BF, device=DEV)[:, :N]
        wd2 = torch.empty(N, K, dtype=BF, device=DEV)
        wt2 = torch.empty(K, Np, dtype=BF, device=DEV)
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % n
            return mods[it[0]]

        def comp():
            q, s = nxt()
            ops.dequantize_nf4(q, s, wd2)
            ops.transpose(wd2, wt2, N, K, Np)
        fns = [lambda: ops.dequantize_nf4_images(*nxt(), wd=wd), lambda: ops.dequantize_nf4_images(*nxt(), wt=wt),
               lambda: ops.dequantize_nf4_images(*nxt(), wd=wd, wt=wt), comp, lambda: ops.dequantize_nf4(*nxt(), wd2)]
        t_d, t_t, t_b, t_c, t_old = _time(fns)
        q, s = mods[0]
        ops.dequantize_nf4_images(q, s, wd=wd, wt=wt)
        ops.dequantize_nf4(q, s, wd2)
        assert torch.equal(wd, wd2) and torch.equal(wt, wd2.t()), "the timed kernel computes something else"
        w = N * K
        res.append({"N": N, "K": K, "wd_only_us": t_d * 1e6, "wt_only_us": t_t * 1e6, "both_us": t_b * 1e6,
                    "dequantize_then_transpose_us": t_c * 1e6, "dequantize_nf4_us": t_old * 1e6,
                    "both_bytes_per_s": w * (0.5 + 4 / 64 + 4) / t_b, "wd_only_bytes_per_s": w * (0.5 + 4 / 64 + 2) / t_d,
                    "wt_only_bytes_per_s": w * (0.5 + 4 / 64 + 2) / t_t, "composition_bytes_per_s": w * (0.5 + 4 / 64 + 2 + 4) / t_c,
                    "gate_not_slower_than_composition": bool(t_b <= t_c)})
        del mods, wd, wt, wd2, wt2
        torch.cuda.empty_cache()
    return res


def step(model, steps, warmup):
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    from a3vlm_amd.optim import FusedAdamW
    from a3vlm_amd.train import TrainEngine
    from a3vlm_amd.util import promote_trainable_params_to_fp32
    B, T = 8, 512
    m, args = bench.build_model(model, DEV, 2048)
    pm = bench.share_into(peft.Transformer, peft.ModelArgs(**dataclasses.asdict(args), lora_rank=16), m, DEV)
    del m                                      # the adapter plugin alone holds the base matrices now: freeing them frees memory
    gc.collect()
    train = pm.get_trainable_params()
    for n, p in pm.named_parameters():
        p.requires_grad = n in train
    # the same weights on both sides: every base matrix becomes its own Wd first
    with torch.no_grad():
        for n, p in pm.named_parameters():
            if "lora_" not in n and (n == "output.weight" or (n.startswith("layers.") and n.endswith(
                    (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight")))):
                q, s, _ = ops.quantize_nf4(p.data.contiguous())
                ops.dequantize_nf4(q, s, p.data)
    promote_trainable_params_to_fp32(pm)
    gen = torch.Generator(device=DEV).manual_seed(100)
    image = torch.randn(B, 3, 336, 336, device=DEV, generator=gen)
    tokens = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=gen)
    tokens[:, 0] = 1
    labels = tokens.clone()
    labels[:, :T // 2] = 0
    timer = bench.Timer(None, DEV)
    out = {"model": model, "B": B, "T": T, "image_words": pm.image_words, "rank": 16, "steps": steps, "warmup": warmup}
    for name in ("lora_bf16", "qlora_nf4"):
        if name == "qlora_nf4":
            pm.quantize_base_weights("nf4")
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        eng = TrainEngine(pm, BF)
        params = [p for p in pm.parameters() if p.requires_grad]
        opt = FusedAdamW(params, lr=2e-5, betas=(0.9, 0.95), weight_decay=0.0, engine=eng)
        one = bench._train_step_fn(eng, opt, None, params, tokens, labels, image)
        sec = timer(one, steps, max(1, warmup))
        out[name] = {"step_ms": sec * 1e3, "loss": float(one.loss), "peak_allocated_gib": torch.cuda.max_memory_allocated() / 2 ** 30,
                     "allocated_before_engine_gib": base / 2 ** 30, "weight_image_gib": eng.weight_image_bytes() / 2 ** 30,
                     "recompute": bool(eng.recompute)}
        pm.zero_grad(set_to_none=True)
        del eng, opt, one, params
    out["qlora_over_lora_step_time"] = out["qlora_nf4"]["step_ms"] / out["lora_bf16"]["step_ms"]
    out["peak_memory_saved_gib"] = out["lora_bf16"]["peak_allocated_gib"] - out["qlora_nf4"]["peak_allocated_gib"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="7b")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "device_copy_bytes_per_s": copy_rate(), "dequantiser": dequantiser()}
    res["gate_all_shapes"] = all(r["gate_not_slower_than_composition"] for r in res["dequantiser"])
    res["step"] = "NOT MEASURED" if a.skip_step else step(a.model, a.steps, a.warmup)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "qlora_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if res["gate_all_shapes"] else 1


if __name__ == "__main__":
    sys.exit(main())
