#!/usr/bin/env python3
"""fp8 frozen base measurement (run on an MI355X from the repository root; writes profiles/fp8_base_bench.json and prints it).

The LoRA step at the headline geometry of BASELINE.json configs[2] (bench.py's lora leg: 7B, B 8, 512 text tokens + one 336^2 image,
rank 16) on a bf16 base against the same step on an fp8 base (``quantize_base_weights("fp8")``):
(a) time: both engines live in ONE process (two adapter plugins over the same base parameters; the fp8 one quantises its own images
    and drops its references), the two legs ALTERNATE round by round, and the table holds the median and the spread of the rounds;
(b) memory: each engine alone, after the other is gone -- torch.cuda.max_memory_allocated over two steps and the weight-image bytes.
``--trace-leg fp8|bf16`` runs only that leg for a few steps (the program under ``rocprofv3 --kernel-trace --stats``; no counters).

usage: tools/fp8_base_bench.py [--rounds R] [--steps K] [--warmup W] [--model 7b] [--trace-leg fp8]"""
import argparse
import dataclasses
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def _peft_over(m, args):
    from a3vlm_amd.model.LLM import llama_ens5_peft as peft
    from a3vlm_amd.util import promote_trainable_params_to_fp32
    pm = bench.share_into(peft.Transformer, peft.ModelArgs(**dataclasses.asdict(args), lora_rank=16), m, DEV)
    for n in [n for n in pm.get_trainable_params() if "lora_" not in n]:      # the trainables are this plugin's own (norms, projector, tags)
        mod, leaf = pm, n.split(".")
        for q in leaf[:-1]:
            mod = getattr(mod, q)
        setattr(mod, leaf[-1], torch.nn.Parameter(getattr(mod, leaf[-1]).detach().clone()))
    train = pm.get_trainable_params()
    for n, p in pm.named_parameters():
        p.requires_grad = n in train
    promote_trainable_params_to_fp32(pm)
    return pm


def _leg(pm, tokens, labels, image):
    from a3vlm_amd.optim import FusedAdamW
    from a3vlm_amd.train import TrainEngine
    eng = TrainEngine(pm, BF)
    params = [p for p in pm.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=2e-5, betas=(0.9, 0.95), weight_decay=0.0, engine=eng)
    return eng, bench._train_step_fn(eng, opt, None, params, tokens, labels, image)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--trace-leg", choices=["fp8", "bf16"], default=None)
    a = ap.parse_args()
    B, T = 8, 512
    m, args = bench.build_model(a.model, DEV, 2048)
    gen = torch.Generator(device=DEV).manual_seed(100)
    image = torch.randn(B, 3, 336, 336, device=DEV, generator=gen)
    tokens = torch.randint(3, args.vocab_size, (B, T), device=DEV, generator=gen)
    tokens[:, 0] = 1
    labels = tokens.clone()
    labels[:, :T // 2] = 0
    timer = bench.Timer(None, DEV)
    if a.trace_leg:
        pm = _peft_over(m, args)
        del m
        if a.trace_leg == "fp8":
            pm.quantize_base_weights("fp8")
        eng, one = _leg(pm, tokens, labels, image)
        print(json.dumps({"leg": a.trace_leg, "step_ms": timer(one, a.steps, max(1, a.warmup)) * 1e3}))
        return 0
    pms = {"lora_bf16": _peft_over(m, args), "lora_fp8_base": _peft_over(m, args)}
    del m
    pms["lora_fp8_base"].quantize_base_weights("fp8")        # (its own images; the bf16 parameters stay alive through the other plugin)
    legs = {k: _leg(pm, tokens, labels, image) for k, pm in pms.items()}
    rounds = {k: [] for k in legs}
    for k, (eng, one) in legs.items():
        timer(one, 1, max(1, a.warmup))
    for r in range(a.rounds):
        for k, (eng, one) in legs.items():
            rounds[k].append(timer(one, a.steps, 1) * 1e3)
    out = {"device": torch.cuda.get_device_name(0), "model": a.model, "B": B, "T": T, "rank": 16, "rounds": a.rounds,
           "steps_per_round": a.steps, "order": "bf16, fp8 alternating per round, one process"}
    for k, (eng, one) in legs.items():
        ts = sorted(rounds[k])
        out[k] = {"step_ms_rounds": rounds[k], "step_ms_median": statistics.median(ts), "step_ms_min": ts[0], "step_ms_max": ts[-1],
                  "loss": float(one.loss), "recompute": bool(eng.recompute), "weight_image_gib": eng.weight_image_bytes() / 2 ** 30,
                  "weight_image_decoder_gib": eng.weight_image_bytes(head=False) / 2 ** 30}
    out["fp8_over_bf16_step_time"] = out["lora_fp8_base"]["step_ms_median"] / out["lora_bf16"]["step_ms_median"]
    # memory: each engine alone.  bf16 first (the fp8 plugin and its engine dropped), then that plugin itself is quantised
    del legs, eng, one
    pm = pms.pop("lora_bf16")
    pms.clear()
    for k in ("lora_bf16", "lora_fp8_base"):
        if k == "lora_fp8_base":
            pm.quantize_base_weights("fp8")
        pm.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        eng, one = _leg(pm, tokens, labels, image)
        timer(one, 2, 1)
        out[k].update({"peak_allocated_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "allocated_before_engine_gib": base / 2 ** 30})
        del eng, one
    out["peak_memory_saved_gib"] = out["lora_bf16"]["peak_allocated_gib"] - out["lora_fp8_base"]["peak_allocated_gib"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fp8_base_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
