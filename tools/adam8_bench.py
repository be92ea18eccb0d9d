#!/usr/bin/env python3
"""a3v_adamw_scaled (fp32 moments) against a3v_adamw8_scaled (blockwise e4m3 moments) on one tensor of the 7B w1|w3
size (22016 x 4096), both with the bf16 image: device events, the two kernels alternating, 30 timed launches each after 4 warm-up,
median [min .. max] and the achieved HBM rate from the bytes each kernel moves per parameter (30 and 18.0625).

Then the memory the feature is for: torch.cuda.max_memory_allocated() of a full fine-tune step in bench.py's geometry (7B, batch 8,
512-token prompt + 579 image words, clip 8, FusedAdamW; the model and the step function are bench.py's own, imported) with fp32
moments as the trainer builds it by default and with moments="e4m3" in the NN input-gradient form (main_finetune --adam8bit), each in
a fresh child process, next to the bytes the optimizer state really holds and the derived 53.9 -> 13.7 GB.  Last, ONE attempt at a
13B step with 8-bit moments on a single GPU (micro-batch 4, per-block recompute: bench.py's 13B replica), under a time limit; if
it does not fit, the peak it reached is recorded.

    python tools/adam8_bench.py [--out profiles/adam8_bench.json] [--rows 22016] [--cols 4096] [--no-memory] [--no-13b]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_FP32 = 4 + 4 + 4 + 4 + 4 + 4 + 4 + 2                 # p, g, m, v read; p, m, v written; bf16 image written
BYTES_E4M3 = 4 + 4 + 1 + 1 + 4 + 1 + 1 + 2 + 2 * 2 * 4 / 256    # p, g, two codes read; p, two codes, image written; two scales read and written


def memory_child(model, moments, batch, recompute):
    """One full fine-tune configuration in this process: 2 steps, then one JSON line with the peak."""
    import bench
    from a3vlm_amd.optim import FusedAdamW
    from a3vlm_amd.train import TrainEngine
    from a3vlm_amd.util import promote_trainable_params_to_fp32
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"model": model, "moments": moments, "batch": batch, "prompt": 512}
    try:
        m, args = bench.build_model(model, dev, 2048)
        for n, p in m.named_parameters():
            p.requires_grad = not n.startswith("clip.")
        promote_trainable_params_to_fp32(m)
        eng = TrainEngine(m, torch.bfloat16) if recompute is None else TrainEngine(m, torch.bfloat16, recompute=recompute)
        if moments == "e4m3":
            eng.nn_dgrad = True                                  # what main_finetune --adam8bit does
        params = [p for p in m.parameters() if p.requires_grad]
        res["trainable_params"] = sum(p.numel() for p in params)
        opt = FusedAdamW(params, lr=2e-5, betas=(0.9, 0.95), weight_decay=0.0, engine=eng, moments=moments)
        gen = torch.Generator(device=dev).manual_seed(100)
        image = torch.randn(batch, 3, 336, 336, device=dev, generator=gen)
        tokens = torch.randint(3, args.vocab_size, (batch, 512), device=dev, generator=gen)
        tokens[:, 0] = 1
        labels = tokens.clone()
        labels[:, :256] = 0
        one = bench._train_step_fn(eng, opt, None, params, tokens, labels, image)
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2):
            one()
        torch.cuda.synchronize()
        res.update(fits=True, loss=float(one.loss), recompute=bool(eng.recompute), nn_dgrad=bool(eng.nn_dgrad),
                   moment_state_GB=round(sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items()
                                             if k != "step") / 1e9, 2))
    except torch.cuda.OutOfMemoryError as e:
        res.update(fits=False, error=repr(e)[:200])
    res["max_memory_allocated_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    res["max_memory_allocated_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print("ADAM8_MEMORY " + json.dumps(res), flush=True)


def memory_leg(with_13b):
    """Every configuration in a fresh child process (its own allocator and peak), one after the other."""
    runs = [("7b", "fp32", 8, None, 420), ("7b", "e4m3", 8, None, 420)] + ([("13b", "e4m3", 4, True, 600)] if with_13b else [])
    out = []
    for model, moments, batch, rec, limit in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--memory-child", model, moments, str(batch), {None: "auto", True: "1"}[rec]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            lines = [l for l in r.stdout.splitlines() if l.startswith("ADAM8_MEMORY ")]
            out.append(json.loads(lines[-1][13:]) if lines else {"model": model, "moments": moments, "error": (r.stderr or r.stdout)[-400:]})
        except subprocess.TimeoutExpired:
            out.append({"model": model, "moments": moments, "error": f"no result within {limit} s"})
            break                                               # nothing more on the device after a step that did not come back
        if r.returncode != 0:
            break
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--memory-child":
        model, moments, batch, rec = sys.argv[2:6]
        return memory_child(model, moments, int(batch), None if rec == "auto" else True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-memory", action="store_true", help="the kernel timing only")
    ap.add_argument("--no-13b", action="store_true", help="skip the single 13B attempt")
    ap.add_argument("--out", default=os.path.join("profiles", "adam8_bench.json"))
    ap.add_argument("--rows", type=int, default=22016)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib as L
    lib = L.load()
    n = a.rows * a.cols
    dev = "cuda"
    p32, p8 = torch.randn(n, device=dev), torch.randn(n, device=dev)
    grad = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    mq, rq = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    ms, rs = (torch.full((n // 256,), 1e-30 / 448, device=dev) for _ in range(2))
    img32, img8 = torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
    hp = (1e-5, 0.9, 0.95, 1e-8, 0.02)
    st = torch.cuda.current_stream().cuda_stream

    def fp32(step):
        L.check(lib.a3v_adamw_scaled(p32.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hp, step, img32.data_ptr(), None, st), "a3v_adamw_scaled")

    def e4m3(step):
        L.check(lib.a3v_adamw8_scaled(p8.data_ptr(), grad.data_ptr(), mq.data_ptr(), ms.data_ptr(), rq.data_ptr(), rs.data_ptr(), n, *hp, step,
                                      img8.data_ptr(), None, st), "a3v_adamw8_scaled")
    times = {"fp32": [], "e4m3": []}
    for it in range(a.warmup + a.iters):
        for name, fn in (("fp32", fp32), ("e4m3", e4m3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(it + 1)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)          # us
    res = {"device": torch.cuda.get_device_name(0), "tensor": [a.rows, a.cols], "elements": n, "warmup": a.warmup, "timed_launches": a.iters,
           "method": "device events around each launch, the two kernels alternating"}
    for name, per in (("fp32", BYTES_FP32), ("e4m3", BYTES_E4M3)):
        t = times[name]
        med = statistics.median(t)
        res[name] = {"kernel": "a3v_adamw_scaled" if name == "fp32" else "a3v_adamw8_scaled", "bytes_per_parameter": per,
                     "us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                     "TB_per_s_at_median": round(per * n / med / 1e6, 3)}
    res["time_ratio_e4m3_over_fp32"] = round(res["e4m3"]["us_median"] / res["fp32"]["us_median"], 3)
    res["expected_from_bytes"] = round(BYTES_E4M3 / BYTES_FP32, 3)
    del p32, p8, grad, m, v, mq, rq, ms, rs, img32, img8
    torch.cuda.empty_cache()
    if not a.no_memory:
        res["memory"] = {"derived_moments_GB_7b": {"fp32": 53.9, "e4m3": 13.7}, "runs": memory_leg(not a.no_13b)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
