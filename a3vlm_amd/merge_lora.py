#!/usr/bin/env python3
"""Fold the LoRA adapters of a ``llama_ens5_peft`` checkpoint into its base weights and write a plain ``llama_ens5`` checkpoint.

    python -m a3vlm_amd.merge_lora --pretrained_path BASE_DIR LORA_DIR --output_dir OUT [--quant_base]

The last step of ``main_finetune`` -> checkpoint -> eval for a LoRA run: the folders are loaded in order as ``from_pretrained`` does
(base weights, then the adapter checkpoint), every decoder linear becomes ``W' = W + lora_b . lora_a`` (``MetaModel.merge_lora``:
a3v_lora_merge, fp32 accumulation, one rounding) and OUT gets ``consolidated.00-of-01.model.pth``, the tokenizer, ``config.json`` and
``meta.json`` in the layout ``save_checkpoint`` writes.  ``MetaModel.from_pretrained(OUT)`` then builds a ``llama_ens5`` model
that takes every inference path of the base plugin (single-call decode step, ``quant="nf4"`` / fp8).

``--quant_base``: quantise the base to NF4 first (``quantize_base_weights("nf4")``) and merge over its dequantised values -- the base
a QLoRA run (``main_finetune --quant``) actually trained against.  The output is still a bf16 checkpoint.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os

import torch

from .model.meta import MetaModel


def get_args_parser():
    p = argparse.ArgumentParser("Merge LoRA adapters into the base weights", add_help=False)
    p.add_argument("--pretrained_path", required=True, type=str, nargs="+", help="checkpoint folders, loaded in order; the last one names the tokenizer and config")
    p.add_argument("--output_dir", required=True, type=str)
    p.add_argument("--quant_base", action="store_true", default=False, help="merge over the NF4-dequantised base (a QLoRA run's base)")
    p.add_argument("--llama_config", type=str, default=None, nargs="*", help="default: config.json of the last folder")
    p.add_argument("--tokenizer_path", type=str, default=None, help="default: the tokenizer of the last folder")
    p.add_argument("--no_visual", action="store_true", default=False, help="text-only model (no vision tower in the checkpoint)")
    p.add_argument("--max_seq_len", type=int, default=4096)
    p.add_argument("--precision", type=str, choices=["bf16", "tf32"], default="bf16", help="tf32 = fp32 parity path (not with --quant_base)")
    p.add_argument("--device", default="cuda")
    return p


def write_merged(model: MetaModel, output_dir: str, save_dtype: torch.dtype) -> str:
    """The model file, tokenizer, config.json and meta.json of ``save_checkpoint``, directly in ``output_dir``."""
    os.makedirs(output_dir, exist_ok=True)
    sd = model.state_dict()
    torch.save({"model": {k: v.to(save_dtype) for k, v in sd.items()}}, os.path.join(output_dir, "consolidated.00-of-01.model.pth"))
    model.tokenizer.save(output_dir)
    with open(os.path.join(output_dir, "config.json"), "w") as f:
        json.dump(dataclasses.asdict(model.llma.args), f, indent=2)
    with open(os.path.join(output_dir, "meta.json"), "w") as f:
        json.dump({"llama_type": model.llama_type}, f, indent=2)
    return output_dir


def main(argv=None):
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(argv)
    if args.quant_base and args.precision != "bf16":
        raise SystemExit("--quant_base builds NF4 images from bf16 weights: use --precision bf16")
    dtype = torch.bfloat16 if args.precision == "bf16" else torch.float32
    model = MetaModel.from_pretrained(args.pretrained_path, llama_type="llama_ens5_peft", llama_config=args.llama_config,
                                      tokenizer_path=args.tokenizer_path, with_visual=not args.no_visual, max_seq_len=args.max_seq_len,
                                      dtype=dtype, device=args.device)
    if args.quant_base:
        model.llma.quantize_base_weights("nf4")
    model.merge_lora()
    out = write_merged(model, args.output_dir, dtype)
    print(f"merged {model.llma.n_layers} layers -> {out}")
    return model


if __name__ == "__main__":
    main()
