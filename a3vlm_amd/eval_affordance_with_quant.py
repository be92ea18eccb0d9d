#!/usr/bin/env python3
"""Batch inference with the reference's ``--quant`` flag (eval_affordance_with_quant.py:300-341): the flow, CLI and record format of
``eval_affordance_v2`` plus ``--quant``, which quantises every decoder linear and the LM head to NF4 after the checkpoint is loaded
(``Transformer.quantize_decode_weights("nf4")``: bitsandbytes nf4 of util/quant.py:95-163, blocksize 64, compressed statistics).

Differences from the reference script, all deliberate:
  * activations are bf16 (``--precision bf16``, the default), as in ``MetaModel.from_pretrained``; the reference's quantised model
    keeps fp32 activations and non-quantised weights (``quantize(model, ...)`` then ``model.cuda()`` without ``.bfloat16()``, :326-337).
    NF4 images are built from bf16 weights here, so ``--quant`` with ``--precision tf32`` is refused;
  * point-cloud inputs and the hard-coded dataset table of the reference script are not part of this entry point: ``--dataset``
    names one JSON file, as for ``eval_affordance_v2``.
"""
from __future__ import annotations

import argparse

from .eval_affordance_v2 import get_args_parser, main as _main


def main(args):
    if args.quant and args.precision != "bf16":
        raise SystemExit("--quant builds NF4 images from bf16 weights: use --precision bf16")
    return _main(args)


if __name__ == "__main__":
    p = argparse.ArgumentParser(parents=[get_args_parser()])
    p.add_argument("--quant", action="store_true", default=False, help="NF4 weight-only decoder linears and LM head (the reference's 4-bit mode)")
    main(p.parse_args())
