#!/usr/bin/env python3
"""Batch inference with the reference's ``--quant`` flag (eval_affordance_with_quant.py:300-341): the flow, CLI and record format of
``eval_affordance_v2`` plus ``--quant``, which quantises every decoder linear and the LM head to NF4 after the checkpoint is loaded
(``Transformer.quantize_decode_weights("nf4")``: bitsandbytes nf4 of util/quant.py:95-163, blocksize 64, compressed statistics).
``--quant_format mxfp4`` (with ``--quant``) selects the OCP MXFP4 images instead (``quantize_decode_weights("mxfp4")``); the default
``nf4`` keeps ``--quant`` alone what it was.

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
        raise SystemExit("--quant builds 4-bit images from bf16 weights: use --precision bf16")
    return _main(args)


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(parents=[get_args_parser()])
    p.add_argument("--quant", action="store_true", default=False, help="4-bit decoder linears and LM head (the reference's 4-bit mode)")
    p.add_argument("--quant_format", choices=["nf4", "mxfp4"], default="nf4",
                   help="with --quant: nf4 (the reference's bitsandbytes format, weight-only) or mxfp4 (OCP MXFP4 on the MI355X scaled MFMA)")
    return p


if __name__ == "__main__":
    main(get_parser().parse_args())
