#!/usr/bin/env python3
"""Batch inference with the reference's ``--quant`` flag (eval_affordance_with_quant.py:300-341): the flow, CLI and record format of
``eval_affordance_v2`` plus ``--quant``, which quantises every decoder linear and the LM head to NF4 after the checkpoint is loaded
(``Transformer.quantize_decode_weights("nf4")``: bitsandbytes nf4 of util/quant.py:95-163, blocksize 64, compressed statistics).
``--quant_format mxfp4`` (with ``--quant``) selects the OCP MXFP4 images instead (``quantize_decode_weights("mxfp4")``); the default
``nf4`` keeps ``--quant`` alone what it was.  ``--quant_prefill`` (MXFP4 only) also runs prefill and decode steps of more than 32
rows on the images (W4A8, ``quantize_decode_weights("mxfp4", prefill=True)``).

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


def check_args(args) -> None:
    """The refusals of this entry point, raised before anything is loaded."""
    if args.quant and args.precision != "bf16":
        raise SystemExit("--quant builds 4-bit images from bf16 weights: use --precision bf16")
    if args.quant_prefill and not (args.quant and args.quant_format == "mxfp4"):
        raise SystemExit("--quant_prefill is an MXFP4 option (the W4A8 GEMM on the images): use it with --quant --quant_format mxfp4")


def main(args):
    check_args(args)
    return _main(args)


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(parents=[get_args_parser()])
    p.add_argument("--quant", action="store_true", default=False, help="4-bit decoder linears and LM head (the reference's 4-bit mode)")
    p.add_argument("--quant_format", choices=["nf4", "mxfp4"], default="nf4",
                   help="with --quant: nf4 (the reference's bitsandbytes format, weight-only) or mxfp4 (OCP MXFP4 on the MI355X scaled MFMA)")
    p.add_argument("--quant_prefill", action="store_true", default=False,
                   help="with --quant --quant_format mxfp4: prefill and decode steps of more than 32 rows run W4A8 on the images "
                        "(quantize_decode_weights('mxfp4', prefill=True)) instead of dequantising every layer; refused with nf4")
    return p


if __name__ == "__main__":
    main(get_parser().parse_args())
