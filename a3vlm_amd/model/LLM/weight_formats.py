"""How ``llama_ens5.Transformer`` holds its decoder weights for inference (``quantize_decode_weights``): the record, the table of what
differs between the formats, and the path policy -- which kernels a product of a given shape runs on.  No tensors are touched at
import time and the policy functions take plain values, so both are checked on the CPU (tests/test_weight_path_policy_cpu.py)."""
from __future__ import annotations

import collections
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch

from ... import lib as _lib
from ... import ops

# one weight image: q = the codes (fp8: e4m3 bytes [N, K]; nf4: nibbles [N, K/2]; mxfp4: e2m1 codes [N, K/2]), s = their scales
# (fp8: fp32 per row [N]; nf4: fp32 per 64-k block [N, K/64]; mxfp4: e8m0 per 32-k block [N, K/32])
WeightImage = collections.namedtuple("WeightImage", "q s")

LAYER_KEYS = ("wqkv", "wo", "w13", "w2")       # the four (packed) matrices of a decoder layer, images keyed f"{key}.{layer}"


@dataclass
class DecodeWeights:
    """What quantize_decode_weights made (``Transformer._weights``; None = the bf16 parameters alone)."""
    fmt: str                               # "fp8" | "nf4" | "mxfp4"
    prefill: bool                          # fp8: W8A8 multi-token forward; mxfp4: W4A8 wherever the GEMV does not run
    images: Dict[str, WeightImage]         # "wqkv.i" "wo.i" "w13.i" "w2.i", and "output" for the 4-bit formats
    version: object = None                 # fp8: the packed-weights version the images were made from (the bf16 weights stay in use)


def _quantize_fp8(w, ws):                  # per-row e4m3 image + fp32 scales by the HIP quantiser (a3v_quantize_rows_fp8)
    q = torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    sc = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
    ops.quantize_rows_fp8(w, q, sc)
    return q, sc


def _check_fp8(m) -> None:
    if m.args.dim % 256 or m.ffn % 256 or (m.n_heads * m.head_dim) % 256 or m._dtype != torch.bfloat16:
        raise ValueError("fp8 decode weights need bf16 parameters and dim, ffn, n_heads*head_dim multiples of 256")


def _check_nf4(m) -> None:
    a = m.args
    if m._dtype != torch.bfloat16 or m._device.type != "cuda":
        raise ValueError("NF4 weights need a bf16 model on the GPU (quantise after .to(device))")
    if a.dim % 256 or m.ffn % 256 or (m.n_heads * m.head_dim) % 256 or a.vocab_size % 4 or a.vocab_size > 65536 or 2 * m.ffn > 65536:
        # the NF4 GEMV (LDS-DMA form only) takes N <= 65536 rows: the LM head and the packed w1|w3 image
        raise ValueError("NF4 weights need dim, ffn, n_heads*head_dim multiples of 256, vocab_size % 4 == 0 and vocab_size, 2*ffn <= 65536")


def _check_mxfp4(m) -> None:
    a = m.args
    HD = m.n_heads * m.head_dim
    if m._dtype != torch.bfloat16:
        raise ValueError(f"MXFP4 weights need a bf16 model, this one is {m._dtype} (fp32 models are refused)")
    if m._device.type != "cuda":
        raise ValueError("MXFP4 weights need the model on the GPU (quantise after .to(device))")
    if a.dim % 128 or m.ffn % 128 or HD % 128:
        raise ValueError(f"MXFP4 weights need dim, ffn and n_heads*head_dim multiples of 128 (got {a.dim}, {m.ffn}, {HD})")
    if a.vocab_size % 16 or (m.n_kv_heads * m.head_dim) % 16 or a.vocab_size > 65536 or 2 * m.ffn > 65536 or max(a.dim, m.ffn) > 16384:
        raise ValueError("MXFP4 weights need vocab_size and n_kv_heads*head_dim multiples of 16, vocab_size, 2*ffn <= 65536 and dim, ffn <= 16384")


@dataclass(frozen=True)
class WeightFormat:
    """What differs between the formats; everything else in llama_ens5.py is written once."""
    name: str                                        # as the messages spell it
    step_code: Optional[int]                         # w8 of the C step entries (a3v_llama_decode_step_form); None: kernel by kernel only
    step_fields: Optional[tuple] = None              # suffixes of an image's (q, s) pointer fields in a3v_llama_layer: wqkv<q> wqkv<s> ...
    check: Optional[Callable] = None                 # (model): the geometry the format needs, raising ValueError
    quantize: Optional[Callable] = None              # (w, ws) -> (q, s)
    quantize_ws_bytes: Optional[Callable] = None     # (N, K) -> bytes of the ws the quantiser is handed (None: it takes none)
    frees_weights: bool = False                      # quantising deletes the bf16 weights (and quantises the LM head too)
    dequantize: Optional[Callable] = None            # (q, s, out [N, K] bf16)
    gemv: Optional[Callable] = None                  # (x, q, s, out, ws, residual=, epilogue=) called from Python on the images
    gemv_ws_bytes: Optional[Callable] = None         # (M, N, K) -> bytes of that GEMV's workspace
    gemv_rows: int = 16                              # rows per GEMV call
    gemv_max_rows: int = 0                           # the most rows that stay on the GEMV (in gemv_rows chunks)


FORMATS: Dict[str, WeightFormat] = {
    "bf16": WeightFormat("bf16", step_code=0),
    # the Python side never runs a GEMV on the fp8 images: the fused C step streams them, every per-kernel path is on the bf16 weights
    "fp8": WeightFormat("fp8", step_code=1, step_fields=("_q", "_s"), check=_check_fp8, quantize=_quantize_fp8),
    "nf4": WeightFormat("NF4", step_code=2, step_fields=("_n4", "_n4s"), check=_check_nf4,
                        quantize=lambda w, ws: ops.quantize_nf4(w, ws=ws)[:2],
                        quantize_ws_bytes=lambda N, K: int(_lib.load().a3v_quantize_nf4_ws_bytes(N, K)), frees_weights=True,
                        dequantize=ops.dequantize_nf4, gemv=ops.gemm_skinny_nf4, gemv_ws_bytes=ops.gemm_skinny_ws_bytes, gemv_max_rows=16),
    "mxfp4": WeightFormat("MXFP4", step_code=None, check=_check_mxfp4, quantize=lambda w, ws: ops.quantize_mxfp4(w), frees_weights=True,
                          dequantize=ops.dequantize_mxfp4, gemv=ops.gemm_skinny_mxfp4, gemv_ws_bytes=ops.gemm_skinny_mxfp4_ws_bytes,
                          gemv_max_rows=32),
}


def layer_path(fmt: str, prefill: bool, rows: int, decode: bool, dim: int, head_dim: int, bf16_stream: bool, ragged: bool = False) -> str:
    """The path of a decoder layer's four products at rows = B*S rows (``decode``: S == 1; ``ragged``: the per-row-position step):
    "bf16" the bf16 weights, "gemv" the GEMV on the images, "dequant" the layer's Wd in the scratch and then the bf16 kernels,
    "w8a8" / "w4a8" the quantised-activation GEMMs on the images."""
    if fmt == "fp8":           # the per-kernel fp8 decode and the ragged per-kernel loop run on the bf16 weights
        return "w8a8" if prefill and rows > 16 and bf16_stream and head_dim in (64, 128) and not ragged else "bf16"
    if fmt == "mxfp4":         # decode rows on the images; anything else W4A8 (opt-in) or weight-only on Wd
        return "gemv" if decode and rows <= FORMATS[fmt].gemv_max_rows else "w4a8" if prefill else "dequant"
    if fmt == "nf4":           # at any S; the SwiGLU form of the NF4 GEMV needs K = dim >= 512 (two K slices)
        return "gemv" if rows <= FORMATS[fmt].gemv_max_rows and dim >= 512 else "dequant"
    return "bf16"


def head_path(fmt: str, prefill: bool, decode: bool, fp32_stream: bool) -> str:
    """The path of the LM head on the last rows of a forward (``decode``: S == 1 and B <= 32): "gemm_nt" plain, "linear" _linear on
    output.weight, "gemv" the 4-bit GEMV in 16-row chunks, "w4a8" / "dequant" as layer_path.  An MXFP4 model runs its head where
    its layers run, so a forward that is weight-only in the layers is weight-only from end to end."""
    if fp32_stream:
        return "gemm_nt"
    if fmt == "mxfp4" and not decode:
        return "w4a8" if prefill else "dequant"
    return "gemv" if fmt in ("nf4", "mxfp4") else "linear"
