"""TEST INFRASTRUCTURE ONLY: the host restatement of the fp8 frozen base of the LoRA step -- the per-row e4m3 quantiser
of oracle.quant_fp8, its column-scaled form, and an fp64 decoder step on the dequantised base Wd = Wq * sw that fake-quantises at exactly
the points the engine quantises: the input rows of every base GEMM group in the forward, and the gradient rows (times the row scales of
W) in its input gradient.  Adapters, norms, attention, head and loss are plain fp64 autograd.  The product quantises and multiplies with
the HIP kernels, never with this file."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from oracle import ref_cpu
from oracle.quant_fp8 import dequantize_rows_fp8, quantize_rows_fp8

GROUPS = {"qkv": ("attention.wq", "attention.wk", "attention.wv"), "wo": ("attention.wo",),
          "w13": ("feed_forward.w1", "feed_forward.w3"), "w2": ("feed_forward.w2",)}


def quantize_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [rows, cols] -> (e4m3fn bytes as uint8, fp32 scales [rows]); scale = max|x| / 448, an all-zero row gets 1e-12 / 448."""
    return quantize_rows_fp8(x)


def dequantize_rows(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return dequantize_rows_fp8(q, s)


def byte_values(q: torch.Tensor) -> torch.Tensor:
    """The e4m3 bytes as numbers (fp64)."""
    return q.view(torch.float8_e4m3fn).double()


def quantize_rows_cs(x: torch.Tensor, cs: torch.Tensor, cols_pad: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The column-scaled quantiser: y = fl32(x * cs), quantised per row; cols_pad >= cols bytes per row, zero beyond cols."""
    y = x.float() * cs.float()[None, :]
    q, s = quantize_rows_fp8(y)
    out = torch.zeros(x.shape[0], cols_pad, dtype=torch.uint8)
    out[:, :x.shape[1]] = q
    return out, s


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """quantise -> dequantise over the last dimension (through fp32, as the kernels), back in x's dtype."""
    x2 = x.reshape(-1, x.shape[-1])
    return dequantize_rows_fp8(*quantize_rows_fp8(x2)).to(x.dtype).view(x.shape)


class Fp8BaseLinear(torch.autograd.Function):
    """One base GEMM group: forward deq(quant_rows(x)) . Wd^T; backward dX = deq(quant_rows(dY * sw)) . Wq (bytes as numbers) -- the exact
    gradient with respect to Wd up to the quantisation of dY * sw, straight through the quantisation of x."""

    @staticmethod
    def forward(ctx, x, wq, sw):
        wnum = byte_values(wq)
        ctx.save_for_backward(wnum, sw.double())
        return fake_quant(x) @ (wnum * sw.double()[:, None]).t()

    @staticmethod
    def backward(ctx, dy):
        wnum, sw = ctx.saved_tensors
        return fake_quant(dy * sw) @ wnum, None, None


def base_linear(x: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, quant: bool = True) -> torch.Tensor:
    if quant:
        return Fp8BaseLinear.apply(x, wq, sw)
    return x @ (byte_values(wq) * sw.double()[:, None]).t()


def quantize_state(sd: Dict[str, torch.Tensor], n_layers: int) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """"<kind>.<layer>" -> (Wq, sw) of the fused bf16 base matrices of ``sd`` (rows in GROUPS order)."""
    out = {}
    for i in range(n_layers):
        for kind, names in GROUPS.items():
            w = torch.cat([sd[f"layers.{i}.{nm}.weight"].to(torch.bfloat16) for nm in names], dim=0)
            out[f"{kind}.{i}"] = quantize_rows(w)
    return out


def wd_state(q8: Dict[str, Tuple[torch.Tensor, torch.Tensor]], sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Per-module bf16 Wd = bf16(Wq * sw) of the fused images ``q8``, under the module names and shapes of ``sd``."""
    out = {}
    for key, (wq, sw) in q8.items():
        kind, i = key.split(".")
        wd, row = dequantize_rows(wq, sw).to(torch.bfloat16), 0
        for nm in GROUPS[kind]:
            n = sd[f"layers.{i}.{nm}.weight"].shape[0]
            out[f"layers.{i}.{nm}.weight"] = wd[row:row + n].clone()
            row += n
    return out


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def step_loss(oargs, params: Dict[str, torch.Tensor], q8, examples: torch.Tensor, labels: torch.Tensor, quant: bool = True) -> torch.Tensor:
    """The LoRA step's loss in fp64 (model/meta.py:234-263: shifted labels, CE with ignore_index 0) on the base ``q8`` ("<kind>.<layer>"
    -> (Wq, sw)); ``params``: fp64 embeddings, norms, head and adapters (leaves that want a gradient have requires_grad set)."""
    H = oargs.n_heads
    Hkv = H if oargs.n_kv_heads is None else oargs.n_kv_heads
    hd = oargs.dim // H
    B, T = examples.shape
    fc = ref_cpu.precompute_freqs_cis(hd, oargs.max_seq_len * 2, theta=oargs.rope_theta, scaling=oargs.rope_scaling)[:T].to(torch.complex128)
    mask = torch.ones(T, T, dtype=torch.bool).tril()

    def group(x, kind, i):
        wq, sw = q8[f"{kind}.{i}"]
        y = base_linear(x, wq, sw, quant)
        parts, row = [], 0
        for nm in GROUPS[kind]:
            a, b = params[f"layers.{i}.{nm}.lora_a.weight"], params[f"layers.{i}.{nm}.lora_b.weight"]
            parts.append(y[:, row:row + b.shape[0]] + (x @ a.t()) @ b.t())
            row += b.shape[0]
        return parts

    def rope(t):
        tc = torch.view_as_complex(t.reshape(*t.shape[:-1], -1, 2))
        return torch.view_as_real(tc * fc.view(1, T, 1, -1)).flatten(3)

    h = F.embedding(examples, params["tok_embeddings.weight"]).reshape(B * T, -1)
    for i in range(oargs.n_layers):
        xn = _rms(h, params[f"layers.{i}.attention_norm.weight"], oargs.norm_eps)
        q, k, v = group(xn, "qkv", i)
        q, k, v = q.view(B, T, H, hd), k.view(B, T, Hkv, hd), v.view(B, T, Hkv, hd)
        q, k = rope(q), rope(k)
        k, v = (t.repeat_interleave(H // Hkv, dim=2).transpose(1, 2) for t in (k, v))
        s = (q.transpose(1, 2) @ k.transpose(-1, -2)) / math.sqrt(hd)
        att = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1) @ v
        h = h + group(att.transpose(1, 2).reshape(B * T, H * hd), "wo", i)[0]
        xn2 = _rms(h, params[f"layers.{i}.ffn_norm.weight"], oargs.norm_eps)
        g, u = group(xn2, "w13", i)
        h = h + group(F.silu(g) * u, "w2", i)[0]
    logits = (_rms(h, params["norm.weight"], oargs.norm_eps) @ params["output.weight"].t()).view(B, T, -1)
    return F.cross_entropy(logits[:, :-1].reshape(B * (T - 1), -1), labels[:, 1:].reshape(-1), ignore_index=0)
