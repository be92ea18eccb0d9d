"""TEST INFRASTRUCTURE ONLY: the host restatement of the fp8 KV-cache format (include/a3vlm_hip.h, "fp8 KV cache") -- the per-row
e4m3 quantiser of oracle.quant_fp8 applied to the hd values of one (batch, kv-head, position), and an fp64 decode attention over
dequantised caches.  The product quantises and attends with the HIP kernels of a3v_kv8.hip, never with this file."""
from __future__ import annotations

import math

import torch

from oracle.quant_fp8 import dequantize_rows_fp8, quantize_rows_fp8

NAN_BYTE = 0x7F          # the e4m3fn NaN code (0xFF is the other one)


def quantize_rows(x: torch.Tensor):
    """x [..., hd] -> (uint8 codes [..., hd], fp32 scales [...]): one scale per leading index."""
    q, s = quantize_rows_fp8(x.reshape(-1, x.shape[-1]))
    return q.view(x.shape), s.view(x.shape[:-1])


def dequantize_rows(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return dequantize_rows_fp8(q.reshape(-1, q.shape[-1]), s.reshape(-1)).view(q.shape)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """quantise -> dequantise over the last dimension, in x's dtype."""
    return dequantize_rows(*quantize_rows(x)).to(x.dtype)


def quantize_kv(k: torch.Tensor, v: torch.Tensor):
    """k, v [B, Hkv, S, hd] (position rows) -> k_q [B,Hkv,S,hd], vt_q [B,Hkv,hd,S], k_scale, v_scale [B,Hkv,S] in the cache layouts."""
    kq, ks = quantize_rows(k)
    vq, vs = quantize_rows(v)
    return kq, vq.transpose(2, 3).contiguous(), ks, vs


def e4m3_step(y: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3fn at |y| (y in code units, |y| <= 448): 2^(e-3) with e = floor(log2|y|) >= -6 (subnormals: 2^-9)."""
    e = torch.floor(torch.log2(y.abs().double().clamp_min(2.0 ** -6)))
    return torch.pow(2.0, e - 3)


def half_step_bound(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """|dequantised - x| allowed by round-to-nearest: half the e4m3 spacing at x / scale, times scale (x [..., hd], scale [...]) --
    reached exactly on a tie -- plus the two fp32 roundings on the way (x / scale, then code * scale: 2^-23 of |x| each)."""
    s = scale.double().unsqueeze(-1)
    return 0.5 * e4m3_step(x.double() / s) * s + 2.0 ** -22 * x.abs().double()


def decode_attention_fp64(q, k_q, vt_q, k_scale, v_scale, Sk: int) -> torch.Tensor:
    """q [B, H, hd]; caches in the cache layouts (uint8, any Smax >= Sk); -> fp64 [B, H, hd] over keys 0 .. Sk-1."""
    B, H, hd = q.shape
    Hkv = k_q.shape[1]
    k = k_q[:, :, :Sk].view(torch.float8_e4m3fn).double() * k_scale[:, :, :Sk, None].double()                  # [B,Hkv,Sk,hd]
    v = vt_q[:, :, :, :Sk].view(torch.float8_e4m3fn).double() * v_scale[:, :, None, :Sk].double()              # [B,Hkv,hd,Sk]
    rep = H // Hkv
    k = k.repeat_interleave(rep, dim=1)
    v = v.repeat_interleave(rep, dim=1)
    s = torch.einsum("bhd,bhkd->bhk", q.double(), k) / math.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhk,bhdk->bhd", p, v)
