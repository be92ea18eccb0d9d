"""CPU restatement of the NF4 weight format of the reference's quantised inference mode
(bitsandbytes ``Linear4bit(quant_type="nf4", compress_statistics=True)``, blocksize 64; reference util/quant.py:95-163).

The format every layer of a3vlm_amd is tested against (include/a3vlm_hip.h, a3v_quantize_nf4):
  * blocks of 64 consecutive elements of the flattened row-major [N, K] matrix (K % 64 == 0), absmax_b = max|w| in fp32;
  * q = argmin_i |w * (1 / absmax_b) - NF4[i]| (fp32 reciprocal, then a product, first minimum on ties); two codes per byte,
    the earlier element in the high nibble; an all-zero block gets code 7 and scale 0;
  * double quantisation: offset = mean(absmax) over the module, absmax - offset quantised in groups of 256 blocks to the
    nearest entry of the signed 8-bit dynamic map with the group's absmax2 = max|absmax - offset|;
  * effective scale s_b = map[qa_b] * absmax2_g + offset (fp32, as dequantize_4bit rebuilds absmax), one per block;
  * Wd = bf16(NF4[q] * s_b).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

NF4 = torch.tensor([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                    -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                    0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
                    0.7229568362236023, 1.0], dtype=torch.float32)

BLOCK = 64          # weights per NF4 block
GROUP = 256         # blocks per double-quantisation group


def dynamic_map() -> torch.Tensor:
    """bitsandbytes create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8): 256 sorted fp32 entries."""
    data = []
    for i in range(7):
        bounds = torch.linspace(0.1, 1, 2 ** i + 1)
        means = (bounds[:-1] + bounds[1:]) / 2.0
        data += ((10 ** (-6 + i)) * means).tolist()
        data += (-(10 ** (-6 + i)) * means).tolist()
    data.append(0)
    data.append(1.0)
    assert len(data) == 256
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


def _nearest(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """argmin_i |x - table[i]| in fp32, first index on ties (torch.argmin), in chunks to bound memory."""
    out = torch.empty(x.shape, dtype=torch.int64)
    xf, of = x.reshape(-1), out.view(-1)
    step = max(1, (1 << 22) // table.numel())
    for a in range(0, xf.numel(), step):
        of[a:a + step] = (xf[a:a + step, None] - table[None, :]).abs().argmin(dim=1)
    return out


def absmax_blocks(w: torch.Tensor) -> torch.Tensor:
    N, K = w.shape
    assert K % BLOCK == 0
    return w.float().reshape(-1, BLOCK).abs().amax(dim=1)


def quantize_codes(w: torch.Tensor, absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """First level: NF4 codes [N, K] (int64, 0..15) from the fp32 block absmax."""
    N, K = w.shape
    am = absmax_blocks(w) if absmax is None else absmax
    x = w.float().reshape(-1, BLOCK)
    rcp = torch.where(am > 0, 1.0 / am, torch.zeros_like(am))     # fp32 division: correctly rounded
    q = _nearest(x * rcp[:, None], NF4)
    q[am == 0] = 7
    return q.reshape(N, K)


def double_quant_scales(absmax: torch.Tensor, offset: Optional[float] = None) -> Tuple[torch.Tensor, float]:
    """Second level: effective fp32 scales s_b (one per block) and the module offset used.  ``offset`` injects the
    offset of another implementation (a reduction: only its rounding may differ)."""
    off = absmax.mean() if offset is None else torch.tensor(offset, dtype=torch.float32)
    d = absmax - off
    nb = d.numel()
    pad = (-nb) % GROUP
    dp = torch.cat([d, torch.zeros(pad)]) if pad else d
    a2 = dp.abs().reshape(-1, GROUP).amax(dim=1)
    rcp = torch.where(a2 > 0, 1.0 / a2, torch.zeros_like(a2))
    x = (dp.reshape(-1, GROUP) * rcp[:, None]).reshape(-1)[:nb]
    dmap = dynamic_map()
    qa = _nearest(x, dmap)
    s = dmap[qa] * a2.repeat_interleave(GROUP)[:nb] + off
    s = torch.where(absmax == 0, torch.zeros_like(s), s)
    return s, float(off)


def pack_nibbles(q: torch.Tensor) -> torch.Tensor:
    """[N, K] codes -> [N, K/2] uint8, the earlier element in the high nibble."""
    q = q.to(torch.uint8)
    return (q[:, 0::2] << 4) | q[:, 1::2]


def unpack_nibbles(b: torch.Tensor) -> torch.Tensor:
    N, H = b.shape
    out = torch.empty(N, 2 * H, dtype=torch.int64)
    out[:, 0::2] = (b >> 4).long()
    out[:, 1::2] = (b & 15).long()
    return out


def quantize(w: torch.Tensor, offset: Optional[float] = None):
    """bf16 [N, K] -> (nibbles [N, K/2] uint8, scales [N, K/64] fp32, offset)."""
    N, K = w.shape
    am = absmax_blocks(w)
    q = quantize_codes(w, am)
    s, off = double_quant_scales(am, offset)
    return pack_nibbles(q), s.reshape(N, K // BLOCK), off


def dequantize(nib: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Wd = bf16(NF4[q] * s_b)."""
    q = unpack_nibbles(nib)
    N, K = q.shape
    return (NF4[q] * scales.float().repeat_interleave(BLOCK, dim=1)).to(torch.bfloat16)


def decoded_f32(nib: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """NF4[q] * s_b in fp32 (the GEMV's arithmetic reference: codes exact, scale applied per block)."""
    q = unpack_nibbles(nib)
    return NF4[q] * scales.float().repeat_interleave(BLOCK, dim=1)


def pack_w13_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """w1 / w3 interleaved in 16-row blocks (the row order of the decode GEMV's SwiGLU epilogue)."""
    nb = a.shape[0] // 16
    return torch.stack([a.reshape(nb, 16, -1), b.reshape(nb, 16, -1)], dim=1).reshape(2 * a.shape[0], -1)
