"""The sampler's three filters restated on the CPU (include/a3vlm_hip.h, a3v_sample_top_k_p), in HF's order: temperature, top-k,
top-p, min-p.

z = one row of fp32 logits (the penalised row when a repetition penalty is on), T > 0, x_i = z_i / T, xm = max x,
e_i = exp(x_i - xm) in fp32.

1. top-k   ``top_k`` = 0 or >= V: off.  t = the k-th largest value of z counting duplicates, K = {i : z_i >= t}: decided on the
           logits themselves, every token tied at t kept (HF's TopKLogitsWarper).  Outside K: mass 0.
2. top-p   the reference's rule (oracle/ref_cpu.py top_p_nucleus, unchanged) on the softmax over K: ranked by probability descending,
           token index ascending; kept iff the mass ranked before the token is <= top_p.
3. min-p   kept iff e_i >= min_p (e_max = 1: p_i >= min_p * p_max under either renormalisation); 0 = off.
4. draw    inverse CDF of the renormalised kept tokens in ranked order at u (ref_cpu.sample_top_p_at's rule).

Inside K both the top-p set and the min-p set are prefixes of the one ranking; the final set is the shorter prefix.  With top-k and
min-p off every function here IS ref_cpu.top_p_nucleus / sample_top_p_at on softmax(z / T)."""
from __future__ import annotations

import torch

from oracle import ref_cpu


def top_k_mask(z: torch.Tensor, top_k: int) -> torch.Tensor:
    """bool [.., V]: K of step 1."""
    V = z.shape[-1]
    if top_k <= 0 or top_k >= V:
        return torch.ones_like(z, dtype=torch.bool)
    t = torch.topk(z, top_k, dim=-1).values[..., -1:]
    return z >= t


def e_values(z: torch.Tensor, T: float) -> torch.Tensor:
    x = z.float() / T
    return torch.exp(x - x.max(dim=-1, keepdim=True).values)


def nucleus(z: torch.Tensor, T: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
    """z fp32 [B, V] -> (ps, idx): the final renormalised probabilities in ranked order (0 for a removed token) and the token ids of
    that order, the shape of ref_cpu.top_p_nucleus's return."""
    assert z.dtype == torch.float32 and z.dim() == 2
    K = top_k_mask(z, top_k)
    probs = torch.softmax(z.masked_fill(~K, float("-inf")) / T, dim=-1)
    ps, idx = ref_cpu.top_p_nucleus(probs, top_p)
    if min_p > 0:
        e = e_values(z, T).gather(-1, idx)
        ps = ps.masked_fill(e < min_p, 0.0)
        ps = ps / ps.sum(dim=-1, keepdim=True)
    return ps, idx


def kept_sets(z: torch.Tensor, T: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
    """Per row the set of token ids a draw can return."""
    ps, idx = nucleus(z, T, top_k, top_p, min_p)
    return [set(i[p > 0].tolist()) for p, i in zip(ps, idx)]


def draw(ps: torch.Tensor, idx: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The inverse CDF of (ps, idx) at u [N] (ps, idx of one row [1, V], or of N rows): the first ranked position whose cumulative
    mass exceeds u, at most the last kept one (ref_cpu.sample_top_p_at's draw)."""
    n_kept = (ps > 0).sum(-1)
    cdf = torch.cumsum(ps.double(), dim=-1)
    pos = (cdf <= u.double().reshape(-1, 1)).sum(-1)
    pos = torch.minimum(pos, n_kept - 1)
    return idx.expand(len(pos), -1).gather(-1, pos.unsqueeze(-1)).squeeze(-1)


def sample_at(z: torch.Tensor, T: float, top_k: int, top_p: float, min_p: float, u: torch.Tensor) -> torch.Tensor:
    """The token the inverse CDF of the final distribution of row b reaches at u[b]."""
    return draw(*nucleus(z, T, top_k, top_p, min_p), u)
