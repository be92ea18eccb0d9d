"""float64 attention oracle with a per-element error bound for the bf16 attention kernels.

``attn_ref`` computes softmax(q k^T / sqrt(hd)) v (right-aligned causal mask as ``ref_cpu.make_causal_mask``, GQA as
``ref_cpu.repeat_kv``), its log-sum-exp and, given dO, its input gradients, all in float64 on the bf16-rounded inputs.  Next to
every output it returns a *scale* tensor from the same float64 intermediates; ``check`` turns it into a bound per element:

    |got - want| <= c * 2^-8 * scale + 2^-8 * |want| + 1e-6

Where the kernels round (and so what the scales are):
  * P = exp(s - lse) is rounded to bf16 before P.V and P^T.dO: a relative error of 2^-9 per term, so
    |dO_err| <= 2^-9 * (P |V|)  and  |dV_err| <= 2^-9 * (P^T |dO|).
  * dS = P (dP - D) is rounded to bf16 before dS.K and dS^T.Q (2^-9 |dS|); D = rowsum(dO * O) is formed from the bf16 output O
    (2^-9 sum_d |dO||O|) and P itself carries 2^-9.  So |dS_err| <= 2^-8 * E with E = P * (|dP - D| + sum_d |dO||O|), and
    |dQ_err| <= 2^-8 * scale * (E |K|),  |dK_err| <= 2^-8 * scale * (E^T |Q|).
  * every output is rounded to bf16 once: the 2^-8 |want| term (one bf16 ulp; a rounding is half of it).
c = 2 leaves a factor of two to four over these first-order sums.  The bound does not grow with S or with the largest entry of a
tensor, unlike a normwise check.  The LSE (fp32 out of fp32 scores) is held to an absolute 2^-8 (``check_lse``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from oracle import ref_cpu

U = 2.0 ** -8          # one bf16 ulp (relative)


def bf(x: torch.Tensor) -> torch.Tensor:
    """bf16 round trip, as float64."""
    return x.detach().cpu().to(torch.bfloat16).double()


def attn_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool,
             do: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """q [B, Sq, H, hd], k / v [B, Sk, Hkv, hd], do [B, Sq, H, hd] (rounded to bf16 here, then float64).

    Returns out [B, Sq, H, hd], lse [B, H, Sq] and out_scale = P |V|; with ``do`` also dq [B, Sq, H, hd], dk / dv [B, Sk, Hkv, hd]
    (summed over the n_rep query heads of each KV head) and dq_scale, dk_scale, dv_scale as in the module docstring."""
    q, k, v = bf(q), bf(k), bf(v)
    B, Sq, H, hd = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    assert H % Hkv == 0 and k.shape == v.shape == (B, Sk, Hkv, hd)
    n_rep = H // Hkv
    scale = 1.0 / math.sqrt(hd)
    mask = ref_cpu.make_causal_mask(Sq, Sk) if causal else None
    r = {"out": torch.empty_like(q), "out_scale": torch.empty_like(q), "lse": torch.empty(B, H, Sq, dtype=torch.float64)}
    if do is not None:
        do = bf(do)
        assert do.shape == q.shape
        r.update(dq=torch.empty_like(q), dq_scale=torch.empty_like(q), dk=torch.empty_like(k), dk_scale=torch.empty_like(k),
                 dv=torch.empty_like(v), dv_scale=torch.empty_like(v))
    for b in range(B):
        for hk in range(Hkv):                   # one KV head and its n_rep query heads at a time (bounded memory)
            hs = slice(hk * n_rep, (hk + 1) * n_rep)
            qq = q[b, :, hs].transpose(0, 1)    # [n_rep, Sq, hd]
            kk, vv = k[b, :, hk], v[b, :, hk]   # [Sk, hd]
            s = torch.matmul(qq, kk.T) * scale
            if mask is not None:
                s = s.masked_fill(~mask, float("-inf"))
            lse = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - lse[..., None])
            o = torch.matmul(p, vv)
            r["out"][b, :, hs] = o.transpose(0, 1)
            r["out_scale"][b, :, hs] = torch.matmul(p, vv.abs()).transpose(0, 1)
            r["lse"][b, hs] = lse
            if do is None:
                continue
            g = do[b, :, hs].transpose(0, 1)    # [n_rep, Sq, hd]
            dp = torch.matmul(g, vv.T)
            Drow = (g * o).sum(-1, keepdim=True)
            ds = p * (dp - Drow)
            r["dq"][b, :, hs] = (torch.matmul(ds, kk) * scale).transpose(0, 1)
            r["dk"][b, :, hk] = torch.matmul(ds.transpose(1, 2), qq).sum(0) * scale
            r["dv"][b, :, hk] = torch.matmul(p.transpose(1, 2), g).sum(0)
            e = p * ((dp - Drow).abs() + (g.abs() * o.abs()).sum(-1, keepdim=True))
            r["dq_scale"][b, :, hs] = (torch.matmul(e, kk.abs()) * scale).transpose(0, 1)
            r["dk_scale"][b, :, hk] = torch.matmul(e.transpose(1, 2), qq.abs()).sum(0) * scale
            r["dv_scale"][b, :, hk] = torch.matmul(p.transpose(1, 2), g.abs()).sum(0)
    return r


def rope_back(x: torch.Tensor, scale: Optional[torch.Tensor] = None, pos0: int = 0):
    """x [B, S, nh, hd] (a gradient w.r.t. RoPE-rotated q or k) -> the gradient w.r.t. the unrotated input: each interleaved
    pair times conj(freqs_cis) (``ref_cpu.precompute_freqs_cis``; the rotation is orthogonal, so its transpose is its backward).
    With ``scale``: also the bound scale of the rotated values, |(s0, s1)| on both members of a pair (a rotation moves an
    error vector of the pair within that radius)."""
    B, S, nh, hd = x.shape
    f = ref_cpu.precompute_freqs_cis(hd, pos0 + S)[pos0:].to(torch.complex128).conj()      # [S, hd/2]
    xc = torch.view_as_complex(x.double().reshape(B, S, nh, hd // 2, 2).contiguous())
    y = torch.view_as_real(xc * f[None, :, None, :]).reshape(B, S, nh, hd)
    if scale is None:
        return y
    s2 = scale.double().reshape(B, S, nh, hd // 2, 2)
    rad = s2.pow(2).sum(-1, keepdim=True).sqrt().expand_as(s2).reshape(B, S, nh, hd)
    return y, rad


_LAYOUT_NAMES = {"bshd": ("b", "row", "h", "col"), "bhs": ("b", "h", "row"), "bhsd": ("b", "h", "row", "col")}


def check(got: torch.Tensor, want: torch.Tensor, scale: torch.Tensor, what: str, c: float = 2.0, rel: float = U,
          layout: str = "bshd") -> float:
    """Assert |got - want| <= c * 2^-8 * scale + rel * |want| + 1e-6 element by element (NaN / inf in ``got`` fail).  On failure
    the message names the first failing element (as (b, h, row, col) of ``layout``), the number of failing elements and the
    largest err / bound.  Returns the largest err / bound."""
    got = got.detach().cpu().double()
    want, scale = want.detach().cpu().double(), scale.detach().cpu().double()
    assert got.shape == want.shape == scale.shape, (what, got.shape, want.shape, scale.shape)
    err = (got - want).abs()
    bound = c * U * scale + rel * want.abs() + 1e-6
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        names = _LAYOUT_NAMES.get(layout, tuple(f"i{j}" for j in range(len(i))))
        at = ", ".join(f"{n}={x}" for n, x in zip(names, i))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements out of bound; first at ({at}): got {float(got[i]):.6g} "
                             f"want {float(want[i]):.6g} bound {float(bound[i]):.3g}; max err/bound {worst:.3g}")
    return worst


def check_lse(got: torch.Tensor, want: torch.Tensor, what: str = "lse") -> float:
    """|got - want| <= 2^-8 absolute, [B, H, Sq]."""
    return check(got, want, torch.ones_like(want, dtype=torch.float64), what, c=1.0, rel=0.0, layout="bhs")
