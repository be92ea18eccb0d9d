"""TEST INFRASTRUCTURE ONLY: the fp8 KV cache on the ragged decode path (a3v_kv8_rows.hip) against the fp64 decode-attention
reference of tests/decode_attn_ref.py.  Pure torch on the CPU; the product runs the HIP kernels, never this file.

What is reused unchanged from decode_attn_ref: ``decode_attention_fp64``, ``bound``, ``kernel_shape`` (form "fp8kv": the walk is
attn_decode_fp8kv_kernel's), ``judge`` and the three input families (``inputs`` at kind "fp8kv").  What is wrapped, because the
functions there branch on ``Case.kind`` and know no fp8 case with per-row key counts or shared prompt keys:
  * ``Kv8Case``: a Case of kind "fp8kv" whose ``shared_len`` follows src / shared whatever the kind, so that ``valid()`` -- and with
    it the dead positions of ``inputs`` (0x7F bytes, inf scales, a sibling's own [0, S_b) included) -- is the shared rows case's;
  * ``inputs``: the inherited generator makes scales that depend on position and kv-head only.  Here the K and V scales of cache
    row b are multiplied by 2^(b mod 3) and 2^((2 b + 1) mod 3): rows differ at the same position, so a kernel that takes the bytes
    of the source row and the scales of its own row computes something else (and, below S_b, reads inf).  Powers of two: the exact
    family stays exact (integer V values times integer scales, sums far below 2^24);
  * ``effective``: byte x scale in the wanted dtype with the gather of include/a3vlm_hip.h "Shared prompt keys" applied to all four
    arrays; ``expected_partials`` is decode_attn_ref's cut at the key ranges on that gather.
``emu`` is a plain fp32 restatement of the rows walk with the mutants of tests/test_kv8_rows_cpu.py.

``rope_kvquant_rows_ref`` restates the quantising write: q and k rotated in fp32, k rounded to bf16, then
tests/kv8_ref.quantize_rows (oracle.quant_fp8) per kv-head on the bf16 k row and the bf16 v row, at position pos[b] of row b."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch

import decode_attn_ref as dar
from decode_attn_ref import BF, F8, F64, NAN, TAIL_K, TAIL_V, Case, bound, decode_attention_fp64, judge, kernel_shape  # noqa: F401
from kv8_ref import quantize_rows

FAMILIES = dar.FAMILIES
MUTANTS = ("own_scales", "boundary_m64", "boundary_p64", "boundary_m1", "boundary_p1", "drop_last", "idle_not_zero", "double_edge")


@dataclass(frozen=True)
class Kv8Case(Case):
    def shared_len(self, b) -> Tuple[int, int]:
        """(source row, S_b) of include/a3vlm_hip.h"""
        if not self.src:
            return b, 0
        s = self.src[b]
        if s < 0 or s >= self.B:
            s = b
        if s == b:
            return b, 0
        return s, max(min(self.shared[b], self.keys()[b]), 0) & ~63


def make_case(tag, H, Hkv, hd, sk, sk_max, plan_fn, src=(), shared=(), pattern="spike") -> Kv8Case:
    """sk per cache row (<= 0: idle; above sk_max: read as sk_max); src / shared: both or neither; the wave plan at (B, H, sk_max)"""
    B = len(sk)
    ns, ch = plan_fn(B, H, sk_max)
    return Kv8Case(id=f"kv8rows-{tag}", group="kv8rows", kind="fp8kv", B=B, H=H, Hkv=Hkv, hd=hd, sk_max=sk_max, sk=tuple(sk), src=tuple(src),
                   shared=tuple(shared), pattern=pattern, nsplit=ns, chunk=ch)


# B 2..4, H 4 / Hkv 2 at hd 64 and H 8 / Hkv 2 at hd 128; the edges 1, 15, 16, 17, 63, 64, 65, 127, 128, 129 over the rows, an
# idle row, a row above sk_max, shared lengths at 0 / 64 / sk & ~63, not a multiple of 64, above sk, src out of range
def cpu_cases(plan_fn):
    mk = lambda *a, **kw: make_case(*a, plan_fn=plan_fn, **kw)
    return [
        mk("a", 4, 2, 64, (129, 65, 0, 300), 200, src=(-1, 0, 0, 0), shared=(0, 64, 64, 128), pattern="spike"),
        mk("b", 8, 2, 128, (128, 127, 17), 128, src=(0, 0, 0), shared=(0, 100, 64), pattern="ramp"),
        mk("c", 4, 2, 64, (1, 15), 64, pattern="offset"),
        mk("d", 8, 2, 128, (16, 63, 64, -3), 64, src=(1, 1, 1, 1), shared=(0, 0, 64, 64), pattern="fall"),
        mk("e", 4, 2, 64, (400, 385, 129), 400, src=(5, 0, 0), shared=(0, 1000, 64), pattern="fall"),
        mk("f", 8, 2, 128, (320, 257, 1, 64), 320, src=(0, 0, 0, 0), shared=(0, 256, 64, 64), pattern="ramp"),
    ]


def inputs(c: Kv8Case, family: str) -> dict:
    """decode_attn_ref.inputs at kind "fp8kv" with scales that differ between cache rows at the same position"""
    inp = dict(dar.inputs(c, family))
    b = torch.arange(c.B)[:, None, None]
    inp["ks"] = inp["ks"] * torch.pow(2.0, (b % 3).float())
    inp["vs"] = inp["vs"] * torch.pow(2.0, ((2 * b + 1) % 3).float())
    return inp


def effective(c: Kv8Case, inp: dict, dtype=F64, shift=0, own_scales=False, tail=None):
    """-> (k, v [B, Hkv, Smax, hd] position rows, cache_row [B]) in ``dtype``: what row b attends over -- bytes AND scales of
    [0, S_b + shift) from row src_row[b] (own_scales: the bytes only).  tail = (k, v): what replaces NaN / inf (None: they stay)."""
    kq, vq = inp["kq"].view(F8).to(dtype).clone(), inp["vtq"].view(F8).to(dtype).transpose(2, 3).contiguous().clone()
    ks, vs = inp["ks"].to(dtype).clone(), inp["vs"].to(dtype).clone()
    src = [t.clone() for t in (kq, vq, ks, vs)]
    for b in range(c.B):
        s, S = c.shared_len(b)
        if s != b and S > 0:
            S = max(S + shift, 0)
            for dst, frm in list(zip((kq, vq, ks, vs), src))[:2 if own_scales else 4]:
                dst[b, :, :S] = frm[s, :, :S]
    k, v = kq * ks.unsqueeze(-1), vq * vs.unsqueeze(-1)
    if tail is not None:
        k = torch.nan_to_num(k, nan=tail[0], posinf=tail[0], neginf=tail[0])
        v = torch.nan_to_num(v, nan=tail[1], posinf=tail[1], neginf=tail[1])
    return k, v, list(range(c.B))


def expected_partials(c: Kv8Case, inp: dict):
    """decode_attn_ref.expected_partials on the gather above: fp64 [B, H, nsplit, hd + 2]"""
    k, v, rows = effective(c, inp)
    k, v = torch.nan_to_num(k, nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    n = torch.tensor(c.keys())
    s = dar._scores(inp["q"].to(F64), k, rows, c.head_map, 1.0 / math.sqrt(c.hd))
    out = torch.zeros(c.B, c.H, c.nsplit, c.hd + 2, dtype=F64)
    j = torch.arange(c.Smax)
    for sp in range(c.nsplit):
        live = ((j[None, :] >= sp * c.chunk) & (j[None, :] < (sp + 1) * c.chunk) & (j[None, :] < n[:, None]))[:, None, :]
        ss = s.masked_fill(~live, -math.inf)
        m = ss.max(2, keepdim=True).values
        p = torch.exp(ss - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(~live, 0.0)
        out[:, :, sp, :c.hd] = dar._pv(p, v, rows, c.head_map)
        out[:, :, sp, c.hd] = m[:, :, 0]
        out[:, :, sp, c.hd + 1] = p.sum(2)
    return out


_REF = {}


def reference(c: Kv8Case, family: str) -> dict:
    """want (fp64), bound, live [B], inp; exact family: expect (bf16), the partial slots of the plan and the rows that write them.
    Computed once per (case, family) and shared."""
    key = (c, family)
    if key not in _REF:
        inp = inputs(c, family)
        k, v, rows = effective(c, inp)
        depth, nfac = kernel_shape(c, "fp8kv")
        aux = dict(depth=depth, nfac=nfac, fp8=True)
        want = decode_attention_fp64(inp["q"], k, v.transpose(2, 3), c.keys(), c.head_map, rows, aux)
        ref = dict(want=want, bound=bound(want, aux), live=aux["live"], inp=inp)
        if family == "exact":
            ref["expect"] = want.float().to(BF)
            ref["partials"] = expected_partials(c, inp).float() if c.nsplit > 1 else None
            ref["written"] = torch.tensor([x > 0 for x in c.keys()])
        _REF[key] = ref
    return _REF[key]


def mutant_applies(c: Kv8Case, mutant: str) -> bool:
    keys = c.keys()
    sib = [c.shared_len(b)[1] for b in range(c.B)]
    if mutant in ("own_scales", "boundary_m64", "boundary_m1"):
        return any(S > 0 for S in sib)
    if mutant == "boundary_p1":                        # the key above the boundary must be a key of the row
        return any(S > 0 and S + 1 <= keys[b] for b, S in enumerate(sib))
    if mutant == "boundary_p64":                       # the 64 keys above the boundary must be keys of the row
        return any(S > 0 and S + 64 <= keys[b] for b, S in enumerate(sib))
    if mutant == "idle_not_zero":
        return any(n <= 0 for n in keys)
    if mutant == "double_edge":
        return c.nsplit > 1 and max(keys) > c.chunk
    return True


def emu(c: Kv8Case, inp: dict, mutant: Optional[str] = None):
    """The rows walk in plain fp32 torch: byte x scale, scores, per key range (max, exp, sum, P V) -> partial slots, the guarded
    combine, one division, the bf16 store, zeros for an idle row.  -> (out bf16 [B, H, hd], partials fp32 [B, H, nsplit, hd + 2])"""
    f32 = torch.float32
    shift = {"boundary_m64": -64, "boundary_p64": 64, "boundary_m1": -1, "boundary_p1": 1}.get(mutant, 0)
    if mutant == "boundary_p64":                       # only where the row has those keys (else the mutant reads no key at all)
        keys = c.keys()
        ok = [c.shared_len(b)[1] > 0 and c.shared_len(b)[1] + 64 <= keys[b] for b in range(c.B)]
        k0, v0, rows = effective(c, inp, f32, tail=(TAIL_K, TAIL_V))
        k1, v1, _ = effective(c, inp, f32, shift=64, tail=(TAIL_K, TAIL_V))
        sel = torch.tensor(ok)[:, None, None, None]
        k, v = torch.where(sel, k1, k0), torch.where(sel, v1, v0)
    else:
        k, v, rows = effective(c, inp, f32, shift=shift, own_scales=mutant == "own_scales", tail=(TAIL_K, TAIL_V))
    ns, ch, hd = c.nsplit, c.chunk, c.hd
    n = torch.tensor(c.keys())
    s = dar._scores(inp["q"].to(f32), k, rows, c.head_map, torch.tensor(1.0 / math.sqrt(hd), dtype=f32))
    j = torch.arange(c.Smax)[None, :]
    part = torch.zeros(c.B, c.H, ns, hd + 2, dtype=f32)
    for sp in range(ns):
        lo, hi = sp * ch, (sp + 1) * ch
        live = (j >= lo) & (j < hi) & (j < n[:, None])
        if mutant == "drop_last":
            live &= j != (n[:, None] - 1)
        if mutant == "double_edge":
            live |= (j == hi) & (j < n[:, None])
        live = live[:, None, :]
        ss = s.masked_fill(~live, -math.inf)
        m = ss.max(2, keepdim=True).values
        empty = torch.isinf(m) & (m < 0)
        p = torch.exp(ss - torch.where(empty, torch.zeros_like(m), m)).masked_fill(~live, 0.0)
        part[:, :, sp, :hd], part[:, :, sp, hd], part[:, :, sp, hd + 1] = dar._pv(p, v, rows, c.head_map), m[:, :, 0], p.sum(2)
    ms = part[..., hd]
    M = ms.max(2, keepdim=True).values
    w = torch.where(torch.isinf(ms) & (ms < 0), torch.zeros_like(ms), torch.exp(ms - M))
    out = (w.unsqueeze(-1) * part[..., :hd]).sum(2) / (w * part[..., hd + 1]).sum(2, keepdim=True)
    idle = (n <= 0)[:, None, None]
    out = torch.where(idle, torch.full_like(out, 1.0 if mutant == "idle_not_zero" else 0.0), out)
    return out.to(BF), part


def rope_kvquant_rows_ref(qkv: torch.Tensor, cos_sin: torch.Tensor, pos, H: int, Hkv: int, hd: int, Smax: int):
    """qkv bf16 [B, (H + 2 Hkv) hd]; cos_sin fp32 [P, hd / 2, 2]; pos per row -> q_out bf16 [B, H hd] and, per running row b, the
    entry (pos[b], k codes [Hkv, hd], k scales [Hkv], v codes [Hkv, hd], v scales [Hkv]) of ``writes[b]`` (None: idle row, whose
    q_out row is zeros)."""
    B = qkv.shape[0]
    x = qkv.float().view(B, H + 2 * Hkv, hd // 2, 2)
    q_out = torch.zeros(B, H * hd, dtype=BF)
    writes = []
    for b in range(B):
        p = int(pos[b])
        if p < 0 or p >= Smax:
            writes.append(None)
            continue
        co, si = cos_sin[p, :, 0], cos_sin[p, :, 1]
        a, bb = x[b, :H + Hkv, :, 0], x[b, :H + Hkv, :, 1]
        rot = torch.stack((a * co - bb * si, a * si + bb * co), -1).reshape(H + Hkv, hd).to(BF)
        q_out[b] = rot[:H].reshape(-1)
        kq, ks = quantize_rows(rot[H:].float())
        vq, vs = quantize_rows(qkv[b].float().view(H + 2 * Hkv, hd)[H + Hkv:])
        writes.append((p, kq, ks, vq, vs))
    return q_out, writes
