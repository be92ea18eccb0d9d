"""TEST INFRASTRUCTURE ONLY: the decode-attention family (a3v_attn.hip, a3v_ragged.hip, a3v_kv8.hip, a3v_spec.hip) against ONE fp64
reference.  Pure torch on the CPU; the product attends with the HIP kernels, never with this file.

Entries (``Case.kind`` -> the forms tests/test_gpu_decode_attn_parity.py runs it through):
  uniform  a3v_attention_decode_fused_bf16 (fused combine), a3v_attention at Sq = 1 with A3V_ATTN_DECODE_WAVE_STANDALONE=1 (wave kernel +
           combine kernel), a3v_attention at Sq = 1 (two-phase kernel, its own plan), a3v_attention_decode_rows at sk[b] = Sk
  rows     a3v_attention_decode_rows, a3v_attention_decode_rows_shared with shared = 0
  shared   a3v_attention_decode_rows_shared
  fp8kv    a3v_attention_decode_fp8kv with and without counters
  verify   a3v_attention_verify_rows (Q = 1 also against a3v_attention_decode_rows)

Reference.  ``decode_attention_fp64(q, k, vt, sk_per_query, head_map)``: query r attends to the first sk[r] keys of its cache row, fp64
throughout, zeros for sk <= 0.  The adapters (``effective``) turn every entry into that call: per-row key counts, the shared-prefix
gather (keys below S_b = min(shared, sk) rounded DOWN to 64 from row src_row[b] -- the contract of include/a3vlm_hip.h), byte x scale
dequantised in fp64, the verify rows as B * Q queries over pos[b] + j + 1 keys.  ``expected_partials`` is the same sum cut at the
library's key ranges: per (query, head, range) the (sum p v, m, l) of slot ((r H + h) nsplit + sp) (hd + 2).

Input families.
  exact    q = 0: every score is 0, every p exactly 1, m = 0, l = the key count.  V^T holds small integers: key j of cache row c, kv
           head hk puts w = 1 + (j // 32 + 3 (j // 8) + hk + 2 c) mod 7 into column j mod hd and 0 elsewhere, so a lost, doubled or
           foreign key moves the integer numerator of one column by >= 1 (w differs between neighbouring 8-key vectors, 32- and 64-key
           tiles, heads and rows).  fp8 caches carry the same integers as bytes with power-of-two V scales 2^((5 j + hk) mod 4).  All
           sums are integers below 2^24: partial slots and (num, den) are exact in fp32, the output is bf16(fp32(num / den)).  num / den
           with den <= 1600 lies >= 1 / (511 den) > 2^-20 (relative) from every bf16 rounding boundary unless it IS one (an exact tie,
           which fp32 division reproduces exactly and round-to-nearest-even decides): ``exact_margin`` measures it,
           tests/test_decode_attn_ref_cpu.py asserts it, so a division off by an fp32 ulp cannot flip the stored value.
  bounded  bf16-exact (e4m3-exact x power-of-two scale) N(0, 1) q / K / V.  fp8 scales differ per position by factors up to 2^4 (K)
           and 2^5 (V).
  stress   one of four patterns per case (rotating inside a group; the CPU test checks every group meets every pattern), written
           into dimension 0 of q (a constant 16) and of K (t_j), so that score j moves by 16 t_j / sqrt(hd):
             spike   +100 on one late key (softmax without the max subtraction overflows);
             ramp    +6 per 64-key tile: the maximum grows tile by tile and key range by key range, early weights underflow;
             fall    -100 per key range (per tile where there is one range): the weight of every later range underflows to 0;
             offset  +60 / -60 (by case) on every score.

The bound.  u = 2^-24.  The kernels compute, per (query, head), num_d = sum_j P_j v_jd and l = sum_j P_j with P_j a product of fp32
exponentials whose arguments telescope to s_j - M, then num / l, then the bf16 store.  Against want = sum p v / sum p:
  1. score.  s_j = fl(q . k_j) scale: bf16 x bf16 products are exact in fp32, the hd additions (any order) give
     gamma_hd sum_e |q_e k_je| scale, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 8.4 / eq. 3.4); the multiplication
     by scale and scale's own rounding (1 / sqrt(128)) 2 u |s_j| (fp8: two more factors, 4 u |s_j|).  An error ds_j multiplies P_j by e^ds.
  2. exponentials.  __expf(x) = v_exp_f32(x log2 e): the instruction is good to 1 ulp = 2 u relative (CDNA ISA guide, v_exp_f32; the
     convention of tests/genctl_ref.py), the product x log2 e, the rounded constant and the fp32 subtraction that formed x each move
     the argument by u |x|: 3 u |x| relative.  Every argument is <= 0 and they sum to s_j - M, so together 3 u d_j, d_j = M - s_j.
     Each of the nfac factors (own exponential, one rescale per further tile of the wave, the wave merge, the split combine) adds
     2 u and the multiplication by it u: 3 u nfac.
  3. sums.  fp32 accumulation in the kernel's tree: ``depth`` additions on the longest path (the 8 / 16 fma of a vector, one per tile
     of the wave, the lane butterfly, 8 waves, nsplit ranges): gamma_depth, relative to sum_j P_j |v_jd| (l: to l).  fp8: p v_scale
     rounds once more, u.
     rel_j = ds_j + 3 u d_j + 3 u nfac + gamma_depth (+ u); e_num_d = sum_j p_j rel_j |v_jd| / l, e_l = sum_j p_j rel_j / l.
  4. division: u |want|.  e32 = 1.01 (e_num + |want| e_l) + u |want| + n 2^-126 max|v| (second-order products; flushed terms).
  5. bf16 store: half an ulp of the stored value, 2^(floor(log2(|want| + e32)) - 8).   bound = e32 + half ulp; fp32 outputs: e32.
Nothing is fitted: every constant is one of the above.  The fp32 part scales with sum_j p_j |v_j|, there is no flat atol.

``emu`` is a plain fp32 restatement of the split walk (per-range partials, combine, bf16 store) with the mutations of
tests/test_decode_attn_ref_cpu.py; ``judge`` is the one verdict both the CPU and the GPU test use."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Callable, Dict, List, Optional, Tuple

import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
F64 = torch.float64
U = 2.0 ** -24
NAN = float("nan")
NAN_BYTE = 0x7F
SENT = -7.0
FAMILIES = ("exact", "bounded", "stress")
PATTERNS = ("spike", "ramp", "fall", "offset")
TAIL_K, TAIL_V = 0.5, 3.0          # what ``emu`` sees where the caches hold NaN (a mutant that reads there gets a finite value)

SK_EDGES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1023, 1024, 1025)


def gamma(n):
    return n * U / (1.0 - n * U)


def up(x, m):
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class Case:
    id: str
    group: str
    kind: str                       # uniform | rows | shared | fp8kv | verify
    B: int
    H: int
    Hkv: int
    hd: int
    sk_max: int
    sk: Tuple[int, ...] = ()        # per cache row (uniform / fp8kv: sk_max for every row)
    src: Tuple[int, ...] = ()
    shared: Tuple[int, ...] = ()
    Q: int = 1
    pos: Tuple[int, ...] = ()
    nq: Tuple[int, ...] = ()
    pattern: str = "spike"
    nsplit: int = 0                 # wave plan at (B, H, sk_max)
    chunk: int = 0
    nsplit2: int = 0                # two-phase plan
    chunk2: int = 0

    @property
    def R(self):
        return self.B * self.Q

    @property
    def Smax(self):
        return up(self.sk_max + 1, 64) + 64

    @property
    def head_map(self):
        g = self.H // self.Hkv
        return tuple(h // g for h in range(self.H))

    def keys(self) -> List[int]:
        """keys of every query (R of them)"""
        if self.kind == "verify":
            out = []
            for b in range(self.B):
                for j in range(self.Q):
                    live = self.pos[b] >= 0 and j < self.nq[b] and self.pos[b] + j < self.sk_max
                    out.append(self.pos[b] + j + 1 if live else 0)
            return out
        return [min(max(s, 0), self.sk_max) for s in self.sk]

    def shared_len(self, b) -> Tuple[int, int]:
        """(source row, S_b) of include/a3vlm_hip.h"""
        if self.kind != "shared":
            return b, 0
        s = self.src[b]
        if s < 0 or s >= self.B:
            s = b
        if s == b:
            return b, 0
        return s, max(min(self.shared[b], self.keys()[b]), 0) & ~63

    def valid(self) -> torch.Tensor:
        """bool [B, Smax]: the cache positions a correct kernel may read; everything else holds NaN (0x7F, inf scales)"""
        v = torch.zeros(self.B, self.Smax, dtype=torch.bool)
        if self.kind == "verify":
            keys = self.keys()
            for b in range(self.B):
                v[b, :max(keys[b * self.Q:(b + 1) * self.Q])] = True
            return v
        keys = self.keys()
        for b in range(self.B):
            s, S = self.shared_len(b)
            v[b, S:keys[b]] = True
            v[s, :S] = True
        return v


# ----------------------------------------------------------------------------------------------------------------- the case table
def _c(group, kind, tag, B, H, Hkv, hd, sk_max, **kw):
    return Case(id=f"{group}-{kind}-{tag}-b{B}h{H}k{Hkv}d{hd}", group=group, kind=kind, B=B, H=H, Hkv=Hkv, hd=hd, sk_max=sk_max, **kw)


def _uniform(group, kind, B, H, Hkv, hd, Sk):
    return _c(group, kind, f"sk{Sk}", B, H, Hkv, hd, Sk, sk=(Sk,) * B)


# geometry per B*H: (B, H, Hkv, hd), alternatives cover hd 64 / 128 and H / Hkv in {1, 4, 8}
SMALL = ((2, 4, 4, 64), (1, 8, 2, 128))                 # B*H = 8: one key range up to 128 keys (the plan's 128-key floor)
ONE_RANGE = ((32, 8, 1, 128), (64, 4, 1, 64))           # B*H = 256: the wave plan gives one key range at any Sk
HALF = ((16, 8, 1, 128), (32, 4, 4, 64))                # B*H = 128: Sk > 1024 gives two ranges of 576: a wave's second tile
RANGE_GEOM = {2: (1, 2, 1, 64), 8: (1, 8, 8, 128), 96: (12, 8, 2, 64)}
FP8_SK = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129, 513, 577, 1025)


def _spec_table():
    """entries that do not need the plan as Case, the others as ("range", ...) / ("rows", ...) tuples expanded by ``cases_for``"""
    T = []
    for i, Sk in enumerate(SK_EDGES):
        # Sk <= 128: one range at any B*H.  129..577: B*H = 256 (within the size limits: Sk <= 640 there).  1023..1025: one range
        # needs B*H >= 256, which the limits forbid at that length; B*H = 128 gives two ranges and, above 1024, chunks of 576 keys.
        geoms = SMALL if Sk <= 128 else ONE_RANGE if Sk <= 577 else HALF
        for g in geoms:
            T.append(_uniform("sk_edges", "uniform", *g, Sk))
    for bh in (2, 8, 96):
        for target in ("2", "3", "8", ">8"):
            T.append(("range", bh, target))
    T.append(_uniform("thresholds", "uniform", 255, 1, 1, 64, 300))
    T.append(_uniform("thresholds", "uniform", 32, 8, 2, 128, 300))
    T.append(_uniform("thresholds", "uniform", 257, 1, 1, 64, 300))
    T.append(_uniform("thresholds", "uniform", 24, 8, 1, 128, 600))
    T.append(_uniform("thresholds", "uniform", 34, 8, 4, 64, 600))
    T.append(("rows", 8, 8, 128, 100))        # one range
    T.append(("rows", 8, 2, 64, 700))         # B*H = 88: three ranges
    T.append(("rows", 2, 2, 128, 1024))       # B*H = 22: eight
    T.append(("rows", 2, 1, 64, 1600))        # nine
    T.append(("rows_below", 4, 1, 128, 300))  # sk_max above every row
    T.append(("shared", 4, 2, 64, 300))
    T.append(("shared", 2, 1, 128, 520))
    T.append(("shared", 8, 2, 128, 300))
    T.append(("shared", 4, 4, 64, 520))
    for i, Sk in enumerate(FP8_SK):
        g = SMALL[i % 2] if Sk <= 128 else ONE_RANGE[i % 2] if Sk <= 577 else HALF[i % 2]
        T.append(_uniform("fp8kv", "fp8kv", *g, Sk))
    T.append(("fp8range", 1, 8, 8, 128))
    T.append(("fp8range", 2, 4, 1, 64))
    for Q in (1, 2, 3, 4, 5, 8):
        T.append(("verify", Q, 4, 1, 64, 300))
        T.append(("verify", Q, 4, 4, 128, 300))
    T.append(("verify", 3, 8, 2, 128, 100))
    T.append(("verify", 8, 8, 2, 64, 100))
    T.append(("verify", 5, 2, 1, 128, 1200))
    T.append(("verify", 8, 2, 2, 64, 1200))
    return T


TABLE = _spec_table()


def _range_edge_sks(plan_fn, B, H, target):
    """Sk values whose plan has the target number of ranges and whose LAST range holds exactly one key, chunk - 1 keys and chunk keys
    (Sk = (ns - 1) chunk + 1, ns chunk - 1, ns chunk): the first of each kind in 129 .. 1600"""
    ok = {"2": lambda n: n == 2, "3": lambda n: n == 3, "8": lambda n: n == 8, ">8": lambda n: n > 8}[target]
    found: Dict[str, int] = {}
    for Sk in range(129, 1601):
        ns, ch = plan_fn(B, H, Sk, True)
        if not ok(ns):
            continue
        last = Sk - (ns - 1) * ch
        kind = "one" if last == 1 else "full" if last == ch else "fullm1" if last == ch - 1 else None
        if kind and kind not in found:
            found[kind] = Sk
    return [found[k] for k in ("one", "fullm1", "full") if k in found]


def _rows_case(plan_fn, H, Hkv, hd, sk_max, below=False):
    if below:
        sk = (5, 64, 65, 0, 129, 40)
        return _c("rows", "rows", f"below{sk_max}", len(sk), H, Hkv, hd, sk_max, sk=sk)
    B = 12
    ns, ch = plan_fn(B, H, sk_max, True)
    want = [sk_max, 1, 0, -1, 40, ch - 1, ch, ch + 1, (ns - 1) * ch - 1, (ns - 1) * ch, (ns - 1) * ch + 1, sk_max + 5]
    sk = tuple(s if s <= sk_max or s == sk_max + 5 else max(sk_max - 1 - i, 1) for i, s in enumerate(want))
    return _c("rows", "rows", f"max{sk_max}", B, H, Hkv, hd, sk_max, sk=sk)


def _shared_case(plan_fn, H, Hkv, hd, sk_max):
    """rows 0..4: idle leaders, valid on [0, S) only, one per distinct S; row 5: a live leader; then the followers"""
    vals = [0, 1, 63, 64, 65, "c-1", "c", "c+1", "sk"]
    B = 6 + len(vals) + 3
    ns, ch = plan_fn(B, H, sk_max, True)
    sk, src, sh = [0, 0, 0, 0, 0, sk_max], [0, 1, 2, 3, 4, 5], [0, 0, 0, 0, 0, 0]
    leader_of: Dict[int, int] = {}
    for i, v in enumerate(vals):
        skb = sk_max - 3 - 7 * i if i % 2 else ch + 70 + i
        skb = min(max(skb, 66), sk_max)
        s = {"c-1": ch - 1, "c": ch, "c+1": ch + 1, "sk": skb}.get(v, v)
        S = min(s, skb) & ~63
        if S not in leader_of:
            leader_of[S] = len(leader_of)
        sk.append(skb); src.append(leader_of[S]); sh.append(s)
    sk += [sk_max - 1, 200, 131]
    src += [len(sk) - 3, -1, 5]           # its own row (plain), outside [0, B) (plain), the live leader
    sh += [64, 64, 128]
    assert len(leader_of) <= 5 and len(sk) == B
    return _c("shared", "shared", f"max{sk_max}", B, H, Hkv, hd, sk_max, sk=tuple(sk), src=tuple(src), shared=tuple(sh))


def _verify_case(plan_fn, Q, H, Hkv, hd, sk_max):
    B = 7
    ns, ch = plan_fn(B, H, sk_max, True)
    half = (Q + 1) // 2
    edge = min(ch, sk_max - Q)                      # the first key-range edge (one range: the end of the keys)
    pos = (32 - half, 64 - half, edge - half, -1, min(edge + 5, sk_max - Q), sk_max - Q, 9)
    nq = (Q, Q, Q, Q, max(Q - 1, 1), Q, 0)
    return _c("verify", "verify", f"q{Q}max{sk_max}", B, H, Hkv, hd, sk_max, Q=Q, pos=pos, nq=nq)


def cases_for(plan_fn: Callable[[int, int, int, bool], Tuple[int, int]]) -> List[Case]:
    """TABLE with every key count placed from the library's plan (plan_fn(B, H, Sk, wave) -> (nsplit, chunk))"""
    out: List[Case] = []
    for t in TABLE:
        if isinstance(t, Case):
            out.append(t)
        elif t[0] == "range":
            B, H, Hkv, hd = RANGE_GEOM[t[1]]
            out += [_uniform("range_edges", "uniform", B, H, Hkv, hd, Sk) for Sk in _range_edge_sks(plan_fn, B, H, t[2])]
        elif t[0] == "fp8range":
            out += [_uniform("fp8kv", "fp8kv", *t[1:], Sk) for Sk in _range_edge_sks(plan_fn, t[1], t[2], "3")]
        elif t[0] in ("rows", "rows_below"):
            out.append(_rows_case(plan_fn, *t[1:], below=t[0] == "rows_below"))
        elif t[0] == "shared":
            out.append(_shared_case(plan_fn, *t[1:]))
        elif t[0] == "verify":
            out.append(_verify_case(plan_fn, *t[1:]))
    done, seen = [], {}
    for c in out:
        i = seen.setdefault(c.group, 0)
        seen[c.group] += 1
        ns, ch = plan_fn(c.B, c.H, c.sk_max, True)
        ns2, ch2 = plan_fn(c.B, c.H, c.sk_max, False)
        done.append(replace(c, pattern=PATTERNS[i % 4], nsplit=ns, chunk=ch, nsplit2=ns2, chunk2=ch2))
    assert len({c.id for c in done}) == len(done)
    return done


def verify_group(hd, Q):
    cap = 4 if hd == 128 else 8
    g = 1
    while g < Q and g < cap:
        g *= 2
    return g


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _rb(t):
    return t.to(BF).float()


def _seed(c, family):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id + family)) % (2 ** 31)


def _exact_w(c):
    """[B, Hkv, Smax] integer weights of the exact family"""
    j = torch.arange(c.Smax)
    b = torch.arange(c.B)[:, None, None]
    hk = torch.arange(c.Hkv)[None, :, None]
    return (1 + (j // 32 + 3 * (j // 8) + hk + 2 * b) % 7).float()


def _pattern_t(c, valid):
    """[B, Smax] the wanted move of score j in units of the softmax argument"""
    j = torch.arange(c.Smax).float()
    t = torch.zeros(c.B, c.Smax)
    if c.pattern == "spike":
        last = (valid.float() * j).max(1).values
        for b in range(c.B):
            t[b, int(max(last[b] - 2, 0))] = 100.0
    elif c.pattern == "ramp":
        t[:] = 6.0 * (j // 64)
    elif c.pattern == "fall":
        unit = c.chunk if c.nsplit > 1 else 64
        t[:] = -100.0 * (j // unit)
    else:
        t[:] = 60.0 if (len(c.id) % 2) else -60.0
    return t


def inputs(c: Case, family: str) -> dict:
    """-> q [R, H, hd] fp32 (bf16-exact); bf16 kinds: k [B, Hkv, Smax, hd], vt [B, Hkv, hd, Smax] fp32 (bf16-exact, NaN where not
    valid); fp8kv: kq / vtq uint8 (0x7F where not valid), ks / vs fp32 [B, Hkv, Smax] (inf where not valid)"""
    g = torch.Generator().manual_seed(_seed(c, family))
    B, H, Hkv, hd, S, R = c.B, c.H, c.Hkv, c.hd, c.Smax, c.R
    valid = c.valid()
    fp8 = c.kind == "fp8kv"
    j = torch.arange(S)
    hk = torch.arange(Hkv)[None, :, None]
    if fp8:
        ks = torch.pow(2.0, ((7 * j + hk) % 5 - 3).float()).expand(B, Hkv, S).clone()
        vs = torch.pow(2.0, ((3 * j + 1 + hk) % 6 - 3).float()).expand(B, Hkv, S).clone()
    q = _rb(torch.randn(R, H, hd, generator=g))
    k = torch.randn(B, Hkv, S, hd, generator=g)
    v = torch.randn(B, Hkv, S, hd, generator=g)
    if family == "exact":
        q.zero_()
        w = _exact_w(c)
        v = torch.zeros(B, Hkv, S, hd)
        v.scatter_(3, (j % hd).view(1, 1, S, 1).expand(B, Hkv, S, 1), w.unsqueeze(-1))
        if fp8:
            vs = torch.pow(2.0, ((5 * j + hk) % 4).float()).expand(B, Hkv, S).clone()
    elif family == "stress":
        q[:, :, 0] = 16.0
        t = _pattern_t(c, valid) * math.sqrt(hd) / 16.0
        k[:, :, :, 0] = t[:, None, :]
    if fp8:
        kq = (k / ks.unsqueeze(-1)).clamp(-448, 448).to(F8)
        vq = (v if family == "exact" else v / vs.unsqueeze(-1)).clamp(-448, 448).to(F8)
        kq, vq = kq.view(torch.uint8).clone(), vq.view(torch.uint8).transpose(2, 3).contiguous()
        dead = ~valid[:, None, :].expand(B, Hkv, S)
        kq[dead] = NAN_BYTE
        vq.transpose(2, 3)[dead] = NAN_BYTE
        ks[dead] = float("inf")
        vs[dead] = float("inf")
        return dict(q=q, kq=kq, vtq=vq, ks=ks, vs=vs)
    k, v = _rb(k), _rb(v)
    dead = ~valid[:, None, :].expand(B, Hkv, S)
    k[dead] = NAN
    v[dead] = NAN
    return dict(q=q, k=k, vt=v.transpose(2, 3).contiguous())


def effective(c: Case, inp: dict, dtype=F64, shift=0, scale_shift=0, tail=None):
    """-> (k [Bc, Hkv, Smax, hd], v [Bc, Hkv, Smax, hd] (position rows), cache_row [R]) in ``dtype``: what query r attends over.
    shared: the gather of include/a3vlm_hip.h with the boundary moved by ``shift`` keys (0: the contract).  fp8kv: byte x scale,
    the scale taken from position j + scale_shift.  tail = (k value, v value): what replaces NaN (None: NaN stays)."""
    if c.kind == "fp8kv":
        ks, vs = inp["ks"], inp["vs"]
        if scale_shift:
            ks, vs = torch.roll(ks, -scale_shift, 2), torch.roll(vs, -scale_shift, 2)
        k = inp["kq"].view(F8).to(dtype) * ks.to(dtype).unsqueeze(-1)
        v = inp["vtq"].view(F8).to(dtype).transpose(2, 3) * vs.to(dtype).unsqueeze(-1)
    else:
        k, v = inp["k"].to(dtype), inp["vt"].to(dtype).transpose(2, 3)
    if tail is not None:
        k = torch.nan_to_num(k, nan=tail[0], posinf=tail[0], neginf=tail[0])
        v = torch.nan_to_num(v, nan=tail[1], posinf=tail[1], neginf=tail[1])
    if c.kind == "shared":
        k, v = k.clone(), v.contiguous().clone()
        k0, v0 = k.clone(), v.clone()
        for b in range(c.B):
            s, S = c.shared_len(b)
            if s != b and S > 0:
                S = max(S + shift, 0)
                k[b, :, :S] = k0[s, :, :S]
                v[b, :, :S] = v0[s, :, :S]
    rows = [r // c.Q for r in range(c.R)]
    return k, v, rows


def _scores(q, k, rows, head_map, scale):
    """[R, H, S]"""
    R, H, _ = q.shape
    s = torch.empty(R, H, k.shape[2], dtype=q.dtype)
    kr = k[rows] if list(rows) != list(range(k.shape[0])) else k
    for hk in sorted(set(head_map)):
        hs = [h for h in range(H) if head_map[h] == hk]
        s[:, hs] = torch.einsum("rgd,rsd->rgs", q[:, hs], kr[:, hk])
    return s * scale


def _pv(p, v, rows, head_map):
    """p [R, H, S], v [Bc, Hkv, S, hd] -> [R, H, hd]"""
    R, H, _ = p.shape
    o = torch.empty(R, H, v.shape[3], dtype=p.dtype)
    vr = v[rows] if list(rows) != list(range(v.shape[0])) else v
    for hk in sorted(set(head_map)):
        hs = [h for h in range(H) if head_map[h] == hk]
        o[:, hs] = torch.einsum("rgs,rsd->rgd", p[:, hs], vr[:, hk])
    return o


def decode_attention_fp64(q, k, vt, sk_per_query, head_map, cache_row=None, aux=None):
    """q [R, H, hd]; k [Bc, Hkv, S, hd], vt [Bc, Hkv, hd, S]; query r attends to keys [0, sk[r]) of cache row cache_row[r] (default r)
    through kv head head_map[h] -> fp64 [R, H, hd], zeros where sk <= 0.  ``aux`` (a dict): filled with what ``bound`` needs."""
    R, H, hd = q.shape
    rows = list(range(R)) if cache_row is None else list(cache_row)
    q, k, v = q.to(F64), k.to(F64), vt.to(F64).transpose(2, 3)
    S = k.shape[2]
    n = torch.tensor([max(int(x), 0) for x in sk_per_query])
    live = (torch.arange(S)[None, :] < n[:, None])[:, None, :]                   # [R, 1, S]
    k, v = torch.nan_to_num(k, nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    scale = 1.0 / math.sqrt(hd)
    s = _scores(q, k, rows, head_map, scale).masked_fill(~live, -math.inf)
    m = s.max(2, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m).masked_fill(~live, 0.0)
    l = p.sum(2, keepdim=True)
    out = _pv(p, v, rows, head_map) / l.clamp_min(1e-300)
    out = torch.where((n > 0)[:, None, None], out, torch.zeros_like(out))
    if aux is not None:
        lsafe = l.clamp_min(1e-300)
        fp8 = aux.get("fp8", False)
        sabs = _scores(q.abs(), k.abs(), rows, head_map, scale)
        ds = gamma(hd) * sabs + (4 if fp8 else 2) * U * s.abs().masked_fill(~live, 0.0)
        d = (m - s).masked_fill(~live, 0.0)
        rel = ds + 3 * U * d + 3 * U * aux["nfac"] + gamma(aux["depth"]) + (U if fp8 else 0.0)
        pr = p * rel
        aux["e_num"] = _pv(pr, v.abs(), rows, head_map) / lsafe
        aux["e_l"] = pr.sum(2, keepdim=True) / lsafe
        aux["flush"] = n.max().item() * 2.0 ** -126 * float(v.abs().max())
        aux["live"] = n > 0
    return out


def kernel_shape(c: Case, form: str):
    """(depth, nfac) of step 2 / 3 of the bound for a form: wave (fused, stand-alone, rows, shared), fp8kv, verify, twophase, generic"""
    if form == "twophase":
        ns, ch = c.nsplit2, c.chunk2
        return max(-(-ch // 256) + 6 + 4, 8 * -(-ch // 512) + 6) + ns, 2
    ns, ch = c.nsplit, c.chunk
    if form == "generic":
        return c.sk_max + -(-c.sk_max // 64), -(-c.sk_max // 64) + 1
    if form == "fp8kv":
        T = -(-ch // 512)
        return 16 + T + 2 + 8 + ns, T + 3
    if form == "verify":
        T = -(-ch // 256)
        return 8 + T + 2 + 8 + ns, T + 3
    T = -(-ch // 512)
    return 8 + T + 3 + 8 + ns, T + 3


def form_of(c: Case):
    return {"fp8kv": "fp8kv", "verify": "verify"}.get(c.kind, "wave")


def bound(want: torch.Tensor, aux: dict, bf16: bool = True) -> torch.Tensor:
    """the docstring's bound, elementwise [R, H, hd]"""
    w = want.abs()
    e32 = 1.01 * (aux["e_num"] + w * aux["e_l"]) + U * w + aux["flush"]
    if not bf16:
        return e32
    mag = (w + e32).clamp_min(2.0 ** -126)
    return e32 + torch.pow(2.0, torch.floor(torch.log2(mag)) - 8)


def old_flat_bound(want):
    """what every decode-attention test used before: 4e-3 + 2^-7 |want|"""
    return 4e-3 + 2.0 ** -7 * want.abs()


def expected_partials(c: Case, inp: dict, nsplit: int, chunk: int):
    """fp64 [R, H, nsplit, hd + 2]: (sum p v, m, l) per key range with p = exp(s - m_range); an empty range: (0, -inf, 0)"""
    k, v, rows = effective(c, inp)
    k, v = torch.nan_to_num(k, nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    q = inp["q"].to(F64)
    n = torch.tensor(c.keys())
    s = _scores(q, k, rows, c.head_map, 1.0 / math.sqrt(c.hd))
    out = torch.zeros(c.R, c.H, nsplit, c.hd + 2, dtype=F64)
    j = torch.arange(c.Smax)
    for sp in range(nsplit):
        live = ((j[None, :] >= sp * chunk) & (j[None, :] < (sp + 1) * chunk) & (j[None, :] < n[:, None]))[:, None, :]
        ss = s.masked_fill(~live, -math.inf)
        m = ss.max(2, keepdim=True).values
        p = torch.exp(ss - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(~live, 0.0)
        out[:, :, sp, :c.hd] = _pv(p, v, rows, c.head_map)
        out[:, :, sp, c.hd] = m[:, :, 0]
        out[:, :, sp, c.hd + 1] = p.sum(2)
    return out


def partial_rows_written(c: Case) -> torch.Tensor:
    """bool [R]: the queries whose partial slots the kernel writes (an idle row, or a verify group with no live query, leaves before)"""
    keys = c.keys()
    if c.kind != "verify":
        return torch.tensor([x > 0 for x in keys])
    G = verify_group(c.hd, c.Q)
    out = []
    for b in range(c.B):
        for j in range(c.Q):
            g0 = j // G * G
            out.append(max(keys[b * c.Q + g0:b * c.Q + min(g0 + G, c.Q)]) > 0)
    return torch.tensor(out)


@lru_cache(maxsize=8)
def _reference_cached(c: Case, family: str, form: str):
    inp = inputs(c, family)
    k, v, rows = effective(c, inp)
    depth, nfac = kernel_shape(c, form)
    aux = dict(depth=depth, nfac=nfac, fp8=c.kind == "fp8kv")
    want = decode_attention_fp64(inp["q"], k, v.transpose(2, 3), c.keys(), c.head_map, rows, aux)
    ref = dict(want=want, bound=bound(want, aux), live=aux["live"], inp=inp)
    if family == "exact":
        ref["expect"] = want.float().to(BF)            # num / den: exact operands, one fp32 division, one bf16 rounding
        ns, ch = (c.nsplit2, c.chunk2) if form == "twophase" else (c.nsplit, c.chunk)
        ref["partials"] = expected_partials(c, inp, ns, ch).float() if ns > 1 else None
        ref["written"] = partial_rows_written(c)
    return ref


def reference(c: Case, family: str, form: Optional[str] = None) -> dict:
    """want (fp64), bound, live [R], inp; exact family: expect (bf16) and the partial slots of the form's plan"""
    return _reference_cached(c, family, form or form_of(c))


def exact_quotients(c: Case, inp: dict):
    """(num, den) fp64 [R, H, hd], [R, 1, 1] of the exact family's live queries"""
    k, v, rows = effective(c, inp)
    v = torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    n = torch.tensor(c.keys())
    live = (torch.arange(c.Smax)[None, :] < n[:, None])[:, None, :].to(F64).expand(c.R, c.H, c.Smax)
    return _pv(live.contiguous(), v, rows, c.head_map), n.to(F64)[:, None, None]


def exact_margin(num, den):
    """smallest relative distance of a quotient to a bf16 rounding boundary (ties and exactly representable values excluded) and
    whether any quotient is an exact tie"""
    ok = (den > 0) & (num > 0)
    x = (num / den.clamp_min(1))[ok.expand_as(num)]
    e = torch.floor(torch.log2(x))
    ulp = torch.pow(2.0, e - 7)
    frac = x / ulp - torch.floor(x / ulp)                  # position inside a bf16 step, boundary at 0.5
    dist = (frac - 0.5).abs() * ulp / x
    tie = dist == 0
    return (float(dist[~tie].min()) if bool((~tie).any()) else 1.0), int(tie.sum())


# ------------------------------------------------------------------------------------------------ fp32 restatement and its mutants
MUTANTS = ("drop_last", "drop_range_first", "double_edge", "tail_in", "combine_w1", "drop_l", "no_guard", "head_mod", "no_max",
           "verify_long", "verify_short", "shared_early", "shared_late", "fp8_scale_next")


def mutant_applies(c: Case, mutant: str) -> bool:
    keys = c.keys()
    if mutant in ("drop_range_first", "double_edge", "combine_w1", "drop_l"):
        return c.nsplit > 1 and max(keys) > c.chunk
    if mutant == "tail_in":
        return any(n > 0 and n % 8 for n in keys)
    if mutant == "no_guard":
        return c.nsplit > 1 and any(0 < n <= (c.nsplit - 1) * c.chunk for n in keys)
    if mutant == "head_mod":
        return 1 < c.Hkv < c.H
    if mutant.startswith("verify"):
        return c.kind == "verify"
    if mutant.startswith("shared"):
        return c.kind == "shared"
    if mutant == "fp8_scale_next":
        return c.kind == "fp8kv"
    return True


def emu(c: Case, inp: dict, mutant: Optional[str] = None, form: str = "wave"):
    """The split walk in plain fp32 torch: scores, per key range (max, exp, sum, P V) -> partial slots, the guarded combine, one
    division, the bf16 store.  -> (out bf16 [R, H, hd], partials fp32 [R, H, nsplit, hd + 2])"""
    f32 = torch.float32
    shift = {"shared_early": -1, "shared_late": 1}.get(mutant, 0)
    k, v, rows = effective(c, inp, f32, shift=shift, scale_shift=1 if mutant == "fp8_scale_next" else 0, tail=(TAIL_K, TAIL_V))
    ns, ch = (c.nsplit2, c.chunk2) if form == "twophase" else (c.nsplit, c.chunk)
    head_map = tuple(h % c.Hkv for h in range(c.H)) if mutant == "head_mod" else c.head_map
    n = torch.tensor(c.keys())
    if mutant == "verify_long":
        n = torch.where(n > 0, n + 1, n)
    if mutant == "verify_short":
        n = torch.where(n > 0, n - 1, n)
    q = inp["q"].to(f32)
    s = _scores(q, k, rows, head_map, torch.tensor(1.0 / math.sqrt(c.hd), dtype=f32))
    j = torch.arange(c.Smax)[None, :]
    hd = c.hd
    part = torch.zeros(c.R, c.H, ns, hd + 2, dtype=f32)
    for sp in range(ns):
        lo, hi = sp * ch, (sp + 1) * ch
        live = (j >= lo) & (j < hi) & (j < n[:, None])
        if mutant == "drop_last":
            live &= j != (n[:, None] - 1)
        if mutant == "drop_range_first" and sp >= 1:
            live &= j != lo
        if mutant == "double_edge":
            live |= (j == hi) & (j < n[:, None])
        if mutant == "tail_in":
            live |= (j == n[:, None]) & (n[:, None] % 8 != 0) & (n[:, None] > 0) & (j >= lo) & (j < hi)
        live = live[:, None, :]
        ss = s.masked_fill(~live, -math.inf)
        m = ss.max(2, keepdim=True).values
        empty = torch.isinf(m) & (m < 0)
        ref = torch.zeros_like(m) if mutant == "no_max" else torch.where(empty, torch.zeros_like(m), m)
        p = torch.exp(ss - ref).masked_fill(~live, 0.0)
        o, l = _pv(p, v, rows, head_map), p.sum(2)
        if mutant == "no_guard":                                 # the unguarded wave merge of an empty range: exp(-inf + inf)
            o = torch.where(empty.expand_as(o), torch.full_like(o, NAN), o)
            l = torch.where(empty[:, :, 0], torch.full_like(l, NAN), l)
        part[:, :, sp, :hd], part[:, :, sp, hd], part[:, :, sp, hd + 1] = o, (torch.zeros_like(m) if mutant == "no_max" else m)[:, :, 0], l
    ms = part[..., hd]
    M = ms.max(2, keepdim=True).values
    if mutant == "combine_w1":
        w = torch.ones_like(ms)
    elif mutant == "no_guard":
        w = torch.exp(ms - M)
    else:
        w = torch.where(torch.isinf(ms) & (ms < 0), torch.zeros_like(ms), torch.exp(ms - M))
    num = (w.unsqueeze(-1) * part[..., :hd]).sum(2)
    wl = w * part[..., hd + 1]
    if mutant == "drop_l" and ns > 1:
        wl = torch.cat([wl[..., :1], wl[..., 2:]], -1)
    den = wl.sum(2, keepdim=True)
    out = num / den
    idle = (torch.tensor(c.keys()) <= 0)[:, None, None]
    out = torch.where(idle, torch.zeros_like(out), out)
    return out.to(BF), part


def judge(c: Case, family: str, ref: dict, out: torch.Tensor, partials: Optional[torch.Tensor] = None, flat: bool = False):
    """out [R, H, hd] (bf16 or float), partials [R, H, nsplit, hd + 2] or None -> (ok, largest err / bound, reasons)"""
    why = []
    g = out.to(F64)
    if not bool(torch.isfinite(g).all()):
        return False, math.inf, ["not finite"]
    idle = ~ref["live"]
    if bool(idle.any()) and float(g[idle].abs().sum()) != 0.0:
        why.append("an idle query is not exactly zero")
    err = (g - ref["want"]).abs()
    bd = old_flat_bound(ref["want"]) if flat else ref["bound"]
    ratio = float((err / bd).max())
    if flat:
        return ratio <= 1.0, ratio, why
    if family == "exact":
        if not torch.equal(out.to(BF), ref["expect"]):
            why.append("exact family: output bits differ")
        if partials is not None and ref["partials"] is not None:
            w = ref["written"]
            if not torch.equal(partials[w].float(), ref["partials"][w]):
                why.append("exact family: partial slots differ")
    elif ratio > 1.0:
        why.append(f"err / bound = {ratio:.3f}")
    return not why, ratio, why
