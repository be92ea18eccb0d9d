"""fp64 references, derived error bounds, input generators and the shape table for the decode GEMV family of a3vlm_amd/csrc/a3v_gemv.hip:
a3v_gemm_skinny (bf16 weights), a3v_gemm_skinny_fp8, a3v_gemm_skinny_nf4 and a3v_gemv_fused (the decode step's building block: RMSNorm
prologue, RoPE + KV-cache epilogue, sum-of-squares side output), in every kernel the plan can name (gemv_dma_bf16_kernel,
gemv_kq_bf16_kernel, gemm_skinny1_bf16_kernel<1|2>).  The scheme and the helpers are those of tests/gemm_ref.py (``within``,
HALF_ULP_BF16, EVAL_F32, TINY, ``ratio``, SENT, U23, LIP and the SwiGLU terms) and tests/rowops_fwd_ref.py (the RoPE bound).

The rounding sequences (gemv_finish, the W8 / N4 branches and the two prologues of a3v_gemv.hip perform them in this order; rbf = round to
nearest even to bf16, every other step ONE fp32 operation):

    accumulator   bf16   acc = sum_k A[m, k] W[n, k]                        fp32, any order, over any number of K slices
                  fp8    acc = (sum_k A[m, k] float(Wq[n, k])) * wscale[n]  one multiply on the summed accumulator, before any rounding
                  NF4    t_b = sum_{k in block b} A[m, k] bf16(NF4[q[n, k]])   per 64-k block; the codes are the bf16 bit patterns listed
                         acc = fmaf(t_b, s[n, b], acc)                      at nf4_bf16x8 (CODES), earlier element in the HIGH nibble
    epilogue      v   = rbf(acc)
                  o   = v + res                        RESIDUAL
                  out = rbf(o), or with OUT_F32 o stored as fp32
                  SWIGLU  out[m, c] = rbf(rbf(silu(rbf(g))) * rbf(u)), g / u the accumulators of the gate / up rows, interleaved in 16-row
                          blocks of W (N counts the interleaved rows, C has N / 2 columns)
    prologue      rinv[m] = rsqrtf(sum_t ssq_in[t][m] / K + eps)            ssq_in [K/16][16] is an INPUT table: it need not be consistent with x
                  a'      = rbf(rbf(x * rinv) * g)                          and the GEMV runs on a'
    ROPEKV        rows n = [H q heads | Hkv k heads | Hkv v heads] x hd, v = rbf(acc); q and k pairs (v0, v1) -> rbf(v0 c - v1 s),
                  rbf(v0 s + v1 c) with (c, s) = cos_sin[pos][d / 2]; q -> C, k -> k_cache[m, h, pos, :], v unrotated -> vt_cache[m, h, :, pos]
    SSQ           ssq_out[n / 16][m] = sum over the tile's 16 columns of rbf(o)^2 (0 for m >= M)

Three input families per table entry.

EXACT: integers that bf16 holds with K max|A| max|W| (+ residual) < 2^24 (``exact_budget_ok``): every product and every partial sum is an
integer below 2^24, exact in fp32 in any order over any slices, so the accumulator IS the fp64 product and the output must equal, bit
for bit, that product put through the sequence (``bits``).  Per format and form:
  fp8       integer-valued e4m3 bytes (|Wq| <= 16: e4m3 holds every such integer) and power-of-two row scales: the one multiply is exact.
  NF4       codes and scales are built directly, not through the quantiser.  Every code is a multiple of 2^-11 and at most 1 in
            magnitude, A holds integers |A| <= a: a block sum is a multiple of 2^-11 below 64 a, exact if 64 a 2^11 < 2^24 (a <= 127).
            The scales are powers of two from {1, 2}: every term of the running sum is a multiple of 2^-11 and every partial sum is
            below 2 sum_k |A[m, k]|, exact if 2 max_m sum_k |A[m, k]| 2^11 < 2^24, i.e. sum_k |A[m, k]| < 2^12.  Where K a exceeds that
            with a = 1, A is {-1, 0, 1} and sparse (a quarter of 2^12 / K dense on average; ``exact_budget_ok`` checks the actual sums).
            The fp32 addition of the residual is ONE correctly rounded operation on two fp32 values and is modelled as such.
  prologue  x = (4-bit integer) 2^j[m], ssq_in integers that sum to K 4^j[m] per row (not uniform over the tiles), eps = 0, g in
            {-2, -1, 1, 2}: the argument of rsqrtf is exactly 4^j (a sum of integers, one exact division) and rinv = 2^-j up to the
            error of rsqrtf.  x rinv is then a 4-bit integer times (1 + d): a 1-ulp (or 100-ulp) error d cannot move its rounding to
            bf16, which has 8 bits, so rbf(x rinv) is that integer whatever v_rsq_f32 returns at a power of four (nobody has measured
            it; the test does not depend on it), and a' = integer g exactly.
  RoPE      cos / sin drawn from {0, +-1, +-1/2}: both products are exact, so v0 c - v1 s is one rounding of an exact sum with or
            without the compiler's fma contraction.
  SSQ       the sums of squares must be bit-equal too, in any order: A in {0, 1}, |W| <= 896 / K and a residual small enough that |o| <= 1023
            (an integer), so 16 o^2 < 2^24.  fp8 / NF4 scales are +-1 there and the NF4 codes are those of -1, 0, 1.  The rows of W keep one
            sign and A is three quarters ones, so that the accumulators reach past 2^8 and need their rounding to bf16.
  SWIGLU    uses the bound on exact inputs: silu is not correctly rounded.

BOUNDED (``same``: all operands positive, ``mixed``: zero-mean with powers of two per row and column, as in gemm_ref): the bound of an
element is |got - ref| <= rel |ref| + E + TINY with E = (K - 1) 2^-23 mag pushed through the epilogue as gemm_ref does, mag the summed
|terms| in fp64, plus
  fp8       one fp32 rounding for the scale: 2^-24 (|acc| + E).
  NF4       63 additions per block on the block's mag (2^-23 each) and one fma rounding per block; the two accumulators of a wave and the
            up to eight slices are merged by at most 15 more additions: (K / 64 + 16) 2^-24 mag in all.
  ROPEKV    v = rbf(acc) carries E + 2^-8 (|v| + E); the pair's error is that of v0 and v1 times |c|, |s| plus EVAL_F32 times the
            summed |terms| (rowops_fwd_ref's bound, which also covers a contracted fma), then the output rounding.
  SSQ       against the fp64 sum of squares of the STORED bf16 values: 16 squares and 15 + 2 additions, all positive: 33 2^-24 relative.
  prologue  the reference normalises in fp64 and rounds at the same two points.  The relative error of the kernel's rinv is below
            RINV_REL(K) = (K / 16 + 8) 2^-24: K / 16 - 1 additions of positive terms, the division, the addition of eps and the product
            x rinv at half an ulp each (2^-24), rsqrtf at its documented 2 ulp (4 2^-24); the halving of the argument's error by the
            square root is not claimed.  An element whose x rinv lies within that of a bf16 rounding boundary is FRAGILE: the kernel
            may round it to the other neighbour.  For a fragile element only, ulp_bf16(a') |W[n, k]| is charged to the bound.  At most
            1 % of the elements of any bounded prologue input may be fragile (FRAGILE_CAP; tests/test_gemv_ref_cpu.py asserts it).

``emu`` restates the arithmetic in fp32 torch in three summation orders (one matmul; the plan's slices in order; 32-k granules last to
first) and MUTANTS are eleven wrong kernels.  tests/test_gemv_ref_cpu.py shows that every restatement stays inside the bound on every
bounded input set and equals ``bits`` on every exact set, and that every mutant leaves the bound on every bounded set it applies to and
changes bits on every exact set it applies to.

TABLE: the smallest shapes that reach each outcome; every entry names the plan it expects (kernel, arows, S, slices as a3v_gemv_plan
reports them; the direct kernels report zeros), checked against a3v_gemv_plan on the CPU (256 CUs) and against the device on the GPU.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

import gemm_ref as G
from gemm_ref import EVAL_F32, HALF_ULP_BF16, LIP, SENT, TINY, U23, U24, ratio, within, _split_swiglu  # noqa: F401

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
F8 = torch.float8_e4m3fn
H = HALF_ULP_BF16
FAMILIES = G.FAMILIES
DMA, KQ, DIRECT1, DIRECT2 = range(4)
ERR_SHAPE, ERR_ARG = -1, -3
EPI = dict(res=8, swiglu=16, out_f32=32)
FMT = dict(bf16=0, fp8=1, nf4=2)
SMAX = 24
MAX_ENTRIES = 120
MAX_MACS = 2 ** 31
FRAGILE_CAP = 0.01
# the bf16 bit patterns of the NF4 code book as nf4_bf16x8 lists them
CODES = (torch.tensor([0xbf80, 0xbf32, 0xbf06, 0xbeca, 0xbe92, 0xbe3d, 0xbdba, 0x0000, 0x3da3, 0x3e25, 0x3e7c, 0x3ead, 0x3ee2, 0x3f10,
                       0x3f39, 0x3f80], dtype=torch.int32).to(torch.int16).view(BF).to(F64))


def RINV_REL(K):
    return (K // 16 + 8) * U24


class Case(NamedTuple):
    fmt: str                   # bf16 | fp8 | nf4
    M: int
    N: int                     # rows of W (SWIGLU: interleaved gate / up rows, C has N / 2 columns; ROPEKV: (H + 2 Hkv) hd)
    K: int
    plan: tuple                # expected (kernel, arows, S, slices) of a3v_gemv_plan
    epi: tuple = ()            # of res swiglu out_f32
    fused: tuple = ()          # of pro rope ssq: a3v_gemv_fused
    geom: tuple = ()           # rope: (H, Hkv, hd, pos)
    kq: Optional[int] = None   # A3V_GEMV_KQ for the call

    @property
    def id(self):
        s = f"{self.fmt}-{self.M}x{self.N}x{self.K}"
        for part in (self.epi, self.fused):
            if part:
                s += "-" + "+".join(part)
        if self.geom:
            s += "-h{}.{}.{}p{}".format(*self.geom)
        if self.kq is not None:
            s += f"-kq{self.kq}"
        return s

    @property
    def macs(self):
        return self.M * self.N * self.K

    @property
    def flags(self):
        return sum(EPI[e] for e in self.epi)

    @property
    def env(self):
        return {} if self.kq is None else {"A3V_GEMV_KQ": self.kq}

    @property
    def entry(self):
        return "a3v_gemv_fused" if self.fused else {"bf16": "a3v_gemm_skinny", "fp8": "a3v_gemm_skinny_fp8", "nf4": "a3v_gemm_skinny_nf4"}[self.fmt]


def _quant(fmt, big_k):
    """fp8 / NF4: K = 256 (S = 1), 512, 768 (uneven slices), the long K at N = 80 (the ring wraps and refills); every epilogue; N = 68"""
    return [
        Case(fmt, 1, 4, 256, (DMA, 8, 1, 1)), Case(fmt, 7, 20, 512, (DMA, 8, 2, 2), ("res",)),
        Case(fmt, 8, 68, 768, (DMA, 8, 2, 2), ("out_f32",)), Case(fmt, 9, 60, 256, (DMA, 16, 1, 1), ("res", "out_f32")),
        Case(fmt, 15, 64, 512, (DMA, 16, 2, 2)), Case(fmt, 16, 132, 768, (DMA, 16, 2, 2), ("res",)),
        Case(fmt, 8, 80, big_k, (DMA, 8, 8, 8), ("res",)), Case(fmt, 16, 80, big_k, (DMA, 16, 8, 8)),
        Case(fmt, 16, 68, 256, (DMA, 16, 1, 1), ("res",)),
        Case(fmt, 8, 96, 512, (DMA, 8, 2, 2), ("swiglu",)), Case(fmt, 16, 64, 768, (DMA, 16, 2, 2), ("swiglu",)),
        # fused forms (no in-block kernel for quantised weights)
        Case(fmt, 9, 64, 256, (DMA, 16, 1, 1), fused=("pro", "rope"), geom=(2, 1, 16, 0)),
        Case(fmt, 8, 384, 512, (DMA, 8, 2, 2), fused=("pro", "rope"), geom=(1, 1, 128, 23)),
        Case(fmt, 15, 64, 512, (DMA, 16, 2, 2), fused=("pro", "rope"), geom=(2, 1, 16, 5)),
        Case(fmt, 16, 96, 512, (DMA, 16, 2, 2), ("swiglu",), fused=("pro",)), Case(fmt, 7, 64, 768, (DMA, 8, 2, 2), ("swiglu",), fused=("pro",)),
        Case(fmt, 7, 64, 512, (DMA, 8, 2, 2), ("res",), fused=("ssq",)), Case(fmt, 16, 80, 256, (DMA, 16, 1, 1), ("res",), fused=("ssq",)) if fmt == "fp8" else
        Case(fmt, 16, 80, 768, (DMA, 16, 2, 2), ("res",), fused=("ssq",)),         # (NF4: 256 ones times codes <= 1 stay below 2^8, where bf16 is exact)
    ]


TABLE = [
    # ---- bf16, across-blocks kernel: M in {1, 7, 8, 9, 15, 16}, N in {4, 20, 60, 64, 68, 132}, K = 128 (S = 1), 256, 384 and 640 (uneven), 1408
    Case("bf16", 1, 4, 128, (DMA, 8, 1, 1)), Case("bf16", 7, 20, 256, (DMA, 8, 2, 2), ("res",)),
    Case("bf16", 8, 60, 384, (DMA, 8, 2, 2), ("out_f32",)), Case("bf16", 9, 64, 640, (DMA, 16, 4, 4), ("res",)),
    Case("bf16", 15, 68, 1408, (DMA, 16, 8, 8), ("res", "out_f32")), Case("bf16", 16, 132, 256, (DMA, 16, 2, 2)),
    Case("bf16", 1, 132, 128, (DMA, 8, 1, 1), ("res",)), Case("bf16", 16, 4, 128, (DMA, 16, 1, 1), ("out_f32",)),
    Case("bf16", 8, 68, 1408, (DMA, 8, 8, 8)), Case("bf16", 7, 60, 640, (DMA, 8, 4, 4)), Case("bf16", 15, 20, 384, (DMA, 16, 2, 2), ("res",)),
    Case("bf16", 8, 80, 3200, (DMA, 8, 8, 8)), Case("bf16", 16, 80, 3200, (DMA, 16, 8, 8), ("res",)),          # 3-4 stages per slice: st + 2 < nst
    Case("bf16", 9, 96, 256, (DMA, 16, 2, 2), ("swiglu",)), Case("bf16", 7, 64, 640, (DMA, 8, 4, 4), ("swiglu",)),
    Case("bf16", 16, 160, 1408, (DMA, 16, 8, 8), ("swiglu",)),
    # ---- bf16, in-block kernel: the default mode at its smallest even spread, then A3V_GEMV_KQ=2 at small N
    Case("bf16", 8, 4096, 256, (KQ, 8, 2, 1)), Case("bf16", 8, 4096, 256, (KQ, 8, 2, 1), ("res",)),            # nkb < 2 slices: one slice
    Case("bf16", 1, 16, 128, (KQ, 8, 1, 1), kq=2), Case("bf16", 7, 48, 256, (KQ, 8, 2, 1), ("res",), kq=2),
    Case("bf16", 8, 80, 640, (KQ, 8, 4, 2), ("out_f32",), kq=2), Case("bf16", 3, 64, 1408, (KQ, 8, 8, 5), ("res", "out_f32"), kq=2),
    Case("bf16", 8, 80, 3200, (KQ, 8, 8, 8), kq=2), Case("bf16", 1, 64, 3200, (KQ, 8, 8, 8), ("res",), kq=2),
    Case("bf16", 8, 64, 3200, (KQ, 8, 8, 6), ("swiglu",), kq=2),                                              # 12 waves
    Case("bf16", 1, 96, 640, (KQ, 8, 4, 2), ("swiglu",), kq=2),
    Case("bf16", 7, 20, 256, (DMA, 8, 2, 2), kq=2),                                                           # N % 16: not in-block
    # ---- bf16, direct-to-VGPR kernel: K = 32 (seven empty waves), 96, 160, 2080 (unrolled loop + tail), SwiGLU without a split, the LDS limit
    Case("bf16", 1, 4, 32, (DIRECT1, 0, 0, 0)), Case("bf16", 7, 20, 96, (DIRECT1, 0, 0, 0), ("res",)),
    Case("bf16", 9, 68, 160, (DIRECT1, 0, 0, 0), ("out_f32",)), Case("bf16", 16, 132, 2080, (DIRECT1, 0, 0, 0), ("res",)),
    Case("bf16", 8, 60, 2080, (DIRECT1, 0, 0, 0)), Case("bf16", 15, 64, 32, (DIRECT1, 0, 0, 0), ("res", "out_f32")),
    Case("bf16", 8, 96, 128, (DIRECT2, 0, 0, 0), ("swiglu",)), Case("bf16", 15, 64, 96, (DIRECT2, 0, 0, 0), ("swiglu",)),
    Case("bf16", 9, 96, 2080, (DIRECT2, 0, 0, 0), ("swiglu",)),
    Case("bf16", 16, 16, 245760, (DIRECT1, 0, 0, 0)),                                                         # 7.5 MiB of weights: above 150 KiB of LDS
    # ---- bf16 fused forms, across blocks (M = 9 .. 16, or A3V_GEMV_KQ=0) and in-block
    Case("bf16", 9, 64, 256, (DMA, 16, 2, 2), fused=("pro", "rope"), geom=(2, 1, 16, 0)),
    Case("bf16", 16, 384, 256, (DMA, 16, 2, 2), fused=("pro", "rope"), geom=(1, 1, 128, 5)),
    Case("bf16", 7, 64, 640, (DMA, 8, 4, 4), fused=("pro", "rope"), geom=(2, 1, 16, 23), kq=0),
    Case("bf16", 9, 96, 256, (DMA, 16, 2, 2), ("swiglu",), fused=("pro",)), Case("bf16", 8, 64, 640, (DMA, 8, 4, 4), ("swiglu",), fused=("pro",), kq=0),
    Case("bf16", 9, 64, 256, (DMA, 16, 2, 2), ("res",), fused=("ssq",)), Case("bf16", 8, 80, 256, (DMA, 8, 2, 2), ("res",), fused=("ssq",), kq=0),
    Case("bf16", 8, 64, 640, (KQ, 8, 4, 2), fused=("pro", "rope"), geom=(2, 1, 16, 5), kq=2),
    Case("bf16", 1, 384, 256, (KQ, 8, 2, 1), fused=("pro", "rope"), geom=(1, 1, 128, 23), kq=2),
    Case("bf16", 5, 64, 1408, (KQ, 8, 8, 5), fused=("pro", "rope"), geom=(2, 1, 16, 0), kq=2),
    Case("bf16", 7, 64, 640, (KQ, 8, 4, 2), ("swiglu",), fused=("pro",), kq=2),
    Case("bf16", 8, 80, 640, (KQ, 8, 4, 2), ("res",), fused=("ssq",), kq=2), Case("bf16", 1, 16, 128, (KQ, 8, 1, 1), ("res",), fused=("ssq",), kq=2),
] + _quant("fp8", 6400) + _quant("nf4", 10496)
BY_ID = {c.id: c for c in TABLE}
assert len(BY_ID) == len(TABLE)

# the refusals of the fused entry point, as return codes only: (case, expected return code)
REFUSALS = [
    (Case("bf16", 8, 64, 128, (), ("swiglu",), fused=("pro",)), ERR_SHAPE),                   # SwiGLU with S = 1
    (Case("fp8", 16, 64, 256, (), ("swiglu",), fused=("pro",)), ERR_SHAPE),
    (Case("nf4", 16, 64, 256, (), ("swiglu",), fused=("pro",)), ERR_SHAPE),
    (Case("bf16", 8, 96, 256, (), fused=("pro", "rope"), geom=(2, 1, 24, 0)), ERR_ARG),        # hd % 16
    (Case("fp8", 8, 96, 256, (), fused=("pro", "rope"), geom=(2, 1, 24, 0)), ERR_ARG),
    (Case("nf4", 8, 96, 256, (), fused=("pro", "rope"), geom=(2, 1, 24, 0)), ERR_ARG),
]


# ------------------------------------------------------------------ layout of a case
def out_cols(c):
    if "swiglu" in c.epi:
        return c.N // 2
    return c.geom[0] * c.geom[2] if "rope" in c.fused else c.N


def out_dtype(c):
    return F32 if "out_f32" in c.epi else BF


def n_slices(c):
    """K slices of the restatements and mutants: the plan's (eight waves for the direct kernels)"""
    return c.plan[3] if c.plan and c.plan[3] else 8


def slice_edges(c):
    """edges of the K slices in 32-k granules, as the planned kernel cuts them (whole ring stages; the direct kernels: whole granules)"""
    Gn = c.K // 32
    if c.plan and c.plan[0] in (DIRECT1, DIRECT2):
        per = (Gn + 7) // 8
        return [min(w * per, Gn) for w in range(9)]
    S = n_slices(c)
    kst = (128 if c.fmt == "bf16" else 256) // 32
    nst = Gn // kst
    return [nst * s // S * kst for s in range(S + 1)]


# ------------------------------------------------------------------ inputs
def _seed(c, family):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id + family)) * 2654435761) % (2 ** 31)


def _rbf64(t):
    return t.to(F32).to(BF).to(F64)


def _pack_nibbles(codes):
    """codes [N, K] 0..15 -> bytes [N, K / 2], the earlier element in the high nibble"""
    return ((codes[:, 0::2] << 4) | codes[:, 1::2]).to(torch.uint8)


def unpack_nibbles(q):
    q = q.to(torch.int64)
    return torch.stack([q >> 4, q & 15], dim=-1).reshape(q.shape[0], -1)


def exact_limits(c):
    """(max |A'| of the matrix the GEMV runs on, max |W value|, residual shift): the budgets of the module docstring"""
    K = c.K
    if "ssq" in c.fused:
        w = max(1, 896 // K) if c.fmt != "nf4" else 1
        return 1, w, int(math.log2((1023 - K * w) // 127))
    budget = 2 ** 24 - 2 ** 17
    if c.fmt == "nf4":
        return max(1, min(127, (2 ** 12 - 1) // K)), 1, 8
    w = min(16 if c.fmt == "fp8" else 127, max(1, math.isqrt(budget // K)))
    return max(1, min(127, budget // (K * w))), w, 8


def _exact_inputs(c, g):
    M, N, K = c.M, c.N, c.K
    a, w, rsh = exact_limits(c)
    d = {}
    if "pro" in c.fused:
        gmax = 2
        xmax = max(1, min(15, a // gmax))
        j = torch.randint(0, 3, (M,), generator=g)
        x = torch.randint(-xmax, xmax + 1, (M, K), generator=g).double()
        d["A"] = (x * 2.0 ** j[:, None].double()).to(BF)
        gw = torch.randint(1, gmax + 1, (K,), generator=g) * (2 * torch.randint(0, 2, (K,), generator=g) - 1)
        d["norm_w"] = gw.double().to(BF)
        ssq = torch.zeros(K // 16, 16)
        ssq[:, :M] = 16.0 * 4.0 ** j[None, :].double()
        delta = torch.randint(1, 16, (K // 32, 16), generator=g).float()           # moved between neighbouring tiles: the sum stays
        ssq[0:2 * (K // 32):2] += delta
        ssq[1:2 * (K // 32):2] -= delta
        ssq[:, M:] = 3.0
        d["ssq_in"], d["eps"] = ssq.to(F32), 0.0
    elif c.fmt == "nf4" and K * a >= 2 ** 12:
        dense = (2 ** 12 / K) / 4
        d["A"] = (torch.randint(-1, 2, (M, K), generator=g) * (torch.rand(M, K, generator=g) < max(dense * 1.5, 0.02))).double().to(BF)
    elif "ssq" in c.fused:                                     # three quarters ones: the sums of a row of W agree in sign and reach past 2^8
        d["A"] = (torch.rand(M, K, generator=g) < 0.75).double().to(BF)
    else:
        d["A"] = torch.randint(-a, a + 1, (M, K), generator=g).double().to(BF)
    ssq = "ssq" in c.fused
    sgn = (2 * torch.randint(0, 2, (N,), generator=g) - 1).double()
    if c.fmt == "bf16":
        Wi = torch.randint(1, w + 1, (N, K), generator=g).double() * sgn[:, None] if ssq else torch.randint(-w, w + 1, (N, K), generator=g).double()
        d["W"] = Wi.to(BF)
    elif c.fmt == "fp8":
        Wi = torch.randint(1, w + 1, (N, K), generator=g) if ssq else torch.randint(-w, w + 1, (N, K), generator=g)
        d["Wq"] = Wi.float().to(F8).view(torch.uint8)
        d["wscale"] = sgn.float() if ssq else 2.0 ** torch.randint(-2, 3, (N,), generator=g).float()
    elif ssq:                                                  # codes of 0 and of +-1, the sign that of the block's scale times the row's
        bs = (2 * torch.randint(0, 2, (N, K // 64), generator=g) - 1).double()
        one = torch.where(bs * sgn[:, None] > 0, 15, 0).repeat_interleave(64, dim=1)
        d["Wq"] = _pack_nibbles(torch.where(torch.rand(N, K, generator=g) < 0.9, one, torch.full_like(one, 7)))
        d["wscale"] = bs.float()
    else:
        d["Wq"] = _pack_nibbles(torch.randint(0, 16, (N, K), generator=g))
        d["wscale"] = 2.0 ** torch.randint(0, 2, (N, K // 64), generator=g).float()
    if "res" in c.epi:
        d["res"] = (torch.randint(-127, 128, (M, N), generator=g) * 2 ** torch.randint(0, rsh + 1, (M, N), generator=g)).double().to(BF)
    if "rope" in c.fused:
        vals = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5])
        d["cos_sin"] = vals[torch.randint(0, 5, (SMAX, c.geom[2] // 2, 2), generator=g)].to(F32)
    return d


def inputs(c: Case, family: str):
    """CPU tensors of the case in the dtypes the entry point takes: A [M, K] bf16 (prologue: the un-normalised x), W [N, K] bf16 or Wq
    (fp8: [N, K] bytes, NF4: [N, K / 2] bytes) with wscale ([N] / [N, K / 64] fp32), res [M, N] bf16, norm_w [K] bf16, ssq_in [K / 16, 16]
    fp32, eps, cos_sin [SMAX, hd / 2, 2] fp32"""
    g = torch.Generator().manual_seed(_seed(c, family))
    if family == "exact":
        return _exact_inputs(c, g)
    M, N, K = c.M, c.N, c.K
    act = "swiglu" in c.epi
    i, j = torch.arange(M), torch.arange(N)
    if family == "same":
        rs, cs = 2.0 ** (i % 3).double(), 2.0 ** ((j.double() * 0.381966) % 1.0)
        gen = lambda *s: torch.rand(*s, generator=g).double() + 0.25          # noqa: E731
    else:
        rs = 2.0 ** torch.randint(-10, 11, (M,), generator=g).double()
        cs = 2.0 ** torch.randint(-10, 11, (N,), generator=g).double()
        gen = lambda *s: torch.randn(*s, generator=g).double()              # noqa: E731
    if act and family == "mixed":
        rs[::2] = 1.0
        cs[:] = 1.0
    A = gen(M, K) * rs[:, None]
    W = gen(N, K)
    if family == "mixed" and K >= 2048:          # as gemm_ref: the two halves of K cancel
        A, W = A.abs(), W.abs()
        W[:, K // 2:] *= -1.0
    pre = (math.sqrt(K) if family == "mixed" else K) if act else 1.0          # a pre-activation of order one at unit scale
    d = {}
    pro = "pro" in c.fused
    if pro:
        d["A"] = A.to(BF)
        x = d["A"].double()
        gw = (gen(K) if family == "same" else 1.0 + 0.25 * gen(K)) / pre
        d["norm_w"] = gw.to(BF)
        t = (x.view(M, K // 16, 16) ** 2).sum(-1).t()                            # [K / 16, M]: the producer's sums, then perturbed
        ssq = torch.ones(K // 16, 16, dtype=F64)
        ssq[:, :M] = t * (0.75 + 0.5 * torch.rand(K // 16, M, generator=g).double())
        d["ssq_in"], d["eps"] = ssq.to(F32), 1e-5
        rs = torch.ones(M, dtype=F64)
    else:
        d["A"] = (A / pre).to(BF)
    if c.fmt == "bf16":
        d["W"] = (W * cs[:, None]).to(BF)
    elif c.fmt == "fp8":
        sc = (W.abs().amax(1) / 448.0)
        d["Wq"] = (W / sc[:, None]).float().to(F8).view(torch.uint8)
        d["wscale"] = (sc * cs).to(F32)
    else:
        d["Wq"] = _pack_nibbles(torch.randint(0, 16, (N, K), generator=g))
        blk = (torch.rand(N, K // 64, generator=g).double() + 0.5) * (2.0 if family == "same" else math.sqrt(3.0))
        if family == "mixed" and K >= 2048:
            blk[:, K // 128:] *= -1.0
        d["wscale"] = (blk * cs[:, None]).to(F32)
    typ = 1.0 if act else K if family == "same" else math.sqrt(K)
    if "res" in c.epi:
        d["res"] = (gen(M, N) * rs[:, None] * cs[None, :] * typ).to(BF)
    if "rope" in c.fused:
        hd = c.geom[2]
        pair = torch.arange(hd // 2).double()                 # the rotary table plus an offset per pair: no two pairs of a position share an angle
        ang = torch.arange(SMAX).double()[:, None] * (10000.0 ** (-pair * 2 / hd))[None, :] + 0.37 * (pair[None, :] + 1.0)
        d["cos_sin"] = torch.stack([ang.cos(), ang.sin()], -1).to(F32)
    return d


def weights64(c, inp):
    """-> (values [N, K] fp64 that enter the MFMA, scales broadcastable to them or None)"""
    if c.fmt == "bf16":
        return inp["W"].to(F64), None
    if c.fmt == "fp8":
        return inp["Wq"].view(F8).to(F64), inp["wscale"].to(F64)[:, None]
    return CODES[unpack_nibbles(inp["Wq"])], inp["wscale"].to(F64).repeat_interleave(64, dim=1)


def _ulp_bf16(t):
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.where(t == 0, torch.zeros_like(t), 2.0 ** (e - 7))


def prologue64(c, inp):
    """-> (a' [M, K] fp64 of bf16 values, fragile [M, K] bool): the fp64 normalisation rounded at the kernel's two points"""
    x, gw = inp["A"].to(F64), inp["norm_w"].to(F64)
    eps32 = torch.tensor(inp["eps"], dtype=F32).to(F64)
    rinv = 1.0 / torch.sqrt(inp["ssq_in"].to(F64).sum(0)[:c.M] / c.K + eps32)
    p = x * rinv[:, None]
    t = _rbf64(p)
    d = RINV_REL(c.K)
    fragile = _rbf64(p * (1.0 - d)) != _rbf64(p * (1.0 + d))
    return _rbf64(t * gw[None, :]), fragile


def effective_a(c, inp):
    if "pro" in c.fused:
        return prologue64(c, inp)
    return inp["A"].to(F64), None


def exact_budget_ok(c, inp):
    A, _ = effective_a(c, inp)
    Wv, sc = weights64(c, inp)
    r = float(inp["res"].abs().max()) if "res" in inp else 0.0
    amax, wmax = float(A.abs().max()), float(Wv.abs().max())
    if "ssq" in c.fused:
        return float(A.abs().sum(1).max()) * wmax * (float(sc.abs().max()) if sc is not None else 1.0) + r <= 1023 and \
            bool((Wv == Wv.round()).all())
    if c.fmt == "nf4":
        s = sc.abs()
        return 64 * amax * 2 ** 11 < 2 ** 24 and float(A.abs().sum(1).max()) * float(s.max() / s.min()) * 2 ** 11 < 2 ** 24
    return bool((A == A.round()).all()) and bool((Wv == Wv.round()).all()) and c.K * amax * wmax + r < 2 ** 24


# ------------------------------------------------------------------ fp64 reference and bound
def accumulator64(c, inp):
    """-> (acc, E): the accumulator in fp64 and its error allowance (module docstring)"""
    A, fragile = effective_a(c, inp)
    Wv, sc = weights64(c, inp)
    Ws = Wv if sc is None else Wv * sc
    acc = A @ Ws.t()
    mag = A.abs() @ Ws.abs().t()
    if c.fmt == "nf4":
        E = 63 * U23 * mag + (c.K // 64 + 16) * U24 * mag
    else:
        E = (c.K - 1) * U23 * mag
        if c.fmt == "fp8":
            E = E + U24 * (acc.abs() + E)
    if fragile is not None:
        E = E + (fragile.double() * _ulp_bf16(A)) @ Ws.abs().t()
    return acc, E


def reference(c: Case, inp, family: str):
    """-> dict of C (and k, vt: the [M, Hkv, hd] windows at pos) -> dict(ref, E, rel, uf, bits) as gemm_ref.reference returns it, and ssq_bits
    ([N / 16, 16], exact family) or None"""
    acc, E = accumulator64(c, inp)
    exact = family == "exact" and "swiglu" not in c.epi
    od = out_dtype(c)
    out = {"ssq_bits": None}
    if "swiglu" in c.epi:
        g, u = _split_swiglu(acc)
        Eg, Eu = _split_swiglu(E)
        Eg, Eu = Eg + H * (g.abs() + Eg), Eu + H * (u.abs() + Eu)
        s = g * torch.sigmoid(g)
        Es = LIP * Eg + EVAL_F32 * g.abs() + H * (s.abs() + LIP * Eg)
        ref = s * u
        Eo = (Es * (u.abs() + Eu) + s.abs() * Eu) * (1.0 + U24) + U24 * ref.abs()
        out["C"] = dict(ref=ref, E=Eo * (1.0 + H), rel=H, uf=(g * u).abs() + Eu * g.abs(), bits=None)
        return out
    vb = _rbf64(acc) if exact else None
    if "rope" in c.fused:
        Hh, Hkv, hd, pos = c.geom
        Ev = E + H * (acc.abs() + E)
        cs = inp["cos_sin"][pos].to(F64)                                         # [hd / 2, 2]
        nqk = (Hh + Hkv) * hd
        co, si = cs[:, 0].repeat(Hh + Hkv)[None, :], cs[:, 1].repeat(Hh + Hkv)[None, :]

        def rot(v, e):
            a, b, ea, eb = v[:, 0:nqk:2], v[:, 1:nqk:2], e[:, 0:nqk:2], e[:, 1:nqk:2]
            r0, r1 = a * co - b * si, a * si + b * co
            m0 = (a * co).abs() + (b * si).abs() + ea * co.abs() + eb * si.abs()
            m1 = (a * si).abs() + (b * co).abs() + ea * si.abs() + eb * co.abs()
            e0, e1 = ea * co.abs() + eb * si.abs() + EVAL_F32 * m0, ea * si.abs() + eb * co.abs() + EVAL_F32 * m1
            return torch.stack([r0, r1], -1).reshape(c.M, nqk), torch.stack([e0, e1], -1).reshape(c.M, nqk)

        ref, Er = rot(acc, Ev)
        bits = rot(vb, torch.zeros_like(vb))[0].to(F32).to(BF) if exact else None
        q = slice(0, Hh * hd)
        out["C"] = dict(ref=ref[:, q], E=Er[:, q] * (1.0 + H), rel=H, uf=None, bits=None if bits is None else bits[:, q])
        k = slice(Hh * hd, nqk)
        out["k"] = dict(ref=ref[:, k].reshape(c.M, Hkv, hd), E=Er[:, k].reshape(c.M, Hkv, hd) * (1.0 + H), rel=H, uf=None,
                        bits=None if bits is None else bits[:, k].reshape(c.M, Hkv, hd))
        v = slice(nqk, c.N)
        out["vt"] = dict(ref=acc[:, v].reshape(c.M, Hkv, hd), E=E[:, v].reshape(c.M, Hkv, hd) * (1.0 + H), rel=H, uf=None,
                         bits=None if vb is None else vb[:, v].reshape(c.M, Hkv, hd).to(BF))
        return out
    if "res" not in c.epi:
        out["C"] = dict(ref=acc, E=E * (1.0 + H), rel=H, uf=None, bits=None if vb is None else vb.to(od))
    else:
        res = inp["res"].to(F64)
        Ev = E + H * (acc.abs() + E)
        v = acc + res
        Ev = Ev + U24 * (v.abs() + Ev)
        o = (vb + res).to(F32) if exact else None                                # one correctly rounded fp32 addition of two fp32 values
        if od == BF:
            out["C"] = dict(ref=v, E=Ev * (1.0 + H), rel=H, uf=None, bits=None if o is None else o.to(BF))
        else:
            out["C"] = dict(ref=v, E=Ev, rel=0.0, uf=None, bits=o)
    if "ssq" in c.fused and exact:
        sq = out["C"]["bits"].to(F64) ** 2
        t = torch.zeros(c.N // 16, 16, dtype=F64)
        t[:, :c.M] = sq.view(c.M, c.N // 16, 16).sum(-1).t()
        out["ssq_bits"] = t.to(F32)
    return out


def ssq_ratio(ssq, stored, M):
    """worst |slot - fp64 sum of squares of the STORED values of its tile| over 33 2^-24 of that sum; slots of rows m >= M must be 0"""
    N = stored.shape[1]
    want = (stored.to(F64) ** 2).view(M, N // 16, 16).sum(-1).t()
    got = ssq.to(F64)
    if got.shape != (N // 16, 16) or not bool(torch.isfinite(got).all()) or bool((got[:, M:] != 0).any()):
        return float("inf")
    return float(((got[:, :M] - want).abs() / (33 * U24 * want + 2.0 ** -149)).max())


def judge(c: Case, r, out):
    """-> (bit-equal: True / False, or None where the reference has no bits; worst ratio to the bound) of an output dict C (k_cache,
    vt_cache: the whole caches, SENT outside the written window; ssq) against ``reference``'s result"""
    od = out_dtype(c)
    equal, worst = True, 0.0
    wins = {"C": out["C"]}
    if "rope" in c.fused:
        pos = c.geom[3]
        kc, vc = out["k_cache"].clone(), out["vt_cache"].clone()
        wins["k"], wins["vt"] = kc[:, :, pos, :].clone(), vc[:, :, :, pos].clone()
        kc[:, :, pos, :] = SENT
        vc[:, :, :, pos] = SENT
        if not (bool((kc == SENT).all()) and bool((vc == SENT).all())):
            return False, float("inf")
    for name, got in wins.items():
        rr = r[name]
        got = got.cpu()
        worst = max(worst, ratio(got, rr, od if name == "C" else BF))
        if rr["bits"] is None:
            equal = None
        elif equal is not None:
            equal = equal and got.dtype == rr["bits"].dtype and torch.equal(got, rr["bits"])
    if "ssq" in c.fused:
        worst = max(worst, ssq_ratio(out["ssq"].cpu(), out["C"].cpu(), c.M))
        if r["ssq_bits"] is not None and equal is not None:
            equal = equal and torch.equal(out["ssq"].cpu(), r["ssq_bits"])
    return equal, worst


# ------------------------------------------------------------------ fp32 restatements and mutants (CPU)
def _rb(t):
    return t.to(BF).to(F32)


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in fp64"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


RESTATEMENTS = ["matmul", "slices", "reverse"]
MUTANTS = ["drop_granule", "double_slice", "res_before_rbf", "fp8_scale_next_row", "nf4_scale_next_block", "nf4_nibble_swap",
           "gate_up_swapped", "rope_neighbour_angle", "vt_pos_minus_1", "pro_no_inner_rbf", "rows_8_15_read_m_and_7"]


def mutant_applies(c, mutant, family):
    if mutant == "double_slice":
        return True
    if mutant == "drop_granule":
        # a granule is 32 / K of the sum: on bounded data it shows only where that exceeds, twice over, what the bound grants a correct
        # kernel (the output rounding and (K - 1) 2^-23 mag); the exact set shows it at every K
        return family == "exact" or 32.0 / c.K > 2.0 * (H + c.K * U23)
    if mutant == "res_before_rbf":
        # against fp64 one rounding fewer is closer, not further: only bits can show it (as gemm_ref's res_before_rounding)
        return family == "exact" and "res" in c.epi
    if mutant == "fp8_scale_next_row":
        return c.fmt == "fp8"
    if mutant in ("nf4_scale_next_block", "nf4_nibble_swap"):
        return c.fmt == "nf4"
    if mutant == "gate_up_swapped":
        return "swiglu" in c.epi
    if mutant == "rope_neighbour_angle":
        return "rope" in c.fused
    if mutant == "vt_pos_minus_1":
        return "rope" in c.fused and c.geom[3] > 0
    if mutant == "pro_no_inner_rbf":
        # the exact family cannot show it (rinv is a power of two there: x rinv is a bf16 number and the inner rounding does nothing), and
        # with same-sign data the (K - 1) 2^-23 mag of the bound exceeds the change: the zero-mean set shows it where the terms cancel
        return "pro" in c.fused and family == "mixed"
    if mutant == "rows_8_15_read_m_and_7":
        return c.M > 8
    raise KeyError(mutant)


def _a32(c, inp, mode):
    A = inp["A"].to(F32)
    if "pro" in c.fused:
        rinv = torch.rsqrt(inp["ssq_in"].sum(0)[:c.M] / float(c.K) + torch.tensor(inp["eps"], dtype=F32))
        p = A * rinv[:, None]
        gw = inp["norm_w"].to(F32)[None, :]
        A = _rb(p * gw) if mode == "pro_no_inner_rbf" else _rb(_rb(p) * gw)
    if mode == "rows_8_15_read_m_and_7":
        A = A.clone()
        A[8:] = A[:c.M - 8]
    return A


def accumulate(c, inp, mode):
    """the fp32 accumulator [M, N] under a summation order or a mutation"""
    A = _a32(c, inp, mode)
    q = inp.get("Wq")
    if mode == "nf4_nibble_swap":
        q = ((q << 4) | (q >> 4)).to(torch.uint8)
    Wv, _ = weights64(c, dict(inp, Wq=q) if q is not None else inp)
    Wv = Wv.to(F32)
    sc = inp["wscale"] if c.fmt != "bf16" else None
    if mode == "fp8_scale_next_row":
        sc = torch.roll(sc, -1, 0)
    if mode == "nf4_scale_next_block":
        sc = torch.roll(sc, -1, 1)
    zero = torch.zeros(c.M, c.N, dtype=F32)
    if mode == "matmul" and c.fmt != "nf4":
        acc = A @ Wv.t()
        return acc if sc is None else acc * sc[None, :]
    Gn = c.K // 32
    ed = slice_edges(c)
    sl = [list(range(ed[s], ed[s + 1])) for s in range(len(ed) - 1)]
    if mode not in ("slices", "drop_granule", "double_slice"):
        sl = [list(range(Gn))]
    filled = [s for s in range(len(sl)) if sl[s]]
    victim = filled[len(filled) // 2]
    dropped = sl[victim][-1] if mode == "drop_granule" else -1

    def gran(g):
        if g == dropped:
            return zero
        return A[:, g * 32:(g + 1) * 32] @ Wv[:, g * 32:(g + 1) * 32].t()

    def chain(gs):
        p = zero
        if c.fmt == "nf4":                                     # blocks of two granules, each block's sum scaled into the running sum
            gs = sorted(gs)
            blocks = [(gs[i], gs[i + 1]) for i in range(0, len(gs), 2)]
            for g0, g1 in (reversed(blocks) if mode == "reverse" else blocks):
                t = gran(g1) + gran(g0) if mode == "reverse" else gran(g0) + gran(g1)
                p = _fma32(t, sc[:, g0 // 2][None, :], p)
            return p
        for g in (reversed(gs) if mode == "reverse" else gs):
            p = p + gran(g)
        return p

    acc = zero
    for s, gs in enumerate(sl):
        p = chain(gs)
        acc = acc + p
        if mode == "double_slice" and s == victim:
            acc = acc + p
    return acc if c.fmt != "fp8" else acc * sc[None, :]


def epilogue_f32(c, inp, acc, mode="matmul"):
    """the rounding sequence of the module docstring on an fp32 accumulator, in fp32 torch -> the output dict ``judge`` takes"""
    od = out_dtype(c)
    M, N = c.M, c.N
    if "swiglu" in c.epi:
        g, u = _split_swiglu(_rb(acc))
        if mode == "gate_up_swapped":
            g, u = u, g
        return {"C": (_rb(g * torch.sigmoid(g)) * u).to(BF)}
    v = _rb(acc)
    if "rope" in c.fused:
        Hh, Hkv, hd, pos = c.geom
        nqk = (Hh + Hkv) * hd
        cs = inp["cos_sin"][pos]
        if mode == "rope_neighbour_angle":
            cs = cs[torch.arange(hd // 2) ^ 1]
        co, si = cs[:, 0].repeat(Hh + Hkv)[None, :], cs[:, 1].repeat(Hh + Hkv)[None, :]
        a, b = v[:, 0:nqk:2], v[:, 1:nqk:2]
        qk = torch.stack([a * co - b * si, a * si + b * co], -1).reshape(M, nqk).to(BF)
        kc = torch.full((M, Hkv, SMAX, hd), SENT, dtype=BF)
        vc = torch.full((M, Hkv, hd, SMAX), SENT, dtype=BF)
        kc[:, :, pos, :] = qk[:, Hh * hd:].reshape(M, Hkv, hd)
        vc[:, :, :, pos - 1 if mode == "vt_pos_minus_1" else pos] = v[:, nqk:].reshape(M, Hkv, hd).to(BF)
        return {"C": qk[:, :Hh * hd].contiguous(), "k_cache": kc, "vt_cache": vc}
    if "res" in c.epi:
        r = inp["res"].to(F32)
        o = _rb(acc + r) if mode == "res_before_rbf" else v + r
    else:
        o = v
    out = {"C": o.to(od)}
    if "ssq" in c.fused:
        hb = _rb(o)
        t = torch.zeros(N // 16, 16, dtype=F32)
        t[:, :M] = (hb * hb).view(M, N // 16, 16).sum(-1).t()
        out["ssq"] = t
    return out


def emu(c, inp, mode):
    """a restatement (RESTATEMENTS) or a mutant (MUTANTS) of the case -> output dict"""
    order = mode if mode in ("matmul", "slices", "reverse", "drop_granule", "double_slice") else "slices" if c.fmt == "nf4" else "matmul"
    pre = mode if mode in ("pro_no_inner_rbf", "rows_8_15_read_m_and_7", "fp8_scale_next_row", "nf4_scale_next_block", "nf4_nibble_swap") else order
    return epilogue_f32(c, inp, accumulate(c, inp, pre), mode)
