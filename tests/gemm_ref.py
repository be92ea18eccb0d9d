"""fp64 references, derived error bounds, input generators and the shape table for the GEMM family of a3vlm_amd/csrc/a3v_gemm.hip and
a3v_strip.hip: a3v_gemm_nt (bf16 with every epilogue it accepts, and the fp32 kernel), a3v_gemm_tn, a3v_gemm_tn_sumsq, a3v_gemm_nn,
a3v_gemm_nt_splitk, a3v_gemm_tn_splitk, a3v_gemm_tn_strip and a3v_splitk_reduce.  The scheme is that of tests/rowops_ref.py and
tests/rowops_fwd_ref.py (whose ``within``, HALF_ULP_BF16, EVAL_F32 and TINY are used here).

Out of scope: the fp8 GEMMs (tests/fp8_base_ref.py states their parity), a3v_gemm_qkv_rope (pinned value for value to a3v_gemm_nt
followed by a3v_rope_kvcache, and the RoPE has fp64 parity in tests/rowops_fwd_ref.py) and the skinny GEMV file a3v_gemv.hip
(tests/gemv_ref.py states its parity in the same scheme).

The rounding sequence (a3vlm_hip.h; gemm_epilogue, splitk_epilogue_kernel and splitk_reduce_kernel perform it in this order; rbf = round
to nearest even to bf16, every other operation one fp32 operation):

    acc  = sum_k A[m, k] W[n, k]                 fp32, any order, over any number of split-K planes summed in fp32
    v    = rbf(acc + bias[n])                    "the bf16 value F.linear returns"; the bias, if any, joins the accumulator first
    v    = rbf(act(v))                           GELU / QUICKGELU
    out  = bf16:    rbf(res + v)                 RESIDUAL (also in place on C); without a residual v itself
           OUT_F32: v (+ res) stored as fp32     no further rounding to bf16
           RES_F32: res + v, res and out fp32
    SWIGLU      out[m, c] = rbf(rbf(silu(g)) u), g = rbf(acc of the gate row), u = rbf(acc of the up row) (16-row blocks interleaved in W)
    SWIGLU_BWD  (d gate, d up) = a3v_swiglu_bwd's expression on (gate, up, rbf(acc)), each rounded once
    a3v_splitk_reduce: out = rnd(rbf(sum_s plane_s)) or rnd(out + rbf(sum_s plane_s)), rnd = the output dtype's rounding
    fp32 kernel: the same without any rbf.

Two input families per table entry.

EXACT: A, W, bias and residual hold integers that bf16 represents (|A|, |W| <= 127; bias and residual a 7-bit integer times 2^0..8),
with K max|A| max|W| + max|bias| + max|res| < 2^24 (``exact_budget_ok``).  Every product and every partial sum is then an integer below
2^24: exact in fp32 whatever the order of the additions and the number of planes, so the accumulator IS the fp64 product and the output
must equal, bit for bit, that product put through the sequence above (``reference``'s ``bits``).  The sums reach the tens of thousands, where
bf16 keeps 8 of ~16 bits: most results need rounding and a quarter of them are round-to-even ties.  A dropped, doubled or misplaced
term and a wrong rounding order (residual added before the rounding, planes rounded before the reduce) all change bits.  The
activation epilogues are not exact (their device functions are not correctly rounded): on exact inputs they are checked with the
bound below.

BOUNDED: bf16-rounded reals, all normal in bf16: ``same`` -- every operand positive (mag = |ref|: the bound is as tight as it can be),
with row scales 2^(i mod 3) and column scales 2^frac(0.381966 j): no two neighbouring outputs agree, and the outputs of a row sweep a
whole binade evenly, so that some lie just above a power of two, where half a bf16 ulp is the full 2^-8 of the value and the bound has no
slack left for a rounding too many; ``mixed`` -- zero-mean with
a power of two from 2^-10 .. 2^10 per row of C and another per column (from K = 2048 on the signs are those of the two halves of K, which
cancel: see ``inputs``).  The bound of an element, in ``within``'s form, is

    |got - ref| <= out_rel |ref| + E + TINY,        E = (K - 1) 2^-23 mag  pushed through the epilogue

where mag = (|A| |W|^T)[m, n] in fp64.  The product of two bf16 values has 16 significant bits and is exact in fp32; only the K - 1
additions round.  2^-23 per addition (a whole ulp of the partial sum, which never exceeds mag) also covers an accumulator that
truncates instead of rounding to nearest: neither kernel guide says which the MFMA does and nobody has measured it here.  Every
further fp32 addition of the epilogue (bias, residual) is one IEEE operation: 2^-24 of its result.  A rounding to bf16 that is
followed by more arithmetic turns an error e of a value v into e + 2^-8 (|v| + e); the last rounding to bf16 is ``out_rel`` = 2^-8 on
|ref| and the factor (1 + 2^-8) on E.  (For the plain epilogue this is 2^-8 |ref| + (1 + 2^-8) (K - 1) 2^-23 mag.)
Activations: an error e of the argument becomes LIP e, LIP = 1.13 >= sup |gelu'| = 1.129, sup |silu'| = sup |quickgelu'| = 1.0998.  The
device functions: gelu_erf_fast is Abramowitz-Stegun 7.1.26 (|erf error| < 1.5e-7, as its comment in a3v_gemm.hip cites) times
|x| / 2, plus a handful of fp32 operations: below EVAL_F32 |x|.  quick_gelu / silu are x rcp(1 + __expf(-a x)): v_rcp_f32 is 1 ulp,
__expf 2 ulp plus the fp32 error of its argument, which is relative to |a x|; the sigmoid's sensitivity to that, s (1 - s) |a x|, never
exceeds 1/e, so the sigmoid is good to a few 2^-24 absolute and the result to EVAL_F32 |x| -- the term rowops_ref.py charges
its SwiGLU, with the same 2^-126 ``underflow`` term where exp overflows.  SWIGLU_BWD is linear in the product: its error is the
product's times |d out / d product|, plus rowops_ref.swiglu_bwd_ref's own EVAL_F32 mag and underflow terms.
a3v_gemm_tn_sumsq: the written slots must sum to the fp64 sum of squares of the STORED fp32 values within (n - 1 + 1) 2^-23 of that
sum (n squares, each rounded once, n - 1 additions, all terms positive); slots beyond a3v_gemm_tn_sumsq_slots keep a sentinel.
The fp32 kernel accumulates with fmaf: K roundings instead of K - 1, no rbf; its GELU is libm erff (a few ulp: EVAL_F32 |x|).

``emu`` restates the arithmetic in fp32 torch in three summation orders (one matmul; 64-wide k-tiles added last to first; S planes
summed in order) and ``MUTANTS`` are five wrong kernels.  tests/test_gemm_ref_cpu.py shows that every restatement stays inside the
bound on every bounded input set and that every mutant leaves it (ratio > 1) on every bounded set it applies to and changes bits on
every exact set: the bound is neither too tight for a correct kernel nor loose enough to hide those errors.

TABLE lists the cases; entries above 2^33 multiply-adds are marked ``subset``: "reference on a row subset" (``ref_rows``: all tail
rows of the dispatch, the first and last row of every 256-row tile row, rows 0..15 and 64 seeded rows).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from rowops_ref import EVAL_F32, F32_MIN_NORMAL, HALF_ULP_BF16, TINY, within, swiglu_bwd_ref  # noqa: F401

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
SENT = -7.0
U23 = 2.0 ** -23
U24 = 2.0 ** -24
LIP = 1.13
BK = 64

EPI = dict(bias=1, gelu=2, quickgelu=4, res=8, swiglu=16, out_f32=32, res_f32=64, swiglu_bwd=128)
TILE = {"128": 1 << 16, "256": 1 << 17, "256pp": 1 << 18, "192pp": 1 << 23}
TILE_ROWS = {"128": 128, "256": 256, "256pp": 256, "192pp": 192}
FAMILIES = ["exact", "same", "mixed"]
MAX_MACS = 2 ** 37
SUBSET_MACS = 2 ** 33
MAX_ENTRIES = 90


class Case(NamedTuple):
    entry: str                 # nt | nt_f32 | tn | tn_sumsq | nn | nt_splitk | tn_splitk | tn_strip | reduce
    M: int                     # rows of the product (tn_strip: R)
    N: int                     # columns of the product (SWIGLU: interleaved rows of W, C has N / 2 columns; SWIGLU_BWD: C has 2 N)
    K: int                     # contracted length (reduce: 0)
    epi: tuple = ()            # of bias gelu quickgelu res inplace swiglu out_f32 res_f32 swiglu_bwd
    tile: Optional[str] = None
    env: tuple = ()            # ((switch, value), ..)
    S: int = 0                 # slices of the split-K entry points / planes of reduce
    acc: int = 0               # split-K entry points and reduce: accumulate into the output
    out: str = "bf16"          # split-K entry points and reduce: output dtype
    subset: bool = False       # "reference on a row subset"

    @property
    def id(self):
        s = f"{self.entry}-{self.M}x{self.N}x{self.K}"
        if self.epi:
            s += "-" + "+".join(self.epi)
        if self.tile:
            s += "-t" + self.tile
        if self.S:
            s += f"-S{self.S}" + ("acc" if self.acc else "") + ("-f32" if self.out == "f32" else "")
        if self.env:
            s += "-" + ",".join(f"{k[4:].lower()}={v}" for k, v in self.env)
        return s

    @property
    def macs(self):
        return self.M * self.N * max(self.K, self.S, 1)

    @property
    def flags(self):
        e = 0
        for name in self.epi:
            e |= EPI.get(name, 0)
        if "inplace" in self.epi:
            e |= EPI["res"]
        return e | (TILE[self.tile] if self.tile else 0)


def _forced(tile):
    t = TILE_ROWS[tile]
    e = {"128": [(), ("bias",), ("res",), ("res_f32",), ("out_f32",)],
         "256": [(), ("bias", "gelu"), ("inplace",), ("bias", "res"), ()],
         "256pp": [("bias", "quickgelu"), ("res",), ("out_f32",), ("inplace",), ("res_f32",)],
         "192pp": [(), ("res",), ("bias",), ("bias", "gelu", "res"), ("res",)]}[tile]
    shapes = [(1, 260, 192), (t - 1, 124, 64), (t, 132, 128), (t + 1, 252, 320), (t + 1, 4, 64)]
    return [Case("nt", M, N, K, epi, tile) for (M, N, K), epi in zip(shapes, e)]


_R192 = (("A3V_GEMM_RING_192", 0),)
TABLE = (
    # ---- direct tile edges of a3v_gemm_nt: M in {1, tile - 1, tile, tile + 1}, N in {4, 124, 132, 252, 260}, K in {64, 128, 192, 320}
    _forced("128") + _forced("256") + _forced("256pp") + _forced("192pp") + [
        Case("nt", 129, 288, 128, ("swiglu",), "128"), Case("nt", 257, 288, 192, ("swiglu",), "256pp"),
        Case("nt", 129, 136, 128, ("swiglu_bwd",), "128"), Case("nt", 257, 136, 192, ("swiglu_bwd",), "256pp"),
        Case("nt", 193, 264, 64, ("swiglu_bwd",), "192pp"),
        Case("nt_f32", 1, 4, 16), Case("nt_f32", 65, 68, 48, ("bias", "res")), Case("nt_f32", 130, 200, 640, ("bias", "gelu")),
        # ---- persistent ring, every form: more than 256 tiles with one k-tile, and with three (a block walks several tiles)
        Case("nt", 4360, 4096, 64, (), "256pp"), Case("nt", 4360, 4096, 192, ("res",), "256pp"),
        Case("nt", 4360, 4096, 64, ("bias",), "256pp"), Case("nt", 4360, 4096, 192, ("bias", "res"), "256pp"),
        Case("nt", 4360, 4096, 64, ("res",), "192pp"), Case("nt", 4360, 4096, 192, (), "192pp"),
        Case("nt", 4360, 4096, 64, ("bias", "res"), "192pp"), Case("nt", 4360, 4096, 192, ("bias",), "192pp"),
        # ---- dispatch outcomes at their smallest shapes (a3v_gemm_plan, 256 CUs, 96 MiB workspace); multi-step ones with a residual
        Case("nt", 100, 132, 64),                                                             # nt_small
        Case("nt", 520, 520, 1536, ("res",)),                                                 # whole-problem ring split, S = 3
        Case("nt", 3080, 4000, 64, ("bias",)), Case("nt", 8456, 1024, 64),                    # RING_PRE; RING_192
        Case("nt", 4360, 4000, 4096, ("res",), subset=True),                                  # RING + ring split tail (S = 8) + REDUCE
        Case("nt", 4360, 4000, 384, ("res_f32",), env=_R192 + (("A3V_GEMM_TAIL_SLICES", 3),)),     # the same, S = 3, fp32 stream
        Case("nt", 4360, 4000, 1024, ("res",), env=_R192 + (("A3V_GEMM_RING_TAIL", 0),), subset=True),   # RING + 128-tile split tail (S = 2) + REDUCE
        Case("nt", 4360, 4000, 384, ("bias", "res"), env=_R192),                              # RING_PRE + plain 128-tile tail
        # ---- TN: K in {8, 63, 64, 65, 130}, M % 8 == 0, ragged N
        Case("tn", 264, 260, 8), Case("tn", 248, 132, 63, ("res",)), Case("tn", 256, 252, 64, ("out_f32",)),
        Case("tn", 264, 4, 65, ("res_f32",)), Case("tn", 8, 260, 130, ("inplace",)),
        Case("tn_sumsq", 264, 260, 130, ("out_f32",)), Case("tn_sumsq", 520, 516, 65, ("res_f32",)),
        Case("tn", 4360, 4000, 2048, ("res",), subset=True),                                  # big rows + split tail (S = 2) + REDUCE
        Case("tn_sumsq", 4360, 4000, 2048, ("res_f32",), subset=True),
        # ---- NN: N % 8 == 0
        Case("nn", 1, 264, 192), Case("nn", 255, 8, 64, ("res",)), Case("nn", 256, 136, 128, ("res_f32",)),
        Case("nn", 257, 248, 320, ("out_f32",)), Case("nn", 257, 136, 128, ("swiglu_bwd",)),
        Case("nn", 4360, 4000, 2048, ("res",), subset=True),
        # ---- split-K forms: S = 1, S = k-tiles, S = 3 and 7 of 7 k-tiles; nt_splitk: the 128 x 128 kernel, the 64-row and the 256-row
        #      streaming blocks (S ceil(M / 256) = 245: inside half-to-all of 256; 105 and 21: outside)
        Case("nt_splitk", 300, 64, 64, S=1), Case("nt_splitk", 130, 96, 448, S=3, out="f32"), Case("nt_splitk", 600, 64, 128, S=2, acc=1, out="f32"),
        Case("nt_splitk", 520, 48, 448, S=7), Case("nt_splitk", 8728, 64, 448, S=7), Case("nt_splitk", 8728, 64, 448, S=3, acc=1),
        Case("tn_splitk", 520, 64, 64, S=1), Case("tn_splitk", 64, 260, 130, S=3, out="f32"), Case("tn_splitk", 264, 48, 448, S=3, acc=1, out="f32"),
        Case("tn_splitk", 128, 64, 440, S=7),
        Case("tn_strip", 8, 132, 130, S=3), Case("tn_strip", 16, 384, 448, S=7, out="f32"), Case("tn_strip", 48, 260, 448, S=3, acc=1, out="f32"),
        Case("tn_strip", 64, 128, 64, S=1),
        Case("reduce", 37, 132, 0, S=5), Case("reduce", 37, 132, 0, S=5, acc=1), Case("reduce", 300, 4, 0, S=1, out="f32"),
        Case("reduce", 37, 132, 0, S=7, acc=1, out="f32"),
    ])
BY_ID = {c.id: c for c in TABLE}
assert len(BY_ID) == len(TABLE)


# ------------------------------------------------------------------ layout of a case
def is_act(c):
    return bool(set(c.epi) & {"gelu", "quickgelu", "swiglu", "swiglu_bwd"})


def out_cols(c):
    return c.N // 2 if "swiglu" in c.epi else 2 * c.N if "swiglu_bwd" in c.epi else c.N


def out_dtype(c):
    if c.entry == "nt_f32":
        return F32
    if c.entry in ("nt_splitk", "tn_splitk", "tn_strip", "reduce"):
        return F32 if c.out == "f32" else BF
    return F32 if set(c.epi) & {"out_f32", "res_f32"} else BF


def res_dtype(c):
    return F32 if ("res_f32" in c.epi or c.entry == "nt_f32") else BF


def has_res(c):
    return bool(set(c.epi) & {"res", "inplace", "res_f32"}) or c.acc == 1


def slices(c):
    """planes of the restatements and mutants: the case's own S, else 2"""
    return c.S if c.S else 2


def ktiles(c):
    return c.S if c.entry == "reduce" else (c.K + BK - 1) // BK


def ref_rows(c, force=False):
    """rows of C the reference is computed for: all of them, or for ``subset`` entries (``force``: any entry) the tail rows of the dispatch (beyond whole
    rounds of 256 tiles of 256 rows; at least the last tile row), the first and last row of every 256-row tile row, rows 0..15 and 64
    seeded rows"""
    if not (c.subset or force):
        return torch.arange(c.M)
    tn = (c.N + 255) // 256
    tm = c.M // 256 if c.entry == "nt" else (c.M + 255) // 256
    m_big = (tm * tn // 256) * 256 // tn * 256
    if m_big <= 0 or m_big >= c.M:
        m_big = (c.M - 1) // 256 * 256
    rows = set(range(m_big, c.M)) | set(range(16))
    for t in range(0, c.M, 256):
        rows |= {t, min(t + 255, c.M - 1)}
    g = torch.Generator().manual_seed(c.M * 7 + c.N)
    rows |= set(torch.randint(0, c.M, (64,), generator=g).tolist())
    return torch.tensor(sorted(rows))


# ------------------------------------------------------------------ inputs
def _seed(c, family):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id + family)) * 2654435761) % (2 ** 31)


def exact_limits(c):
    """(max |A| = max |W|, max |bias|, max |res|): K a^2 + bias + res < 2^24"""
    k = max(c.K, 1)
    a = min(127, int(math.isqrt((2 ** 24 - 2 ** 17) // k)))
    return a, 127 * 256, 127 * 256


def exact_budget_ok(c, inp):
    a = float(inp["A"].abs().max()) * float(inp["W"].abs().max()) * max(c.K, 1) if c.entry != "reduce" else float(inp["planes"].abs().sum(0).max())
    b = float(inp["bias"].abs().max()) if inp.get("bias") is not None else 0.0
    r = float(inp["res"].abs().max()) if inp.get("res") is not None else 0.0
    return a + b + r < 2 ** 24


def _int_sparse(shape, g):
    """7-bit signed integers times 2^0..8: bf16 holds them exactly"""
    return (torch.randint(-127, 128, shape, generator=g) * 2 ** torch.randint(0, 9, shape, generator=g)).double()


def inputs(c: Case, family: str):
    """CPU tensors of the case in the dtypes the entry point takes: A [M, K] (tn kinds: At [K, M]), W [N, K] (tn kinds / nn: Wt [K, N]),
    bias [N], res [M, out columns] (SWIGLU_BWD: gu [M, 2 N]; accumulating split-K forms: the initial output), planes [S, M, N] (reduce)."""
    g = torch.Generator().manual_seed(_seed(c, family))
    M, N, K = c.M, c.N, c.K
    f32 = c.entry == "nt_f32"
    opd = F32 if f32 else BF
    d = {}
    if family == "exact":
        a, bmax, rmax = exact_limits(c)
        rs = cs = None
        A = torch.randint(-a, a + 1, (M, K), generator=g).double() if K else None
        W = torch.randint(-a, a + 1, (N, K), generator=g).double() if K else None
    else:
        i, j = torch.arange(M), torch.arange(N)
        if family == "same":
            rs, cs = 2.0 ** (i % 3).double(), 2.0 ** ((j.double() * 0.381966) % 1.0)
            gen = lambda *s: torch.rand(*s, generator=g).double() + 0.25          # noqa: E731
        else:
            rs = 2.0 ** torch.randint(-10, 11, (M,), generator=g).double()
            cs = 2.0 ** torch.randint(-10, 11, (N,), generator=g).double()
            gen = lambda *s: torch.randn(*s, generator=g).double()              # noqa: E731
        if is_act(c) and family == "mixed":          # activations: half the rows and columns (SWIGLU: every column, gate and up rows
            rs[::2] = 1.0                            # pair up) at unit scale, so that the curved part of the function is hit
            cs[::1 if "swiglu" in c.epi else 2] = 1.0
        A = gen(M, K) * rs[:, None] if K else None
        W = gen(N, K) * cs[:, None] if K else None
        if family == "mixed" and K >= 2048:          # long K: zero-mean terms would let (K - 1) 2^-23 mag swamp half a bf16 ulp of a plane; here the
            A, W = A.abs(), W.abs()                  # two halves of K cancel instead (|plane| ~ mag / 2, |ref| ~ mag / sqrt(K)), as hard a case as
            W[:, K // 2:] *= -1.0                    # zero-mean data for a correct kernel and a visible one for a plane rounded too early
        if is_act(c):                                # ... and a pre-activation of order one at unit scale
            A = A / (math.sqrt(K) if family == "mixed" else K)
    if c.entry == "reduce":
        S = c.S
        if family == "exact":
            d["planes"] = torch.randint(-(2 ** 20), 2 ** 20, (S, M, N), generator=g).float()
        else:
            p = gen(S, M, N)
            if family == "mixed":                    # planes that cancel in pairs, as the slices of a zero-mean product do
                common = 16.0 * gen(M, N)
                for s in range(S - S % 2):
                    p[s] += common if s % 2 == 0 else -common
            d["planes"] = (p * rs[None, :, None] * cs[None, None, :]).float()
        typ = float((d["planes"].double().sum(0) / (rs[:, None] * cs[None, :])).abs().mean()) if family != "exact" else 1.0
    else:
        d["A"] = (A.t().contiguous() if c.entry in ("tn", "tn_sumsq", "tn_splitk", "tn_strip") else A).to(opd)
        d["W"] = (W.t().contiguous() if c.entry in ("tn", "tn_sumsq", "tn_splitk", "tn_strip", "nn") else W).to(opd)
        typ = 1.0 if (is_act(c) and family != "exact") else K if family == "same" else math.sqrt(K)
    scale2 = (lambda: rs[:, None] * cs[None, :] * typ)
    if "bias" in c.epi:
        d["bias"] = (_int_sparse((N,), g) if family == "exact" else gen(N) * cs * typ).to(opd)
    if "swiglu_bwd" in c.epi:
        d["res"] = (2.0 * torch.randn(M, 2 * N, generator=g)).to(BF)
    elif has_res(c):
        if family == "exact":
            r = _int_sparse((M, out_cols(c)), g)
            if c.entry == "reduce":
                r = r * 16
        else:
            r = gen(M, out_cols(c)) * scale2()
        d["res"] = r.to(out_dtype(c) if c.acc else res_dtype(c))
    return d


def logical(c, inp, rows=None):
    """(A [rows, K], W [N, K]) in fp64, whatever the entry point's layout"""
    A, W = inp["A"], inp["W"]
    if c.entry in ("tn", "tn_sumsq", "tn_splitk", "tn_strip"):
        A = A.t()
    if c.entry in ("tn", "tn_sumsq", "tn_splitk", "tn_strip", "nn"):
        W = W.t()
    if rows is not None:
        A = A[rows]
    return A.to(F64), W.to(F64)


# ------------------------------------------------------------------ fp64 reference and bound
def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _quickgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def _split_swiglu(p):
    """interleaved 16-row blocks of W -> (gate, up) columns of the product"""
    r, n = p.shape
    q = p.reshape(r, n // 32, 2, 16)
    return q[:, :, 0].reshape(r, n // 2), q[:, :, 1].reshape(r, n // 2)


def product64(c, inp, rows=None):
    """(prod, mag) in fp64 on ``rows``: the accumulator's value and its summed |terms|"""
    if c.entry == "reduce":
        p = inp["planes"].to(F64)
        p = p if rows is None else p[:, rows]
        return p.sum(0), p.abs().sum(0)
    A, W = logical(c, inp, rows)
    return A @ W.t(), A.abs() @ W.abs().t()


def n_roundings(c):
    """roundings of the accumulation: K - 1 additions (fmaf in the fp32 kernel: K; planes: S - 1)"""
    return c.S - 1 if c.entry == "reduce" else c.K if c.entry == "nt_f32" else c.K - 1


def reference(c: Case, inp, rows=None):
    """-> dict(ref fp64, E absolute error allowance beyond the output rounding, rel the output rounding, uf underflow sensitivity or
    None, bits the exact expected output or None (exact inputs, no activation))"""
    sub = (lambda t: t if (rows is None or t is None) else t[rows])
    prod, mag = product64(c, inp, rows)
    f32k = c.entry == "nt_f32"
    H = 0.0 if f32k else HALF_ULP_BF16
    rnd = (lambda t: t) if f32k else (lambda t: t.to(F32).to(BF).to(F64))
    od = out_dtype(c)
    E = n_roundings(c) * U23 * mag
    v, bits, uf = prod, prod, None
    if "bias" in c.epi:
        b = inp["bias"].to(F64)[None, :]
        v, bits = v + b, bits + b
        E = E + U24 * (v.abs() + E)
    res = sub(inp.get("res"))
    res64 = res.to(F64) if res is not None else None
    if "swiglu" in c.epi:
        g, u = _split_swiglu(v)
        Eg, Eu = _split_swiglu(E)
        Eg, Eu = Eg + H * (g.abs() + Eg), Eu + H * (u.abs() + Eu)
        s = g * torch.sigmoid(g)
        Es = LIP * Eg + EVAL_F32 * g.abs() + H * (s.abs() + LIP * Eg)
        ref = s * u
        E = (Es * (u.abs() + Eu) + s.abs() * Eu) * (1.0 + U24) + U24 * ref.abs()
        return dict(ref=ref, E=E * (1.0 + H), rel=H, uf=(g * u).abs() + Eu * g.abs(), bits=None)
    if "swiglu_bwd" in c.epi:
        N = c.N
        g, u = res64[:, :N], res64[:, N:2 * N]
        E = E + H * (v.abs() + E)                                   # rbf(acc) = d(act)
        dg, mag_dg, uf_dg, du, mag_du, uf_du = swiglu_bwd_ref(g, u, v)
        sig, nsig = torch.sigmoid(g), torch.sigmoid(-g)
        sens_g, sens_u = u.abs() * sig * (1.0 + g * nsig).abs(), g.abs() * sig          # |d out / d product|
        ref = torch.cat([dg, du], 1)
        Eo = torch.cat([E * sens_g + EVAL_F32 * (mag_dg + E * sens_g), E * sens_u + EVAL_F32 * (mag_du + E * sens_u)], 1)
        ufo = torch.cat([uf_dg + E * (u.abs() * (1 + g.abs())), uf_du + E * g.abs()], 1)
        return dict(ref=ref, E=Eo * (1.0 + H), rel=H, uf=ufo, bits=None)
    more = bool(set(c.epi) & {"gelu", "quickgelu"}) or res64 is not None
    final_is_rbf = not more and not f32k                      # the rbf of the accumulator is the output rounding itself
    if not final_is_rbf and not f32k:
        E = E + H * (v.abs() + E)
    bits = rnd(bits)
    v_exact = bits                                            # the exact chain continues from the rounded value
    if "gelu" in c.epi or "quickgelu" in c.epi:
        fn = _gelu64 if "gelu" in c.epi else _quickgelu64
        E = LIP * E + EVAL_F32 * v.abs()
        v = fn(v)
        bits = None
        if res64 is not None and not f32k:
            E = E + H * (v.abs() + E)
    if res64 is not None:
        v = v + res64
        E = E + U24 * (v.abs() + E)
        if bits is not None:
            bits = v_exact + res64
    if od == BF:
        return dict(ref=v, E=E * (1.0 + H), rel=H, uf=None, bits=None if bits is None else bits.to(F32).to(BF))
    # fp32 outputs: a value that is only rbf'd (OUT_F32 without a residual, a split-K sum stored to fp32) carries the bf16 rounding
    rel = H if final_is_rbf else 0.0
    if final_is_rbf:
        E = E * (1.0 + H)
    return dict(ref=v, E=E, rel=rel, uf=uf, bits=None if bits is None else bits.to(F32))


def ratio(got, r, od):
    """worst |got - ref| / bound of ``reference``'s result, through rowops_ref.within"""
    return within(got, r["ref"], r["E"] / EVAL_F32, od, rel=r["rel"], underflow=r["uf"])


def sumsq_ratio(slots_sum: float, stored) -> float:
    """|sum of the written slots - fp64 sum of squares of the stored fp32 values| over its bound"""
    s = float((stored.to(F64) ** 2).sum())
    n = stored.numel()
    return abs(float(slots_sum) - s) / (n * U23 * s + 2.0 ** -149)


# ------------------------------------------------------------------ fp32 restatements and mutants (CPU)
def _rb(t):
    return t.to(BF).to(F32)


def _tiles(c, inp, rows):
    """fp32 partial products per 64-wide k-tile (reduce: per plane), as a generator"""
    if c.entry == "reduce":
        for s in range(c.S):
            yield inp["planes"][s] if rows is None else inp["planes"][s][rows]
        return
    A, W = logical(c, inp, rows)
    A, W = A.to(F32), W.to(F32)
    for k0 in range(0, c.K, BK):
        yield A[:, k0:k0 + BK] @ W[:, k0:k0 + BK].t()


def _slice_edges(n_tiles, S):
    return [n_tiles * s // S for s in range(S + 1)]


def accumulate(c, inp, rows, mode):
    """the fp32 accumulator under a summation order or a mutation"""
    if mode == "matmul" and c.entry != "reduce":
        A, W = logical(c, inp, rows)
        return A.to(F32) @ W.to(F32).t()
    tiles = list(_tiles(c, inp, rows))
    nt, S = len(tiles), min(slices(c), len(tiles))
    if mode in ("matmul", "forward"):
        acc = torch.zeros_like(tiles[0])
        for t in tiles:
            acc = acc + t
        return acc
    if mode == "reverse":
        acc = torch.zeros_like(tiles[0])
        for t in reversed(tiles):
            acc = acc + t
        return acc
    if mode == "ktile_bf16":
        acc = torch.zeros_like(tiles[0])
        for t in tiles:
            acc = _rb(acc + t)
        return acc
    ed = _slice_edges(nt, S)
    planes = []
    for s in range(S):
        p = torch.zeros_like(tiles[0])
        last = ed[s + 1] - (1 if (mode == "drop_tile" and s == S // 2) else 0)
        for t in tiles[ed[s]:last]:
            p = p + t
        planes.append(_rb(p) if mode == "planes_bf16" else p)
    acc = torch.zeros_like(tiles[0])
    for p in planes:
        acc = acc + p
    return acc


def epilogue_f32(c, inp, acc, rows=None, res_first=False):
    """the rounding sequence of the module docstring on an fp32 accumulator, in fp32 torch -> the output in its dtype"""
    sub = (lambda t: t if (rows is None or t is None) else t[rows])
    f32k = c.entry == "nt_f32"
    rb = (lambda t: t) if f32k else _rb
    od = out_dtype(c)
    v = acc
    res = sub(inp.get("res"))
    if "bias" in c.epi:
        v = v + inp["bias"].to(F32)[None, :]
    if "swiglu" in c.epi:
        g, u = _split_swiglu(rb(v))
        return (rb(g * torch.sigmoid(g)) * u).to(od)
    if "swiglu_bwd" in c.epi:
        N = c.N
        g, u, da = res[:, :N].float(), res[:, N:2 * N].float(), rb(v)
        sig = 1.0 / (1.0 + torch.exp(-g))
        return torch.cat([da * u * (sig * (1.0 + g * (1.0 - sig))), da * (g * sig)], 1).to(od)
    if res_first and res is not None:                          # mutant: the residual joins before the rounding
        return rb(v + res.to(F32)).to(od)
    v = rb(v)
    if "gelu" in c.epi:
        v = rb(0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440)))
    elif "quickgelu" in c.epi:
        v = rb(v * torch.sigmoid(1.702 * v))
    if res is not None:
        v = res.to(F32) + v
    return v.to(od)


RESTATEMENTS = ["matmul", "reverse", "planes"]
MUTANTS = ["ktile_bf16", "planes_bf16", "drop_tile", "transpose_block", "res_before_rounding"]


def mutant_applies(c, mutant, family):
    if mutant in ("ktile_bf16", "planes_bf16"):
        # one rounding too many: needs two k-tiles and a bf16 kernel.  Behind a non-linear activation the bound holds three or four
        # roundings to bf16 and same-sign data cannot show a fifth (nothing cancels: the extra half ulp stays inside the sum of the
        # others' worst cases); the mixed and the exact set of the same case show it through the cancelling partial sums.
        nonlinear = bool(set(c.epi) & {"gelu", "quickgelu", "swiglu"})
        return ktiles(c) >= 2 and c.entry != "nt_f32" and not (nonlinear and family == "same")
    if mutant == "drop_tile":
        return True
    if mutant == "transpose_block":
        return c.M >= 16 and out_cols(c) >= 16
    if mutant == "res_before_rounding":
        return family == "exact" and res_dtype(c) == BF and bool(set(c.epi) & {"res", "inplace"}) and not is_act(c)
    raise KeyError(mutant)


def emu(c, inp, mode, rows=None):
    """a restatement (RESTATEMENTS) or a mutant (MUTANTS) of the case on ``rows`` -> output tensor"""
    if mode == "transpose_block":
        out = epilogue_f32(c, inp, accumulate(c, inp, rows, "matmul"), rows).clone()
        out[:16, :16] = out[:16, :16].t().clone()
        return out
    if mode == "res_before_rounding":
        return epilogue_f32(c, inp, accumulate(c, inp, rows, "matmul"), rows, res_first=True)
    return epilogue_f32(c, inp, accumulate(c, inp, rows, mode), rows)
