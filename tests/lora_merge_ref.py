"""fp64 restatement of the LoRA merge (include/a3vlm_hip.h, a3v_lora_merge) and a generator of inputs on which it is EXACT.

    out[n,k] = round_to_dtype( base[n,k] + sum_r B[n,r] * A[r,k] )        (fp32 accumulation, one rounding)

Exact inputs: B and A entries are integers in [-4, 4] times 2^-3, the base is bf16 values that are multiples of 2^-6 in [-4, 4].
Every product is a multiple of 2^-6 of magnitude <= 1/4, every partial sum over R <= 256 terms plus the base a multiple of 2^-6 of
magnitude <= 68: at most 13 significant bits, so every product and every partial sum is exact in fp32 IN ANY ORDER and the only rounding
of a correct kernel is the final one to bf16.  A kernel that rounds twice (bf16(acc) + base) differs on these inputs wherever
|acc| >= 4 (a bf16 then no longer holds a multiple of 2^-6), which the sums over R = 256 terms reach on a few percent of the elements.
"""
from __future__ import annotations

import torch


def merge_ref64(base: torch.Tensor, B: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """fp64 [N, K]: base + B . A (the value the kernel rounds once)"""
    return base.double() + B.double() @ A.double()


def abs_terms64(base: torch.Tensor, B: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """|base| + sum_r |B||A| in fp64: the magnitude the fp32 accumulation error scales with"""
    return base.double().abs() + B.double().abs() @ A.double().abs()


def exact_inputs(N: int, K: int, R: int, seed: int = 0):
    """(base [N, K], B [N, R], A [R, K]) as bf16 CPU tensors, exact in the sense of the module docstring"""
    g = torch.Generator().manual_seed(seed)
    B = torch.randint(-4, 5, (N, R), generator=g).float() * 2.0 ** -3
    A = torch.randint(-4, 5, (R, K), generator=g).float() * 2.0 ** -3
    base = torch.randint(-256, 257, (N, K), generator=g).float() * 2.0 ** -6
    out = tuple(t.to(torch.bfloat16) for t in (base, B, A))
    assert all(torch.equal(o.float(), t) for o, t in zip(out, (base, B, A)))      # the values ARE bf16 values
    return out


def random_inputs(N: int, K: int, R: int, dtype: torch.dtype, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    B = (torch.randn(N, R, generator=g) * 0.05).to(dtype)
    A = (torch.randn(R, K, generator=g) * 0.05).to(dtype)
    return base, B, A
