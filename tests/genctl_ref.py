"""Restatement of the generation controls (include/a3vlm_hip.h, "Generation controls"; a3v_genctl.hip).  Test infrastructure only.

Seen set: one bitmap per cache row, uint32 [R, words_per_row]; token t is bit t & 31 of word t >> 5.  It holds the row's prompt text
tokens and every token generated so far (HF RepetitionPenaltyLogitsProcessor: the whole input_ids); ids outside [0, V) are ignored.
Penalty p > 0 on the raw fp32 logits z:  z / p if seen and z > 0;  z * p if seen and z <= 0;  z otherwise -- a true fp32 division,
before temperature and top-p; greedy = first-index argmax of the result.
Log-prob: lp = z[tok] - logsumexp(z) on the RAW logits at temperature 1, fp32, max-subtracted; sequence score = fp64 sum of the kept
tokens' lp on the host.

The bound of the device logsumexp (``lse_bound``), derived from the kernel's reduction shape (header comment), u = 2^-24:
  The row's exact value is lse = M + log S, S = sum_i exp(x_i - M) >= 1.  The kernel forms S as a sum of non-negative terms, so
  relative errors of the terms bound the relative error of S.  One term x_i goes through
    1. its own exponential: expf is good to 1 ulp = 2 u relative; the ARGUMENTS of this exponential and of every rescale factor it is
       later multiplied by are fp32 differences, each rounded (u relative to itself); they are all <= 0 and telescope to x_i - M, so
       together they move the term by at most u d_i relative, d_i = M - x_i.  Weighted by the terms that is u D, D = sum_i p_i d_i
       (p = softmax; computed here in fp64 from the inputs -- it is the row's entropy-like spread, a few units for N(0, 4) rows);
    2. summation depth: 3 additions inside its vector, then per fold of the owning thread one rescale (exp 2 u + multiply u) and one
       addition (u) -- k folds, k = the number of vectors (plus tail elements) a thread owns, ceil(ceil(V / 4) / 1024) + 1 at most
       for the 16-byte walk and ceil(V / 1024) for the element walk of an unaligned row, the larger is taken --, the wave's rescale
       (3 u) and 6 butterfly additions, the block's rescale (3 u) and 16 additions:  (4 k + 3 + 3 + 6 + 3 + 16) u = (4 k + 31) u;
    with the 2 u of its own exponential:  |dS| / S <= (4 k + 33 + D) u, times 1.01 for the second-order products.
  3. the final log and add: logf is good to 1 ulp of its result, 2 u |log S|; d(log S) = dS / S; the addition M + log S rounds once,
     u |lse|.
  bound = 1.01 (4 k + 33 + D) u + 2 u |log S| + u |lse|.   (Terms below 2^-126 are flushed or denormal: an absolute 2^-126 V, nothing.)
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

U32 = 2.0 ** -24


def words(V: int) -> int:
    return (V + 31) // 32


def seen_bitmap(rows: Sequence[Sequence[int]], V: int, words_per_row: Optional[int] = None, start=None) -> torch.Tensor:
    """int64 [R, words_per_row] holding the uint32 words (compare with the device's int32 storage & 0xffffffff)."""
    wpr = words(V) if words_per_row is None else words_per_row
    bm = torch.zeros((len(rows), wpr), dtype=torch.int64) if start is None else start.clone()
    for r, ids in enumerate(rows):
        for t in ids:
            if 0 <= t < V:
                bm[r, t >> 5] |= 1 << (t & 31)
    return bm


def as_u32(t: torch.Tensor) -> torch.Tensor:
    """The device's int32 storage as the uint32 words it holds (int64)."""
    return t.cpu().to(torch.int64) & 0xFFFFFFFF


def seen_mask(bm: torch.Tensor, V: int) -> torch.Tensor:
    """bool [R, V] of a bitmap."""
    t = torch.arange(V)
    return ((bm[:, t >> 5] >> (t & 31)) & 1).bool()


def penalise(z: torch.Tensor, seen: torch.Tensor, p: float) -> torch.Tensor:
    """fp32 [.., V], bool seen: the rule in torch fp32 (what HF's processor computes)."""
    assert z.dtype == torch.float32
    pt = torch.tensor(p, dtype=torch.float32)
    return torch.where(seen, torch.where(z > 0, z / pt, z * pt), z)


def lse32(z: torch.Tensor) -> torch.Tensor:
    """fp32 max-subtracted logsumexp of the rows of z (the restated form; the device differs from it in summation order only)."""
    assert z.dtype == torch.float32
    m = z.max(dim=-1, keepdim=True).values
    m = torch.where(m.isinf(), torch.zeros_like(m), m)
    return (m + (z - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(-1)


def logprob32(z: torch.Tensor, tok: torch.Tensor, lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lp = z[tok] - lse, one fp32 subtraction (lse: the given fp32 values, default the restated ones)."""
    lse = lse32(z) if lse is None else lse
    return z.gather(-1, tok.reshape(-1, 1)).squeeze(-1) - lse


def lse64(z: torch.Tensor) -> torch.Tensor:
    return torch.logsumexp(z.double(), dim=-1)


def lse_bound(z: torch.Tensor) -> torch.Tensor:
    """Per row of the fp32 logits z [B, V] (finite maximum): the bound of |device lse - fp64 lse| derived in the module docstring."""
    V = z.shape[-1]
    x = z.double()
    M = x.max(dim=-1, keepdim=True).values
    d = M - x
    e = torch.exp(-d)
    S = e.sum(-1)
    D = (e * torch.where(d.isinf(), torch.zeros_like(d), d)).sum(-1) / S
    k = max(math.ceil(math.ceil(V / 4) / 1024) + 1, math.ceil(V / 1024))
    lse = M.squeeze(-1) + S.log()
    return 1.01 * (4 * k + 33 + D) * U32 + 2 * U32 * S.log().abs() + U32 * lse.abs()


def generate_record(logits, lse, tokens, seen_bm, logprob, V, *, col=0, cur=None, stopped_before=None, idx=0, prompt_len=None):
    """a3v_generate_record on CPU tensors, in place: logits fp32 [B, V], lse fp32 [B], tokens int64 [B, W], seen_bm int64 words [B, wpr]
    or None, logprob fp32 [B, L] or None."""
    B, W = tokens.shape
    for b in range(B):
        if stopped_before is not None and bool(stopped_before[b]):
            continue
        c = int(cur[b]) - 1 if cur is not None else col
        if c < 0 or c >= W:
            continue
        g = c - int(prompt_len[b]) if prompt_len is not None else idx
        if g < 0:
            continue
        t = int(tokens[b, c])
        if t < 0 or t >= V:
            continue
        if logprob is not None and g < logprob.shape[1]:
            logprob[b, g] = logits[b, t] - lse[b]              # fp32 tensors: one fp32 subtraction
        if seen_bm is not None:
            seen_bm[b, t >> 5] |= 1 << (t & 31)


def oracle_replay(ref_cpu, dec, prompt_tokens: List[List[int]], max_gen_len: int, eos_id: int, penalty: float = 1.0, extra_seen=None):
    """oracle/ref_cpu.py generate_greedy on a batch of prompts with the rule applied on the CPU: the seen set of a row is its prompt
    plus what it generated (a teacher-forced position contributes the prompt token it already holds).  Returns the generated id
    lists and, per row, the fp64 log-softmax of the RAW logits at every kept token.  ``extra_seen``: ids that are in every row's seen
    set from the start (what a refilled cache row would inherit if its bitmap were not cleared)."""
    V = dec.args.vocab_size
    start = min(len(t) for t in prompt_tokens)
    seen = [set(t) | set(extra_seen or ()) for t in prompt_tokens]
    lps = [dict() for _ in prompt_tokens]

    def sampler(step, logits):
        z = logits.float()
        mask = torch.zeros_like(z, dtype=torch.bool)
        for b, s in enumerate(seen):
            mask[b, [t for t in s if 0 <= t < V]] = True
        nxt = torch.argmax(penalise(z, mask, penalty), dim=-1)
        ls = torch.log_softmax(z.double(), dim=-1)
        for b in range(z.shape[0]):
            g = start + step - len(prompt_tokens[b])
            if g >= 0:                                          # not teacher-forced: this is the row's token
                t = int(nxt[b])
                seen[b].add(t)
                lps[b][g] = float(ls[b, t])
        return nxt

    _, outs = ref_cpu.generate_greedy(dec, prompt_tokens, max_gen_len=max_gen_len, eos_id=eos_id, sampler=sampler)
    return outs, [[lp[g] for g in range(len(o))] for lp, o in zip(lps, outs)]
