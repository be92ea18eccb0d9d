"""Device state of the opt-in generation controls of ``MetaModel.generate`` / ``generate_many`` / ``stream_generate``: the seen-token
bitmap of the repetition penalty and the per-token log-probabilities (include/a3vlm_hip.h, "Generation controls").

Made only when ``repetition_penalty != 1`` or ``return_logprobs``: with the defaults nothing here is allocated or launched.  Per
step it adds ``a3v_logits_prepare`` in front of the sampler / step kernel and ``a3v_generate_record`` behind it, no host-visible op."""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import ops


def check_penalty(repetition_penalty: float) -> float:
    p = float(repetition_penalty)
    if not p > 0:
        raise ValueError(f"repetition_penalty must be > 0 (1.0 = off), got {repetition_penalty}")
    return p


def check_filters(top_k: int, min_p: float):
    """The sampler's two opt-in filters: ``top_k`` an integer >= 0 (0 = off), ``min_p`` in [0, 1] (0 = off)."""
    if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k}")
    m = float(min_p)
    if not 0.0 <= m <= 1.0:
        raise ValueError(f"min_p must be in [0, 1] (0 = off), got {min_p}")
    return int(top_k), m


def wanted(repetition_penalty: float, return_logprobs: bool) -> bool:
    return check_penalty(repetition_penalty) != 1.0 or bool(return_logprobs)


def score(logprobs: List[float]) -> dict:
    """The score record of one answer: the kept tokens' log-probs and their fp64 sum."""
    return {"logprobs": logprobs, "sum": float(sum(logprobs))}


class GenControls:
    """``rows`` cache rows, vocabulary ``V``, at most ``max_new`` generated tokens per row."""

    def __init__(self, rows: int, V: int, max_new: int, repetition_penalty: float, return_logprobs: bool, device):
        self.V, self.penalty = V, check_penalty(repetition_penalty)
        pen = self.penalty != 1.0
        self.seen = torch.zeros((rows, (V + 31) // 32), dtype=torch.int32, device=device) if pen else None
        self.out = torch.empty((rows, V), dtype=torch.float32, device=device) if pen else None
        self.lse = torch.empty(rows, dtype=torch.float32, device=device) if return_logprobs else None
        self.lp = torch.zeros((rows, max(max_new, 1)), dtype=torch.float32, device=device) if return_logprobs else None
        self.prompt_len = torch.zeros(rows, dtype=torch.int32, device=device)
        self.row_ids = torch.arange(rows, dtype=torch.int32, device=device)
        self.stopped_before = torch.zeros(rows, dtype=torch.bool, device=device)

    def mark_prompts(self, tokens: torch.Tensor, row: Optional[int] = None) -> None:
        """The prompt tokens of every row (``row``: of that one row, its bitmap cleared first) enter the seen set;
        ``self.prompt_len`` is already set."""
        if self.seen is None:
            return
        if row is None:
            ops.seen_mark(tokens, self.prompt_len, self.seen, self.V)
        else:
            ops.seen_clear_rows(self.seen, self.row_ids[row:row + 1])
            ops.seen_mark(tokens[row:row + 1], self.prompt_len[row:row + 1], self.seen[row:row + 1], self.V)

    def prepare(self, logits: torch.Tensor) -> torch.Tensor:
        """The logits the choice is made from: the penalised copy, or the raw ones when there is no penalty."""
        assert logits.shape[1] == self.V, (tuple(logits.shape), self.V)
        ops.logits_prepare(logits, self.seen, self.penalty, self.out, self.lse)
        return self.out if self.seen is not None else logits

    def snapshot(self, stopped: torch.Tensor) -> None:
        self.stopped_before.copy_(stopped)

    def record(self, logits: torch.Tensor, tokens: torch.Tensor, *, col: int = 0, cur=None, stopped_before=None) -> None:
        ops.generate_record(logits, self.lse, tokens, self.seen, self.lp, col=col, cur=cur, stopped_before=stopped_before,
                            prompt_len=self.prompt_len)


class VerifyControls:
    """Device state of ``generate_many(lookup=D, lookup_verify="choice")`` (include/a3vlm_hip.h, "Lookup decoding: sample and match"):
    ``rows`` cache rows of ``Q`` queries each.  ``gc`` (a ``GenControls`` or None) lends its seen bitmap, penalty, log-prob array
    and ``prompt_len``; ``cs`` (a ``constrain.ConstraintState`` or None) its table and states.  Per step ``prepare`` is one
    ``a3v_verify_prepare`` launch (none when neither is given: the choice reads the raw rows), ``uniforms`` one
    ``a3v_verify_uniforms`` launch and ``accept`` one ``a3v_accept_rows_chosen`` launch."""

    def __init__(self, rows: int, Q: int, V: int, device, gc: Optional[GenControls] = None, cs=None, sampling: bool = False):
        self.Q, self.V, self.gc, self.cs = Q, V, gc, cs
        n = rows * Q
        self.prompt_len = gc.prompt_len if gc is not None else torch.zeros(rows, dtype=torch.int32, device=device)
        self.seen = gc.seen if gc is not None else None
        self.lp = gc.lp if gc is not None else None
        self.lse = torch.zeros(n, dtype=torch.float32, device=device) if self.lp is not None else None
        self.active = self.seen is not None or self.lp is not None or cs is not None
        self.out = torch.empty((n, V), dtype=torch.float32, device=device) if self.active else None
        self.chosen = torch.zeros(n, dtype=torch.long, device=device)
        self.u = torch.zeros(n, dtype=torch.float32, device=device) if sampling else None
        self.row_base = torch.zeros(rows, dtype=torch.long, device=device)      # index of the row's answer in the flat uniforms

    def prepare(self, vlogits: torch.Tensor, x: torch.Tensor, nq: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        """The rows the choice is made from; the raw ``vlogits`` are never written."""
        if not self.active:
            return vlogits
        cs = self.cs
        return ops.verify_prepare(vlogits, x, nq, pos, self.out, seen=self.seen, penalty=self.gc.penalty if self.seen is not None else 1.0,
                                  trans=cs.trans if cs is not None else None, state=cs.state if cs is not None else None, lse=self.lse)

    def uniforms(self, uni: torch.Tensor, cur: torch.Tensor) -> torch.Tensor:
        return ops.verify_uniforms(uni, self.row_base, cur, self.prompt_len, self.Q, self.u)

    def accept(self, vlogits, x, nq, tokens, cur, limit, pos_base, stop_seq, stop_off, n_stop, stopped, stop_pos, next_tok, pos, stats) -> None:
        cs = self.cs
        ops.accept_rows_chosen(self.chosen, x, nq, tokens, cur, limit, pos_base, stop_seq, stop_off, n_stop, stopped, stop_pos, next_tok, pos,
                               stats, V=self.V, logits=vlogits if self.lp is not None else None, lse=self.lse, logprob=self.lp,
                               prompt_len=self.prompt_len, seen=self.seen, trans=cs.trans if cs is not None else None,
                               state=cs.state if cs is not None else None)
