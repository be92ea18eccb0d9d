"""Host-side bookkeeping of ``MetaModel.generate_many``: which prompt sits in which KV-cache row, and how far every row has got.

Pure Python, no torch: the device keeps the per-row token state (``a3v_generate_step_rows``); the host only needs to know which rows
are free, which prompt comes next, and an upper bound of the largest cache position (positions advance by one per step, so the
host counts them instead of reading them back)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple


class RowScheduler:
    """``prompt_lens[i]`` tokens of prompt i are prefilled, ``limits[i]`` is one past the last index of its token row that may be
    written, ``pos_base`` the image words in front of every prompt in the cache.

    * ``refill()`` hands pending prompts to free rows: prompts in input order, lowest free row first.  A prompt whose limit leaves
      nothing to write (``limits[i] <= prompt_lens[i]``) never takes a row: it is reported in ``finished_at_once``.
    * ``advance()`` is one decode step of every occupied row and returns the largest cache position of that step (an upper bound:
      a row that has stopped on the device but is not released yet still counts, capped by its own limit).
    * ``release(row)`` frees the row of a finished prompt."""

    def __init__(self, prompt_lens: Sequence[int], limits: Sequence[int], batch_rows: int, pos_base: int = 0):
        assert len(prompt_lens) == len(limits) and batch_rows > 0 and pos_base >= 0
        self.prompt_lens, self.limits, self.pos_base = list(prompt_lens), list(limits), pos_base
        self.rows: List[Optional[int]] = [None] * batch_rows      # prompt index per row
        self.next_pos: List[int] = [-1] * batch_rows              # cache position of the row's next decode step
        self.generated: List[int] = [0] * batch_rows              # ids written by the row's prompt so far
        self.next_prompt = 0
        self.finished_at_once: List[int] = []
        self.steps = 0

    def occupied(self) -> List[Tuple[int, int]]:
        return [(r, i) for r, i in enumerate(self.rows) if i is not None]

    def pending(self) -> int:
        return len(self.prompt_lens) - self.next_prompt

    def done(self) -> bool:
        return self.pending() == 0 and not self.occupied()

    def refill(self) -> List[Tuple[int, int]]:
        out = []
        for r in range(len(self.rows)):
            if self.rows[r] is not None:
                continue
            while self.next_prompt < len(self.prompt_lens) and self.limits[self.next_prompt] <= self.prompt_lens[self.next_prompt]:
                self.finished_at_once.append(self.next_prompt)
                self.next_prompt += 1
            if self.next_prompt == len(self.prompt_lens):
                break
            i = self.next_prompt
            self.next_prompt += 1
            self.rows[r] = i
            self.next_pos[r] = self.pos_base + self.prompt_lens[i]        # the first generated id lands behind the prompt
            self.generated[r] = 0
            out.append((r, i))
        return out

    def advance(self) -> int:
        occ = self.occupied()
        assert occ, "advance() without an occupied row"
        pos_max = 0
        for r, i in occ:
            pos_max = max(pos_max, min(self.next_pos[r], self.pos_base + self.limits[i] - 1))
            self.next_pos[r] += 1
            self.generated[r] += 1
        self.steps += 1
        return pos_max

    def release(self, row: int) -> int:
        i = self.rows[row]
        assert i is not None, row
        self.rows[row] = None
        self.next_pos[row] = -1
        return i
