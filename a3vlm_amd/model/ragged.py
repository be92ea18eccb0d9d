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


class GroupScheduler:
    """Parallel sampling (``generate_many(..., n=...)``): every prompt runs ``n`` samples that share the prompt's keys, which are
    stored once, in the row of the group's leader.

    * Prompts are admitted in input order, and only when ``n`` rows are free: a prompt takes the n lowest free rows.  The lowest
      is the leader (it is prefilled and runs sample 0), the others run samples 1..n-1 in row order.
    * ``refill()`` returns the admitted groups as ``(prompt, [rows])``; ``sample[row]`` is the sample a row runs.
    * ``release(row)`` ends the row's sample.  A sibling's row is free at once.  The leader's row is free only when the last
      sample of its group has been released, because its prefix is read until then: a leader that stopped earlier sits idle
      meanwhile (it is no longer occupied: ``advance()`` does not count it).
    * ``advance()`` / ``occupied()`` / ``pending()`` / ``done()`` / ``finished_at_once`` / ``steps`` as in ``RowScheduler``; with
      ``n == 1`` the assignments, the ``pos_max`` values and ``steps`` are that class's on any script of finishes."""

    def __init__(self, prompt_lens: Sequence[int], limits: Sequence[int], batch_rows: int, pos_base: int = 0, n: int = 1):
        assert len(prompt_lens) == len(limits) and batch_rows > 0 and pos_base >= 0
        assert 1 <= n <= batch_rows, (n, batch_rows)
        self.prompt_lens, self.limits, self.pos_base, self.n = list(prompt_lens), list(limits), pos_base, n
        self.rows: List[Optional[int]] = [None] * batch_rows      # prompt index per row that runs a sample
        self.sample: List[int] = [0] * batch_rows                 # which of the prompt's n samples
        self.leader: List[int] = [-1] * batch_rows                # the leader row of the row's group
        self.left: List[int] = [0] * batch_rows                   # per leader row: samples of its group not yet released
        self.next_pos: List[int] = [-1] * batch_rows
        self.generated: List[int] = [0] * batch_rows
        self.next_prompt = 0
        self.finished_at_once: List[int] = []
        self.steps = 0

    def occupied(self) -> List[Tuple[int, int]]:
        return [(r, i) for r, i in enumerate(self.rows) if i is not None]

    def free_rows(self) -> List[int]:
        """rows that run nothing and whose prefix nobody reads"""
        return [r for r, i in enumerate(self.rows) if i is None and self.left[r] == 0]

    def held(self) -> List[int]:
        """leader rows that have finished their own sample and wait for their group"""
        return [r for r, i in enumerate(self.rows) if i is None and self.left[r] > 0]

    def pending(self) -> int:
        return len(self.prompt_lens) - self.next_prompt

    def done(self) -> bool:
        return self.pending() == 0 and not self.occupied()

    def refill(self) -> List[Tuple[int, List[int]]]:
        out = []
        while True:
            free = self.free_rows()
            if len(free) < self.n:
                break
            while self.next_prompt < len(self.prompt_lens) and self.limits[self.next_prompt] <= self.prompt_lens[self.next_prompt]:
                self.finished_at_once.append(self.next_prompt)
                self.next_prompt += 1
            if self.next_prompt == len(self.prompt_lens):
                break
            i = self.next_prompt
            self.next_prompt += 1
            rows = free[:self.n]
            self.left[rows[0]] = self.n
            for s, r in enumerate(rows):
                self.rows[r], self.sample[r], self.leader[r] = i, s, rows[0]
                self.next_pos[r] = self.pos_base + self.prompt_lens[i]
                self.generated[r] = 0
            out.append((i, rows))
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
        self.left[self.leader[row]] -= 1
        return i


class LookupBound:
    """Lookup decoding (``generate_many(..., lookup=D)``): a row advances by 1 .. Q = D + 1 positions per step and only the device
    knows by how many, so the host keeps an UPPER BOUND of every running row's cache position instead of the exact count.

    * ``start(row, pos, last)``: the row's next step runs at cache position ``pos`` exactly (a refill); ``last`` is the largest
      position it can ever decode at (prompt positions + max_gen_len - 1, below the cache length).
    * ``step()`` returns the bound of the largest position of this step, then lets every running row grow by Q, clamped by its
      ``last``.
    * ``resync(row, pos)``: the exact position read back from the device (the read that already fetches ``stopped``).
    * ``release(row)``: the row no longer runs.

    The bound never falls below a running row's true position (a row gains at most Q per step and never passes ``last``), and it
    never reaches the cache length because no ``last`` does."""

    def __init__(self, batch_rows: int, Q: int):
        assert batch_rows > 0 and Q >= 1
        self.Q = Q
        self.bound: List[Optional[int]] = [None] * batch_rows
        self.last: List[int] = [0] * batch_rows

    def start(self, row: int, pos: int, last: int) -> None:
        assert 0 <= pos <= last, (pos, last)
        self.bound[row], self.last[row] = pos, last

    def resync(self, row: int, pos: int) -> None:
        if self.bound[row] is not None:
            self.bound[row] = min(max(pos, 0), self.last[row])

    def release(self, row: int) -> None:
        self.bound[row] = None

    def step(self) -> int:
        run = [r for r, b in enumerate(self.bound) if b is not None]
        assert run, "step() without a running row"
        pos_max = max(self.bound[r] for r in run)
        for r in run:
            self.bound[r] = min(self.bound[r] + self.Q, self.last[r])
        return pos_max


def prefix_groups(prompt_tokens: Sequence[Sequence[int]], image_keys: Sequence[object], pos_base: int = 0) -> List[Tuple[List[int], int]]:
    """Prefix sharing (``generate_many(..., prefix_sharing=True)``): the input list cut into runs ``(members, P)`` of ADJACENT
    prompts with the same image key (``image_keys[i] == image_keys[j]``) whose caches start with the same P positions.

    A prompt's cache is [BOS | pos_base image words | text]: with L the longest common token prefix of the run (BOS included) the
    common cache prefix is C = pos_base + L, and P = min(C, shortest member's cache length - 1) & ~63 -- every member keeps at
    least one token of its own (its last-position logits start its answer), and P is a multiple of 64 because the attention
    kernels switch between the prefix row and the own row at 64-key tiles only.  P must also cover BOS and the image words
    (P >= pos_base + 1 when there is an image: the prefix is prefilled with the image in front, whole), else it counts as 0.
    A run is extended greedily while its P stays > 0; a run of one, or P == 0, is ``([i], 0)``: today's path."""
    assert len(prompt_tokens) == len(image_keys)

    def shared_len(members):
        first = prompt_tokens[members[0]]
        L = min(len(prompt_tokens[i]) for i in members)
        for i in members[1:]:
            t, k = prompt_tokens[i], 0
            while k < L and t[k] == first[k]:
                k += 1
            L = k
        P = min(pos_base + L, pos_base + min(len(prompt_tokens[i]) for i in members) - 1) & ~63
        return P if P > 0 and (pos_base == 0 or P >= pos_base + 1) else 0

    out: List[Tuple[List[int], int]] = []
    i, N = 0, len(prompt_tokens)
    while i < N:
        members, P = [i], 0
        j = i + 1
        while j < N and image_keys[j] == image_keys[i]:
            Pj = shared_len(members + [j])
            if Pj == 0:
                break
            members, P = members + [j], Pj
            j += 1
        out.append((members, P if len(members) > 1 else 0))
        i = j
    return out


class PrefixScheduler(RowScheduler):
    """``RowScheduler`` over the runs of ``prefix_groups``: a run of several prompts stores its common prefix ONCE, in the row its
    first member is admitted to (the leader row), and every member runs its own suffix over it.

    * ``refill()`` admits prompts in input order, lowest free row first, and returns a list of
      ``(leader_row, P, new, [(row, prompt), ...])``: ``P == 0`` is a plain refill of one row (``leader_row == row``); otherwise the
      members listed are extended over the P prefix positions held in ``leader_row``, and ``new`` says that the prefix has to be
      prefilled there first (the run's first admission).  The first member of a run takes the leader row itself.
    * Members that find no free row wait; no later prompt overtakes them.  They are admitted when a row frees -- any free row, or
      the run's own leader row once its current member has finished (its prefix stays where it is).
    * The leader row is HELD while any member of its run runs or waits: it takes no prompt of another run until the last member
      has been released (``GroupScheduler``'s rule for the leader of n samples).
    * ``advance()`` / ``occupied()`` / ``release()`` / ``finished_at_once`` / ``steps`` as in ``RowScheduler``; with runs of one only
      the assignments are that class's."""

    def __init__(self, prompt_lens: Sequence[int], limits: Sequence[int], batch_rows: int, pos_base: int,
                 groups: Sequence[Tuple[Sequence[int], int]]):
        super().__init__(prompt_lens, limits, batch_rows, pos_base)
        assert [i for members, _ in groups for i in members] == list(range(len(prompt_lens))), "the runs cover the prompts in order"
        self.group_of: List[int] = [0] * len(prompt_lens)
        self.groups = [(list(members), int(P)) for members, P in groups]
        for g, (members, _) in enumerate(self.groups):
            for i in members:
                self.group_of[i] = g
        self.leader_of_group: List[int] = [-1] * len(self.groups)    # the row that holds the run's prefix, -1 before / after
        self.left: List[int] = [0] * len(self.groups)                 # members of the run not yet released (running or waiting)

    def held(self) -> List[int]:
        """rows whose prefix a run still needs"""
        return [r for g, r in enumerate(self.leader_of_group) if r >= 0 and self.left[g] > 0]

    def release(self, row: int) -> int:
        i = super().release(row)
        g = self.group_of[i]
        if self.groups[g][1] > 0:
            self.left[g] -= 1
            if self.left[g] == 0:
                self.leader_of_group[g] = -1
        return i

    def refill(self):
        out = []
        N = len(self.prompt_lens)
        while True:
            while self.next_prompt < N and self.limits[self.next_prompt] <= self.prompt_lens[self.next_prompt]:
                i = self.next_prompt                       # nothing to write: never takes a row, leaves its run at once
                self.finished_at_once.append(i)
                self.next_prompt += 1
                g = self.group_of[i]
                if self.groups[g][1] > 0:
                    if i == self.groups[g][0][0]:
                        self.left[g] = len(self.groups[g][0])
                    self.left[g] -= 1
                    if self.left[g] == 0:
                        self.leader_of_group[g] = -1
            if self.next_prompt == N:
                break
            i = self.next_prompt
            g = self.group_of[i]
            members, P = self.groups[g]
            held = set(self.held())
            lead = self.leader_of_group[g] if P > 0 else -1
            free = [r for r, x in enumerate(self.rows) if x is None and (r not in held or r == lead)]
            if not free:
                break
            if P > 0 and i == members[0]:
                self.left[g] = len(members)
            new = P > 0 and lead < 0
            r = free[0]
            if new:
                lead = self.leader_of_group[g] = r
            self.next_prompt += 1
            self.rows[r] = i
            self.next_pos[r] = self.pos_base + self.prompt_lens[i]
            self.generated[r] = 0
            if P > 0 and out and out[-1][0] == lead and out[-1][1] == P and self.group_of[out[-1][3][0][1]] == g:
                out[-1][3].append((r, i))                  # one extend for every member admitted together
            else:
                out.append((lead if P > 0 else r, P, new, [(r, i)]))
        return out
