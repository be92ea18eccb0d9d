"""Arena and job table of the one-launch gradient finish (``a3v_grad_finish_multi``, csrc/a3v_finish.hip).

The producers of a LoRA backward -- the adapter weight-gradient strips (``a3v_gemm_tn_strip``) and the RMSNorm backward -- leave
fp32 partials behind: split-K planes and per-block partial rows.  ``FinishPlan`` gives every producer call of a step (one per layer
and GEMM group / norm) a slice of ONE step-long arena and describes how its partials become gradients; the engine launches the
whole table once after the last block's backward.

The planning is plain Python over integers (offsets in floats, device pointers as ints) so that it can be checked without a GPU;
``GradFinisher`` adds the arena tensor and the device copies of the table.  A table depends on what varies from step to step only
through each job's plane count S / partial-row count, so a training run with a fixed batch shape builds exactly one.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

PLANES, SCATTER, COLSUM = 0, 1, 2            # a3v_finish_job.kind (include/a3vlm_hip.h)
JOB_FIELDS = 22                              # int64 fields of a3v_finish_job
SCATTER_TILE = 64                            # n per scatter unit (FIN_TN)
COLSUM_CHUNKS = 16                           # row chunks of a column sum (FIN_CHUNKS)
SLICE_ALIGN = 64                             # floats: every slice starts on a 256-byte boundary
DEFAULT_BUDGET = 6 * 2 ** 30                 # bytes; the 7B headline step (8 x 1091 tokens, rank 16) needs about 2.9 GiB


def job_units(kind: int, R: int, N: int, njs: Sequence[int] = ()) -> int:
    """Work units of one job -- the counts the kernel assumes (csrc/a3v_finish.hip)."""
    if kind == PLANES:
        return -(-(R * (N // 4)) // 256)
    if kind == SCATTER:
        return sum(-(-n // SCATTER_TILE) for n in njs)
    return COLSUM_CHUNKS * (-(-N // 1024))


class Slot:
    """One producer call's slice of the arena and what the finish does with it.  ``count_cap``: the most planes (PLANES / SCATTER) or
    partial rows (COLSUM) the slice holds; ``R``: rows of a plane (0 for COLSUM, whose row count is the per-step count)."""
    __slots__ = ("key", "kind", "offset", "floats", "count_cap", "R", "N", "dsts", "ldo", "accumulate", "r", "row0s", "njs")

    def signature(self) -> tuple:
        return (self.kind, self.R, self.N, self.dsts, self.ldo, self.accumulate, self.r, self.row0s, self.njs)

    def row(self, count: int, src_ptr: int, unit0: int) -> List[int]:
        """The a3v_finish_job of this slot with ``count`` planes / partial rows, its slice at device address ``src_ptr``."""
        if not 1 <= count <= self.count_cap:
            raise ValueError(f"finish job {self.key}: {count} planes / rows, the slice holds {self.count_cap}")
        col = self.kind == COLSUM
        pad = lambda xs: list(xs) + [0] * (4 - len(xs))                         # noqa: E731
        return ([self.kind, src_ptr, 1 if col else count, count if col else self.R, self.N, self.ldo, int(self.accumulate), self.r,
                 len(self.njs)] + pad(self.dsts) + pad(self.row0s) + pad(self.njs) + [unit0])

    def units(self) -> int:
        return job_units(self.kind, self.R, self.N, self.njs)


class FinishPlan:
    """Slices of the arena, in the order the slots were added; ``close()`` fixes the size and says whether it fits the budget."""

    def __init__(self, budget_bytes: int = DEFAULT_BUDGET):
        self.budget_bytes = int(budget_bytes)
        self.slots: Dict[object, Slot] = {}
        self.total_floats = 0
        self.closed = False

    @property
    def bytes(self) -> int:
        return 4 * self.total_floats

    @property
    def fits(self) -> bool:
        return self.closed and 0 < self.bytes <= self.budget_bytes

    def _add(self, key, kind, floats, count_cap, R, N, dsts, ldo, accumulate, r=0, row0s=(), njs=()) -> Slot:
        if self.closed:
            raise RuntimeError("FinishPlan is closed")
        if key in self.slots:
            raise ValueError(f"finish slot {key!r} planned twice")
        dsts, row0s, njs = tuple(int(d) for d in dsts), tuple(int(x) for x in row0s), tuple(int(x) for x in njs)
        # the kernel's accesses are 16 bytes wide and unchecked on the device: everything it assumes is checked here
        if count_cap < 1 or N < 4 or N % 4 or ldo % 4 or not dsts or len(dsts) > 4 or any(d <= 0 or d % 16 for d in dsts):
            raise ValueError(f"finish slot {key!r}: shape or alignment the kernel does not take")
        if kind != COLSUM and (R < 1 or floats != count_cap * R * N):
            raise ValueError(f"finish slot {key!r}: slice size")
        if kind == PLANES and ldo < N:
            raise ValueError(f"finish slot {key!r}: destination rows overlap")
        if kind == SCATTER:
            if not (len(dsts) == len(row0s) == len(njs)) or r < 4 or r % 4 or r > 64 or len(njs) * r > R:
                raise ValueError(f"finish slot {key!r}: adapter blocks")
            if any(n < 4 or n % 4 or o < 0 or o % 4 or o + n > N for o, n in zip(row0s, njs)):
                raise ValueError(f"finish slot {key!r}: a block's columns")
        s = Slot()
        s.key, s.kind, s.offset, s.floats, s.count_cap = key, kind, self.total_floats, int(floats), int(count_cap)
        s.R, s.N, s.dsts, s.ldo, s.accumulate, s.r, s.row0s, s.njs = int(R), int(N), dsts, int(ldo), bool(accumulate), int(r), row0s, njs
        self.slots[key] = s
        self.total_floats += -(-s.floats // SLICE_ALIGN) * SLICE_ALIGN
        return s

    def add_planes(self, key, R: int, N: int, S_cap: int, dst: int, ldo: int, accumulate: bool = True) -> Slot:
        """dst [R, N] (row stride ldo) (+)= the sum of up to ``S_cap`` planes [R][N]."""
        return self._add(key, PLANES, S_cap * R * N, S_cap, R, N, (dst,), ldo, accumulate)

    def add_scatter(self, key, R: int, N: int, S_cap: int, r: int, dsts: Sequence[int], row0s: Sequence[int], njs: Sequence[int]) -> Slot:
        """Module j's [njs[j], r] gradient += rows j r .. (j + 1) r, columns row0s[j] .. + njs[j] of the plane sum, transposed."""
        return self._add(key, SCATTER, S_cap * R * N, S_cap, R, N, dsts, 0, True, r, row0s, njs)

    def add_colsum(self, key, rows_cap: int, cols: int, dst: int) -> Slot:
        """dst [cols] += the column sum of up to ``rows_cap`` partial rows."""
        return self._add(key, COLSUM, rows_cap * cols, rows_cap, 0, cols, (dst,), 0, True)

    def close(self) -> bool:
        self.closed = True
        return self.fits

    def rows(self, counts: Dict[object, int], base_ptr: int) -> Tuple[List[List[int]], int]:
        """(a3v_finish_job rows, total units) for the slots named in ``counts`` (slot -> planes / partial rows this step), in plan
        order; ``base_ptr``: device address of the arena (16-byte aligned)."""
        if base_ptr <= 0 or base_ptr % 16:
            raise ValueError("arena address")
        out, unit0 = [], 0
        for key, s in self.slots.items():
            c = counts.get(key)
            if c is None:
                continue
            out.append(s.row(c, base_ptr + 4 * s.offset, unit0))
            unit0 += s.units()
        if len(out) != len(counts):
            raise KeyError("finish counts name a slot that was not planned")
        return out, unit0


class GradFinisher:
    """A ``FinishPlan`` with its arena and the device tables, as the engine holds it.  Life cycle: the first backward of an engine
    only records its producer calls (``plan`` open, the calls themselves finish their sums as before); ``commit()`` then closes the
    plan and allocates the arena if it fits the budget; from the next backward on the producers write into ``slice_of(...)`` and
    report their counts to ``pending``, and ``launch()`` finishes all of them."""
    MAX_TABLES = 8

    def __init__(self, budget_bytes: int, flat_ptr: int):
        self.plan = FinishPlan(budget_bytes)
        self.flat_ptr = flat_ptr
        self.arena = None
        self.pending: Dict[object, int] = {}
        self._tables: Dict[tuple, tuple] = {}
        self.tables_built = 0
        self.last_counts: Dict[object, int] = {}            # slot -> planes / partial rows of the last launch

    def commit(self, device) -> bool:
        import torch
        if self.plan.close():
            self.arena = torch.empty(self.plan.total_floats, dtype=torch.float32, device=device)
        return self.arena is not None

    def slice_of(self, slot: Slot, floats: int):
        return self.arena[slot.offset:slot.offset + floats]

    def table(self, counts: Dict[object, int]) -> tuple:
        """(device table, jobs, units) for this step's counts: built on first use, then reused for every step of the same shape."""
        key = tuple(sorted(counts.items(), key=lambda kv: self.plan.slots[kv[0]].offset))
        ent = self._tables.get(key)
        if ent is None:
            import torch
            rows, units = self.plan.rows(counts, self.arena.data_ptr())
            if len(self._tables) >= self.MAX_TABLES:
                self._tables.pop(next(iter(self._tables)))
            ent = self._tables[key] = (torch.tensor(rows, dtype=torch.int64).to(self.arena.device), len(rows), units)
            self.tables_built += 1
        return ent

    def launch(self, max_blocks: int = 0) -> None:
        if not self.pending:
            return
        from . import ops
        tab, n, units = self.table(self.pending)
        ops.grad_finish_multi(tab, n, units, max_blocks)
        self.last_counts, self.pending = self.pending, {}
