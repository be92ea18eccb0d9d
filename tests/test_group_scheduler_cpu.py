"""GroupScheduler (a3vlm_amd/model/ragged.py) without a GPU: with n = 1 it is RowScheduler step for step; with n > 1 the group rules
(leader = lowest row, a leader's row is held until its whole group is done, siblings are free at once, input order, n samples each)."""
import random

import pytest

from a3vlm_amd.model.ragged import GroupScheduler, RowScheduler


def _script(seed):
    rng = random.Random(seed)
    N, R = rng.randint(0, 9), rng.randint(1, 5)
    lens = [rng.randint(1, 6) for _ in range(N)]
    limits = [ln + rng.randint(0, 5) for ln in lens]          # some prompts have nothing to write
    return rng, N, R, lens, limits


@pytest.mark.parametrize("seed", range(40))
def test_n1_equals_row_scheduler_step_for_step(seed):
    rng, N, R, lens, limits = _script(seed)
    a, b = RowScheduler(lens, limits, R, 3), GroupScheduler(lens, limits, R, 3, 1)
    while True:
        x, y = a.refill(), b.refill()
        assert [(rows[0], i) for i, rows in y] == x and all(len(rows) == 1 for _, rows in y)
        assert a.finished_at_once == b.finished_at_once
        assert a.occupied() == b.occupied() and a.pending() == b.pending() and a.done() == b.done()
        if not a.occupied():
            break
        assert a.advance() == b.advance()
        assert a.next_pos == b.next_pos and a.generated == b.generated
        for r, i in a.occupied():
            if rng.random() < 0.3 or a.generated[r] >= limits[i] - lens[i]:
                assert a.release(r) == b.release(r)
    assert a.steps == b.steps and b.done() and a.next_prompt == b.next_prompt == N


@pytest.mark.parametrize("n,R", [(2, 4), (3, 4), (2, 5), (3, 5)])
@pytest.mark.parametrize("seed", range(10))
def test_group_rules(n, R, seed):
    rng = random.Random(100 * n + 10 * R + seed)
    N = rng.randint(1, 8)
    lens = [rng.randint(1, 6) for _ in range(N)]
    limits = [ln + rng.randint(0, 6) for ln in lens]
    s = GroupScheduler(lens, limits, R, 2, n)
    group_rows = {}                      # prompt -> its rows (leader first)
    running = {}                         # prompt -> samples not yet released
    ran = {i: [] for i in range(N)}      # prompt -> samples that ran
    admitted, at_once = [], []
    freed_last_round = set()
    while True:
        free_before = set(s.free_rows())
        for i, rows in s.refill():
            assert len(rows) == n and rows == sorted(rows) and set(rows) <= free_before, (rows, free_before)
            assert rows == sorted(free_before)[:n], "the n lowest free rows"
            assert rows[0] == min(rows) and s.leader[rows[0]] == rows[0], "the leader is the lowest row"
            for j, lead_rows in group_rows.items():      # a leader row is never handed out while a sample of its group runs
                assert not (running[j] and lead_rows[0] in rows), (j, rows)
            assert [s.sample[r] for r in rows] == list(range(n)) and all(s.leader[r] == rows[0] for r in rows)
            assert all(s.next_pos[r] == 2 + lens[i] for r in rows)
            group_rows[i], running[i] = rows, set(range(n))
            admitted.append(i)
            free_before -= set(rows)
        at_once += s.finished_at_once
        s.finished_at_once.clear()
        if not s.occupied():
            break
        freed_last_round.clear()
        s.advance()
        for r, i in s.occupied():
            if rng.random() < 0.35 or s.generated[r] >= limits[i] - lens[i]:
                smp = s.sample[r]
                assert s.release(r) == i
                running[i].discard(smp)
                ran[i].append(smp)
                lead = group_rows[i][0]
                if r != lead:
                    assert r in s.free_rows(), "a sibling's row is reusable at once"
                if running[i]:
                    assert lead not in s.free_rows(), "the leader's prefix is still read"
                    if r == lead:
                        assert lead in s.held()
                else:
                    assert lead in s.free_rows() and not s.held().count(lead)
    assert s.done() and not s.held() and len(s.free_rows()) == R
    assert admitted == sorted(admitted), "input order"
    assert sorted(admitted + at_once) == list(range(N))
    assert at_once == [i for i in range(N) if limits[i] <= lens[i]], "prompts with nothing to write take no row"
    for i in admitted:
        assert sorted(ran[i]) == list(range(n)), "every prompt runs exactly n samples"
    for i in at_once:
        assert ran[i] == [] and i not in group_rows


def test_a_prompt_waits_for_n_free_rows():
    s = GroupScheduler([2, 2, 2], [6, 6, 6], 4, 0, 3)
    assert s.refill() == [(0, [0, 1, 2])]              # one free row is not enough for prompt 1
    s.advance()
    s.release(0)                                       # the leader stops first: held, row 0 is not free
    assert s.free_rows() == [3] and s.held() == [0] and s.refill() == []
    s.release(2)
    assert s.free_rows() == [2, 3] and s.refill() == []
    assert s.advance() == 3                            # only row 1 runs: position 2 + 1
    s.release(1)
    assert s.held() == [] and s.refill() == [(1, [0, 1, 2])]


def test_more_samples_than_rows_asserts():
    with pytest.raises(AssertionError):
        GroupScheduler([1], [4], 2, 0, 3)
    with pytest.raises(AssertionError):
        GroupScheduler([1], [4], 2, 0, 0)
