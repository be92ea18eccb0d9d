"""CPU (-m "not gpu"): the host restatements of the ragged-decode kernels against hand-worked cases, and generate_many's
RowScheduler (pure Python): order, refill, seven prompts on three rows, a prompt whose limit is reached at once."""
import math

import torch

import ragged_ref as R
from a3vlm_amd.model.ragged import RowScheduler


def test_rope_rows_by_hand():
    # one head, hd = 2, angle pi/2 at position 1: (a, b) -> (-b, a); position 0 is the identity
    cs = torch.tensor([[[1.0, 0.0]], [[0.0, 1.0]]])                      # [P = 2, hd/2 = 1, (cos, sin)]
    qkv = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] * 3)             # q | k | v, H = Hkv = 1
    q, writes = R.rope_rows_fp64(qkv, cs, [1, 0, 2], H=1, Hkv=1, hd=2, Smax=2)
    assert q[0].tolist() == [[-2.0, 1.0]] and q[1].tolist() == [[1.0, 2.0]] and q[2].tolist() == [[0.0, 0.0]]
    assert set(writes) == {(0, 1), (1, 0)}, "position Smax is an idle row"
    k, v = writes[(0, 1)]
    assert k.tolist() == [[-4.0, 3.0]] and v.tolist() == [[5.0, 6.0]]


def test_decode_attention_rows_by_hand():
    # hd = 1: scores are q * k; two keys with equal scores average their values, the NaN behind sk never shows
    q = torch.tensor([[[2.0]], [[1.0]], [[1.0]]])                        # [B = 3, H = 1, hd = 1]
    k = torch.tensor([[[[0.0], [0.0], [float("nan")]]]] * 3, dtype=torch.float64)        # [B, 1, Smax = 3, 1]
    vt = torch.tensor([[[[1.0, 3.0, float("nan")]]]] * 3)                # [B, 1, 1, Smax]
    k[1, 0, 1, 0] = math.log(3.0)                                         # row 1: weights 1/4, 3/4
    out = R.decode_attention_rows_fp64(q, k, vt, [2, 2, 0])
    assert out[0, 0, 0].item() == 2.0
    assert abs(out[1, 0, 0].item() - 2.5) < 1e-12
    assert out[2, 0, 0].item() == 0.0 and torch.isfinite(out).all()
    assert R.decode_attention_rows_fp64(q, k, vt, [1, 1, -1])[:, 0, 0].tolist() == [1.0, 1.0, 0.0]


def test_generate_step_rows_by_hand():
    stop = [[2], [7, 8]]
    # row 0 runs on; row 1 completes 7 8; row 2 was stopped before; row 3 writes its last index; row 4 hits EOS
    tokens = [[1, 5, 0, 0], [1, 7, 0, 0], [1, 9, 9, 9], [1, 4, 0, 0], [1, 4, 0, 0]]
    cur, limit = [2, 2, 3, 2, 2], [4, 4, 4, 3, 4]
    stopped, stop_pos = [False, False, True, False, False], [0, 0, 2, 0, 0]
    logits = [[0, 0, 0, 9, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 5, 5], None, [3, 0, 0, 3, 0, 0, 0, 0, 0, 0], [0, 0, 9, 0, 0, 0, 0, 0, 0, 0]]
    nt, pos = R.generate_step_rows(logits, None, tokens, cur, limit, 10, stop, stopped, stop_pos)
    assert tokens == [[1, 5, 3, 0], [1, 7, 8, 0], [1, 9, 9, 9], [1, 4, 0, 0], [1, 4, 2, 0]]      # row 3: argmax tie -> index 0
    assert cur == [3, 3, 3, 3, 3]
    assert stopped == [False, True, True, True, True]
    assert stop_pos == [3, 1, 2, 3, 2]
    assert nt == [3, 0, 0, 0, 0] and pos == [12, -1, -1, -1, -1]
    # sampled ids replace the argmax; a row whose cur is already at its limit stops without a write
    tokens, cur, limit = [[1, 0], [1, 0]], [1, 2], [2, 2]
    stopped, stop_pos = [False, False], [0, 0]
    nt, pos = R.generate_step_rows(None, [6, 6], tokens, cur, limit, 0, stop, stopped, stop_pos)
    assert tokens == [[1, 6], [1, 0]] and stopped == [True, True] and cur == [2, 2] and nt == [0, 0] and pos == [-1, -1]


def _run(lens, gens, rows, poll_every=1, base=0):
    """Drive the scheduler like generate_many does, with answers of exactly gens[i] ids; returns (assignment log, finish order, steps)."""
    limits = [l + g for l, g in zip(lens, gens)]
    s = RowScheduler(lens, limits, rows, base)
    log, order, at_once = [], [], []
    while True:
        new = s.refill()
        log += [(s.steps, r, i) for r, i in new]
        at_once += s.finished_at_once
        s.finished_at_once.clear()
        if not s.occupied():
            break
        pm = s.advance()
        assert pm == max(min(base + lens[i] + s.generated[r] - 1, base + limits[i] - 1) for r, i in s.occupied())
        if s.steps % poll_every == 0:
            for r, i in s.occupied():
                if s.generated[r] >= gens[i]:
                    order.append(s.release(r))
    assert s.done()
    return log, order, at_once, s.steps


def test_scheduler_order_and_refill():
    log, order, at_once, steps = _run([3, 3, 3, 3], [2, 5, 1, 1], rows=2)
    # prompts in input order to the lowest free row; prompt 2 enters row 0 when prompt 0 leaves after two steps, prompt 3 one step later
    assert log == [(0, 0, 0), (0, 1, 1), (2, 0, 2), (3, 0, 3)]
    assert order == [0, 2, 3, 1] and at_once == [] and steps == 5


def test_scheduler_seven_prompts_on_three_rows():
    lens, gens = [4, 2, 6, 3, 5, 1, 2], [3, 9, 2, 4, 1, 6, 2]
    log, order, at_once, steps = _run(lens, gens, rows=3, base=7)
    assert [i for _, _, i in log] == list(range(7)), "input order"
    assert sorted(order) == list(range(7)) and at_once == []
    assert log[:3] == [(0, 0, 0), (0, 1, 1), (0, 2, 2)]
    assert log[3] == (2, 2, 3) and log[4] == (3, 0, 4) and log[5] == (4, 0, 5) and log[6] == (6, 2, 6)
    # the rows never idle while prompts are pending: total steps = the longest chain of answers that shared a row
    assert steps == max(3 + 1 + 6, 9, 2 + 4 + 2)
    # with a coarser poll the same prompts finish, later
    log4, order4, _, steps4 = _run(lens, gens, rows=3, poll_every=4)
    assert sorted(order4) == list(range(7)) and [i for _, _, i in log4] == list(range(7)) and steps4 >= steps


def test_scheduler_limit_reached_at_once():
    # prompt 1 fills its limit (nothing to write): it never takes a row; prompt 3 likewise, at the end of the list
    log, order, at_once, steps = _run([3, 8, 2, 5], [2, 0, 1, 0], rows=2)
    assert at_once == [1, 3]
    assert log == [(0, 0, 0), (0, 1, 2)] and sorted(order) == [0, 2] and steps == 2
    log, order, at_once, steps = _run([4], [0], rows=3)
    assert log == [] and order == [] and at_once == [0] and steps == 0
