"""Beam search, no GPU: the restatement (tests/beam_ref.py) against exhaustive enumeration and hand cases, the wrong walks it must
tell apart (mutants), the group scheduler as beam search drives it, the refusals of the arguments, and the C-ABI surface."""
import itertools
import os

import numpy as np
import pytest

import beam_ref as B
from a3vlm_amd import lib
from a3vlm_amd.model import beam
from a3vlm_amd.model.ragged import GroupScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
V, EOS = 5, 0


def _table_model(seed, viable=V):
    """A deterministic 'model' on V = 5: the logits behind a sequence depend on its last two tokens and its length; tokens at and
    above ``viable`` are impossible (-inf)."""
    rng = np.random.default_rng(seed)
    tab = rng.standard_normal((4, V + 1, V + 1, V)).astype(F) * 2
    tab[..., viable:] = -np.inf

    def row(seq):
        a = seq[-1] if len(seq) >= 1 else V
        b = seq[-2] if len(seq) >= 2 else V
        return tab[min(len(seq), 3), a, b]
    return row


def _exhaustive(row, limit, penalty, viable=V):
    """every hypothesis (EOS-ended, or cut at the limit) with its fp64 score, best first"""
    out = []
    lsm = lambda z: z - np.log(np.exp(z[np.isfinite(z)]).sum())
    for n in range(limit + 1):
        for seq in itertools.product(range(1, viable), repeat=n):
            lp = sum(lsm(row(list(seq[:j])).astype(np.float64))[seq[j]] for j in range(n))
            if n < limit:
                lp += lsm(row(list(seq)).astype(np.float64))[EOS]
            out.append((lp / max(n, 1) ** penalty, list(seq)))
    return sorted(out, key=lambda x: -x[0])


@pytest.mark.parametrize("penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_with_enough_beams_the_search_is_the_exhaustive_enumeration(seed, penalty):
    """K = 8 and three possible tokens (EOS and two others), limit 2: a step has at most 3 * 2 = 6 <= K candidates, so every EOS
    candidate has rank < K, every other one is taken, and the 1 + 2 + 4 = 7 hypotheses all fit the pool: the pool IS the
    enumeration, best first.  (With all of V = 5 possible and length <= 4 no K <= 8 is 'enough': 4 ** 3 live prefixes, and HF's walk
    drops an EOS candidate at rank >= K whatever its score, so the exact statement is made at the size where it can hold; the
    test below covers V = 5 and lengths 3 and 4 with what stays true under pruning.)"""
    row = _table_model(seed, viable=3)
    pool, _ = B.search(lambda seqs: np.stack([row(s) for s in seqs]), 8, 2, EOS, V, length_penalty=penalty, early_stopping=False)
    best = _exhaustive(row, 2, penalty, viable=3)
    assert [h[2] for h in pool] == [s for _, s in best], (pool, best)
    assert all(abs(h[0] - sc) < 1e-5 for h, (sc, _) in zip(pool, best))


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("limit", [3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_hypothesis_of_a_pruned_search_is_real_and_truly_scored(seed, limit, K):
    """V = 5, length <= 4: beams are pruned here, so the pool is a subset of the enumeration -- each entry with its true score,
    and the pool in order."""
    row = _table_model(seed)
    pool, _ = B.search(lambda seqs: np.stack([row(s) for s in seqs]), K, limit, EOS, V, length_penalty=1.0, early_stopping=False)
    true = {tuple(s): sc for sc, s in _exhaustive(row, limit, 1.0)}
    assert 0 < len(pool) <= K
    for sc, cum, ids in pool:
        assert abs(sc - true[tuple(ids)]) < 1e-4, (ids, sc, true[tuple(ids)])
    assert [p[0] for p in pool] == sorted((p[0] for p in pool), reverse=True)


def _one_group(K, limit, ld=4, state0=-1):
    st = B.State(1, K, ld)
    st.start(0, 10, limit, state0)
    return st, np.zeros((K, ld), np.int64), np.zeros((K, ld), np.int64)


def _cands(K, items):
    sc = np.full((1, 2 * K), -np.inf, F)
    be = np.full((1, 2 * K), -1, np.int32)
    to = np.full((1, 2 * K), -1, np.int32)
    for j, (s, b, t) in enumerate(items):
        sc[0, j], be[0, j], to[0, j] = s, b, t
    return sc, be, to


LD = B.len_div_table(8, 1.0)


def test_select_tie_goes_to_the_lower_flat_index():
    z = np.zeros((2, V), F)
    z[0, 3] = z[1, 1] = z[0, 4] = 1.0
    sc, be, to, gap = B.select(z, np.zeros(2, F), np.zeros(2, F), np.ones(2, np.uint8), 2)
    assert list(zip(be[0], to[0])) == [(0, 3), (0, 4), (1, 1), (0, 0)]
    assert gap[0] == 0.0
    msc, mbe, mto, _ = B.select(z, np.zeros(2, F), np.zeros(2, F), np.ones(2, np.uint8), 2, mutant="tie")
    assert list(zip(mbe[0], mto[0])) != list(zip(be[0], to[0])), "the wrong tie order is told apart"


def test_select_never_takes_minus_inf_or_nan_and_leaves_unfilled_slots():
    z = np.full((2, V), -np.inf, F)
    z[0, 2], z[1] = 0.5, np.nan
    sc, be, to, _ = B.select(z, np.zeros(2, F), np.zeros(2, F), np.ones(2, np.uint8), 2)
    assert (be[0].tolist(), to[0].tolist()) == ([0, -1, -1, -1], [2, -1, -1, -1]) and sc[0, 0] == F(0.5) and np.all(sc[0, 1:] == -np.inf)


def test_eos_below_rank_k_enters_the_pool_and_above_is_dropped():
    st, tin, tout = _one_group(2, 4)
    B.advance(*_cands(2, [(-1.0, 0, 3), (-1.5, 0, EOS), (-2.0, 0, EOS), (-2.5, 0, 1)]), st, tin, tout, V, EOS, True, LD, 64)
    assert st.pool_n[0] == 1 and st.pool_cum[0, 0] == F(-1.5), "rank 1 < K enters, rank 2 >= K is dropped"
    assert st.next_tok.tolist() == [3, 1] and st.alive.tolist() == [1, 1] and st.pos.tolist() == [10, 10] and st.glen[0] == 1
    assert tout[:, 0].tolist() == [3, 1]


def test_full_pool_keeps_the_best_and_a_tie_keeps_the_earlier_entry():
    # (the walk takes the ranks as they come: the scripted lists need not be sorted)
    st, tin, tout = _one_group(2, 4)
    B.advance(*_cands(2, [(-1.0, 0, EOS), (-1.0, 0, EOS), (-0.5, 0, 1), (-0.8, 0, 2)]), st, tin, tout, V, EOS, False, LD, 64)
    assert st.pool_n[0] == 2 and st.pool_seq[0].tolist() == [0, 1] and not st.done[0]
    tin, tout = tout, tin
    # a tie with the worst entry is dropped; a better one replaces the LATER of the two tied entries
    B.advance(*_cands(2, [(-2.0, 0, EOS), (-2.5, 1, 3), (-2.6, 1, 4)]), st, tin, tout, V, EOS, False, B.len_div_table(8, 1.0), 64)
    assert st.pool_score[0].tolist() == [-1.0, -1.0], "-2 / 1 does not beat -1"
    st2, tin, tout = _one_group(2, 4)
    B.advance(*_cands(2, [(-1.0, 0, EOS), (-1.0, 0, EOS), (-0.5, 0, 1), (-0.8, 0, 2)]), st2, tin, tout, V, EOS, False, LD, 64)
    B.advance(*_cands(2, [(-0.5, 0, EOS), (-3.5, 1, 3), (-3.6, 1, 4)]), st2, tout, tin, V, EOS, False, LD, 64)
    assert st2.pool_seq[0].tolist() == [0, 2] and st2.pool_score[0].tolist() == [-1.0, -0.5], "the earlier of the tied entries stays"
    assert [h[0] for h in st2.pool(0)] == [-0.5, -1.0]


def test_fewer_than_k_takers_leave_dead_rows():
    st, tin, tout = _one_group(3, 4)
    B.advance(*_cands(3, [(-1.0, 0, 3)]), st, tin, tout, V, EOS, True, LD, 64)
    assert st.alive.tolist() == [1, 0, 0] and st.pos.tolist() == [10, -1, -1] and st.next_tok.tolist() == [3, 0, 0]
    assert st.parent.tolist() == [0, 1, 2] and st.cum[1] == -np.inf and not st.done[0]


def test_the_limit_finalises_the_group_by_the_same_division():
    st, tin, tout = _one_group(2, 2)
    B.advance(*_cands(2, [(-1.0, 0, 3), (-2.0, 0, 4)]), st, tin, tout, V, EOS, True, LD, 64)
    assert not st.done[0]
    B.advance(*_cands(2, [(-3.0, 1, 1), (-5.0, 0, 2)]), st, tout, tin, V, EOS, True, LD, 64)
    assert st.done[0] and st.alive.tolist() == [0, 0] and st.pos.tolist() == [-1, -1]
    assert st.pool(0) == [(-1.5, -3.0, [4, 1]), (-2.5, -5.0, [3, 2])]
    before = (st.cum.copy(), st.pool_score.copy(), tin.copy())
    B.advance(*_cands(2, [(-0.1, 0, EOS)]), st, tin, tout, V, EOS, True, LD, 64)          # a done group is not touched
    assert np.array_equal(st.cum, before[0]) and np.array_equal(st.pool_score, before[1]) and st.glen[0] == 2


def test_both_stopping_rules():
    c1 = [(-1.0, 0, EOS), (-1.2, 0, EOS), (-1.1, 0, 1), (-1.4, 0, 2)]
    st, tin, tout = _one_group(2, 4)
    B.advance(*_cands(2, c1), st, tin, tout, V, EOS, True, LD, 64)
    assert st.done[0], "early stopping: the pool is full"
    st, tin, tout = _one_group(2, 4)
    B.advance(*_cands(2, c1), st, tin, tout, V, EOS, False, LD, 64)
    assert not st.done[0], "-1.1 / 1 can still beat -1.2"
    B.advance(*_cands(2, [(-2.6, 0, 3), (-2.7, 1, 3)]), st, tout, tin, V, EOS, False, LD, 64)
    assert st.done[0], "-2.6 / 2 = -1.3 <= -1.2: no live beam can beat the worst hypothesis"


def test_child_steps_its_parents_state():
    trans = np.array([[-1, 1, 1, 0, 0], [0, 0, 1, 1, -1]], np.int16)
    for mutant, want in ((None, [1, 0]), ("stale", [0, -1])):
        st, tin, tout = _one_group(2, 4, state0=0)
        st.alive[:] = 1
        st.state[:] = [1, 0]
        st.cum[:] = [-1, -1]
        B.advance(*_cands(2, [(-1.0, 1, 1), (-2.0, 0, 0)]), st, tin, tout, V, 9, True, LD, 64, trans, mutant)
        assert st.state.tolist() == want, mutant           # row 0 <- beam 1 (state 0) on token 1; row 1 <- beam 0 (state 1) on token 0


@pytest.mark.parametrize("mutant", ["tie", "div", "stale"])
def test_each_wrong_walk_fails_the_comparison(mutant):
    """whole searches on the table model under an automaton: the mutant's pool differs from the restatement's on some seed"""
    trans = np.array([[1, 1, -1, 0, 2], [2, -1, 1, 1, 2], [0, 2, 0, -1, 1]], np.int16)
    differs = 0
    for seed in range(8):
        row = _table_model(seed)
        q = lambda seqs: np.round(np.stack([row(s) for s in seqs]))         # integer logits: exact score ties
        for penalty in (1.0, 2.0):
            kw = dict(length_penalty=penalty, early_stopping=False, trans=trans, state0=0)
            differs += B.search(q, 3, 4, EOS, V, **kw)[0] != B.search(q, 3, 4, EOS, V, mutant=mutant, **kw)[0]
    assert differs > 0, mutant


def test_len_div_is_the_fp64_power_rounded_once():
    t = B.len_div_table(6, 0.7)
    assert t.dtype == F and t[0] == 1 and t[1] == 1 and t[3] == F(3.0 ** 0.7)
    assert np.array_equal(t, beam.len_div_table(6, 0.7).numpy())


# ------------------------------------------------------------------ scheduler
def test_group_scheduler_hands_out_whole_aligned_groups_when_groups_are_released_together():
    K, R = 3, 6
    lens, limits = [5, 9, 2, 4, 7], [8, 9, 6, 5, 12]        # prompt 1 has nothing to write
    s = GroupScheduler(lens, limits, R, pos_base=10, n=K)
    got = s.refill()
    assert got == [(0, [0, 1, 2]), (2, [3, 4, 5])] and s.finished_at_once == [1]
    assert s.advance() == 10 + 5 and s.generated[0] == 1
    for r in (3, 4, 5):
        s.release(r)
    assert s.refill() == [(3, [3, 4, 5])], "the freed group, whole and aligned, to the next prompt in input order"
    assert s.advance() == max(10 + 6, 10 + 4)
    for r in (0, 1, 2):
        s.release(r)
    assert s.refill() == [(4, [0, 1, 2])] and s.pending() == 0
    for r in range(6):
        s.release(r)
    assert s.done()


# ------------------------------------------------------------------ refusals and surface
@pytest.mark.parametrize("kw,match", [
    (dict(num_beams=0, batch_rows=4), "num_beams"), (dict(num_beams=9, batch_rows=16), "num_beams"),
    (dict(num_beams=4, batch_rows=3), "batch_rows"), (dict(num_beams=2, batch_rows=4, num_return_sequences=3), "num_return_sequences"),
    (dict(num_beams=2, batch_rows=4, temperature=0.7), "temperature=0"), (dict(num_beams=2, batch_rows=4, repetition_penalty=1.1), "repetition_penalty=1.0"),
    (dict(num_beams=2, batch_rows=4, lookup=2), "lookup=0"), (dict(num_beams=2, batch_rows=4, additional_stop_symbols=["#"]), "additional_stop_symbols")])
def test_argument_refusals_name_the_way_out(kw, match):
    with pytest.raises(ValueError, match=match):
        beam.check_beam_args(**kw)


def test_valid_arguments_pass():
    assert beam.check_beam_args(1, 1) == 1 and beam.check_beam_args(8, 8, 8) == 8


def test_the_three_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = open(os.path.join(ROOT, "a3vlm_amd", "csrc", "a3v_beam.hip")).read()
    for name in ("a3v_beam_select", "a3v_beam_advance", "a3v_kv_permute_tails"):
        assert f"int {name}(" in header and f'extern "C" int {name}(' in src and name in lib.SIGNATURES
        assert len(lib.SIGNATURES[name][1]) == header.split(f"int {name}(")[1].split(");")[0].count(",") + 1, name
    assert "a3v_beam.hip" in open(os.path.join(ROOT, "a3vlm_amd", "csrc", "Makefile")).read()
    from a3vlm_amd.model.meta import MetaModel
    assert callable(MetaModel.beam_search)


# ------------------------------------------------------------------ the eval entry's flags
def _eval_args(*argv):
    import argparse
    from a3vlm_amd import eval_affordance_v2 as ev
    return ev, argparse.ArgumentParser(parents=[ev.get_args_parser()]).parse_args(list(argv))


def test_eval_flags_default_to_the_path_as_it_was():
    ev, a = _eval_args()
    assert (a.num_beams, a.length_penalty, a.beam_early_stopping) == (0, 1.0, False) and ev.check_num_beams(a) == 0
    from a3vlm_amd import eval_affordance_with_quant as evq
    import argparse
    assert argparse.ArgumentParser(parents=[evq.get_args_parser()]).parse_args(["--num_beams", "2"]).num_beams == 2, "the shared parser"


@pytest.mark.parametrize("argv,match", [
    (["--num_beams", "9", "--continuous_rows", "16", "--temperature", "0"], "0 \\(off\\) .. 8"),
    (["--num_beams", "4", "--continuous_rows", "3", "--temperature", "0"], "--continuous_rows R with R >= 4"),
    (["--num_beams", "4", "--temperature", "0"], "--continuous_rows"),
    (["--num_beams", "2", "--continuous_rows", "2"], "--temperature 0"),
    (["--num_beams", "2", "--continuous_rows", "2", "--temperature", "0", "--num_samples", "2"], "--num_samples 1"),
    (["--num_beams", "2", "--continuous_rows", "2", "--temperature", "0", "--lookup_decoding", "3"], "--lookup_decoding 0"),
    (["--num_beams", "2", "--continuous_rows", "2", "--temperature", "0", "--repetition_penalty", "1.2"], "--repetition_penalty 1.0")])
def test_eval_flag_refusals_name_the_way_out(argv, match):
    ev, a = _eval_args(*argv)
    with pytest.raises(SystemExit, match=match):
        ev.check_num_beams(a)


def test_eval_flags_accept_beams_with_a_regex():
    ev, a = _eval_args("--num_beams", "4", "--continuous_rows", "8", "--temperature", "0", "--answer_regex", r"\[\d{1,3}\]",
                       "--length_penalty", "0.8", "--beam_early_stopping")
    assert ev.check_num_beams(a) == 4 and ev.check_num_samples(a) == 1 and ev.check_lookup(a) == 0 and ev.check_answer_regex(a)
    src = open(ev.__file__).read()
    assert src.index("num_beams = check_num_beams(args)") < src.index("MetaModel(args.llama_type"), "checked before the model is built"
