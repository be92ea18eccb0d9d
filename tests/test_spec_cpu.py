"""CPU (-m "not gpu") checks of lookup decoding: the entry points exist in the header, the built library and the ctypes table; the
draft and accept rules of tests/spec_ref.py on hand-written rows; the host's position bound on random scripts of acceptances; the
eval parsers take --lookup_decoding; generate_many's refusals are raised with no GPU."""
import os
import random
import re

import pytest

import spec_ref as S
from a3vlm_amd.model.ragged import LookupBound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("a3v_rope_kvcache_spans", "a3v_attention_verify_rows", "a3v_attention_verify_rows_splits", "a3v_lookup_draft_rows",
           "a3v_accept_rows", "a3v_llama_decode_step_verify", "a3v_llama_decode_step_verify_form")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from a3vlm_amd import lib
    return lib


def test_entries_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = built.load()
    for name in ENTRIES:
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in include/a3vlm_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    # refusals that need no device: the pointers of a refused call are never used
    p = 4096
    assert lib.a3v_llama_decode_step_verify_form(5, 8, 512, 4, 4, 128, 1536, 0) == 0                  # B * Q > 32
    assert lib.a3v_llama_decode_step_verify_form(2, 9, 512, 4, 4, 128, 1536, 0) == 0                  # Q > 8
    assert lib.a3v_rope_kvcache_spans(p, 256, p, 256, p, p, p, p, p, 1, 9, 2, 2, 64, 64, 0, None) == -1
    assert lib.a3v_lookup_draft_rows(p, 8, p, p, p, p, p, 1, 8, 3, 64, p, p, None) == -1              # D > 7
    assert lib.a3v_accept_rows(None, 8, 1, 2, 8, p, p, p, 8, p, p, 0, None, None, 0, p, p, p, p, None, None) == -3
    assert lib.a3v_attention_verify_rows_splits(1, 8, 64) == lib.a3v_attention_decode_rows_splits(1, 8, 64) == 1
    assert lib.a3v_attention_verify_rows_splits(3, 8, 300) == lib.a3v_attention_decode_rows_splits(3, 8, 300) > 1


# ------------------------------------------------------------------ the draft rule
def _draft(row, D=3, ngram=3, limit=None, pos=None, Smax=1000, stopped=False):
    c = len(row)
    t = row + [0] * 16
    x, nq = S.lookup_draft_rows([t], [c], [limit if limit is not None else c + 16], [pos if pos is not None else c - 1], [stopped],
                                [row[-1]], D, ngram, Smax)
    return x[0], nq[0]


def test_draft_the_longest_ngram_wins():
    # tail (7, 8): the 2-gram occurs at i = 1 (followed by 9), the 1-gram (8) occurs later at i = 5 (followed by 4): n = 2 is tried first
    assert _draft([5, 7, 8, 9, 1, 8, 4, 2, 7, 8], ngram=2) == ([8, 9, 1, 8], 4)
    assert _draft([5, 7, 8, 9, 1, 8, 4, 2, 7, 8], ngram=1) == ([8, 4, 2, 7], 4)


def test_draft_the_latest_match_wins():
    assert _draft([3, 4, 10, 11, 3, 4, 20, 21, 3, 4], ngram=2) == ([4, 20, 21, 3], 4)


def test_draft_a_match_that_ends_at_cur_minus_1_gives_one_draft():
    # c = [9, 6, 6]: tail (6) matches at i = 1, i + n = 2 = cur - 1: only c[2] is behind it
    assert _draft([9, 6, 6], ngram=3) == ([6, 6, 0, 0], 2)


def test_draft_no_match_and_rows_that_do_not_run():
    assert _draft([1, 2, 3, 4]) == ([4, 0, 0, 0], 1)
    assert _draft([3, 4, 3, 4], stopped=True) == ([4, 0, 0, 0], 1)
    assert _draft([3, 4, 3, 4], pos=-1) == ([4, 0, 0, 0], 1)
    assert _draft([7]) == ([7, 0, 0, 0], 1)                       # nothing in front of the last token


def test_draft_clamps_by_limit_and_by_the_cache():
    row = [3, 4, 10, 11, 12, 3, 4]
    assert _draft(row, ngram=2) == ([4, 10, 11, 12], 4)
    assert _draft(row, ngram=2, limit=len(row) + 2) == ([4, 10, 0, 0], 2)      # indices cur, cur + 1 are writable: one draft
    assert _draft(row, ngram=2, limit=len(row) + 1) == ([4, 0, 0, 0], 1)
    assert _draft(row, ngram=2, pos=97, Smax=100) == ([4, 10, 11, 0], 3)       # positions 97, 98, 99
    assert _draft(row, ngram=2, pos=99, Smax=100) == ([4, 0, 0, 0], 1)
    assert _draft(row, D=1, ngram=2) == ([4, 10], 2)


# ------------------------------------------------------------------ the accept rule
def _onehot(ids, V=16):
    return [[1.0 if i == t else 0.0 for i in range(V)] for t in ids]


def _accept(model_ids, x, nq, row, limit, stops=()):
    """one cache row, Q = len(x): the model's choices per query, the drafts, the row's tokens so far"""
    Q = len(x)
    tokens = [row + [0] * 12]
    cur, lim, stopped, stop_pos, stats = [len(row)], [limit], [False], [len(row) + 1], [0, 0]
    nt, ps = S.accept_rows(_onehot(model_ids + [0] * (Q - len(model_ids))), [x], [nq], tokens, cur, lim, 5, stops, stopped, stop_pos, stats)
    return tokens[0][len(row):cur[0]], cur[0], stopped[0], stop_pos[0], nt[0], ps[0], stats


def test_accept_all_drafts():
    out = _accept([7, 8, 9, 10], [6, 7, 8, 9], 4, [1, 2, 6], 20)
    assert out == ([7, 8, 9, 10], 7, False, 7, 10, 5 + 7 - 1, [3, 3])


def test_accept_first_draft_rejected():
    out = _accept([7, 8, 9, 10], [6, 5, 8, 9], 4, [1, 2, 6], 20)
    assert out == ([7], 4, False, 4, 7, 5 + 4 - 1, [3, 0])


def test_accept_only_live_drafts_count():
    out = _accept([7, 8, 9, 10], [6, 7, 8, 9], 2, [1, 2, 6], 20)          # nq = 2: one draft, whatever x holds behind it
    assert out == ([7, 8], 5, False, 5, 8, 5 + 5 - 1, [1, 1])


def test_accept_stop_sequence_completed_by_an_accepted_draft():
    # the stop sequence (8, 9) is completed by the emission of t_2 = 9: the row stops there, t_3 is not emitted
    out = _accept([7, 8, 9, 10], [6, 7, 8, 9], 4, [1, 2, 6], 20, stops=((15,), (8, 9)))
    assert out == ([7, 8, 9], 6, True, 4, 0, -1, [3, 2])


def test_accept_limit_reached_in_the_middle():
    out = _accept([7, 8, 9, 10], [6, 7, 8, 9], 4, [1, 2, 6], 5)            # indices 3 and 4 are writable
    assert out == ([7, 8], 5, True, 5, 0, -1, [3, 1])


def test_accept_leaves_a_stopped_row_alone():
    tokens, cur, stopped, stop_pos, stats = [[1, 2, 0, 0]], [2], [True], [2], [0, 0]
    assert S.accept_rows(_onehot([3, 3]), [[2, 3]], [2], tokens, cur, [4], 0, (), stopped, stop_pos, stats) == ([0], [-1])
    assert (tokens, cur, stopped, stop_pos, stats) == ([[1, 2, 0, 0]], [2], [True], [2], [0, 0])


# ------------------------------------------------------------------ the position bound
def test_position_bound_on_random_scripts():
    rng = random.Random(5)
    for trial in range(200):
        Q, rows, Smax = rng.randint(1, 8), rng.randint(1, 4), 96
        bound = LookupBound(rows, Q)
        true, last, ended = [None] * rows, [0] * rows, [False] * rows    # a row that ended on the device counts until it is read
        for step in range(60):
            for r in range(rows):
                if true[r] is None and rng.random() < 0.5:
                    start = rng.randint(0, 40)
                    last[r] = min(start + rng.randint(0, 50), Smax - 1)
                    true[r], ended[r] = start, False
                    bound.start(r, start, last[r])
            held = [r for r in range(rows) if true[r] is not None]
            if not held:
                continue
            pos_max = bound.step()
            assert pos_max >= max(true[r] for r in held if not ended[r]) if any(not ended[r] for r in held) else True, (trial, step)
            assert 0 <= pos_max < Smax, (trial, step, pos_max)
            for r in held:                                         # the device accepts 0 .. Q - 1 drafts, or the row ends
                if ended[r]:
                    continue
                nxt = true[r] + rng.randint(1, Q)
                if nxt > last[r] or rng.random() < 0.05:
                    ended[r] = True
                else:
                    true[r] = nxt
            if step % 4 == 3:                                      # the read-back: finished rows leave, the others are exact again
                for r in held:
                    if ended[r]:
                        bound.release(r)
                        true[r] = None
                    else:
                        bound.resync(r, true[r])
                        assert bound.bound[r] == true[r]


# ------------------------------------------------------------------ parsers and refusals
def test_eval_parsers_take_lookup_decoding():
    import argparse

    from a3vlm_amd import eval_affordance_v2 as e2
    from a3vlm_amd import eval_affordance_with_quant as eq
    a = argparse.ArgumentParser(parents=[e2.get_args_parser()]).parse_args(["--lookup_decoding", "3", "--continuous_rows", "2", "--temperature", "0"])
    assert a.lookup_decoding == 3 and e2.check_lookup(a) == 3
    assert eq.get_parser().parse_args(["--lookup_decoding", "2"]).lookup_decoding == 2
    assert argparse.ArgumentParser(parents=[e2.get_args_parser()]).parse_args([]).lookup_decoding == 0
    for argv, word in ((["--lookup_decoding", "3"], "--continuous_rows"),
                       (["--lookup_decoding", "3", "--continuous_rows", "2"], "--temperature 0"),
                       (["--lookup_decoding", "3", "--continuous_rows", "9", "--temperature", "0"], "<= 32"),
                       (["--lookup_decoding", "8", "--continuous_rows", "1", "--temperature", "0"], "7")):
        with pytest.raises(SystemExit, match=word):
            e2.check_lookup(argparse.ArgumentParser(parents=[e2.get_args_parser()]).parse_args(argv))


def test_generate_many_lookup_refusals_need_no_gpu():
    from a3vlm_amd.model.meta import MetaModel
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=64)
    for kw, word in ((dict(lookup=3, temperature=0.5), "temperature=0"),
                     (dict(lookup=3, temperature=0.5, n=2, batch_rows=2), "temperature=0"),
                     (dict(lookup=3, repetition_penalty=1.2), "repetition_penalty=1.0"),
                     (dict(lookup=3, return_logprobs=True), "return_logprobs=False"),
                     (dict(lookup=3, batch_rows=9), "batch_rows <= 8"),
                     (dict(lookup=8), "1 .. 7")):
        kw = {"batch_rows": 1, **kw}
        with pytest.raises(ValueError, match=word):
            mm.generate_many(["Lid?"], None, max_gen_len=2, **kw)
    with pytest.raises(ValueError, match="n=1"):
        # n > 1 needs temperature > 0, which lookup refuses first; at temperature 0 the existing n-check names its own way out
        mm.generate_many(["Lid?"], None, batch_rows=2, max_gen_len=2, n=2, lookup=3)
