"""CPU (-m "not gpu") checks of lookup decoding's sample-and-match form: the entries exist in the header, the built library and
the ctypes table and refuse bad arguments with no device; the restatements of tests/spec_ctl_ref.py on hand-worked cases, each with
the mutation that a plausible wrong implementation would be; generate_many's new refusals, and the old ones with lookup_verify left
at its default; the eval parsers."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import genctl_ref as G
import spec_ctl_ref as SC
import spec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("a3v_verify_prepare", "a3v_accept_rows_chosen", "a3v_verify_uniforms")


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
    assert "a3v_spec_ctl.hip" in open(os.path.join(ROOT, "a3vlm_amd", "csrc", "Makefile")).read()
    # refusals that need no device: the pointers of a refused call are never used
    p, q = 4096, 8192
    vp = lib.a3v_verify_prepare
    assert vp(None, 64, 1, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, q, 64, None) == -3         # NULL logits
    assert vp(p, 64, 1, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, None, 64, None) == -3         # NULL out
    assert vp(p, 64, 1, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, p, 64, None) == -3            # out aliases logits
    assert vp(p, 63, 1, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, q, 64, None) == -3            # ld < V
    assert vp(p, 64, 1, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, q, 63, None) == -3            # ld_out < V
    assert vp(p, 64, 0, 2, 64, p, p, p, None, 0, 1.0, None, 0, None, None, q, 64, None) == -3            # B <= 0
    assert vp(p, 64, 1, 2, 64, p, p, p, p, 1, 1.2, None, 0, None, None, q, 64, None) == -3               # words_per_row < ceil(V / 32)
    assert vp(p, 64, 1, 2, 64, p, p, p, p, 2, 0.0, None, 0, None, None, q, 64, None) == -3               # penalty <= 0
    assert vp(p, 64, 1, 2, 64, p, p, p, None, 0, 1.0, p, 5, None, None, q, 64, None) == -3               # a table without states
    assert vp(p, 64, 1, 2, 64, p, p, p, None, 0, 1.0, p, 40000, p, None, q, 64, None) == -3              # n_states > 32767
    assert vp(p, 64, 1, 9, 64, p, p, p, None, 0, 1.0, None, 0, None, None, q, 64, None) == -1            # Q > 8
    ac = lib.a3v_accept_rows_chosen
    base = [p, 1, 2, p, p, p, 8, p, p, 0, None, None, 0, p, p, p, p, None]
    none = [None, 0, 0, None, None, 0, 0, None, None, 0, None, 0, None, None]
    assert ac(*([None] + base[1:] + none)) == -3                                                           # NULL chosen
    assert ac(*(base[:2] + [9] + base[3:] + none)) == -1                                                   # Q > 8
    assert ac(*(base[:12] + [1] + base[13:] + none)) == -3                                                 # stop sequences without arrays
    assert ac(*(base + [p, 64, 64, p, p, 4, 4, None, None, 0, None, 0, None, None])) == -3                 # log-probs without prompt_len
    assert ac(*(base + [None, 64, 64, None, p, 4, 4, p, None, 0, None, 0, None, None])) == -3              # log-probs without logits / lse
    assert ac(*(base + [None, 0, 64, None, None, 0, 0, p, p, 1, None, 0, None, None])) == -3               # bitmap rows too short
    assert ac(*(base + [None, 0, 64, None, None, 0, 0, p, None, 0, None, 0, p, None])) == -3               # states without a table
    assert lib.a3v_verify_uniforms(None, 4, p, p, p, 1, 2, p, None) == -3
    assert lib.a3v_verify_uniforms(p, 0, p, p, p, 1, 2, p, None) == -3
    assert lib.a3v_verify_uniforms(p, 4, p, p, p, 1, 9, p, None) == -1


# ------------------------------------------------------------------ the prepare rule
def _table():
    """3 states over 8 tokens: state 0 allows 1 -> 1 and 2 -> 2; state 1 allows 3 -> 0 and 4 -> 1; state 2 allows 5 -> 2 only."""
    t = np.full((3, 8), -1, dtype=np.int16)
    t[0, 1], t[0, 2] = 1, 2
    t[1, 3], t[1, 4] = 0, 1
    t[2, 5] = 2
    return t


def test_prepare_draft_prefix_joins_the_seen_set():
    V, Q = 8, 3
    z = torch.tensor([[1.0, 2.0, -1.0, 0.5, -0.5, 3.0, 0.0, -2.0]] * Q)
    x, nq, pos = [[6, 1, 2]], [3], [4]
    bm = G.seen_bitmap([[6]], V)                                  # the prompt holds token 6 (x[b][0] is in the bitmap already)
    out = SC.verify_prepare(z, x, nq, pos, seen_bm=bm, penalty=2.0)
    assert out[0].tolist() == [1.0, 2.0, -1.0, 0.5, -0.5, 3.0, 0.0, -2.0]          # query 0: only token 6 (0.0 * 2 = 0.0)
    assert out[1].tolist() == [1.0, 1.0, -1.0, 0.5, -0.5, 3.0, 0.0, -2.0]          # query 1: draft 1 is seen, positive: divided
    assert out[2].tolist() == [1.0, 1.0, -2.0, 0.5, -0.5, 3.0, 0.0, -2.0]          # query 2: drafts 1 and 2; non-positive: multiplied
    mutant = SC.verify_prepare(z, x, nq, pos, seen_bm=bm, penalty=2.0, drafts_in_seen=False)
    assert not torch.equal(mutant, out) and torch.equal(mutant[0], out[0])
    assert S.argmax_first(out[1].tolist()) == 5 and out[1, 1] == 1.0 and mutant[1, 1] == 2.0
    # a draft outside the vocabulary is ignored; an idle query is zeros
    out = SC.verify_prepare(z, [[6, 99, -3]], [2], pos, seen_bm=bm, penalty=2.0)
    assert torch.equal(out[1], out[0]) and out[2].tolist() == [0.0] * V
    assert SC.verify_prepare(z, x, nq, [-1], seen_bm=bm, penalty=2.0).abs().sum() == 0


def test_prepare_walks_the_constraint_state():
    V, Q, ninf = 8, 4, float("-inf")
    z = torch.arange(1.0, 9.0).repeat(Q, 1)
    t = _table()
    x, nq, pos = [[7, 1, 4, 3]], [4], [2]
    out = SC.verify_prepare(z, x, nq, pos, trans=t, state=[0])

    def allowed(row):
        return [i for i, v in enumerate(row.tolist()) if v != ninf]
    assert [allowed(out[j]) for j in range(Q)] == [[1, 2], [3, 4], [3, 4], [1, 2]]        # states 0, 1 (after 1), 1 (after 4), 0 (after 3)
    assert all(out[j, i] == z[j, i] for j in range(Q) for i in allowed(out[j]))
    mutant = SC.verify_prepare(z, x, nq, pos, trans=t, state=[0], walk_state=False)
    assert [allowed(mutant[j]) for j in range(Q)] == [[1, 2]] * Q and not torch.equal(mutant, out)
    # a forbidden draft at k = 1 kills queries 1.., at k = nq - 1 only the last one; the query in front masks the draft itself
    dead1 = SC.verify_prepare(z, [[7, 3, 4, 3]], nq, pos, trans=t, state=[0])
    assert allowed(dead1[0]) == [1, 2] and all(allowed(dead1[j]) == [] for j in (1, 2, 3)) and dead1[0, 3] == ninf
    dead3 = SC.verify_prepare(z, [[7, 1, 4, 5]], nq, pos, trans=t, state=[0])
    assert [allowed(dead3[j]) for j in range(Q)] == [[1, 2], [3, 4], [3, 4], []] and dead3[2, 5] == ninf
    assert allowed(SC.verify_prepare(z, [[7, 1, 99, 3]], nq, pos, trans=t, state=[0])[2]) == []        # an id outside the vocabulary
    # an out-of-range start state: unconstrained for every j
    for s in (-1, 3):
        assert torch.equal(SC.verify_prepare(z, x, nq, pos, trans=t, state=[s]), z)
    # penalty first, then the mask: a kept value is the penalised one
    bm = G.seen_bitmap([[]], V)
    both = SC.verify_prepare(z, x, nq, pos, seen_bm=bm, penalty=2.0, trans=t, state=[0])
    assert both[1, 3] == z[1, 3] and both[2, 4] == z[2, 4] / 2 and both[3, 1] == z[3, 1] / 2 and both[3, 2] == z[3, 2]


# ------------------------------------------------------------------ the accept rule
def _accept(chosen, logits, x, nq, *, limit=16, stops=((15,),), book=True, n_lp=8, use_choice=True, stopped=False, V=20):
    B, Q = len(x), len(x[0])
    tokens = [[1, 2, 6] + [0] * 13 for _ in range(B)]
    cur, lim, st, sp, stats = [3] * B, [limit] * B, [stopped] * B, [4] * B, [0, 0]
    kw = {}
    if book:
        kw = dict(logits=logits, lse=G.lse32(logits), logprob=torch.zeros(B, n_lp), prompt_len=[3] * B, seen_bm=G.seen_bitmap([[1, 2, 6]] * B, V),
                  trans=None, state=None, V=V)
    nt, ps = SC.accept_rows_chosen(chosen, x, nq, tokens, cur, lim, 5, stops, st, sp, stats, use_choice=use_choice, **kw)
    return dict(tokens=tokens, cur=cur, stopped=st, stop_pos=sp, stats=stats, next_tok=nt, pos=ps, **kw)


def test_accept_follows_the_choice_not_the_argmax():
    Q, V = 4, 20
    logits = torch.zeros(Q, V)
    for j, t in enumerate([7, 8, 9, 10]):
        logits[j, t] = 5.0                                          # the raw argmax of query j
    x, nq = [[6, 7, 8, 9]], [4]
    greedy = _accept([7, 8, 9, 10], logits, x, nq)
    assert greedy["tokens"][0][3:7] == [7, 8, 9, 10] and greedy["cur"] == [7] and greedy["stats"] == [3, 3]
    # the choice (a sample, or the argmax of the PREPARED row) differs from the raw argmax at query 1: the run ends there
    chosen = [7, 11, 9, 10]
    got = _accept(chosen, logits, x, nq)
    assert got["tokens"][0][3:6] == [7, 11, 0] and got["cur"] == [5] and got["stats"] == [3, 1] and got["next_tok"] == [11] and got["pos"] == [9]
    mutant = _accept(chosen, logits, x, nq, use_choice=False)
    assert mutant["tokens"] != got["tokens"] and mutant["tokens"] == greedy["tokens"]
    # the bookkeeping of the two emissions: raw logits of the producing query, bits of both ids, nothing else
    lse = G.lse32(logits)
    assert got["logprob"][0, :3].tolist() == [float(logits[0, 7] - lse[0]), float(logits[1, 11] - lse[1]), 0.0]
    assert torch.equal(got["seen_bm"], G.seen_bitmap([[1, 2, 6, 7, 11]], V))
    # all bookkeeping off: the integer outputs are the same
    bare = _accept(chosen, logits, x, nq, book=False)
    assert all(bare[k] == got[k] for k in ("tokens", "cur", "stopped", "stop_pos", "stats", "next_tok", "pos"))
    # with the argmax as the choice the rule is spec_ref.accept_rows
    tokens = [[1, 2, 6] + [0] * 13]
    cur, lim, st, sp, stats = [3], [16], [False], [4], [0, 0]
    nt, ps = S.accept_rows(logits.tolist(), x, nq, tokens, cur, lim, 5, ((15,),), st, sp, stats)
    assert (tokens, cur, st, sp, stats, nt, ps) == tuple(greedy[k] for k in ("tokens", "cur", "stopped", "stop_pos", "stats", "next_tok", "pos"))


def test_accept_records_the_stopping_token_and_nothing_behind_it():
    Q, V = 4, 20
    logits = torch.randn(Q, V, generator=torch.Generator().manual_seed(1))
    x, nq = [[6, 7, 8, 9]], [4]
    got = _accept([7, 8, 9, 10], logits, x, nq, stops=((15,), (7, 8)))      # the stop sequence completes at the second emission
    assert got["cur"] == [5] and got["stopped"] == [True] and got["stop_pos"] == [3] and got["next_tok"] == [0] and got["pos"] == [-1]
    assert torch.equal(got["seen_bm"], G.seen_bitmap([[1, 2, 6, 7, 8]], V))                  # 8 stops the row and is recorded; 9 is not
    assert got["logprob"][0, 1] != 0 and got["logprob"][0, 2:].abs().sum() == 0
    lim = _accept([7, 8, 9, 10], logits, x, nq, limit=5)                                     # the limit in the middle of the run
    assert lim["cur"] == [5] and lim["stopped"] == [True] and lim["stop_pos"] == [5] and lim["stats"] == [3, 1]
    short = _accept([7, 8, 9, 10], logits, x, nq, n_lp=2)                                    # g >= n_lp is not written, the bits are
    assert short["cur"] == [7] and short["logprob"].shape == (1, 2) and torch.equal(short["seen_bm"], G.seen_bitmap([[1, 2, 6, 7, 8, 9, 10]], V))
    idle = _accept([7, 8, 9, 10], logits, x, nq, stopped=True)
    assert idle["cur"] == [3] and idle["tokens"][0][3] == 0 and idle["stats"] == [0, 0] and idle["logprob"].abs().sum() == 0


def test_accept_advances_the_state_per_emission():
    t = _table()
    logits = torch.zeros(3, 8)
    tokens, cur, state = [[0, 0, 0, 0, 0, 0]], [1], np.array([0], dtype=np.int32)
    SC.accept_rows_chosen([1, 4, 3], [[7, 1, 4]], [3], tokens, cur, [6], 0, ((2,),), [False], [2], [0, 0], prompt_len=[1], trans=t, state=state,
                          V=8)
    assert tokens[0][1:4] == [1, 4, 3] and cur == [4] and state.tolist() == [0]                # 0 -1-> 1 -4-> 1 -3-> 0
    state = np.array([0], dtype=np.int32)
    SC.accept_rows_chosen([1, 3, 3], [[7, 1, 4]], [3], [[0] * 6], [1], [6], 0, ((2,),), [False], [2], [0, 0], prompt_len=[1], trans=t, state=state,
                          V=8)
    assert state.tolist() == [0]                                                               # 0 -1-> 1 -3-> 0: the run ended at the mismatch
    assert SC.uniform_index([10, 40], [5, 9], [3, 9], 3, 45) == [12, 13, 14, 40, 41, 42]
    assert SC.uniform_index([43], [5], [3], 3, 45) == [44, 44, 44] and SC.uniform_index([0], [0], [3], 2, 45) == [0, 0]


# ------------------------------------------------------------------ the host's refusals and the parsers
@pytest.fixture(scope="module")
def mm():
    from a3vlm_amd.model.meta import MetaModel
    return MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=64)


def test_choice_refusals_need_no_gpu(mm):
    for kw, word in ((dict(lookup=3, temperature=0.5, n=2, batch_rows=2), "n=1"),
                     (dict(lookup=3, batch_rows=9), "batch_rows <= 8"),
                     (dict(lookup=8), "1 .. 7"),
                     (dict(lookup=-1), "1 .. 7"),
                     (dict(lookup=3, lookup_ngram=0), "lookup_ngram"),
                     (dict(lookup=3, repetition_penalty=0.0), "repetition_penalty must be > 0"),
                     (dict(lookup=3, constraint=7), "TokenAutomaton or a pattern string")):
        with pytest.raises(ValueError, match=word):
            mm.generate_many(["Lid?"], None, max_gen_len=2, lookup_verify="choice", **{"batch_rows": 1, **kw})
    for lookup in (0, 3):
        with pytest.raises(ValueError, match="'argmax'.*'choice'"):
            mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=2, lookup=lookup, lookup_verify="sample")


def test_old_refusals_still_fire_at_the_default(mm):
    for kw, word, names_choice in ((dict(lookup=3, temperature=0.5), "temperature=0", True),
                                   (dict(lookup=3, repetition_penalty=1.2), "repetition_penalty=1.0", True),
                                   (dict(lookup=3, return_logprobs=True), "return_logprobs=False", True),
                                   (dict(lookup=3, constraint=r"\[0\]"), "lookup=0", True),
                                   (dict(lookup=3, batch_rows=9), "batch_rows <= 8", False),
                                   (dict(lookup=8), "1 .. 7", False)):
        for extra in ({}, {"lookup_verify": "argmax"}):
            with pytest.raises(ValueError, match=word) as e:
                mm.generate_many(["Lid?"], None, max_gen_len=2, **{"batch_rows": 1, **kw, **extra})
            assert ("lookup_verify='choice'" in str(e.value)) == names_choice          # the way out these messages now also name
    with pytest.raises(ValueError, match="n=1"):
        mm.generate_many(["Lid?"], None, batch_rows=2, max_gen_len=2, n=2, lookup=3)


def test_eval_parsers_take_lookup_verify():
    from a3vlm_amd import eval_affordance_v2 as e2
    from a3vlm_amd import eval_affordance_with_quant as eq

    def parse(argv):
        return argparse.ArgumentParser(parents=[e2.get_args_parser()]).parse_args(argv)
    assert parse([]).lookup_verify == "argmax" and eq.get_parser().parse_args(["--lookup_verify", "choice"]).lookup_verify == "choice"
    with pytest.raises(SystemExit):
        parse(["--lookup_verify", "sample"])
    a = parse(["--lookup_decoding", "3", "--lookup_verify", "choice", "--continuous_rows", "2", "--temperature", "0.1", "--answer_regex", r"\[\d\]",
               "--repetition_penalty", "1.2", "--save_scores"])
    assert e2.check_lookup(a) == 3 and e2.check_answer_regex(a) == r"\[\d\]"
    for argv, word in ((["--lookup_decoding", "3", "--lookup_verify", "choice", "--continuous_rows", "2", "--num_samples", "2"], "--num_samples 1"),
                       (["--lookup_decoding", "3", "--lookup_verify", "choice"], "--continuous_rows"),
                       (["--lookup_decoding", "3", "--lookup_verify", "choice", "--continuous_rows", "9"], "<= 32"),
                       (["--lookup_decoding", "8", "--lookup_verify", "choice", "--continuous_rows", "1"], "7"),
                       (["--lookup_decoding", "3", "--continuous_rows", "2"], "--temperature 0"),
                       (["--lookup_decoding", "3", "--lookup_verify", "argmax", "--continuous_rows", "2"], "--temperature 0")):
        with pytest.raises(SystemExit, match=word):
            e2.check_lookup(parse(argv))
    for verify in ([], ["--lookup_verify", "argmax"]):
        with pytest.raises(SystemExit, match="--lookup_decoding 0"):
            e2.check_answer_regex(parse(["--lookup_decoding", "3", "--continuous_rows", "2", "--temperature", "0", "--answer_regex", r"\[\d\]"] + verify))
    # a namespace without the field (the existing tests build such) behaves as before
    ns = argparse.Namespace(lookup_decoding=3, continuous_rows=2, temperature=0.5, num_samples=1)
    with pytest.raises(SystemExit, match="--temperature 0"):
        e2.check_lookup(ns)
    with pytest.raises(SystemExit, match="--lookup_decoding 0"):
        e2.check_answer_regex(argparse.Namespace(lookup_decoding=3, answer_regex=r"\[\d\]"))
