"""CPU: the regex -> token-automaton compiler (a3vlm_amd/model/constrain.py) against the brute-force oracle of tests/constrain_ref.py
(the language enumerated from ``re``'s own syntax tree), its refusals, and the mutation check of the reference kernels the GPU tests
compare a3v_constrain.hip with."""
import os
import random
import re

import numpy as np
import pytest

import constrain_ref as CR
from a3vlm_amd.model import constrain as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vocab():
    return CR.synthetic_vocabulary()


@pytest.fixture(scope="module")
def box(vocab):
    pieces, eos = vocab
    return C.compile_constraint(CR.BOX, pieces, eos, allow_leading_space=False), CR.Oracle(CR.BOX)


# ------------------------------------------------------------------ 1. the compiler against the oracle
def test_vocabulary_is_what_the_issue_asks_for(vocab):
    pieces, eos = vocab
    assert len(pieces) == 300 and pieces[eos] is None and "" in pieces and pieces.count(None) >= 4
    for p in ("0.", ",0", "12", "],", " [", "[", "5"):
        assert p in pieces, p


def test_box_automaton_agrees_with_the_oracle_on_every_sampled_prefix(vocab, box):
    pieces, eos = vocab
    A, oracle = box
    assert len(oracle.words) == 4096
    assert A.trans.dtype.is_floating_point is False and A.trans.shape == (A.n_states, len(pieces)) and A.trans.numpy().dtype == np.int16
    assert A.start == 0 and A.done == A.n_states - 1
    bad = CR.check_automaton(A, oracle, pieces, eos, max_prefixes=4000)
    assert not bad, bad[:5]
    t = A.trans.numpy()
    assert (t[:, [v for v, p in enumerate(pieces) if p is None and v != eos]] == -1).all(), "a piece that contributes no text is never allowed"
    assert (t[:, pieces.index("")] == -1).all(), "an empty piece is never allowed"
    assert (t[A.done, np.arange(len(pieces)) != eos] == -1).all() and t[A.done, eos] == A.done, "DONE allows only EOS"


@pytest.mark.parametrize("pattern,alphabet", [
    (r"(ab|a)(b|c)?x{0,2}", "abcx"),
    (r"[^a]b.{1,2}", "ab\n0"),
    (r"(?:0|1\.5){2}(,\d)?", "01.5,29"),
    (r"a?(b|)(c{2}|c)\\\.", "abc\\."),
    (r"\[(0|1)(,(0|1)){0,3}\]|none", "[]01,noe"),
])
@pytest.mark.parametrize("leading_space", [False, True])
def test_small_patterns_agree_with_the_oracle_on_every_prefix(pattern, alphabet, leading_space):
    rng = random.Random(1)
    chars = alphabet + " "
    pieces = [None, None, None, ""] + list(dict.fromkeys(chars)) + [" " + c for c in alphabet]
    seen = set(pieces[3:])
    while len(pieces) < 120:
        p = "".join(rng.choice(chars) for _ in range(rng.randint(2, 4)))
        if p not in seen:
            seen.add(p)
            pieces.append(p)
    eos = 2
    A = C.compile_constraint(pattern, pieces, eos, allow_leading_space=leading_space)
    oracle = CR.Oracle(pattern, alphabet + " ", leading_space=leading_space)
    bad = CR.check_automaton(A, oracle, pieces, eos, max_prefixes=10 ** 9)
    assert not bad, bad[:5]
    for w in oracle.words:
        assert A.accepts(w) and A.viable_prefix(w[:len(w) // 2])


def test_accepts_agrees_with_re_fullmatch(box):
    A, oracle = box
    rx = re.compile(CR.BOX)
    for w in oracle.words:
        assert A.accepts(w) and rx.fullmatch(w)
    rng = random.Random(7)
    words = sorted(oracle.words)
    n_match = 0
    for k in range(1000):
        if k % 2:                                         # a word with a few characters changed, dropped or doubled: near misses
            w = list(rng.choice(words))
            for _ in range(rng.randint(0, 2)):
                i = rng.randrange(len(w))
                w[i] = rng.choice(["", w[i] * 2, rng.choice("[]01.5,2 ")])
            s = "".join(w)
        else:
            s = "".join(rng.choice("[]01.5,2 ") for _ in range(rng.randint(0, 26)))
        want = rx.fullmatch(s) is not None
        n_match += want
        assert A.accepts(s) == want, s
        assert A.viable_prefix(s) == (s in oracle.prefixes), s
    assert 0 < n_match < 1000, n_match
    # the subset's other constructs against re on random strings
    for pattern, chars in ((r"(a|bc)*d+[^x-z]?", "abcdxyz"), (r".\d{2,3}(\.|,)?", "a1.,\n"), (r"[]a]+[a\-c]\]", "]a-c")):
        dfa = C.compile_regex(pattern)
        rx = re.compile(pattern)
        for _ in range(1000):
            s = "".join(rng.choice(chars) for _ in range(rng.randint(0, 6)))
            st = dfa.walk(0, s)
            assert (st >= 0 and bool(dfa.accepting[st])) == (rx.fullmatch(s) is not None), (pattern, s)


def test_the_golden_tokenizer_spells_a_box():
    from a3vlm_amd.model.tokenizer import Tokenizer
    tok = Tokenizer(os.path.join(ROOT, "tests", "golden", "tokenizer.model"))
    pieces = tok.pieces()
    assert len(pieces) == tok.n_words and pieces[tok.bos_id] is None and pieces[tok.eos_id] is None and pieces[0] is None
    assert all(p is None or "▁" not in p for p in pieces) and " t" in pieces and "[0." in pieces
    pattern = r"\[[01]\.\d{2}(, ?[01]\.\d{2}){3}\]"
    A = C.compile_constraint(pattern, pieces, tok.eos_id)
    text = "[0.12,0.50, 1.00,0.99]"
    s = A.start
    for t in tok.encode(text, bos=False, eos=True):        # SentencePiece's own segmentation walks the automaton to DONE
        s = int(A.trans[s, t])
        assert s >= 0, (t, pieces[t])
    assert s == A.done and A.accepts(text) and A.accepts(" " + text) and not A.accepts(text[:-1]) and A.viable_prefix(text[:-1])


# ------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("pattern,names", [
    (r"^a", "anchor"), (r"a$", "anchor"), (r"(a)\1", "back-reference"), (r"\w+", r"\\w"), (r"\s", r"\\s"), (r"a\b", r"\\b"),
    (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a{2}?", "lazy"), (r"a*+", "possessive"), (r"(?=a)b", r"\(\?"), (r"(?P<n>a)", r"\(\?"), (r"(?i)a", r"\(\?"),
    (r"a{2,}", "open-ended"), (r"a{,2}", "open-ended"), (r"a{", "repeat"), (r"a{3,2}", "repeat"), (r"(a", "unbalanced"), (r"a)", "unbalanced"),
    (r"[a", "unterminated"), (r"*a", "nothing to repeat"), (r"[[:alpha:]]", "POSIX"), (r"[z-a]", "reversed"), (r"\x41", r"\\x"),
    ("a\\", "trailing backslash"),
])
def test_constructs_outside_the_subset_raise_naming_the_construct(pattern, names):
    with pytest.raises(ValueError, match=names):
        C.compile_regex(pattern)
    with pytest.raises(ValueError, match=names):
        C.compile_constraint(pattern, ["a", None], 1)


def test_dead_end_under_the_vocabulary_is_refused_with_the_prefix(vocab):
    pieces, eos = vocab
    # the vocabulary has no 'q': after "[0." + "0" the automaton cannot go on
    with pytest.raises(ValueError, match=r"dead end.*after the prefix '\[0\.0' the automaton has no allowed token"):
        C.compile_constraint(r"\[0\.0q\]", pieces, eos, allow_leading_space=False)
    # nothing can even start
    with pytest.raises(ValueError, match=r"dead end.*after the prefix ''"):
        C.compile_constraint(r"qq", pieces, eos, allow_leading_space=False)
    with pytest.raises(ValueError, match=r"dead end.*after the prefix ' '"):      # the optional leading space is spelled, then nothing
        C.compile_constraint(r"qq", pieces, eos)
    # tokens exist but only go round: "a" then "bb" for ever, the closing "c" cannot be spelled -- no state on the way can reach
    # a match, the start (the shortest prefix) included
    with pytest.raises(ValueError, match=r"dead end.*after the prefix '' the automaton allows only tokens that never lead to a match"):
        C.compile_constraint(r"a(bb)*c", [None, None, None, "a", "bb"], 2, allow_leading_space=False)
    # an unreachable hole is no dead end: "ab" is one piece here, the state after a lone "a" is never entered
    A = C.compile_constraint(r"ab", [None, None, None, "ab"], 2, allow_leading_space=False)
    assert int(A.trans[0, 3]) >= 0


def test_too_many_states_and_too_large_a_table_are_refused():
    with pytest.raises(ValueError, match="32767"):
        C.compile_regex(r"(a|b)*a(a|b){15}")              # 2 ** 16 subsets
    with pytest.raises(ValueError, match="64 MiB"):
        C.compile_constraint(r"a{1000}", ["a"] + [None] * 40000, 1)      # 1002 states x 40001 tokens x 2 bytes
    with pytest.raises(ValueError, match="eos_id"):
        C.compile_constraint(r"a", ["a"], 5)
    with pytest.raises(ValueError, match="must be a TokenAutomaton or a pattern string"):
        C.check_constraint(3)


# ------------------------------------------------------------------ 3. the references notice a wrong kernel / a wrong table
def test_reference_mask_notices_a_mask_off_by_one_token():
    for B, V, ld in ((3, 9, 12), (1, 1, 1), (32, 511, 511)):
        x, trans, state = CR.logits_case(B, V, ld, seed=V)
        before = np.full_like(x, 0x12345678)
        want = CR.constrain_logits_ref(x, V, trans, state, before)
        assert (want[:, V:] == 0x12345678).all(), "padding columns are untouched"
        for b in range(B):
            s = int(state[b])
            if 0 <= s < trans.shape[0]:
                ok = trans[s] >= 0
                assert (want[b, :V][ok] == x[b, :V][ok]).all() and (want[b, :V][~ok] == CR.NEG_INF_BITS).all()
            else:
                assert (want[b, :V] == x[b, :V]).all()
        if V > 1:
            mutant = CR.constrain_logits_ref(x, V, np.roll(trans, 1, axis=1), state, before)
            assert not np.array_equal(mutant, want), (B, V)
    nan_kept = False
    x, trans, state = CR.logits_case(32, 511, 514, seed=3)
    want = CR.constrain_logits_ref(x, 511, trans, state, x)
    for b in range(32):
        s = int(state[b])
        if 0 <= s < trans.shape[0]:
            nan_kept |= bool(((want[b, :511] & 0x7FFFFFFF) > 0x7F800000).any())
    assert nan_kept, "the case carries NaN payloads in allowed slots"


def test_oracle_notices_eos_allowed_in_a_non_accepting_state(vocab, box):
    pieces, eos = vocab
    A, oracle = box
    import copy
    M = copy.copy(A)
    M.trans = A.trans.clone()
    s = A.dfa.walk(0, "[0.55")                             # a live state that does not accept
    assert s >= 0 and not A.dfa.accepting[s] and int(M.trans[s, eos]) == -1
    M.trans[s, eos] = A.done
    bad = CR.check_automaton(M, oracle, pieces, eos, max_prefixes=10 ** 9)
    assert bad and all(v == eos and want == -1 for _, v, _, want in bad)
    # and a mask off by one token at the table level
    M.trans = A.trans.roll(1, dims=1)
    assert CR.check_automaton(M, oracle, pieces, eos, max_prefixes=500)


def test_reference_advance_notices_a_state_that_advances_on_a_prompt_token():
    noticed = 0
    for case in CR.advance_cases():
        want = CR.constrain_advance_ref(**case)
        mutant = CR.constrain_advance_ref(**case, honour_first=False)
        noticed += not np.array_equal(want, mutant)
        st, n_states = case["state"], case["trans"].shape[0]
        out_of_range = (st < 0) | (st >= n_states)
        assert (want[out_of_range] == st[out_of_range]).all(), "an unconstrained row stays one"
        assert (want[3:6] == st[3:6]).all(), "ids outside [0, V) change nothing"
        if case["stopped_before"] is not None:
            assert (want[case["stopped_before"]] == st[case["stopped_before"]]).all()
        assert (want != st).any()
    assert noticed == len(CR.advance_cases()), noticed
