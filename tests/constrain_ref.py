"""Oracle of constrained decoding (a3vlm_amd/model/constrain.py, a3v_constrain.hip) that shares no code with the DFA compiler.

* The language of a pattern with bounded repeats is ENUMERATED from the syntax tree Python's own ``re`` parser builds (no NFA, no DFA):
  ``language(pattern)`` is the finite set of its words, ``Oracle(pattern)`` answers ``allowed(prefix, piece)`` (some word starts with
  prefix + piece) and ``eos_allowed(prefix)`` (prefix is a word) by set look-ups.
* ``constrain_logits_ref`` / ``constrain_advance_ref`` restate the two kernels in plain numpy on integers (bit patterns in, bit
  patterns out), and the ``*_cases`` builders make the inputs both the CPU mutation checks and the GPU tests run on.
* ``check_automaton`` compares a ``TokenAutomaton`` with the oracle over every prefix of the language and returns the mismatches."""
import itertools
import random

import numpy as np

try:
    from re import _parser as sre_parse
    from re import _constants as sre
except ImportError:                                   # Python < 3.11
    import sre_constants as sre
    import sre_parse

NEG_INF_BITS = 0xFF800000
BOX = r"\[[01]\.[05]{2}(,[01]\.[05]{2}){3}\]"          # the answer's shape over a reduced digit set: (2 * 4) ** 4 = 4096 words


# ---------------------------------------------------------------------------------------------------------------- the language
def _set_chars(items, alphabet):
    chars, negate = set(), False
    for op, av in items:
        if op is sre.NEGATE:
            negate = True
        elif op is sre.LITERAL:
            chars.add(chr(av))
        elif op is sre.RANGE:
            chars.update(chr(c) for c in range(av[0], av[1] + 1))
        elif op is sre.CATEGORY and av is sre.CATEGORY_DIGIT:
            chars.update("0123456789")
        else:
            raise NotImplementedError((op, av))
    return sorted(set(alphabet) - chars) if negate else sorted(chars)


def _words(seq, alphabet, cap):
    """the set of words of a parsed sequence: the concatenation of its items' word sets"""
    out = {""}
    for op, av in seq:
        if op is sre.LITERAL:
            part = {chr(av)}
        elif op is sre.NOT_LITERAL:
            part = set(alphabet) - {chr(av)}
        elif op is sre.ANY:
            part = set(alphabet) - {"\n"}
        elif op is sre.IN:
            part = set(_set_chars(av, alphabet))
        elif op is sre.BRANCH:
            part = set().union(*(_words(alt, alphabet, cap) for alt in av[1]))
        elif op is sre.SUBPATTERN:
            part = _words(av[-1], alphabet, cap)
        elif op is sre.MAX_REPEAT:
            lo, hi, sub = av
            assert hi is not sre.MAXREPEAT, "the oracle enumerates finite languages: bounded repeats only"
            one = _words(sub, alphabet, cap)
            part, power = set(), {""}
            for k in range(hi + 1):
                if k >= lo:
                    part |= power
                if k < hi:
                    power = {a + b for a in power for b in one}
                    assert len(power) <= cap, "language too large to enumerate"
        else:
            raise NotImplementedError(op)
        out = {a + b for a in out for b in part}
        assert len(out) <= cap, "language too large to enumerate"
    return out


def language(pattern, alphabet="", cap=200000):
    """Every word of ``pattern`` (``alphabet``: the characters '.' and negated classes range over)."""
    return _words(sre_parse.parse(pattern), alphabet, cap)


class Oracle:
    def __init__(self, pattern, alphabet="", leading_space=False):
        self.words = language(pattern, alphabet)
        if leading_space:
            self.words = self.words | {" " + w for w in self.words}
        self.prefixes = {w[:k] for w in self.words for k in range(len(w) + 1)}

    def allowed(self, prefix, piece):
        return bool(piece) and (prefix + piece) in self.prefixes

    def eos_allowed(self, prefix):
        return prefix in self.words


def synthetic_vocabulary(seed=0):
    """About 300 pieces around the box alphabet: every single character, multi-character pieces ("0.", ",0", "12", "],", ...), pieces
    with a leading space, an empty piece, pieces that contribute no text (None) and pieces of other characters.  Returns
    (pieces, eos_id)."""
    rng = random.Random(seed)
    chars = "[]01.5,"
    pieces = [None, None, None, ""]                       # <unk>, <s>, </s> (id 2 = eos), an empty piece
    pieces += list(chars) + list("23456789 abxyz-")
    pieces += ["0.", ",0", "12", "],", "[0", "[1.", ".5", ".0", "00", "05", "50", "55", "5,", "0,", "5]", "0]", "]]", ",,", "0.5", "1.0",
               ",1.", "[0.0", "[0.05", "00,", "55,1", "05]", ".55,", "5,0.5", "0,1.0", "50]", "1.50,0.05"]
    pieces += [" [", " [0", " [1.", " 0", " ,", " ", "  ", " [0.5", " ]"]
    seen = set(p for p in pieces if p)
    while len(pieces) < 300:
        p = "".join(rng.choice(chars + chars + "2 a") for _ in range(rng.randint(2, 5)))
        if p not in seen:
            seen.add(p)
            pieces.append(p)
    pieces[150] = None                                    # a control token in the middle of the vocabulary
    return pieces, 2


def check_automaton(A, oracle, pieces, eos_id, max_prefixes=4000, seed=0):
    """Mismatches between ``A.trans`` and the oracle over the prefixes of the language (all of them, or a seeded sample of
    ``max_prefixes`` that always holds the empty prefix and every word): a list of (prefix, token id, got, want) -- empty when they agree."""
    prefixes = sorted(oracle.prefixes)
    if len(prefixes) > max_prefixes:
        rng = random.Random(seed)
        keep = {""} | set(rng.sample(sorted(oracle.words), min(len(oracle.words), max_prefixes // 4)))
        keep |= set(rng.sample(prefixes, max_prefixes - len(keep)))
        prefixes = sorted(keep)
    trans = A.trans.numpy()
    bad = []
    for prefix in prefixes:
        s = A.dfa.walk(0, prefix)
        if s < 0:
            bad.append((prefix, None, s, "a live state"))
            continue
        row = trans[s]
        for v, piece in enumerate(pieces):
            if v == eos_id:
                want = A.done if oracle.eos_allowed(prefix) else -1
            elif piece is not None and oracle.allowed(prefix, piece):
                want = A.dfa.walk(0, prefix + piece)      # the state of the longer prefix (>= 0: checked when its turn comes)
            else:
                want = -1
            if int(row[v]) != want:
                bad.append((prefix, v, int(row[v]), want))
    return bad


# ---------------------------------------------------------------------------------------------------------------- the kernels
def constrain_logits_ref(logits_bits, V, trans, state, out_bits):
    """logits_bits / out_bits: uint32 [B, ld] / [B, ld_out] (the fp32 bit patterns; out_bits is the buffer's content BEFORE the call).
    Returns the buffer after the call: columns [0, V) of a row with an in-range state are the input's bits where the token is
    allowed and -inf's elsewhere, of any other row the input's bits; columns [V, ld_out) keep what they held."""
    out = out_bits.copy()
    n_states = trans.shape[0]
    for b in range(logits_bits.shape[0]):
        s = int(state[b])
        row = logits_bits[b, :V]
        if 0 <= s < n_states:
            out[b, :V] = np.where(trans[s, :V] >= 0, row, np.uint32(NEG_INF_BITS))
        else:
            out[b, :V] = row
    return out


def constrain_advance_ref(tokens, col, cur, first, stopped_before, trans, state, *, honour_first=True):
    """The state array after a3v_constrain_advance.  ``honour_first=False`` is the mutant that advances on prompt tokens."""
    n_states, V = trans.shape
    new = np.array(state, dtype=np.int32).copy()
    B, ld_tok = tokens.shape
    for b in range(B):
        if stopped_before is not None and stopped_before[b]:
            continue
        c = int(cur[b]) - 1 if cur is not None else int(col)
        if c < 0 or c >= ld_tok:
            continue
        if honour_first and c < int(first[b]):
            continue
        s = int(new[b])
        if not 0 <= s < n_states:
            continue
        t = int(tokens[b, c])
        if not 0 <= t < V:
            continue
        new[b] = int(trans[s, t])
    return new


def random_table(n_states, V, seed, density=0.4):
    """an int16 table of random transitions, about ``density`` of them allowed; every state allows at least one token"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, n_states, size=(n_states, V), dtype=np.int64).astype(np.int16)
    t[rng.random((n_states, V)) >= density] = -1
    for s in range(n_states):
        if not (t[s] >= 0).any():
            t[s, rng.integers(0, V)] = s
    return t


def logits_case(B, V, ld, seed, n_states=5):
    """(bits uint32 [B, ld], trans, state int32 [B]): random finite values, +-inf, +-0 and NaNs with distinct payloads spread over
    the row (padding columns included); states span the range and include -1 and n_states (two unconstrained rows) when B allows."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, ld)).astype(np.float32).view(np.uint32).copy()
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001], dtype=np.uint32)
    idx = rng.integers(0, B * ld, size=max(B * ld // 7, 1))
    x.reshape(-1)[idx] = special[rng.integers(0, len(special), size=idx.size)]
    trans = random_table(n_states, V, seed + 1)
    cycle = [0, n_states - 1, -1, 2 % n_states, n_states, 1 % n_states, -7, 2 ** 31 - 1]
    state = np.array([cycle[b % len(cycle)] for b in range(B)], dtype=np.int32)
    if B == 1:
        state[0] = n_states - 1
    return x, trans, state


def advance_cases(seed=0):
    """Inputs of a3v_constrain_advance, both forms: a list of dicts (tokens int64 [B, ld_tok], col, cur or None, first, stopped_before
    or None, trans, state).  Rows cover: first above / at / below the column, stopped_before set and clear, tokens < 0 and >= V, states
    -1 and n_states, idle ragged rows (cur = 0, cur > ld_tok), and a forbidden token (the state becomes -1)."""
    rng = np.random.default_rng(seed)
    n_states, V, B, ld_tok = 6, 50, 70, 12                # 70 rows: more than one 64-thread block
    trans = random_table(n_states, V, seed + 3)
    tokens = rng.integers(0, V, size=(B, ld_tok)).astype(np.int64)
    tokens[3, :] = -1
    tokens[4, :] = V
    tokens[5, :] = 2 ** 40
    state = rng.integers(0, n_states, size=B).astype(np.int32)
    state[6], state[7], state[8] = -1, n_states, -2 ** 31
    first = rng.integers(0, ld_tok, size=B).astype(np.int32)
    stopped = (rng.random(B) < 0.3)
    stopped[:9] = False
    cases = []
    for col in (0, 5, ld_tok - 1):
        f = first.copy()
        f[0], f[1], f[2] = col + 1, col, max(col - 1, 0)  # above, at and below the column
        cases.append(dict(tokens=tokens, col=col, cur=None, first=f, stopped_before=stopped, trans=trans, state=state))
    cases.append(dict(tokens=tokens, col=4, cur=None, first=first, stopped_before=None, trans=trans, state=state))
    cur = rng.integers(1, ld_tok + 1, size=B).astype(np.int32)
    cur[9], cur[10], cur[11], cur[12] = 0, ld_tok + 1, -5, ld_tok    # idle, past the row, negative, the last column
    f = np.minimum(first, np.maximum(cur - 1, 0)).astype(np.int32)
    f[0], f[1], f[2] = cur[0], cur[1] - 1, 0
    cases.append(dict(tokens=tokens, col=0, cur=cur, first=f, stopped_before=stopped, trans=trans, state=state))
    cases.append(dict(tokens=tokens, col=0, cur=cur, first=f, stopped_before=None, trans=trans, state=state))
    return cases
