"""Constrained decoding, host side: a regular expression compiled to a token automaton (the device side is
a3v_constrain.hip / include/a3vlm_hip.h, "Constrained decoding").  Pure Python + numpy, no GPU: everything here runs, and every
refusal is raised, before the first launch.

    pattern --parse--> syntax tree --Thompson--> NFA --subset construction--> DFA --trim--> DFA whose every state can still accept
    DFA x vocabulary pieces --walk--> trans int16 [n_states, V]:  trans[s, v] = state after token v from state s, -1 = not allowed

The regex subset: literals and escapes (``\\.`` ``\\[`` ... and ``\\n`` ``\\t`` ``\\r``), ``.`` (any character but a newline, as
``re``), ``\\d`` ([0-9]), classes ``[...]`` with ranges and ``^`` negation, groups ``(...)`` / ``(?:...)``, ``|``, ``?``, ``*``, ``+``,
``{m}``, ``{m,n}``.  The match is always a full match; anything else raises ``ValueError`` naming the construct.

The alphabet of the DFA is the set of characters the pattern names plus ONE symbol for every other character (``.`` and negated
classes match it), so a vocabulary of arbitrary Unicode pieces walks the same small table."""
from __future__ import annotations

from collections import deque
from typing import Dict, FrozenSet, List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["TokenAutomaton", "compile_constraint", "compile_regex", "parse_regex", "MAX_STATES", "MAX_TABLE_BYTES"]

MAX_STATES = 32767                   # states are int16 in the device table
MAX_TABLE_BYTES = 64 << 20
MAX_REPEAT = 1000                    # {m,n} is expanded: a bound on n keeps a typo from building a million NFA states

_DIGITS = frozenset("0123456789")
_ESC_LITERAL = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v", "0": "\0"}
_ESC_REFUSED = {"w": "\\w (word class)", "W": "\\W (class)", "s": "\\s (space class)", "S": "\\S (class)", "D": "\\D (class)",
                "b": "\\b (word-boundary anchor)", "B": "\\B (anchor)", "A": "\\A (anchor)", "Z": "\\Z (anchor)", "z": "\\z (anchor)",
                "x": "\\x (hex escape)", "u": "\\u (unicode escape)", "U": "\\U (unicode escape)", "N": "\\N (named character)",
                "p": "\\p (unicode property)", "P": "\\P (unicode property)", "k": "\\k (named back-reference)", "g": "\\g (back-reference)"}


class CharSet:
    """A set of characters: ``chars``, or every character but ``chars`` when ``negated``."""
    __slots__ = ("chars", "negated")

    def __init__(self, chars, negated: bool = False):
        self.chars, self.negated = frozenset(chars), bool(negated)

    def __contains__(self, c: str) -> bool:
        return (c in self.chars) != self.negated


# ---------------------------------------------------------------------------------------------------------------- parser
# syntax tree: ("set", CharSet) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n) with n = None for unbounded
class _Parser:
    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"constraint pattern {self.p!r}: {what} at offset {self.i} is outside the supported regex subset "
                         "(literals, escapes, '.', '\\d', [...] classes, groups, '|', '?', '*', '+', '{m}', '{m,n}')")

    def peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.repeat())
        return items[0] if len(items) == 1 else ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "?":
                m, n = 0, 1
            elif c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "{":
                m, n = self.braces()
            else:
                return node
            if c != "{":
                self.i += 1
            if self.peek() == "?":
                self.fail("lazy quantifier")
            if self.peek() == "+":
                self.fail("possessive quantifier")
            node = ("rep", node, m, n)

    def braces(self) -> Tuple[int, int]:
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j >= 0 else ""
        parts = body.split(",")
        if j < 0 or len(parts) > 2 or not all(x.isascii() and x.isdigit() for x in parts):
            self.fail("repeat '{' that is not {m} or {m,n}" + (" (open-ended {m,} / {,n})" if j >= 0 and "" in parts else ""))
        m, n = int(parts[0]), int(parts[-1])
        if n < m or n > MAX_REPEAT:
            self.fail(f"repeat {{{body}}} (need m <= n <= {MAX_REPEAT})")
        self.i = j + 1
        return m, n

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    self.fail("group extension '(?' (look-around, named group or flags)")
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.klass())
        if c == ".":
            return ("set", CharSet("\n", negated=True))
        if c == "\\":
            return ("set", self.escape(in_class=False))
        if c in "^$":
            self.i -= 1
            self.fail(f"anchor '{c}' (the match is always a full match)")
        if c in "?*+{":
            self.i -= 1
            self.fail(f"quantifier '{c}' with nothing to repeat")
        if c == "}":
            self.i -= 1
            self.fail("unescaped '}'")
        return ("set", CharSet(c))

    def escape(self, in_class: bool) -> CharSet:
        c = self.peek()
        if c is None:
            self.fail("trailing backslash")
        self.i += 1
        if c == "d":
            return CharSet(_DIGITS)
        if c in _ESC_REFUSED and not (in_class and c == "b"):
            self.i -= 2
            self.fail(_ESC_REFUSED[c])
        if c.isdigit() and c != "0":
            self.i -= 2
            self.fail(f"back-reference \\{c}")
        if c in _ESC_LITERAL:
            return CharSet(_ESC_LITERAL[c])
        if c.isalnum():
            self.i -= 2
            self.fail(f"escape \\{c}")
        return CharSet(c)

    def klass(self) -> CharSet:
        negated = self.peek() == "^"
        if negated:
            self.i += 1
        chars, first = set(), True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unterminated '['")
            if c == "]" and not first:
                self.i += 1
                return CharSet(chars, negated)
            first = False
            if c == "[" and self.p[self.i:self.i + 2] in ("[:", "[.", "[="):
                self.fail("POSIX class '[:'")
            self.i += 1
            lo = self.escape(in_class=True) if c == "\\" else CharSet(c)
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                d = self.peek()
                self.i += 1
                hi = self.escape(in_class=True) if d == "\\" else CharSet(d)
                if len(lo.chars) != 1 or len(hi.chars) != 1:
                    self.fail("class range with a class escape as an end")
                a, b = ord(next(iter(lo.chars))), ord(next(iter(hi.chars)))
                if b < a:
                    self.fail(f"reversed class range {chr(a)}-{chr(b)}")
                if b - a > 4096:
                    self.fail(f"class range {chr(a)!r}-{chr(b)!r} wider than 4096 characters")
                chars.update(chr(x) for x in range(a, b + 1))
            else:
                chars.update(lo.chars)


def parse_regex(pattern: str):
    """The syntax tree of ``pattern`` (tests/constrain_ref.py enumerates finite languages from it)."""
    if not isinstance(pattern, str):
        raise ValueError(f"constraint pattern must be a str, got {type(pattern).__name__}")
    return _Parser(pattern).parse()


# ---------------------------------------------------------------------------------------------------------------- NFA / DFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edge: List[Optional[Tuple[CharSet, int]]] = []      # at most one character edge per state (Thompson)

    def state(self) -> int:
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """(entry, exit) of the fragment of ``node``"""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            self.edge[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.state()
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = self.state()
        for _ in range(m):                                       # m mandatory copies
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if n is None:                                            # then a star
            x, y = self.build(sub)
            end = self.state()
            self.eps[b] += [x, end]
            self.eps[y] += [x, end]
            return a, end
        end = self.state()
        for _ in range(n - m):                                   # then n - m optional copies, each may leave
            x, y = self.build(sub)
            self.eps[b] += [x, end]
            b = y
        self.eps[b].append(end)
        return a, end


class CharDFA:
    """``delta[s][k]`` = next state on symbol k (-1: dead), symbols = ``alphabet`` in order plus one last symbol for every other
    character; ``accepting[s]``.  Every state can reach an accepting one; state 0 is the start."""

    def __init__(self, alphabet: Sequence[str], delta: np.ndarray, accepting: np.ndarray):
        self.alphabet, self.delta, self.accepting = list(alphabet), delta, accepting
        self.sym: Dict[str, int] = {c: k for k, c in enumerate(self.alphabet)}
        self.other = len(self.alphabet)

    def walk(self, state: int, text: str) -> int:
        for c in text:
            if state < 0:
                return -1
            state = int(self.delta[state, self.sym.get(c, self.other)])
        return state


def _charsets(node, out: List[CharSet]):
    if node[0] == "set":
        out.append(node[1])
    elif node[0] == "rep":
        _charsets(node[1], out)
    else:
        for sub in node[1]:
            _charsets(sub, out)


def compile_regex(pattern: str, *, allow_leading_space: bool = False) -> CharDFA:
    tree = parse_regex(pattern)
    if allow_leading_space:
        tree = ("cat", [("rep", ("set", CharSet(" ")), 0, 1), tree])
    sets: List[CharSet] = []
    _charsets(tree, sets)
    alphabet = sorted(set().union(*(s.chars for s in sets))) if sets else []
    nfa = _NFA()
    entry, final = nfa.build(tree)
    n = len(nfa.eps)
    # epsilon closure of every NFA state, once
    closure: List[FrozenSet[int]] = []
    for s in range(n):
        seen, stack = {s}, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        closure.append(frozenset(seen))
    K = len(alphabet) + 1
    # per symbol, the character-edge targets of every NFA state (the last symbol: a character the pattern never names)
    step: List[List[int]] = []
    for k in range(K):
        c = alphabet[k] if k < K - 1 else None
        row = []
        for s in range(n):
            e = nfa.edge[s]
            row.append(e[1] if e is not None and ((c in e[0]) if c is not None else e[0].negated) else -1)
        step.append(row)
    start = closure[entry]
    ids: Dict[FrozenSet[int], int] = {start: 0}
    order, rows = [start], []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row = []
        for k in range(K):
            sk = step[k]
            nxt = set()
            for s in cur:
                t = sk[s]
                if t >= 0:
                    nxt |= closure[t]
            if not nxt:
                row.append(-1)
                continue
            key = frozenset(nxt)
            j = ids.get(key)
            if j is None:
                j = ids[key] = len(order)
                order.append(key)
                if j >= MAX_STATES:
                    raise ValueError(f"constraint pattern {pattern!r}: more than {MAX_STATES} DFA states (states are int16 on the device); "
                                     "simplify the pattern")
            row.append(j)
        rows.append(row)
    delta = np.array(rows, dtype=np.int32).reshape(len(order), K)
    acc = np.array([final in st for st in order], dtype=bool)
    # trim: keep the states from which an accepting state is reachable (backward reachability), renumber in BFS order from the start
    N = len(order)
    back: List[List[int]] = [[] for _ in range(N)]
    for s in range(N):
        for t in set(int(x) for x in delta[s] if x >= 0):
            back[t].append(s)
    live = acc.copy()
    stack = [int(s) for s in np.flatnonzero(acc)]
    while stack:
        for s in back[stack.pop()]:
            if not live[s]:
                live[s] = True
                stack.append(s)
    if not live[0]:
        raise ValueError(f"constraint pattern {pattern!r} matches no string at all")
    new = np.full(N + 1, -1, dtype=np.int32)                     # (index -1 -> -1)
    q, cnt = deque([0]), 1
    new[0] = 0
    kept = [0]
    while q:
        s = q.popleft()
        for t in delta[s]:
            t = int(t)
            if t >= 0 and live[t] and new[t] < 0:
                new[t] = cnt
                cnt += 1
                kept.append(t)
                q.append(t)
    d2 = delta[kept]
    d2 = np.where((d2 >= 0) & live[np.maximum(d2, 0)], new[d2], -1).astype(np.int32)
    return CharDFA(alphabet, d2, acc[kept])


# ---------------------------------------------------------------------------------------------------------------- tokens
class TokenAutomaton:
    """``trans`` int16 [n_states, V] on the CPU (``device_table`` moves it once per device and keeps it): ``trans[s, v]`` is the state
    after token v from state s, -1 when v is not allowed there.  States 0 .. n_states - 2 are the DFA's (``start`` = 0), the last one
    is DONE: reached by ``eos_id`` from an accepting state, and only ``eos_id`` (-> DONE) is allowed in it.

    ``accepts`` / ``viable_prefix`` speak about TEXT: a full match of the pattern / a prefix of one.  With ``allow_leading_space``
    the language is the pattern's with one optional space in front (the decoded text of an answer normally has lost it)."""

    def __init__(self, pattern: str, dfa: CharDFA, trans: torch.Tensor, eos_id: int, allow_leading_space: bool):
        self.pattern, self.dfa, self.trans, self.eos_id, self.allow_leading_space = pattern, dfa, trans, int(eos_id), allow_leading_space
        self.start, self.n_states, self.done = 0, int(trans.shape[0]), int(trans.shape[0]) - 1
        self._device: Dict[str, torch.Tensor] = {}

    @property
    def vocab_size(self) -> int:
        return int(self.trans.shape[1])

    def accepts(self, text: str) -> bool:
        s = self.dfa.walk(0, text)
        return s >= 0 and bool(self.dfa.accepting[s])

    def viable_prefix(self, text: str) -> bool:
        return self.dfa.walk(0, text) >= 0

    def device_table(self, device) -> torch.Tensor:
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = self.trans.to(device).contiguous()
        return self._device[key]

    @classmethod
    def allow_all(cls, V: int, eos_id: int = 0) -> "TokenAutomaton":
        """One state that allows every token and stays where it is (tests: a constraint that must change nothing)."""
        self = cls.__new__(cls)
        self.pattern, self.dfa, self.eos_id, self.allow_leading_space = None, None, int(eos_id), False
        self.trans = torch.zeros((1, int(V)), dtype=torch.int16)
        self.start, self.n_states, self.done, self._device = 0, 1, -1, {}
        return self


def _shortest_prefixes(table: np.ndarray, pieces: Sequence[Optional[str]], eos_id: int) -> Dict[int, str]:
    """state -> a shortest (in tokens) text that reaches it from the start over allowed tokens"""
    reach = {0: ""}
    q = deque([0])
    while q:
        s = q.popleft()
        row = table[s]
        for v in np.flatnonzero(row >= 0):
            t = int(row[v])
            if t not in reach:
                reach[t] = reach[s] + ("" if int(v) == eos_id else (pieces[v] or ""))
                q.append(t)
    return reach


def compile_constraint(pattern: str, pieces: Sequence[Optional[str]], eos_id: int, *, allow_leading_space: bool = True) -> TokenAutomaton:
    """``pieces[v]``: the text token v contributes (SentencePiece's U+2581 already read as a space), ``None`` for a token that
    contributes no text (BOS, pad, control, unknown): never allowed.  An empty piece is never allowed either (it would not move the
    automaton).  ``eos_id`` is allowed exactly in accepting states.  Raises ``ValueError`` for a pattern outside the subset, for more
    than 32767 states, for a table above 64 MiB and for a dead end: a state the vocabulary can reach but not leave towards a match."""
    V = len(pieces)
    eos_id = int(eos_id)
    if not 0 <= eos_id < V:
        raise ValueError(f"compile_constraint: eos_id = {eos_id} outside the vocabulary of {V} pieces")
    dfa = compile_regex(pattern, allow_leading_space=allow_leading_space)
    n = dfa.delta.shape[0]
    n_states = n + 1
    if n_states > MAX_STATES:
        raise ValueError(f"constraint pattern {pattern!r}: {n_states} states > {MAX_STATES} (states are int16 on the device)")
    if n_states * V * 2 > MAX_TABLE_BYTES:
        raise ValueError(f"constraint pattern {pattern!r}: the table of {n_states} states x {V} tokens takes {n_states * V * 2} bytes "
                         f"> {MAX_TABLE_BYTES} (64 MiB); simplify the pattern")
    # the DFA with a sink row n (index -1 lands there too), walked by all states at once, one numpy gather per character
    K = dfa.delta.shape[1]
    ext = np.full((n + 1, K), n, dtype=np.int32)
    ext[:n] = np.where(dfa.delta >= 0, dfa.delta, n)
    dead_sym = (ext[:n] == n).all(axis=0)                        # a character no state takes: its pieces are dead everywhere
    table = np.full((n_states, V), -1, dtype=np.int16)
    ident = np.arange(n, dtype=np.int32)
    sym, other = dfa.sym, dfa.other
    for v, piece in enumerate(pieces):
        if not piece or v == eos_id:
            continue
        ks = [sym.get(c, other) for c in piece]
        if any(dead_sym[k] for k in ks):
            continue
        cur = ident
        for k in ks:
            cur = ext[cur, k]
        table[:n, v] = np.where(cur == n, -1, cur)
    done = n
    table[:n, eos_id] = np.where(dfa.accepting, done, -1)
    table[done, eos_id] = done
    # dead ends: a state the vocabulary reaches from the start, from which it cannot reach DONE (no allowed token at all, or only
    # tokens that go round without ever accepting): the device could only answer with garbage there
    reach = _shortest_prefixes(table, pieces, eos_id)
    back: List[set] = [set() for _ in range(n_states)]
    for s in reach:
        for t in set(int(x) for x in table[s] if x >= 0):
            back[t].add(s)
    ok = {done} if done in reach else set()
    stack = list(ok)
    while stack:
        for s in back[stack.pop()]:
            if s not in ok:
                ok.add(s)
                stack.append(s)
    bad = [s for s in reach if s not in ok]
    if bad:
        empty = [s for s in bad if not (table[s] >= 0).any()]
        s = min(empty or bad, key=lambda x: (len(reach[x]), reach[x]))
        why = "has no allowed token" if empty else "allows only tokens that never lead to a match"
        raise ValueError(f"constraint pattern {pattern!r}: dead end under this vocabulary: after the prefix {reach[s]!r} the automaton "
                         f"{why} (the vocabulary cannot spell the rest of the pattern)")
    return TokenAutomaton(pattern, dfa, torch.from_numpy(table), eos_id, allow_leading_space)


def check_constraint(constraint):
    """A ``TokenAutomaton``, a pattern string, or None -- anything else is refused before any device use."""
    if constraint is not None and not isinstance(constraint, (str, TokenAutomaton)):
        raise ValueError(f"constraint must be a TokenAutomaton or a pattern string, got {type(constraint).__name__}")
    return constraint


class ConstraintState:
    """Device state of one constrained generation call: the table, one int32 state per cache row, the masked-logits buffer."""

    def __init__(self, automaton: TokenAutomaton, rows: int, V: int, device):
        from .. import ops
        if automaton.vocab_size != V:
            raise ValueError(f"constraint: the automaton was compiled for {automaton.vocab_size} tokens, the model has {V}")
        self.ops, self.a, self.V = ops, automaton, V
        self.trans = automaton.device_table(device)
        self.state = torch.full((rows,), automaton.start, dtype=torch.int32, device=device)
        self.first = torch.zeros(rows, dtype=torch.int32, device=device)
        self.out = torch.empty((rows, V), dtype=torch.float32, device=device)
        self.stopped_before = torch.zeros(rows, dtype=torch.bool, device=device)

    def reset(self, row: int, first: int) -> None:
        self.state[row] = self.a.start
        self.first[row] = first

    def mask(self, z: torch.Tensor, raw: torch.Tensor) -> torch.Tensor:
        """The row set the choice is made from.  ``z`` is the penalised copy (masked in place) or ``raw`` itself (masked into this
        object's buffer: the raw logits stay what they are for the log-probs)."""
        out = z if z.data_ptr() != raw.data_ptr() else self.out[:z.shape[0]]
        return self.ops.constrain_logits(z, self.trans, self.state, out)

    def advance(self, tokens: torch.Tensor, *, col: int = 0, cur=None, stopped_before=None) -> None:
        self.ops.constrain_advance(tokens, self.trans, self.state, self.first, col=col, cur=cur, stopped_before=stopped_before)
