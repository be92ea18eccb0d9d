"""Restatement of beam search as the device runs it (include/a3vlm_hip.h, "Beam search"): ``select`` and ``advance`` in numpy fp32,
bit for bit what a3v_beam_select / a3v_beam_advance compute, and ``search``: a whole search of one prompt over a logits callback.
This file is the contract; the kernels and model/beam.py follow it.

Groups of K consecutive rows.  A candidate (beam b, token v) of a live beam scores s = cum[b] + (z[b, v] - lse[b]) in fp32, in that
order; the best 2K of a group are ordered by s descending, then b * V + v ascending; -inf and NaN are never taken.  ``advance``
walks them in rank order as HF's BeamSearchScorer does.

``mutant`` (tests only) selects one deliberately wrong walk: "tie" (ties by index DEscending), "div" (the sum added after the
division), "stale" (a child keeps the state of its own row instead of stepping its parent's)."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

F = np.float32
NEG = F(-np.inf)


def len_div_table(n: int, length_penalty: float) -> np.ndarray:
    """len_div[j] = fp32(max(j, 1) ** length_penalty), computed in fp64 on the host."""
    return np.array([float(max(j, 1)) ** float(length_penalty) for j in range(n)], dtype=np.float64).astype(F)


class State:
    """The device state of G groups of K rows (numpy mirrors, same dtypes)."""

    def __init__(self, G: int, K: int, ld_tok: int):
        R = G * K
        self.G, self.K, self.ld_tok = G, K, ld_tok
        self.cum = np.full(R, NEG, F)
        self.alive = np.zeros(R, np.uint8)
        self.state = np.full(R, -1, np.int32)
        self.parent = np.arange(R, dtype=np.int32)
        self.next_tok = np.zeros(R, np.int64)
        self.pos = np.full(R, -1, np.int32)
        self.glen = np.zeros(G, np.int32)
        self.done = np.ones(G, np.uint8)
        self.base = np.zeros(G, np.int32)
        self.limit = np.zeros(G, np.int32)
        self.pool_n = np.zeros(G, np.int32)
        self.pool_added = np.zeros(G, np.int32)
        self.pool_score = np.zeros((G, K), F)
        self.pool_cum = np.zeros((G, K), F)
        self.pool_len = np.zeros((G, K), np.int32)
        self.pool_seq = np.zeros((G, K), np.int32)
        self.pool_ids = np.zeros((G, K, ld_tok), np.int64)
        # bookkeeping of the restatement alone (no device counterpart): which branches the walk took, and the |gap| of every
        # comparison between two scores that decided something (a full pool's admission, the stop rule without early stopping)
        self.events: List[str] = []
        self.gaps: List[float] = []

    def start(self, g: int, base: int, limit: int, state0: int = -1) -> None:
        """A fresh prompt in group g: only beam 0 is alive, cum = [0, -inf, ...]."""
        K = self.K
        r = slice(g * K, g * K + K)
        self.cum[r] = NEG
        self.cum[g * K] = 0
        self.alive[r] = 0
        self.alive[g * K] = 1
        self.state[r] = state0
        self.parent[r] = np.arange(g * K, g * K + K)
        self.next_tok[r] = 0
        self.pos[r] = -1
        self.glen[g], self.done[g], self.base[g], self.limit[g] = 0, 0, base, limit
        self.pool_n[g] = self.pool_added[g] = 0

    def pool(self, g: int):
        """The group's hypotheses, best first: (score, cum, ids) by score descending, then entry order."""
        n = int(self.pool_n[g])
        order = sorted(range(n), key=lambda j: (-float(self.pool_score[g, j]), int(self.pool_seq[g, j])))
        return [(float(self.pool_score[g, j]), float(self.pool_cum[g, j]), self.pool_ids[g, j, :self.pool_len[g, j]].tolist()) for j in order]


def select(z: np.ndarray, lse: np.ndarray, cum: np.ndarray, alive: np.ndarray, K: int, trans: Optional[np.ndarray] = None,
           state: Optional[np.ndarray] = None, mutant: Optional[str] = None):
    """z [R, V] fp32 raw logits -> (cand_score [G, 2K] fp32, cand_beam, cand_tok int32); also the smallest gap between the last
    taken and the first not-taken score per group (inf when nothing is left out)."""
    z = np.asarray(z, F)
    R, V = z.shape
    G = R // K
    score = np.full((G, 2 * K), NEG, F)
    beam = np.full((G, 2 * K), -1, np.int32)
    tok = np.full((G, 2 * K), -1, np.int32)
    gap = np.full(G, np.inf)
    for g in range(G):
        ss, ff = [], []
        for b in range(K):
            r = g * K + b
            if not alive[r]:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                s = (F(cum[r]) + (z[r] - F(lse[r]))).astype(F)          # two fp32 operations, in this order
            ok = s > NEG                                                # drops -inf and NaN
            if trans is not None and 0 <= int(state[r]) < trans.shape[0]:
                ok &= trans[int(state[r])] >= 0
            v = np.nonzero(ok)[0]
            ss.append(s[v])
            ff.append(b * V + v)
        if not ss:
            continue
        ss, ff = np.concatenate(ss), np.concatenate(ff)
        with np.errstate(invalid="ignore"):
            order = np.lexsort((-ff if mutant == "tie" else ff, -ss.astype(np.float64)))      # score descending, then index ascending
        top = order[:2 * K]
        n = len(top)
        score[g, :n], beam[g, :n], tok[g, :n] = ss[top], ff[top] // V, ff[top] % V
        if len(order) > n:
            with np.errstate(invalid="ignore"):
                gap[g] = float(ss[top[-1]]) - float(ss[order[n]])
    return score, beam, tok, gap


def advance(cand_score, cand_beam, cand_tok, st: State, tokens_in: np.ndarray, tokens_out: np.ndarray, V: int, eos: int,
            early_stopping: bool, len_div: np.ndarray, pos_cap: int, trans: Optional[np.ndarray] = None, mutant: Optional[str] = None) -> None:
    G, K, ld = st.G, st.K, st.ld_tok
    n_states = trans.shape[0] if trans is not None else 0
    for g in range(G):
        if st.done[g]:
            continue                                                    # a done group is not touched
        row0 = g * K
        L, b0 = int(st.glen[g]), int(st.base[g])
        lim = min(int(st.limit[g]), ld, len(len_div) - 1)
        lim = 0 if b0 < 0 else min(lim, pos_cap - b0)
        dn = False
        if L < 0 or L >= lim:
            dn = True
        else:
            old_state = st.state[row0:row0 + K].copy()

            def pool_add(score, cumv, ids):
                n = int(st.pool_n[g])
                if n < K:
                    slot = n
                    st.pool_n[g] = n + 1
                    st.events.append("full" if n + 1 == K else "append")
                else:                                                   # a full pool keeps the best K; a tie keeps the earlier entry
                    slot = 0
                    for j in range(1, K):
                        if st.pool_score[g, j] < st.pool_score[g, slot] or (st.pool_score[g, j] == st.pool_score[g, slot]
                                                                            and st.pool_seq[g, j] > st.pool_seq[g, slot]):
                            slot = j
                    st.gaps.append(abs(float(score) - float(st.pool_score[g, slot])))
                    if not score > st.pool_score[g, slot]:
                        st.events.append("tie_rejected" if score == st.pool_score[g, slot] else "rejected")
                        return
                    st.events.append("replaced")
                st.pool_score[g, slot], st.pool_cum[g, slot], st.pool_len[g, slot] = score, cumv, len(ids)
                st.pool_seq[g, slot] = st.pool_added[g]
                st.pool_added[g] += 1
                st.pool_ids[g, slot, :len(ids)] = ids

            taken = []
            for rank in range(2 * K):
                s, b, t = F(cand_score[g, rank]), int(cand_beam[g, rank]), int(cand_tok[g, rank])
                if not s > NEG or b < 0 or b >= K or t < 0 or t >= V:
                    continue                                            # an unfilled slot, or not a candidate
                if t == eos:
                    if rank < K:
                        if mutant == "div":                             # the sum added after the division
                            prev = F(st.cum[row0 + b])
                            pool_add(F(prev + F(F(s - prev) / len_div[L])), s, tokens_in[row0 + b, :L].copy())
                        else:
                            pool_add(F(s / len_div[L]), s, tokens_in[row0 + b, :L].copy())
                    continue
                if len(taken) < K:
                    taken.append((b, t, s))
            G1 = L + 1
            st.glen[g] = G1
            for j in range(K):
                r = row0 + j
                if j < len(taken):
                    b, t, s = taken[j]
                    so = int(old_state[j] if mutant == "stale" else old_state[b])
                    st.parent[r], st.next_tok[r], st.cum[r], st.alive[r], st.pos[r] = row0 + b, t, s, 1, b0 + L
                    st.state[r] = int(trans[so, t]) if (trans is not None and 0 <= so < n_states) else so
                    tokens_out[r, :L] = tokens_in[row0 + b, :L]
                    tokens_out[r, L] = t
                else:
                    st.parent[r], st.next_tok[r], st.cum[r], st.alive[r], st.pos[r] = r, 0, NEG, 0, -1
            if len(taken) < K:
                st.events.append("fewer" if taken else "none")
            if not taken:
                dn = True
            elif G1 >= lim:
                st.events.append("limit")                                             # the limit: every live beam is a hypothesis at its sum
                for j, (b, t, s) in enumerate(taken):
                    pool_add(F(s / len_div[G1]), s, tokens_out[row0 + j, :G1].copy())
                dn = True
            elif int(st.pool_n[g]) == K:
                if early_stopping:
                    dn = True
                else:
                    best, worst = F(taken[0][2] / len_div[G1]), st.pool_score[g].min()
                    st.gaps.append(abs(float(best) - float(worst)))
                    dn = bool(best <= worst)
                    st.events.append("stop_rule" if dn else "goes_on")
        if dn:
            for j in range(K):
                r = row0 + j
                st.parent[r], st.next_tok[r], st.alive[r], st.pos[r] = r, 0, 0, -1
            st.done[g] = 1


def lse_rows(z: np.ndarray) -> np.ndarray:
    """logsumexp of every row in fp64, rounded to fp32 (the device value differs from it by a3v_logits_prepare's bound)."""
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m[:, 0] + np.log(np.exp(z - m).sum(axis=1))).astype(F)


def _margin(sc, to, gap_next, K, eos) -> float:
    """The smallest score gap of one step whose sign decides what the walk takes: between neighbours in rank order of which one is
    taken (a live beam, or a hypothesis) and the other is not -- the first candidate behind the 2K counts as not taken -- and
    between an EOS candidate and either neighbour (its rank against K decides whether it enters the pool)."""
    flags, scores, is_eos, beams = [], [], [], 0
    for rank in range(2 * K):
        if not sc[rank] > NEG:
            break
        e = int(to[rank]) == eos
        took = rank < K if e else beams < K
        beams += (not e) and took
        flags.append(took), scores.append(float(sc[rank])), is_eos.append(e)
    if len(flags) == 2 * K and np.isfinite(gap_next):
        flags.append(False), scores.append(scores[-1] - gap_next), is_eos.append(False)
    m = np.inf
    for j in range(len(flags) - 1):
        if flags[j] != flags[j + 1] or is_eos[j] or is_eos[j + 1]:
            m = min(m, scores[j] - scores[j + 1])
    return m


def search(logits_fn: Callable[[List[List[int]]], np.ndarray], K: int, limit: int, eos: int, V: int, length_penalty: float = 1.0,
           early_stopping: bool = True, trans: Optional[np.ndarray] = None, state0: int = -1, mutant: Optional[str] = None):
    """One prompt, one group.  ``logits_fn(seqs)`` returns the raw logits [K, V] behind each of the K generated-id sequences (rows of
    dead beams are ignored; at the start every row is the empty sequence).  Returns (pool best first, the smallest deciding score gap: ``_margin`` of every step, the admissions to a full pool and
    the stop rule without early stopping; the ORDER of two hypotheses inside the pool is not guarded: compare them by their ids)."""
    st = State(1, K, max(limit, 1))
    st.start(0, 0, limit, state0)
    ld = len_div_table(limit + 2, length_penalty)
    tin = np.zeros((K, max(limit, 1)), np.int64)
    tout = np.zeros_like(tin)
    margin = np.inf
    while not st.done[0]:
        L = int(st.glen[0])
        z = np.asarray(logits_fn([tin[b, :L].tolist() for b in range(K)]), F)
        sc, be, to, gap = select(z, lse_rows(z), st.cum, st.alive, K, trans, st.state, mutant)
        margin = min(margin, _margin(sc[0], to[0], float(gap[0]), K, eos))
        advance(sc, be, to, st, tin, tout, V, eos, early_stopping, ld, 1 << 30, trans, mutant)
        tin, tout = tout, tin
    return st.pool(0), min([margin] + st.gaps)
