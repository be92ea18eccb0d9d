"""-m gpu: lookup decoding under sampling, penalty, log-probs and constraints (a3v_spec_ctl.hip; generate_many(lookup=D,
lookup_verify="choice")).  The prepare kernel bit for bit against the plain loop's two kernels run per virtual row on an explicitly
built bitmap and state; the accept kernel bit for bit against tests/spec_ctl_ref.py and against a3v_accept_rows; dead queries are
never examined; the loop against a host loop over ``forward_verify_rows`` (oracle a) and against the plain loop (oracle b)."""
import json
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import genctl_ref as G
import sampler_ref as SR
import spec_ctl_ref as SC
import spec_ref as S
from a3vlm_amd import ops
from a3vlm_amd.model import constrain as C
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
NINF = 0xFF800000


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def words_dev(bm):
    """int64 words of genctl_ref -> the device's int32 storage"""
    return bm.where(bm < 2 ** 31, bm - 2 ** 32).to(torch.int32).to(DEV)


def phased(rows, ld, V, ph, fill=None):
    """a [rows, V] fp32 view of row stride ld whose first element sits ph floats behind a 16-byte boundary"""
    flat = torch.zeros(rows * ld + 8, dtype=torch.float32, device=DEV)
    off = (-(flat.data_ptr() // 4) % 4 + ph) % 4
    v = flat[off:off + rows * ld].view(rows, ld)[:, :V]
    assert (v.data_ptr() // 4) % 4 == ph
    if fill is not None:
        v.copy_(fill)
    return v


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def bitmap(rows, V, wpr):
    """genctl_ref.seen_bitmap for long id lists (numpy): int64 words [R, wpr]"""
    bm = np.zeros((len(rows), wpr), dtype=np.int64)
    for r, ids in enumerate(rows):
        a = np.array([t for t in ids if 0 <= t < V], dtype=np.int64)
        np.bitwise_or.at(bm[r], a >> 5, np.int64(1) << (a & 31))
    return torch.from_numpy(bm)


# ------------------------------------------------------------------ 1. the prepare kernel
def prepare_case(V, Q, B, seed, specials=True):
    """Rows cycle through: a draft chain the automaton allows (its first two drafts unseen, with a positive and a non-positive logit) /
    a draft that dies at k = 1 (NaN, +-inf payloads in its rows) / one that dies at k = nq - 1 / an unconstrained row with draft ids
    outside [0, V) / an idle row."""
    rng = np.random.default_rng(seed)
    n_states = 5
    trans = CR.random_table(n_states, V, seed + 1)
    z = (2.0 * rng.standard_normal((B * Q, V))).astype(np.float32)
    seen_ids = [[int(t) for t in np.nonzero(rng.random(V) < 0.1)[0]] for _ in range(B)]
    x, nq, pos, state = [], [], [], []
    for b in range(B):
        kind = b % 5
        s = int(rng.integers(0, n_states))
        row, cs = [int(rng.integers(0, V))], s
        for k in range(1, Q):                                   # an allowed chain
            ok = np.nonzero(trans[cs] >= 0)[0]
            t = int(ok[rng.integers(0, len(ok))])
            row.append(t)
            cs = int(trans[cs, t])
        n = Q
        if kind == 0:
            for k, val in ((1, 1.5), (2, -0.75)):
                if k < Q:
                    seen_ids[b] = [t for t in seen_ids[b] if t != row[k]]
                    z[b * Q:(b + 1) * Q, row[k]] = val
        if kind in (1, 2) and Q > 1:
            k = 1 if kind == 1 else n - 1
            ps = s
            for t in row[1:k]:
                ps = int(trans[ps, t])
            bad = np.nonzero(trans[ps] < 0)[0]
            if len(bad):
                row[k] = int(bad[0])
        if kind == 1 and specials:
            sp = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], dtype=np.uint32)
            idx = rng.integers(0, V, size=max(V // 5, 1))
            for j in range(Q):
                z[b * Q + j].view(np.uint32)[idx] = sp[rng.integers(0, len(sp), size=idx.size)]
        if kind == 3:
            s = -1 if b % 2 else n_states
            if Q > 1:
                row[1] = V + 5
            if Q > 2:
                row[2] = -2
            n = max(Q - 1, 1)
        x.append(row)
        nq.append(n)
        pos.append(-1 if kind == 4 else 3 + b)
        state.append(s)
    return dict(z=torch.from_numpy(z), x=x, nq=nq, pos=pos, state=state, trans=trans, seen_ids=seen_ids, n_states=n_states)


def run_prepare(c, V, Q, B, pad, ph, pen, con, want_lse, penalty=1.3):
    """(device out bits, device lse bits) and the reference pair built from a3v_logits_prepare + a3v_constrain_logits per virtual row"""
    ld = V + pad
    zin = phased(B * Q, ld, V, 0, c["z"].to(DEV))
    out = phased(B * Q, ld, V, ph)
    out.fill_(7.0)
    x, nq, pos = torch.tensor(c["x"], device=DEV), i32(c["nq"]), i32(c["pos"])
    wpr = G.words(V) + 1
    if "bm" not in c:
        c["bm"] = bitmap(c["seen_ids"], V, wpr)
        assert V > 100 or torch.equal(c["bm"], G.seen_bitmap(c["seen_ids"], V, wpr))
    bm = c["bm"]
    trans = torch.from_numpy(c["trans"]).to(DEV)
    lse = torch.full((B * Q,), 3.0, device=DEV) if want_lse else None
    ops.verify_prepare(zin, x, nq, pos, out, seen=words_dev(bm) if pen else None, penalty=penalty, trans=trans if con else None,
                       state=i32(c["state"]) if con else None, lse=lse)
    # the reference: one bitmap and one state per VIRTUAL row, the plain loop's kernels over the B * Q rows
    vbm = torch.cat([G.seen_bitmap([c["x"][b][1:j + 1]], V, wpr, start=bm[b:b + 1]) if pen else bm[b:b + 1] * 0 for b in range(B) for j in range(Q)])
    vstate, dead, idle = [], [], []
    for b in range(B):
        for j in range(Q):
            s = c["state"][b]
            idle.append(not SC.live(c["pos"], c["nq"], Q, b, j))
            w = SC.walk(c["trans"], s, c["x"][b][1:j + 1]) if con and 0 <= s < c["n_states"] and not idle[-1] else -1
            dead.append(w is None)
            vstate.append(-1 if w is None else w)
    ref = phased(B * Q, ld, V, ph)
    lse_ref = torch.zeros(B * Q, device=DEV)
    ops.logits_prepare(zin, words_dev(vbm), penalty if pen else 1.0, ref, lse_ref)          # the same rows, an out row on the same phase
    if not pen:
        ref.copy_(zin)                                                                     # (penalty 1.0 would quieten a signalling NaN)
        if ph == 0 and (ld % 4 == 0):                                                      # every row on a boundary: also the lse-only form
            l2 = torch.zeros(B * Q, device=DEV)
            ops.logits_prepare(zin, None, 1.0, None, l2)
            assert torch.equal(bits(l2), bits(lse_ref))
    if con:
        ops.constrain_logits(ref, trans, i32(vstate), ref)
    rb, lb = bits(ref), bits(lse_ref)
    for m in range(B * Q):
        if idle[m]:
            rb[m], lb[m] = 0, 0
        elif dead[m]:
            rb[m] = torch.tensor(NINF - 2 ** 32, dtype=torch.int64).to(torch.int32)
    return bits(out), (bits(lse) if want_lse else None), rb, lb, idle, dead, zin


@pytest.mark.parametrize("Q", [1, 2, 4, 8])
@pytest.mark.parametrize("V", [1, 37, 512, 1000, 2049, 32000])
def test_verify_prepare_is_bit_equal_to_the_plain_loops_kernels(V, Q):
    """Every out phase of 16 bytes, ld = V and ld = V + 3 (rows off the boundary: the element walk), B * Q = 32 at Q = 4 and 8.  lse:
    bit-equal to a3v_logits_prepare's, and inside genctl_ref.lse_bound of fp64 on the rows without NaN / inf payloads."""
    B = {1: 5, 2: 5, 4: 8, 8: 4}[Q]
    c = prepare_case(V, Q, B, seed=V + Q)
    n_dead = n_idle = 0
    for pad in (0, 3):
        for ph in range(4):
            got, lse, want, lse_want, idle, dead, zin = run_prepare(c, V, Q, B, pad, ph, True, True, True)
            assert torch.equal(got, want), (pad, ph, (got != want).nonzero()[:5])
            assert torch.equal(lse, lse_want), (pad, ph)
            n_dead, n_idle = sum(dead), sum(idle)
    assert n_idle >= 1 and (Q == 1 or V == 1 or n_dead > 0), (n_idle, n_dead)
    lse_f = lse.view(torch.float32)
    clean = [m for m in range(B * Q) if not idle[m] and (m // Q) % 5 != 1]
    z = c["z"][clean]
    err = (lse_f[clean].double() - G.lse64(z)).abs()
    bound = G.lse_bound(z)
    print(f"V {V} Q {Q}: max |lse - fp64| = {float(err.max()):.3e}, bound {float(bound.min()):.3e} .. {float(bound.max()):.3e}; dead {n_dead}, idle {n_idle}")
    assert bool((err <= bound).all()), (err, bound)
    assert torch.equal(bits(zin), bits(c["z"].to(DEV))), "the raw logits are never written"


@pytest.mark.parametrize("pen,con,want_lse", [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
                                              (False, True, True), (True, False, True), (False, False, False)])
def test_verify_prepare_forms(pen, con, want_lse):
    V, Q, B = 1000, 4, 5
    c = prepare_case(V, Q, B, seed=11)
    for pad, ph in ((0, 0), (0, 2), (3, 0)):
        got, lse, want, lse_want, idle, dead, _ = run_prepare(c, V, Q, B, pad, ph, pen, con, want_lse)
        assert torch.equal(got, want), (pad, ph)
        if want_lse:
            assert torch.equal(lse, lse_want), (pad, ph)


def test_verify_prepare_penalty_branches_on_the_drafts():
    """a draft equal to an unseen token is penalised from its own query on: divided when its logit is positive, multiplied when not"""
    V, Q, B = 512, 4, 1
    c = prepare_case(V, Q, B, seed=5)
    got = run_prepare(c, V, Q, B, 0, 0, True, False, False, penalty=2.0)[0].view(torch.float32)
    d1, d2 = c["x"][0][1], c["x"][0][2]
    assert got[0, d1] == 1.5 and got[1, d1] == 0.75 and got[3, d1] == 0.75
    assert got[1, d2] == -0.75 and got[2, d2] == -1.5 and got[3, d2] == -1.5


# ------------------------------------------------------------------ 2. the accept kernel
def _accept_device(chosen, logits, x, nq, tokens, cur, limit, base, stops, stopped, stop_pos, book, n_lp, prompt_len, seen_bm, trans, state, V):
    B = len(tokens)
    d = dict(tokens=torch.tensor(tokens, device=DEV), cur=i32(cur), limit=i32(limit), stopped=torch.tensor(stopped, device=DEV),
             stop_pos=torch.tensor(stop_pos, device=DEV), next_tok=torch.full((B,), -3, dtype=torch.long, device=DEV),
             pos=torch.full((B,), -3, dtype=torch.int32, device=DEV), stats=torch.zeros(2, dtype=torch.long, device=DEV))
    seq = torch.tensor([t for s in stops for t in s], device=DEV)
    offs = [0]
    for s in stops:
        offs.append(offs[-1] + len(s))
    kw = {}
    if book:
        lg = logits.to(DEV)
        lse = torch.empty(lg.shape[0], device=DEV)
        ops.logits_prepare(lg, None, 1.0, None, lse)
        kw = dict(V=V, logits=lg, lse=lse, logprob=torch.full((B, n_lp), 9.0, device=DEV), prompt_len=i32(prompt_len),
                  seen=words_dev(seen_bm), trans=torch.from_numpy(trans).to(DEV), state=i32(state.tolist()))
    ops.accept_rows_chosen(torch.tensor(chosen, device=DEV), torch.tensor(x, device=DEV), i32(nq), d["tokens"], d["cur"], d["limit"], base, seq,
                           i32(offs), len(stops), d["stopped"], d["stop_pos"], d["next_tok"], d["pos"], d["stats"], **kw)
    return d, kw


def test_accept_rows_chosen_is_the_restatement_and_the_argmax_form_is_accept_rows():
    """all accepted / the choice leaves the drafts at query 1 / a stop sequence completed by the second emission of an accepted run (the
    stopping token is recorded, later ones are not) / the limit in the middle / nq < Q / a stopped row / an idle row / rows at their
    limit; g >= n_lp (n_lp = 2) is not written."""
    Q, V, W, base, n_lp = 4, 50, 16, 5, 2
    model = [7, 8, 9, 10]
    cases = [  # x, nq, limit, stopped, chosen
        ([6, 7, 8, 9], 4, 16, False, model), ([6, 7, 8, 9], 4, 16, False, [7, 30, 9, 10]), ([6, 7, 8, 9], 2, 16, False, model),
        ([6, 7, 8, 9], 4, 5, False, model), ([6, 7, 8, 9], 4, 16, True, model), ([0, 0, 0, 0], 1, 16, True, model),
        ([6, 7, 8, 9], 4, 3, False, model), ([6, 7, 8, 9], 4, 4, False, model), ([6, 31, 8, 9], 4, 16, False, [31, 8, 9, 10])]
    B = len(cases)
    logits = torch.randn(B * Q, V, generator=torch.Generator().manual_seed(2))
    for b in range(B):
        for j in range(Q):
            logits[b * Q + j, model[j]] = 9.0
    trans = CR.random_table(6, V, 3, density=0.7)
    for stops in (((15,), (8, 9)), ((15,),)):
        for book in (True, False):
            tokens = [[1, 2, 6] + [0] * (W - 3) for _ in range(B)]
            cur, limit = [3] * B, [c[2] for c in cases]
            stopped, stop_pos, stats = [c[3] for c in cases], [4] * B, [0, 0]
            x, nq, chosen = [c[0] for c in cases], [c[1] for c in cases], [t for c in cases for t in c[4]]
            plen = [3] * B
            plen[2] = 4                                             # g = -1 at the first emission of row 2: not scored, not marked, no advance
            seen_bm = G.seen_bitmap([[1, 2, 6]] * B, V, G.words(V) + 1)
            state = np.array([b % 7 - 1 for b in range(B)], dtype=np.int32)      # -1 and 6..: unconstrained rows among them
            d, kw = _accept_device(chosen, logits, x, nq, tokens, cur, limit, base, stops, stopped, stop_pos, book, n_lp, plen, seen_bm, trans, state, V)
            ref = {}
            if book:
                ref = dict(logits=logits, lse=kw["lse"].cpu(), logprob=torch.full((B, n_lp), 9.0), prompt_len=plen, seen_bm=seen_bm, trans=trans,
                           state=state, V=V)
            nt, ps = SC.accept_rows_chosen(chosen, x, nq, tokens, cur, limit, base, stops, stopped, stop_pos, stats, **ref)
            got = (d["tokens"].tolist(), d["cur"].tolist(), d["stopped"].tolist(), d["stop_pos"].tolist(), d["next_tok"].tolist(),
                   d["pos"].tolist(), d["stats"].tolist())
            assert got == (tokens, cur, stopped, stop_pos, nt, ps, stats), (got, (tokens, cur, stopped, stop_pos, nt, ps, stats))
            if book:
                assert torch.equal(bits(kw["logprob"]), bits(ref["logprob"]))
                assert torch.equal(G.as_u32(kw["seen"]), seen_bm) and kw["state"].tolist() == state.tolist()
                assert float(ref["logprob"][0, 0]) != 9.0 and float(ref["logprob"][4, 0]) == 9.0          # written; a stopped row is not
    assert cur[0] == 7 and cur[1] == 5 and cur[8] == 7
    # all bookkeeping NULL and the argmax as the choice: a3v_accept_rows on the same inputs, stats included
    am = torch.empty(B * Q, dtype=torch.long, device=DEV)
    ops.argmax(logits.to(DEV), am)
    for stops in (((15,), (8, 9)), ((15,),)):
        outs = []
        for form in ("chosen", "argmax"):
            tokens = [[1, 2, 6] + [0] * (W - 3) for _ in range(B)]
            d = dict(tokens=torch.tensor(tokens, device=DEV), cur=i32([3] * B), limit=i32([c[2] for c in cases]),
                     stopped=torch.tensor([c[3] for c in cases], device=DEV), stop_pos=torch.tensor([4] * B, device=DEV),
                     next_tok=torch.full((B,), -3, dtype=torch.long, device=DEV), pos=torch.full((B,), -3, dtype=torch.int32, device=DEV),
                     stats=torch.zeros(2, dtype=torch.long, device=DEV))
            seq = torch.tensor([t for s in stops for t in s], device=DEV)
            offs = i32([0] + list(np.cumsum([len(s) for s in stops])))
            xs, ns = torch.tensor([c[0] for c in cases], device=DEV), i32([c[1] for c in cases])
            args = (xs, ns, d["tokens"], d["cur"], d["limit"], base, seq, offs, len(stops), d["stopped"], d["stop_pos"], d["next_tok"], d["pos"], d["stats"])
            if form == "chosen":
                ops.accept_rows_chosen(am, *args)
            else:
                ops.accept_rows(logits.to(DEV), *args)
            outs.append({k: v.tolist() for k, v in d.items()})
        assert outs[0] == outs[1]


def test_verify_uniforms_is_the_plain_loops_index():
    B, Q, n = 5, 3, 40
    uni = torch.rand(n, device=DEV)
    base, cur, plen = [0, 8, 16, 38, 24], [5, 9, 4, 7, 2], [3, 9, 4, 5, 6]
    u = torch.zeros(B * Q, device=DEV)
    ops.verify_uniforms(uni, torch.tensor(base, device=DEV), i32(cur), i32(plen), Q, u)
    assert torch.equal(u, uni[torch.tensor(SC.uniform_index(base, cur, plen, Q, n), device=DEV)])


# ------------------------------------------------------------------ 3. dead queries are never examined
@pytest.mark.parametrize("n_allowed", [1, 2, 37])
def test_a_dead_query_is_never_examined(n_allowed):
    """2000 rows whose only draft is a token the automaton forbids: query 1 is dead (all -inf), the choice of query 0 comes from the
    masked row and can never equal the draft, so every row emits exactly one token, an allowed one.  T 1 and 0.1, both samplers and
    the argmax (the counts of the masked-sampler test of constrained decoding)."""
    B, Q, V, W = 2000, 2, 512, 6
    g = torch.Generator().manual_seed(n_allowed)
    allowed = torch.randperm(V, generator=g)[:n_allowed].tolist()
    trans = np.full((2, V), -1, dtype=np.int16)
    trans[0, allowed] = 0
    trans[1, :] = 1
    forbidden = [t for t in range(V) if t not in allowed]
    logits = (3.0 * torch.randn(B * Q, V, generator=g)).to(DEV)
    logits[::2, forbidden[:8]] += 6.0                              # the forbidden tokens carry most of the raw mass
    x = torch.tensor([[0, forbidden[b % len(forbidden)]] for b in range(B)], device=DEV)
    nq, pos, state = i32([2] * B), i32([4] * B), i32([0] * B)
    out = torch.empty_like(logits)
    ops.verify_prepare(logits, x, nq, pos, out, trans=torch.from_numpy(trans).to(DEV), state=state)
    assert bool((out[1::2] == float("-inf")).all()), "query 1 of every row is dead"
    seq, offs = torch.tensor([V + 1], device=DEV), i32([0, 1])
    for T in (1.0, 0.1, 0.0):
        for filt in ((0, 0.0), (5, 0.05)) if T > 0 else ((0, 0.0),):
            chosen = torch.zeros(B * Q, dtype=torch.long, device=DEV)
            if T > 0:
                u = torch.rand(B * Q, generator=g).to(DEV)
                (ops.sample_top_k_p(out, T, filt[0], 0.9, filt[1], u, chosen) if filt[0] else ops.sample_top_p(out, T, 0.9, u, chosen))
            else:
                ops.argmax(out, chosen)
            tokens = torch.zeros((B, W), dtype=torch.long, device=DEV)
            cur, stopped = i32([2] * B), torch.zeros(B, dtype=torch.bool, device=DEV)
            stats = torch.zeros(2, dtype=torch.long, device=DEV)
            ops.accept_rows_chosen(chosen, x, nq, tokens, cur, i32([W] * B), 0, seq, offs, 1, stopped, torch.zeros(B, dtype=torch.long, device=DEV),
                                   torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV), stats)
            assert cur.tolist() == [3] * B and stats.tolist() == [B, 0], (T, filt, stats.tolist())
            assert set(tokens[:, 2].tolist()) <= set(allowed) and bool((tokens[:, 3:] == 0).all()), (T, filt)


# ------------------------------------------------------------------ 4. model level, fp32: two oracles
PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
PATTERN = r"\[[01]\.\d{2}(,[01]\.\d{2}){3}\]"             # the pattern of tests/test_gpu_constrain.py: every answer ends within 23 tokens
GEN = 26
REL = 1e-3                                                 # the fp32 model bound of tests/test_gpu_genctl.py


@pytest.fixture(scope="module")
def tiny():
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=96)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(torch.float32).to(DEV)
    return mm, mm.constraint_automaton(PATTERN)


def perfect_drafter(mm, prompts, want, D):
    """drafts the known continuation ``want`` of every prompt (tests/test_gpu_spec.py's scripted drafter, right answers only)"""
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in prompts]
    eos = mm.tokenizer.eos_id

    def draft(tokens, cur, limit, pos, stopped, next_tok, x, nq):
        tk, cu, li, st, nt = tokens.tolist(), cur.tolist(), limit.tolist(), stopped.tolist(), next_tok.tolist()
        xs, ns = [], []
        for r in range(len(tk)):
            row, nd = [nt[r]] + [0] * D, 0
            if not st[r]:
                i = next(i for i, t in enumerate(pt) if tk[r][:len(t)] == t and cu[r] > len(t) and tk[r][len(t):cu[r]] == (want[i] + [eos])[:cu[r] - len(t)])
                full = pt[i] + want[i]
                nd = max(min(D, len(full) - cu[r], li[r] - 1 - cu[r]), 0)
                row[1:1 + nd] = full[cu[r]:cu[r] + nd]
            xs.append(row)
            ns.append(1 + nd)
        x.copy_(torch.tensor(xs, device=DEV))
        nq.copy_(i32(ns))
    return draft


def host_choice_loop(mm, prompts, max_gen_len, D, drafter, *, A=None, penalty=1.0, logprobs=False, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0,
                     uniforms=None, ngram=3):
    """Oracle (a): generate_many(lookup=D, lookup_verify="choice") for len(prompts) <= rows restated on the host.  The model runs on
    the device (prefill_row, forward_verify_rows) and hands its logits over; everything behind them is tests/spec_ctl_ref.py: the
    prepared rows, the choice (first-index argmax, or sampler_ref's inverse CDF at the plain loop's uniform), the accept rule with
    its record and advance.  The lse of a raw row is a3v_logits_prepare's (the order the header fixes).  Polls every step."""
    tok, V, llma = mm.tokenizer, mm.llma.args.vocab_size, mm.llma
    pt = [tok.encode(p, bos=True, eos=False) for p in prompts]
    B, Q = len(pt), D + 1
    lens, limits = [len(t) for t in pt], [min(llma.args.max_seq_len, max_gen_len + len(t)) for t in pt]
    width = max(limits)
    tokens = [t + [0] * (width - len(t)) for t in pt]
    cur, stopped, stop_pos, pos = list(lens), [False] * B, [n + 1 for n in lens], [n - 1 for n in lens]
    x, nq, stats = [[0] * Q for _ in range(B)], [1] * B, [0, 0]
    seen_bm = G.seen_bitmap(pt, V) if penalty != 1.0 else None
    trans = A.trans.numpy() if A is not None else None
    state = np.full(B, A.start, dtype=np.int32) if A is not None else None
    lp = torch.zeros(B, max_gen_len) if logprobs else None
    llma.allocate_rows(B)
    vlogits = torch.zeros((B * Q, V), dtype=torch.float32, device=DEV)
    for b in range(B):
        vlogits[b * Q].copy_(llma.prefill_row(b, torch.tensor([pt[b]], device=DEV), None)[0])
    smax = llma._k_cache[0].shape[2]
    while not all(stopped):
        raw = vlogits.cpu()
        z = SC.verify_prepare(raw, x, nq, pos, seen_bm=seen_bm, penalty=penalty, trans=trans, state=state)
        lse = None
        if logprobs:
            lse = torch.empty(B * Q, device=DEV)
            ops.logits_prepare(vlogits, None, 1.0, None, lse)
            lse = lse.cpu()
        if temperature > 0:
            ui = SC.uniform_index([b * uniforms.shape[1] for b in range(B)], cur, lens, Q, uniforms.numel())
            chosen = SR.sample_at(z, temperature, top_k, top_p, min_p, uniforms.reshape(-1)[ui]).tolist()
        else:
            chosen = [S.argmax_first(r) for r in z.tolist()]
        nt, pos = SC.accept_rows_chosen(chosen, x, nq, tokens, cur, limits, 0, ((tok.eos_id,),), stopped, stop_pos, stats, logits=raw, lse=lse,
                                        logprob=lp, prompt_len=lens, seen_bm=seen_bm, trans=trans, state=state, V=V)
        if all(stopped):
            break
        d = [torch.tensor(tokens, device=DEV), i32(cur), i32(limits), i32(pos), torch.tensor(stopped, device=DEV), torch.tensor(nt, device=DEV)]
        xq, nqd = torch.zeros((B, Q), dtype=torch.long, device=DEV), torch.ones(B, dtype=torch.int32, device=DEV)
        if drafter is not None:
            drafter(*d, xq, nqd)
        else:
            ops.lookup_draft_rows(*d, D, ngram, smax, xq, nqd)
        x, nq = xq.tolist(), nqd.tolist()
        llma.forward_verify_rows(xq, d[3], nqd, max(p for p in pos if p >= 0), out=vlogits)
    ids = [tokens[b][lens[b]:stop_pos[b]] for b in range(B)]
    return ids, ([lp[b, :len(ids[b])].tolist() for b in range(B)] if logprobs else None), seen_bm, state, stats


def test_choice_greedy_with_a_constraint_equals_the_host_loop_and_the_plain_loop(tiny):
    """Temperature 0 + a constraint: refused with the pinned ValueError before this feature.  Oracle (a): ids, log-probs, final seen
    bitmaps (penalty 1.2 in the second run) and states equal the host loop's exactly.  Oracle (b): the ids are the plain loop's."""
    mm, A = tiny
    D, R = 3, len(PROMPTS)
    plain = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, return_ids=True, constraint=A, return_logprobs=True)
    assert all(re.fullmatch(PATTERN, t) for t in plain[0]), plain[0]
    for drafter in (perfect_drafter(mm, PROMPTS, plain[1], D), None):
        got = mm.generate_many(PROMPTS, None, batch_rows=R, max_gen_len=GEN, return_ids=True, constraint=A, return_logprobs=True, lookup=D,
                               lookup_verify="choice", lookup_drafter=drafter, poll_every=1)
        st, state = dict(mm.last_lookup_stats), mm.last_lookup_state["state"].tolist()
        ids, lps, _, hstate, hstats = host_choice_loop(mm, PROMPTS, GEN, D, drafter, A=A, logprobs=True)
        assert got[1] == ids and [s["logprobs"] for s in got[2]] == lps and state == hstate.tolist()
        assert [st["drafted"], st["accepted"]] == hstats
        assert got[1] == plain[1], "oracle (b): the plain loop's ids"
        if drafter is not None:
            print("perfect drafter:", st)
            assert st["drafted"] > 0 and st["accepted"] == st["drafted"] and st["tokens"] == st["steps"] + st["accepted"]
    # refill (2 rows for 5 prompts), every poll cadence: still the plain loop's ids and, within the model tolerance, its log-probs
    for pe in (1, 4):
        got = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, return_ids=True, constraint=A, return_logprobs=True, lookup=D,
                               lookup_verify="choice", poll_every=pe)
        assert got[1] == plain[1] and got[0] == plain[0], pe
        _lp_close(mm, got[2], plain[2])
    # with a penalty: the seen bitmaps too
    kw = dict(max_gen_len=GEN, return_ids=True, constraint=A, repetition_penalty=1.2)
    plain = mm.generate_many(PROMPTS, None, batch_rows=2, **kw)
    got = mm.generate_many(PROMPTS, None, batch_rows=R, lookup=D, lookup_verify="choice", poll_every=1, **kw)
    seen = G.as_u32(mm.last_lookup_state["seen"])
    ids, _, hseen, _, _ = host_choice_loop(mm, PROMPTS, GEN, D, None, A=A, penalty=1.2)
    assert got[1] == ids == plain[1] and torch.equal(seen, hseen)


_TOL = {}


def _lp_tol(mm):
    """the model-level tolerance of tests/test_gpu_genctl.py for a log-prob: two logit errors (z[tok] and the lse) at REL of the
    logits' scale (max |logit| of the second prompt, as there), plus lse_bound at this vocabulary"""
    if "tol" not in _TOL:
        V = mm.llma.args.vocab_size
        pt = mm.tokenizer.encode(PROMPTS[1], bos=True, eos=False)
        scale = float(mm.llma.forward_inference(torch.tensor([pt], device=DEV), 0).abs().max())
        _TOL["tol"] = 2 * REL * scale + G.U32 * (1.01 * (4 * 2 + 33 + 2 * scale) + 2 * math.log(V) + (scale + math.log(V)) + (2 * scale + math.log(V)))
    return _TOL["tol"]


def _lp_close(mm, a, b):
    tol = _lp_tol(mm)
    for sa, sb in zip(a, b):
        assert len(sa["logprobs"]) == len(sb["logprobs"])
        err = max((abs(p - q) for p, q in zip(sa["logprobs"], sb["logprobs"])), default=0.0)
        assert err <= tol, (err, tol)


def test_choice_sampled_with_every_control_equals_the_host_loop_and_the_plain_loop(tiny):
    """Temperature 0.8, top-k 20, top-p 0.9, min-p 0.02, penalty 1.2, log-probs, seed 0.  A draw can differ between the verify step's
    logits and the plain step's only where a uniform sits on a CDF boundary; no prompt is left out of either comparison."""
    mm, _ = tiny
    D, R = 3, len(PROMPTS)
    gen = 12
    uni = torch.rand(R, gen, generator=torch.Generator().manual_seed(0))
    kw = dict(max_gen_len=gen, return_ids=True, temperature=0.8, top_k=20, top_p=0.9, min_p=0.02, repetition_penalty=1.2, return_logprobs=True,
              sample_uniforms=uni)
    plain = mm.generate_many(PROMPTS, None, batch_rows=2, **kw)
    for drafter in (perfect_drafter(mm, PROMPTS, plain[1], D), None):
        got = mm.generate_many(PROMPTS, None, batch_rows=R, lookup=D, lookup_verify="choice", lookup_drafter=drafter, poll_every=1, **kw)
        st, seen = dict(mm.last_lookup_stats), G.as_u32(mm.last_lookup_state["seen"])
        ids, lps, hseen, _, hstats = host_choice_loop(mm, PROMPTS, gen, D, drafter, penalty=1.2, logprobs=True, temperature=0.8, top_k=20, top_p=0.9,
                                                      min_p=0.02, uniforms=uni)
        assert got[1] == ids and [s["logprobs"] for s in got[2]] == lps and torch.equal(seen, hseen)
        assert [st["drafted"], st["accepted"]] == hstats
        assert got[1] == plain[1], "oracle (b): the plain loop's ids for the same uniforms"
        _lp_close(mm, got[2], plain[2])
        if drafter is not None:
            print("perfect drafter, sampled:", st)
            assert st["drafted"] > 0 and st["accepted"] == st["drafted"]
    got = mm.generate_many(PROMPTS, None, batch_rows=2, lookup=D, lookup_verify="choice", **kw)            # with refills
    assert got[1] == plain[1]


def test_choice_with_an_allow_everything_automaton_is_the_argmax_mode(tiny):
    mm, _ = tiny
    A1 = C.TokenAutomaton.allow_all(mm.llma.args.vocab_size, mm.tokenizer.eos_id)
    gens = [3, 9, 2, 6, 4]
    for rows in (1, 2):
        want = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=gens, return_ids=True, lookup=3)
        a = dict(mm.last_lookup_stats)
        got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=gens, return_ids=True, lookup=3, lookup_verify="choice", constraint=A1)
        assert got == want and mm.last_lookup_stats == a
        assert mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=gens, return_ids=True, lookup=3, lookup_verify="choice") == want


def test_choice_drafts_hit_on_a_repetitive_answer_with_the_lookup_kernel(tiny):
    """the real lookup kernel on prompts that repeat themselves: the plain loop's ids under penalty-free sampling controls, and drafts
    are accepted on at least one of them"""
    mm, _ = tiny
    texts = ["the lid the lid the lid the", "1 2 3 1 2 3 1 2 3 1 2", "Open Open Open Open", "a b a b a b a b a b"]
    kw = dict(max_gen_len=40, return_ids=True, return_logprobs=True)
    plain = mm.generate_many(texts, None, batch_rows=2, **kw)
    got = mm.generate_many(texts, None, batch_rows=2, lookup=3, lookup_verify="choice", **kw)
    st = mm.last_lookup_stats
    print(st)
    assert got[1] == plain[1] and st["drafted"] > 0 and st["accepted"] > 0 and st["tokens"] / st["steps"] > 1
    _lp_close(mm, got[2], plain[2])


# ------------------------------------------------------------------ 5. bf16 stream
def test_choice_bf16_verify_logits_stay_inside_the_model_bound():
    """bf16: the logits the choice loop prepares come from forward_verify_rows; query j against the oracle fed the same tokens one by
    one, within the bf16 model bound of tests/test_gpu_spec.py (4e-2 of max |logit|), seen through a3v_verify_prepare with nothing
    masked or penalised (an allow-everything automaton).  No id-equality claim."""
    VOCAB = 640
    geom = dict(dim=512, n_layers=2, n_heads=8, n_kv_heads=4, multiple_of=256)
    oargs = ref_cpu.OracleArgs(vocab_size=VOCAB, max_seq_len=128, **geom)
    sd = ref_cpu.make_decoder_weights(oargs, seed=0, std=0.05)
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=128, max_batch_size=32, **geom))
    m.load_state_dict(sd)
    m.to(torch.bfloat16).to(DEV)
    sdb = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    lens, nq, Q = [9, 30], [4, 3], 4
    B = len(lens)
    ex = torch.randint(3, VOCAB, (B, 40), generator=torch.Generator().manual_seed(3))
    ex[:, 0] = 1
    m.allocate_rows(B)
    for b, n in enumerate(lens):
        m.prefill_row(b, ex[b:b + 1, :n].to(DEV))
    x = torch.stack([ex[b, n:n + Q] for b, n in enumerate(lens)]).to(DEV)
    raw = m.forward_verify_rows(x, i32(lens), i32(nq), max(lens))
    A1 = C.TokenAutomaton.allow_all(VOCAB, 2)
    out, lse = torch.empty_like(raw), torch.empty(B * Q, device=DEV)
    ops.verify_prepare(raw, x, i32(nq), i32(lens), out, trans=A1.device_table(DEV), state=i32([A1.start] * B), lse=lse)
    got = out.cpu()
    for b, n in enumerate(lens):
        d = ref_cpu.OracleDecoder(oargs, sdb)
        d.forward_inference(ex[b:b + 1, :n], 0)
        for j in range(Q):
            if j >= nq[b]:
                assert float(got[b * Q + j].abs().max()) == 0.0
                continue
            w = d.forward_inference(ex[b:b + 1, n + j:n + j + 1], n + j).float()
            e = float((got[b * Q + j:b * Q + j + 1] - w).abs().max() / w.abs().max())
            print(f"row {b} query {j}: {e:.3e} of max |logit| {float(w.abs().max()):.3e}")
            assert e < 4e-2, (b, j, e)


# ------------------------------------------------------------------ 6. the eval entry
def test_eval_entry_lookup_choice_with_regex_and_scores(tmp_path, tiny):
    """--lookup_decoding 3 --lookup_verify choice --answer_regex ... --save_scores end to end on the demo fixture: the records of the
    same run without lookup decoding, plus accepted_per_step; log-probs within the model tolerance (the text model's: the same decoder)."""
    from a3vlm_amd import checkpoint as ck
    pattern = r"\[\d{1,3}(,\d{1,3}){3}\]"
    vit = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({**{k: v for k, v in TINY.items() if k != "max_seq_len"}, **vit}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, **TINY), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    ckdir = ck.save_checkpoint(str(tmp_path / "ck"), types.SimpleNamespace(precision="tf32", only_save_trainable=False), mm, None, None, None, epoch=0)
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_v2", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2", "--num_workers", "0",
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "20", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32",
           "--continuous_rows", "2", "--answer_regex", pattern, "--save_scores"]
    for flag, extra in (("rows", []), ("choice", ["--lookup_decoding", "3", "--lookup_verify", "choice"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = json.load(open(tmp_path / "logs" / "rows" / "demo.json"))
    b = json.load(open(tmp_path / "logs" / "choice" / "demo.json"))
    assert len(a) == len(b) == 3
    for ra, rb in zip(a, b):
        assert isinstance(rb.pop("accepted_per_step"), float) and re.fullmatch(pattern, rb["answer"]), rb
        lpa, lpb = ra.pop("logprobs"), rb.pop("logprobs")
        ra.pop("logprob_sum"), rb.pop("logprob_sum")
        assert json.dumps(ra, ensure_ascii=False) == json.dumps(rb, ensure_ascii=False)
        _lp_close(tiny[0], [{"logprobs": lpa}], [{"logprobs": lpb}])
