"""Host restatements of the two kernels of lookup decoding's sample-and-match form (a3v_spec_ctl.hip; include/a3vlm_hip.h, "Lookup
decoding: sample and match"), composed from the restatements the plain loop's kernels already have: the penalty and the record of
genctl_ref, the mask and the advance of constrain_ref, the token step of ragged_ref (as spec_ref.accept_rows uses it).  No GPU.
tests/test_spec_ctl_cpu.py pins them with mutation checks, tests/test_gpu_spec_ctl.py holds the kernels and the loop to them.

The switches ``drafts_in_seen`` / ``walk_state`` / ``use_choice`` exist for those mutation checks: each one switched off is a
plausible wrong implementation, and the checks show that it changes a result."""
import numpy as np
import torch

import constrain_ref as C
import genctl_ref as G
import ragged_ref as R
import spec_ref as S


def live(pos, nq, Q, b, j):
    return pos[b] >= 0 and j < min(max(nq[b], 1), Q)


def walk(trans, s, drafts):
    """The automaton state behind ``drafts`` from state s, or None when a draft is forbidden (or outside the vocabulary)."""
    n_states, V = trans.shape
    for t in drafts:
        if not 0 <= t < V:
            return None
        s = int(trans[s, t])
        if not 0 <= s < n_states:
            return None
    return s


def verify_prepare(logits, x, nq, pos, *, seen_bm=None, penalty=1.0, trans=None, state=None, drafts_in_seen=True, walk_state=True):
    """a3v_verify_prepare without the lse.  logits: torch fp32 [B*Q, V]; x [B][Q], nq, pos: lists; seen_bm: int64 words [B, wpr]
    (genctl_ref.seen_bitmap) or None; trans int16 [n_states, V] / state [B] or None.  Returns out, torch fp32 [B*Q, V]: query j of row
    b prepared as if drafts x[b][1..j] had been emitted; an idle query is zeros, a dead one all -inf."""
    B, Q = len(x), len(x[0])
    V = logits.shape[1]
    out = torch.zeros_like(logits)
    for b in range(B):
        for j in range(Q):
            m = b * Q + j
            if not live(pos, nq, Q, b, j):
                continue
            drafts = [int(t) for t in x[b][1:j + 1]]
            z = logits[m:m + 1]
            if seen_bm is not None:
                bm = G.seen_bitmap([drafts if drafts_in_seen else []], V, seen_bm.shape[1], start=seen_bm[b:b + 1])
                z = G.penalise(z, G.seen_mask(bm, V), penalty)
            if trans is not None and 0 <= int(state[b]) < trans.shape[0]:
                s = walk(trans, int(state[b]), drafts) if walk_state else int(state[b])
                bits = z.numpy().view(np.uint32)
                if s is None:
                    bits = np.full_like(bits, C.NEG_INF_BITS)
                else:
                    bits = C.constrain_logits_ref(bits, V, trans, [s], bits.copy())
                z = torch.from_numpy(bits.view(np.float32).copy())
            out[m] = z[0]
    return out


def accept_rows_chosen(chosen, x, nq, tokens, cur, limit, pos_base, stop_seqs, stopped, stop_pos, stats, *, logits=None, lse=None,
                       logprob=None, prompt_len=None, seen_bm=None, trans=None, state=None, V=None, use_choice=True):
    """a3v_accept_rows_chosen, in place (Python lists as spec_ref.accept_rows; logits fp32 [B*Q, V], lse fp32 [B*Q], logprob fp32 [B, L],
    seen_bm int64 words [B, wpr], state int32 numpy [B]: each of the last three may be None; V: the vocabulary size, with any of them).  ``use_choice=False`` is the mutant
    that accepts on the first-index argmax of ``logits`` instead of the handed-in choice.  Returns (next_tok, pos)."""
    B, Q = len(tokens), len(x[0])
    next_tok, pos = [0] * B, [-1] * B
    for b in range(B):
        if stopped[b]:
            continue
        nd = min(max(nq[b], 1), Q) - 1
        if use_choice:
            t = [int(chosen[b * Q + j]) for j in range(nd + 1)]
        else:
            t = [S.argmax_first(logits[b * Q + j].tolist()) for j in range(nd + 1)]
        emitted = 0
        for j in range(nd + 1):
            if j > 0 and t[j - 1] != x[b][j]:
                break
            c0 = cur[b]
            tk, cu, li, st, sp = [tokens[b]], [cur[b]], [limit[b]], [False], [stop_pos[b]]
            nt, ps = R.generate_step_rows(None, [t[j]], tk, cu, li, pos_base, stop_seqs, st, sp)
            wrote = cu[0] != c0
            cur[b], stopped[b], stop_pos[b], next_tok[b], pos[b] = cu[0], st[0], sp[0], nt[0], ps[0]
            if wrote:                     # the plain loop's record and advance of this emission: column c0, the raw row of query j
                emitted += 1
                m = b * Q + j
                row = torch.tensor([tokens[b]], dtype=torch.long)
                if logprob is not None or seen_bm is not None:
                    G.generate_record(logits[m:m + 1] if logits is not None else None, lse[m:m + 1] if lse is not None else None, row,
                                      seen_bm[b:b + 1] if seen_bm is not None else None, logprob[b:b + 1] if logprob is not None else None, V,
                                      cur=[c0 + 1], prompt_len=[prompt_len[b]])
                if state is not None:
                    state[b] = C.constrain_advance_ref(row.numpy(), 0, np.array([c0 + 1]), np.array([prompt_len[b]]), None, trans, state[b:b + 1])[0]
            if st[0]:
                break
        if emitted:
            stats[0] += nd
            stats[1] += emitted - 1
    return next_tok, pos


def uniform_index(row_base, cur, prompt_len, Q, n_uni):
    """a3v_verify_uniforms' index per virtual row."""
    return [min(max(row_base[b] + (cur[b] - prompt_len[b]) + j, 0), n_uni - 1) for b in range(len(cur)) for j in range(Q)]
