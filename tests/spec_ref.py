"""Host restatements of the integer kernels of lookup decoding (a3v_spec.hip): the prompt-lookup draft rule and the accept rule,
on Python lists.  No GPU; tests/test_spec_cpu.py pins them against hand-worked cases, tests/test_gpu_spec.py holds the kernels to
them bit for bit.  The accept rule is ragged_ref's token step, once per emission."""
import ragged_ref as R


def lookup_draft_rows(tokens, cur, limit, pos, stopped, next_tok, D, max_ngram, Smax):
    """a3v_lookup_draft_rows.  tokens: list of rows; cur, limit, pos, stopped, next_tok: lists.  Returns (x [B][D+1], nq [B])."""
    B, Q = len(tokens), D + 1
    x, nq = [[0] * Q for _ in range(B)], [1] * B
    for b in range(B):
        x[b][0] = int(next_tok[b])
        c = cur[b]
        if stopped[b] or pos[b] < 0 or c < 1 or c > len(tokens[b]):
            continue
        t = tokens[b]
        at = -1
        for n in range(min(max_ngram, c - 1), 0, -1):
            tail = t[c - n:c]
            hits = [i for i in range(0, c - n) if t[i:i + n] == tail]          # i + n <= c - 1
            if hits:
                at = hits[-1] + n                                               # the latest match; the drafts start behind it
                break
        if at < 0:
            continue
        nd = max(min(D, c - at, limit[b] - 1 - c, Smax - 1 - pos[b]), 0)
        for e in range(1, nd + 1):
            x[b][e] = int(t[at + e - 1])
        nq[b] = 1 + nd
    return x, nq


def argmax_first(row):
    return max(range(len(row)), key=lambda i: (row[i], -i))


def accept_rows(logits, x, nq, tokens, cur, limit, pos_base, stop_seqs, stopped, stop_pos, stats):
    """a3v_accept_rows, in place.  logits: list of B*Q rows (virtual row b*Q + j), x [B][Q], nq [B]; stats = [drafted, accepted].
    Returns (next_tok, pos)."""
    B, Q = len(tokens), len(x[0])
    next_tok, pos = [0] * B, [-1] * B
    for b in range(B):
        if stopped[b]:
            continue
        nd = min(max(nq[b], 1), Q) - 1
        t = [argmax_first(logits[b * Q + j]) for j in range(nd + 1)]
        emitted = 0
        for j in range(nd + 1):
            if j > 0 and t[j - 1] != x[b][j]:
                break
            # one token step of the ragged loop for this row alone, with the chosen id handed over as `sampled`
            tk, cu, li, st, sp = [tokens[b]], [cur[b]], [limit[b]], [False], [stop_pos[b]]
            nt, ps = R.generate_step_rows(None, [t[j]], tk, cu, li, pos_base, stop_seqs, st, sp)
            wrote = cu[0] != cur[b]
            cur[b], stopped[b], stop_pos[b], next_tok[b], pos[b] = cu[0], st[0], sp[0], nt[0], ps[0]
            emitted += 1 if wrote else 0
            if st[0]:
                break
        if emitted:
            stats[0] += nd
            stats[1] += emitted - 1
    return next_tok, pos
