"""Host restatements of the ragged-decode kernels (a3v_ragged.hip): fp64 for the floating-point ones, plain integers for the token
bookkeeping.  No GPU; tests/test_ragged_cpu.py pins them against hand-worked cases, tests/test_gpu_ragged.py holds the kernels to them."""
import math

import torch


def rope_rows_fp64(qkv, cos_sin, pos, H, Hkv, hd, Smax):
    """qkv [B, (H+2Hkv)*hd], cos_sin [P, hd/2, 2], pos: list of ints.  Returns (q [B,H,hd] rotated; zeros for an idle row,
    {(b, p): (k [Hkv,hd] rotated, v [Hkv,hd])} for the rows that write position p of their cache row)."""
    B = qkv.shape[0]
    x = qkv.double().view(B, H + 2 * Hkv, hd)
    q = torch.zeros(B, H, hd, dtype=torch.float64)
    writes = {}
    for b, p in enumerate(pos):
        if p < 0 or p >= Smax:
            continue
        co, si = cos_sin[p, :, 0].double(), cos_sin[p, :, 1].double()
        a, bb = x[b, :H + Hkv, 0::2], x[b, :H + Hkv, 1::2]
        rot = torch.stack([a * co - bb * si, a * si + bb * co], dim=-1).reshape(H + Hkv, hd)
        q[b] = rot[:H]
        writes[(b, p)] = (rot[H:], x[b, H + Hkv:].clone())
    return q, writes


def decode_attention_rows_fp64(q, k, vt, sk):
    """q [B,H,hd], k [B,Hkv,Smax,hd], vt [B,Hkv,hd,Smax], sk: list of ints (<= 0: idle row, zeros).  Only keys 0 .. sk[b]-1 are read:
    whatever the cache holds behind them (NaN included) cannot reach the result.  fp64 [B,H,hd]."""
    B, H, hd = q.shape
    Hkv = k.shape[1]
    out = torch.zeros(B, H, hd, dtype=torch.float64)
    for b in range(B):
        n = int(sk[b])
        if n <= 0:
            continue
        for h in range(H):
            hk = h // (H // Hkv)
            s = (k[b, hk, :n].double() @ q[b, h].double()) / math.sqrt(hd)
            p = torch.softmax(s, dim=0)
            out[b, h] = vt[b, hk, :, :n].double() @ p
    return out


def generate_step_rows(logits, sampled, tokens, cur, limit, pos_base, stop_seqs, stopped, stop_pos):
    """a3v_generate_step_rows on Python lists, in place (tokens: list of rows; cur, limit, stopped, stop_pos: lists).  ``logits``:
    list of rows (argmax, first index on ties) or None with ``sampled`` ids.  Returns (next_tok, pos)."""
    B = len(tokens)
    next_tok, pos = [0] * B, [-1] * B
    for b in range(B):
        if stopped[b]:
            continue
        c, lim = cur[b], limit[b]
        if c < 0 or c >= lim or c >= len(tokens[b]):
            stopped[b] = True
            continue
        if sampled is not None:
            nxt = int(sampled[b])
        else:
            row = logits[b]
            nxt = max(range(len(row)), key=lambda i: (row[i], -i))
        tokens[b][c] = nxt
        st, sp = False, c + 1
        for seq in stop_seqs:
            n = len(seq)
            if c + 1 - n < 0 or st:
                continue
            if tokens[b][c + 1 - n:c + 1] == list(seq):
                sp, st = c + 1 - n, True
        c += 1
        cur[b] = c
        if c >= lim:
            st = True
        stopped[b] = st
        stop_pos[b] = sp
        if not st:
            next_tok[b], pos[b] = nxt, pos_base + c - 1
    return next_tok, pos
