"""-m gpu: lookup decoding (a3v_spec.hip, Transformer.forward_verify_rows, MetaModel.generate_many(lookup=)) -- the span kernels
against the per-row entries they restate (bit for bit where the walk is the same) and against fp64, the integer kernels against
tests/spec_ref.py, the step against the per-kernel sequence, the model level against the plain loop and the oracle."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import ragged_ref as R
import spec_ref as S
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY, synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _live(pos, nq, Q, bound):
    """live[b][j]: query j of row b is live (position inside ``bound``)"""
    return [[p >= 0 and j < n and p + j < bound for j in range(Q)] for p, n in zip(pos, nq)]


def _strides(H, Hkv, hd, Smax):
    return (H * hd, H * hd, hd, Hkv * Smax * hd, Smax * hd, hd, Hkv * hd * Smax, hd * Smax, Smax, H * hd, H * hd, hd)


# ------------------------------------------------------------------ 1. rope_kvcache_spans
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kvcache_spans_equals_the_rows_entry_query_by_query(hd, dtype):
    B, Q, H, Hkv, Smax = 3, 4, 4, 2, 72
    pos, nq = [62, -1, Smax - 2], [4, 1, 4]
    live = _live(pos, nq, Q, Smax)
    assert [sum(r) for r in live] == [4, 0, 2]
    qkv = gen(B * Q, (H + 2 * Hkv) * hd, seed=hd).to(dtype).to(DEV)
    cs = plugin.precompute_cos_sin(hd, Smax, 10000.0, None).to(DEV)
    k0 = torch.full((B, Hkv, Smax, hd), 77.0, dtype=dtype, device=DEV)             # canary
    v0 = torch.full((B, Hkv, hd, Smax), 77.0, dtype=dtype, device=DEV)
    kw, vw, qw = k0.clone(), v0.clone(), torch.zeros(B * Q, H * hd, dtype=dtype, device=DEV)
    for j in range(Q):                                                             # Q calls of the rows entry, one per query index
        pj = [pos[b] + j if live[b][j] else -1 for b in range(B)]
        qj = torch.zeros(B, H * hd, dtype=dtype, device=DEV)
        ops.rope_kvcache_rows(qkv[j::Q].contiguous(), qj, kw, vw, cs, i32(pj), B, H, Hkv, hd)
        qw[j::Q] = qj
    kg, vg = k0.clone(), v0.clone()
    qg = torch.full((B * Q, H * hd), 7.0, dtype=dtype, device=DEV)
    ops.rope_kvcache_spans(qkv, qg, kg, vg, cs, i32(pos), i32(nq), B, Q, H, Hkv, hd)
    assert torch.equal(qg, qw), "q rows (idle queries: zeros)"
    assert torch.equal(kg, kw) and torch.equal(vg, vw), "whole caches: the written positions and every other byte"
    for b in range(B):
        changed = (kg[b, 0] != 77.0).any(dim=1).nonzero().flatten().tolist()
        assert changed == [pos[b] + j for j in range(Q) if live[b][j]], (b, changed)
        for j in range(Q):
            if not live[b][j]:
                assert float(qg[b * Q + j].float().abs().sum()) == 0


# ------------------------------------------------------------------ 2. attention_verify_rows
def _verify(q, k, vt, pos, nq, sk_max, B, Q, H, Hkv, hd):
    Smax = k.shape[2]
    out = torch.full((B * Q, H * hd), float("nan"), dtype=q.dtype, device=DEV)
    scratch = ctr = None
    if q.dtype == BF and hd in (64, 128):
        scratch = torch.full((ops.attention_verify_rows_scratch_floats(B, Q, H, hd, sk_max),), float("nan"), dtype=torch.float32, device=DEV)
        ctr = torch.zeros(2 * B * H, dtype=torch.int32, device=DEV)
    ops.attention_verify_rows(q, k, vt, out, i32(pos), i32(nq), sk_max, B, Q, H, Hkv, hd, _strides(H, Hkv, hd, Smax), scratch, ctr)
    if ctr is not None:
        assert int(ctr.abs().sum()) == 0, "the arrival counters are left at zero"
    return out


def _span_caches(B, Hkv, hd, Smax, pos, live, seed, dtype=BF):
    """bf16-exact caches; everything behind a row's last live key holds NaN"""
    k = gen(B, Hkv, Smax, hd, seed=seed).to(dtype)
    vt = gen(B, Hkv, hd, Smax, seed=seed + 1).to(dtype)
    for b, p in enumerate(pos):
        n = max(p + sum(live[b]), 0)
        k[b, :, n:] = float("nan")
        vt[b, :, :, n:] = float("nan")
    return k.to(DEV), vt.to(DEV)


@pytest.mark.parametrize("sk_max", [64, 300])
@pytest.mark.parametrize("Q", [1, 2, 5, 8])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2)])
@pytest.mark.parametrize("hd", [64, 128])
def test_attention_verify_rows_bf16(hd, H, Hkv, Q, sk_max):
    """Reference: fp64 attention per query over its own key count.  Bound: the project's bf16 decode-attention bound,
    4e-3 + 2^-7 |want| (tests/test_gpu_kernels.py, tests/test_gpu_kv8.py).  Row 0's queries straddle the 64-key tile edge, row 1's
    the first key-range edge of the plan (128 at sk_max 300), row 2 is idle, row 3 has nq < Q."""
    B, Smax = 4, 320
    ns = ops.attention_verify_rows_splits(B, H, sk_max)
    if sk_max == 64:
        assert ns == 1
        pos = [62, 30, -1, 5]
    else:
        assert ns == 3, ns            # 300 keys in three ranges: the range length is 128
        pos = [62, 126, -1, 290]
    nq = [Q, Q, Q, min(Q, 2)]
    live = _live(pos, nq, Q, sk_max)
    q = gen(B * Q, H * hd, seed=3 + Q).to(BF).to(DEV)
    k, vt = _span_caches(B, Hkv, hd, Smax, pos, live, seed=4)
    got = _verify(q, k, vt, pos, nq, sk_max, B, Q, H, Hkv, hd)
    sk = [pos[b] + j + 1 if live[b][j] else 0 for b in range(B) for j in range(Q)]
    kq, vq = k.cpu().repeat_interleave(Q, 0), vt.cpu().repeat_interleave(Q, 0)
    want = R.decode_attention_rows_fp64(q.float().cpu().view(B * Q, H, hd), kq, vq, sk).float()
    g = got.float().cpu().view(B * Q, H, hd)
    assert torch.isfinite(g).all()
    err = (g - want).abs()
    print(f"hd {hd}, H {H}/{Hkv}, Q {Q}, sk_max {sk_max} ({ns} key ranges): max err {float(err.max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    assert bool((err <= 4e-3 + 2 ** -7 * want.abs()).all()), float(err.max())
    for m, n in enumerate(sk):
        if n == 0:
            assert float(g[m].abs().sum()) == 0, m
    assert float(want[0].abs().max()) > 0 and float(want[3 * Q].abs().max()) > 0
    # query 0 of every row does not depend on whether the later queries of its row are live (same sk_max, same cache)
    alone = _verify(q, k, vt, pos, [1] * B, sk_max, B, Q, H, Hkv, hd)
    assert torch.equal(alone[0::Q], got[0::Q])
    if Q > 1:
        assert float(alone[1::Q].float().abs().sum()) == 0


@pytest.mark.parametrize("hd,dtype", [(16, torch.float32), (32, BF)], ids=["fp32-hd16", "bf16-hd32"])
def test_attention_verify_rows_one_wave_form_equals_the_rows_entry(hd, dtype):
    B, Q, H, Hkv, Smax, sk_max = 3, 4, 4, 2, 128, 110
    pos, nq = [62, -1, 100], [4, 1, 3]
    live = _live(pos, nq, Q, sk_max)
    q = gen(B * Q, H * hd, seed=10).to(dtype).to(DEV)
    k, vt = _span_caches(B, Hkv, hd, Smax, pos, live, seed=11, dtype=dtype)
    got = _verify(q, k, vt, pos, nq, sk_max, B, Q, H, Hkv, hd)
    assert torch.isfinite(got.float()).all()
    for j in range(Q):
        sk = [pos[b] + j + 1 if live[b][j] else 0 for b in range(B)]
        out = torch.full((B, H * hd), float("nan"), dtype=dtype, device=DEV)
        ops.attention_decode_rows(q[j::Q].contiguous(), k, vt, out, i32(sk), sk_max, B, H, Hkv, hd, _strides(H, Hkv, hd, Smax))
        assert torch.equal(got[j::Q], out), j
    assert float(got[Q:2 * Q].float().abs().sum()) == 0 and float(got[2 * Q + 3].float().abs().sum()) == 0


# ------------------------------------------------------------------ 3. the integer kernels
DRAFT_ROWS = [[5, 7, 8, 9, 1, 8, 4, 2, 7, 8], [3, 4, 10, 11, 3, 4, 20, 21, 3, 4], [9, 6, 6], [1, 2, 3, 4], [7], [3, 4, 10, 11, 12, 3, 4],
              [3, 4, 3, 4], [3, 4, 3, 4], [3, 4, 10, 11, 12, 3, 4], [3, 4, 10, 11, 12, 3, 4]]


@pytest.mark.parametrize("D,ngram", [(3, 3), (3, 1), (1, 2), (7, 2)])
def test_lookup_draft_rows_is_the_integer_restatement(D, ngram):
    W, Smax = 24, 100
    B = len(DRAFT_ROWS)
    tokens = [r + [0] * (W - len(r)) for r in DRAFT_ROWS]
    cur = [len(r) for r in DRAFT_ROWS]
    limit = [W] * B
    pos = [c - 1 for c in cur]
    stopped = [False] * B
    stopped[6] = True                              # a stopped row
    pos[7] = -1                                    # an idle row
    limit[8] = cur[8] + 2                          # a row next to its limit
    pos[9] = Smax - 2                              # a row next to the end of the cache
    next_tok = [r[-1] for r in DRAFT_ROWS]
    wx, wn = S.lookup_draft_rows(tokens, cur, limit, pos, stopped, next_tok, D, ngram, Smax)
    x = torch.full((B, D + 1), -5, dtype=torch.long, device=DEV)
    nq = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    ops.lookup_draft_rows(torch.tensor(tokens, device=DEV), i32(cur), i32(limit), i32(pos), torch.tensor(stopped, device=DEV),
                          torch.tensor(next_tok, device=DEV), D, ngram, Smax, x, nq)
    assert x.tolist() == wx and nq.tolist() == wn, (x.tolist(), wx, nq.tolist(), wn)
    assert max(wn) > 1 and min(wn) == 1


def test_lookup_draft_rows_long_row():
    """more tokens than one pass of the block: the latest of many matches"""
    g = torch.Generator().manual_seed(1)
    row = torch.randint(3, 9, (700,), generator=g).tolist()
    tokens, cur = [row + [0] * 20], [len(row)]
    wx, wn = S.lookup_draft_rows(tokens, cur, [720], [699], [False], [row[-1]], 4, 3, 4096)
    x = torch.zeros((1, 5), dtype=torch.long, device=DEV)
    nq = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.lookup_draft_rows(torch.tensor(tokens, device=DEV), i32(cur), i32([720]), i32([699]), torch.tensor([False], device=DEV),
                          torch.tensor([row[-1]], device=DEV), 4, 3, 4096, x, nq)
    assert x.tolist() == wx and nq.tolist() == wn and wn[0] == 5


def test_accept_rows_is_the_integer_restatement():
    """all accepted / first draft rejected / a stop sequence completed by an accepted draft / the limit in the middle / nq < Q, and
    a batch that also holds a stopped row, an idle (stopped) row and a row at its limit; ties go to the first index."""
    Q, V, W, base = 4, 50, 16, 5
    stops = ((15,), (8, 9))
    model = [7, 8, 9, 10]
    cases = [  # x, nq, limit, stopped
        ([6, 7, 8, 9], 4, 16, False), ([6, 5, 8, 9], 4, 16, False), ([6, 7, 8, 9], 2, 16, False), ([6, 7, 8, 9], 4, 5, False),
        ([6, 7, 8, 9], 4, 16, True), ([0, 0, 0, 0], 1, 16, True), ([6, 7, 8, 9], 4, 3, False), ([6, 7, 8, 9], 4, 4, False)]
    B = len(cases)
    logits = gen(B * Q, V, seed=2)
    for b in range(B):
        for j in range(Q):
            logits[b * Q + j, model[j]] = 9.0
    logits[0 * Q + 1, 30] = 9.0                     # a tie on query 1 of row 0: the first index (8) wins
    for st in (stops, ((15,),)):
        tokens = [[1, 2, 6] + [0] * (W - 3) for _ in range(B)]
        cur, limit = [3] * B, [c[2] for c in cases]
        stopped, stop_pos, stats = [c[3] for c in cases], [4] * B, [0, 0]
        x, nq = [c[0] for c in cases], [c[1] for c in cases]
        d = dict(tokens=torch.tensor(tokens, device=DEV), cur=i32(cur), limit=i32(limit), stopped=torch.tensor(stopped, device=DEV),
                 stop_pos=torch.tensor(stop_pos, device=DEV), next_tok=torch.full((B,), -3, dtype=torch.long, device=DEV),
                 pos=torch.full((B,), -3, dtype=torch.int32, device=DEV), stats=torch.zeros(2, dtype=torch.long, device=DEV))
        seq = torch.tensor([t for s in st for t in s], device=DEV)
        offs = [0]
        for s in st:
            offs.append(offs[-1] + len(s))
        ops.accept_rows(logits.to(DEV), torch.tensor(x, device=DEV), i32(nq), d["tokens"], d["cur"], d["limit"], base, seq, i32(offs), len(st),
                        d["stopped"], d["stop_pos"], d["next_tok"], d["pos"], d["stats"])
        nt, ps = S.accept_rows(logits.tolist(), x, nq, tokens, cur, limit, base, st, stopped, stop_pos, stats)
        got = (d["tokens"].tolist(), d["cur"].tolist(), d["stopped"].tolist(), d["stop_pos"].tolist(), d["next_tok"].tolist(),
               d["pos"].tolist(), d["stats"].tolist())
        assert got == (tokens, cur, stopped, stop_pos, nt, ps, stats), (got, (tokens, cur, stopped, stop_pos, nt, ps, stats))
    assert cur[0] == 7 and cur[1] == 4 and stats[1] > 0


# ------------------------------------------------------------------ models
VOCAB = 640
# (hd 64 at dim 512: the fp8 and NF4 GEMVs of the fused step need K >= 512, as in the fp8-KV and ragged step tests)
GEOM = {64: dict(dim=512, n_layers=2, n_heads=8, n_kv_heads=4, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}


def _model(hd, weights=None, dtype=BF, max_seq_len=128, max_batch_size=32):
    oargs = ref_cpu.OracleArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, **GEOM[hd])
    sd = ref_cpu.make_decoder_weights(oargs, seed=0, std=0.05)
    m = plugin.Transformer(plugin.ModelArgs(vocab_size=VOCAB, max_seq_len=max_seq_len, max_batch_size=max_batch_size, **GEOM[hd]))
    m.load_state_dict(sd)
    m.to(dtype).to(DEV)
    if weights is not None:
        m.quantize_decode_weights(weights)
    return m, oargs, sd


# ------------------------------------------------------------------ 4. the step
def _per_kernel_step_verify(m, x, pos, nq, pos_max):
    """One verify step as the sequence of public entries over the chunks of the C call: rmsnorm, GEMV, a3v_rope_kvcache_spans,
    a3v_attention_verify_rows, GEMV + residual, rmsnorm, GEMV SwiGLU, GEMV + residual."""
    a = m.args
    B, Q = x.shape
    M = B * Q
    H, Hkv, hd, dim = m.n_heads, m.n_kv_heads, m.head_dim, a.dim
    hh = torch.empty(M, dim, dtype=BF, device=DEV)
    ops.embed_assemble(x.view(M, 1), m.tok_embeddings.weight, hh, M, 1, 0, dim)
    pk, fmt, images = m._pack(), m.weight_format, None if m._weights is None else m._weights.images
    smax = m._k_cache[0].shape[2]
    sk_max = min(pos_max + Q, smax)
    Bc = B if M <= 16 else 16 // Q
    for b0 in range(0, B, Bc):
        nbr = min(Bc, B - b0)
        nb = nbr * Q
        h, p, n = hh[b0 * Q:b0 * Q + nb], pos[b0:b0 + nbr].contiguous(), nq[b0:b0 + nbr].contiguous()
        xn, qkv = torch.empty_like(h), torch.empty(nb, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
        att, act = torch.empty(nb, H * hd, dtype=BF, device=DEV), torch.empty(nb, m.ffn, dtype=BF, device=DEV)
        scratch = torch.empty(ops.attention_verify_rows_scratch_floats(nbr, Q, H, hd, sk_max), dtype=torch.float32, device=DEV)
        ctr = torch.zeros(2 * nbr * H, dtype=torch.int32, device=DEV)

        def lin(xx, i, key, out, **kw):
            idx = ("wqkv", "wo", "w13", "w2").index(key)
            ws = m._skinny_ws(nb, out.shape[1] * (2 if kw.get("epilogue") == ops.EPI_SWIGLU else 1), xx.shape[1])
            if fmt == "nf4":
                return ops.gemm_skinny_nf4(xx, *images[f"{key}.{i}"], out, ws, **kw)
            if fmt == "fp8":
                return ops.gemm_skinny_fp8(xx, *images[f"{key}.{i}"], out, ws, **kw)
            assert fmt == "bf16"
            lyr = m.layers[i]
            w = (pk[f"wqkv.{i}"], lyr.attention.wo.weight, pk[f"w13.{i}"], lyr.feed_forward.w2.weight)[idx]
            return ops.gemm_skinny(xx, w, out, ws, **kw)
        ldq = (H + 2 * Hkv) * hd
        for i, lyr in enumerate(m.layers):
            kc, vc = m._k_cache[i][b0:b0 + nbr], m._vt_cache[i][b0:b0 + nbr]
            ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
            lin(xn, i, "wqkv", qkv)
            ops.rope_kvcache_spans(qkv, qkv, kc, vc, m._cos_sin_dev(), p, n, nbr, Q, H, Hkv, hd)
            ops.attention_verify_rows(qkv, kc, vc, att, p, n, sk_max, nbr, Q, H, Hkv, hd, (ldq, ldq, hd) + _strides(H, Hkv, hd, smax)[3:], scratch, ctr)
            lin(att, i, "wo", h, residual=h, epilogue=ops.EPI_RESIDUAL)
            ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
            lin(xn, i, "w13", act, epilogue=ops.EPI_SWIGLU)
            lin(act, i, "w2", h, residual=h, epilogue=ops.EPI_RESIDUAL)
        assert int(ctr.abs().sum()) == 0
    xn = torch.empty_like(hh)
    ops.rmsnorm(hh, m.norm.weight, xn, a.norm_eps)
    logits = torch.empty(M, a.vocab_size, dtype=torch.float32, device=DEV)
    m._lm_head_f32(xn, logits)
    return logits


@pytest.mark.parametrize("B,Q,pos,nq", [(3, 4, [5, -1, 40], [4, 1, 2]), (4, 8, [5, 0, -1, 100], [8, 3, 1, 8])], ids=["B3Q4", "B4Q8-two-chunks"])
@pytest.mark.parametrize("weights", [None, "fp8", "nf4"])
@pytest.mark.parametrize("hd", [64, 128])
def test_step_verify_equals_the_per_kernel_sequence(hd, weights, B, Q, pos, nq):
    m, _, _ = _model(hd, weights)
    w8 = {None: 0, "fp8": 1, "nf4": 2}[weights]
    assert lib.load().a3v_llama_decode_step_verify_form(B, Q, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, w8) == 2
    m.allocate_rows(B)
    before = []
    for i in range(m.n_layers):                              # an arbitrary earlier context in every cache row
        m._k_cache[i].copy_(gen(*m._k_cache[i].shape, seed=20 + i).to(BF))
        m._vt_cache[i].copy_(gen(*m._vt_cache[i].shape, seed=30 + i).to(BF))
        before.append((m._k_cache[i].clone(), m._vt_cache[i].clone()))
    x = torch.randint(3, VOCAB, (B, Q), generator=torch.Generator().manual_seed(B)).to(DEV)
    p, n = i32(pos), i32(nq)
    pos_max = max(pos)
    fused = m.forward_verify_rows(x, p, n, pos_max).clone()
    after = [(k.clone(), v.clone()) for k, v in zip(m._k_cache, m._vt_cache)]
    for i, (k, v) in enumerate(before):
        m._k_cache[i].copy_(k)
        m._vt_cache[i].copy_(v)
    per = _per_kernel_step_verify(m, x, p, n, pos_max)
    assert torch.isfinite(fused).all()
    live = _live(pos, nq, Q, m._k_cache[0].shape[2])
    for i, (k, v) in enumerate(after):
        assert torch.equal(m._k_cache[i], k) and torch.equal(m._vt_cache[i], v), i
        for b, pb in enumerate(pos):                         # only the live positions of row b changed
            keep = torch.ones(k.shape[2], dtype=torch.bool, device=DEV)
            for j in range(Q):
                if live[b][j]:
                    keep[pb + j] = False
            assert torch.equal(k[b][:, keep], before[i][0][b][:, keep]) and torch.equal(v[b][:, :, keep], before[i][1][b][:, :, keep]), (i, b)
    assert torch.equal(fused, per)
    if weights is None and B == 3:                            # the plugin's own kernel-by-kernel path
        for i, (k, v) in enumerate(before):
            m._k_cache[i].copy_(k)
            m._vt_cache[i].copy_(v)
        m._per_kernel_decode = True
        assert torch.equal(m.forward_verify_rows(x, p, n, pos_max), per)


# ------------------------------------------------------------------ 5. model level, fp32
def _tiny_meta(dtype=torch.float32, max_seq_len=96):
    cfg = os.path.join(GD, "tiny_params.json")
    mm = MetaModel("llama_ens5", cfg, os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=max_seq_len)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(dtype).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": max_seq_len}), sd)
    return mm, dec


PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
GEN = [3, 9, 2, 6, 4]


@pytest.fixture(scope="module")
def text_case():
    mm, dec = _tiny_meta()
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in PROMPTS]
    want = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, return_ids=True)[1]
    return mm, dec, pt, want


def _scripted(mm, pt, want, D, right):
    """a drafter that knows the greedy continuation of every prompt: ``right`` drafts it, else drafts ids the model never picks"""
    V = mm.tokenizer.n_words

    def draft(tokens, cur, limit, pos, stopped, next_tok, x, nq):
        tk, cu, li, st, nt = tokens.tolist(), cur.tolist(), limit.tolist(), stopped.tolist(), next_tok.tolist()
        xs, ns = [], []
        for r in range(len(tk)):
            row, nd = [nt[r]] + [0] * D, 0
            if not st[r]:
                i = next(i for i, t in enumerate(pt) if tk[r][:len(t)] == t and cu[r] > len(t) and tk[r][len(t):cu[r]] == (want[i] + [mm.tokenizer.eos_id])[:cu[r] - len(t)])
                full = pt[i] + want[i]
                room = li[r] - 1 - cu[r]
                if right:
                    nd = max(min(D, len(full) - cu[r], room), 0)
                    row[1:1 + nd] = full[cu[r]:cu[r] + nd]
                else:
                    nd = max(min(D, room), 0)
                    nxt = full[cu[r]] if cu[r] < len(full) else mm.tokenizer.eos_id
                    row[1:1 + nd] = [(nxt + 1) % V] * nd
            xs.append(row)
            ns.append(1 + nd)
        x.copy_(torch.tensor(xs, device=DEV))
        nq.copy_(i32(ns))
    return draft


@pytest.mark.parametrize("rows", [1, 2])
def test_generate_many_lookup_equals_the_plain_loop(text_case, rows):
    mm, _, pt, want = text_case
    assert mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True)[1] == want
    D = 3
    got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, lookup=D)
    assert got[1] == want and got[0] == [mm.tokenizer.decode(t) for t in want]
    got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, lookup=D, lookup_drafter=_scripted(mm, pt, want, D, True))
    st = dict(mm.last_lookup_stats)
    print("perfect drafter:", st)
    assert got[1] == want
    assert st["drafted"] > 0 and st["accepted"] == st["drafted"] and st["tokens"] == st["steps"] + st["accepted"]
    got = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, lookup=D, lookup_drafter=_scripted(mm, pt, want, D, False))
    st = dict(mm.last_lookup_stats)
    print("wrong drafter:", st)
    assert got[1] == want
    assert st["drafted"] > 0 and st["accepted"] == 0 and st["steps"] == st["tokens"]      # one token per row step: the plain loop's count
    for pe in (1, 3):
        assert mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, lookup=D, poll_every=pe)[1] == want, pe
    stops = ("li", "ab")
    one = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=12, additional_stop_symbols=stops, return_ids=True)[1]
    for D2 in (1, 7):
        assert mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=12, additional_stop_symbols=stops, return_ids=True, lookup=D2)[1] == one, D2


def test_generate_many_lookup_with_image_equals_the_plain_loop():
    TK = dict(dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=256)
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
    m = plugin.Transformer(plugin.ModelArgs(**TK, vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1), with_visual=True)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(**TK), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    m.load_state_dict({**sd, **vsd})
    mm.llma = m.to(DEV)
    prompts, gens = PROMPTS[:3], [5, 2, 4]
    img = synth_image(3, size=112, seed=3)
    want = mm.generate_many(prompts, img, batch_rows=2, max_gen_len=gens, return_ids=True)[1]
    for rows in (1, 2):
        assert mm.generate_many(prompts, img, batch_rows=rows, max_gen_len=gens, return_ids=True, lookup=3)[1] == want, rows


# ------------------------------------------------------------------ 6. model level, bf16
def test_forward_verify_rows_bf16_against_the_oracle():
    """Rows prefilled with prompts of different lengths, then one verify step of Q = 4 queries: the logits of query j against the
    oracle fed the same tokens one by one, within the bf16 model bound of tests/test_gpu_ragged.py (4e-2 of max |logit|)."""
    m, oargs, sd = _model(64)
    sdb = {k: v.to(BF) for k, v in sd.items()}
    lens, nq, Q = [9, 1, 30], [4, 2, 3], 4
    B = len(lens)
    ex = torch.randint(3, VOCAB, (B, 40), generator=torch.Generator().manual_seed(3))
    ex[:, 0] = 1
    assert lib.load().a3v_llama_decode_step_verify_form(B, Q, m.args.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, 0) == 2
    m.allocate_rows(B)
    for b, n in enumerate(lens):
        m.prefill_row(b, ex[b:b + 1, :n].to(DEV))
    x = torch.stack([ex[b, n:n + Q] for b, n in enumerate(lens)]).to(DEV)
    got = m.forward_verify_rows(x, i32(lens), i32(nq), max(lens)).cpu()
    for b, n in enumerate(lens):
        d = ref_cpu.OracleDecoder(oargs, sdb)
        d.forward_inference(ex[b:b + 1, :n], 0)
        for j in range(nq[b]):
            w = d.forward_inference(ex[b:b + 1, n + j:n + j + 1], n + j).float()
            e = float((got[b * Q + j:b * Q + j + 1] - w).abs().max() / w.abs().max())
            print(f"row {b} query {j}: {e:.3e} of max |logit| {float(w.abs().max()):.3e}")
            assert e < 4e-2, (b, j, e)


# ------------------------------------------------------------------ 7. lookup really drafts
def test_lookup_drafts_hit_on_a_repetitive_answer():
    """The oracle's greedy answer is searched (on the CPU, tests/spec_ref.py) for a prompt on which prompt lookup has drafts
    accepted; that prompt then runs on the device: same ids, drafted > 0, more than one token per row step."""
    mm, dec = _tiny_meta(max_seq_len=96)
    eos, D, N = mm.tokenizer.eos_id, 3, 48
    pick = None
    for text in ("the lid the lid the lid the", "1 2 3 1 2 3 1 2 3 1 2", "Open Open Open Open", "a b a b a b a b a b"):
        t = mm.tokenizer.encode(text, bos=True, eos=False)
        ids = ref_cpu.generate_greedy(dec, [t], max_gen_len=N, eos_id=eos)[1][0]
        full, hits = t + ids, 0
        c = len(t) + 1
        while c < len(full):                                   # replay: the drafts of every step against the known continuation
            x, nq = S.lookup_draft_rows([full[:c] + [0] * 8], [c], [len(t) + N], [c - 1], [False], [full[c - 1]], D, 3, 4096)
            acc = 0
            while acc < nq[0] - 1 and c + acc < len(full) and x[0][1 + acc] == full[c + acc]:
                acc += 1
            hits += acc
            c += 1 + acc
        if hits > 0:
            pick = (text, ids)
            break
    assert pick is not None, "no candidate prompt has an answer on which lookup drafts are accepted"
    text, ids = pick
    plain = mm.generate_many([text], None, batch_rows=1, max_gen_len=N, return_ids=True)[1][0]
    got = mm.generate_many([text], None, batch_rows=1, max_gen_len=N, return_ids=True, lookup=D)[1][0]
    st = mm.last_lookup_stats
    print(text, st, "equals the oracle's ids:", plain == ids)
    assert got == plain
    assert st["drafted"] > 0 and st["accepted"] > 0 and st["tokens"] / st["steps"] > 1


# ------------------------------------------------------------------ 8. the eval entry
def test_eval_entry_lookup_decoding_writes_the_same_records(tmp_path):
    from a3vlm_amd import checkpoint as ck
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
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "10", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32",
           "--continuous_rows", "2"]
    for flag, extra in (("rows", []), ("lookup", ["--lookup_decoding", "3"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = json.load(open(tmp_path / "logs" / "rows" / "demo.json"))
    b = json.load(open(tmp_path / "logs" / "lookup" / "demo.json"))
    assert len(a) == len(b) > 0
    for ra, rb in zip(a, b):
        assert "accepted_per_step" not in ra and isinstance(rb.pop("accepted_per_step"), float)
        assert json.dumps(ra, ensure_ascii=False) == json.dumps(rb, ensure_ascii=False)
