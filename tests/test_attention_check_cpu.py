"""oracle/attn_check.py on the host: its per-element bound accepts a float32 model of where the bf16 attention kernels round,
and rejects that model with one bug class of those kernels put in (a dropped key tile, an off-by-one causal diagonal, swapped
heads, a GQA head left out of the dK / dV sum, a shifted LSE, a wrong softmax scale, a dropped ragged dV row)."""
import math

import pytest
import torch

from oracle import attn_check as ac
from oracle import ref_cpu

BF = torch.bfloat16


def rt(x):
    return x.to(BF).float()


def inputs(B, S, H, Hkv, hd, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (rt(torch.randn(*s, generator=g)) for s in ((B, S, H, hd), (B, S, Hkv, hd), (B, S, Hkv, hd), (B, S, H, hd)))
    return q, k, v, do


def emulate(q, k, v, do, causal, mut=None):
    """float32 model of the prefill forward + MFMA backward: scores in fp32, P = exp(s - lse) rounded to bf16 before P.V and
    P^T.dO, O rounded to bf16 before D = rowsum(dO * O), dS = P (dP - D) rounded to bf16 before dS.K and dS^T.Q, every output
    rounded to bf16 (lse stays fp32).  ``mut`` puts one bug in."""
    B, S, H, hd = q.shape
    Hkv = k.shape[2]
    n_rep = H // Hkv
    scale = 1.0 / math.sqrt(hd) * (1 + 2 ** -6 if mut == "scale" else 1.0)
    qi, ki = torch.arange(S)[:, None], torch.arange(S)[None, :]
    allow = ref_cpu.make_causal_mask(S, S) if causal else torch.ones(S, S, dtype=torch.bool)
    if mut == "diag_excluded":
        allow = ki < qi
    elif mut == "past_diag":
        allow = ki <= qi + 1
    elif mut == "drop_tile":                       # key tile 0 (keys 0..63) skipped by the last 32-row query block
        allow = allow & ~((qi >= S - 32) & (ki < 64))
    out = torch.empty(B, S, H, hd)
    lse_o = torch.empty(B, H, S)
    dq = torch.empty(B, S, H, hd)
    dk = torch.empty(B, S, Hkv, hd)
    dv = torch.empty(B, S, Hkv, hd)
    for b in range(B):
        for hk in range(Hkv):
            hs = slice(hk * n_rep, (hk + 1) * n_rep)
            qq, kk, vv, g = q[b, :, hs].transpose(0, 1), k[b, :, hk], v[b, :, hk], do[b, :, hs].transpose(0, 1)
            s = torch.matmul(qq, kk.T) * scale
            s = s.masked_fill(~allow, float("-inf"))
            lse = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - lse[..., None])
            o = rt(torch.matmul(rt(p), vv))
            if mut == "lse":
                lse = lse + 2 ** -6
                p = torch.exp(s - lse[..., None])         # the backward recomputes P from the stored LSE
            Drow = (g * o).sum(-1, keepdim=True)
            ds = rt(p * (torch.matmul(g, vv.T) - Drow))
            heads = n_rep - 1 if mut == "kv_sum" else n_rep
            out[b, :, hs] = o.transpose(0, 1)
            lse_o[b, hs] = lse
            dq[b, :, hs] = rt(torch.matmul(ds, kk) * scale).transpose(0, 1)
            dk[b, :, hk] = rt(torch.matmul(ds[:heads].transpose(1, 2), qq[:heads]).sum(0) * scale)
            dv[b, :, hk] = rt(torch.matmul(rt(p[:heads]).transpose(1, 2), g[:heads]).sum(0))
    if mut == "swap_heads":                         # heads 0 and 1 (one KV group when n_rep > 1) trade places
        for t in (out, dq):
            t[:, :, [0, 1]] = t[:, :, [1, 0]]
        lse_o[:, [0, 1]] = lse_o[:, [1, 0]]
    if mut == "zero_last_dv":
        dv[:, S - 1] = 0
    return dict(out=out, lse=lse_o, dq=dq, dk=dk, dv=dv)


def compare(got, ref):
    """{tensor: None if within the bound, else the AssertionError message}."""
    res = {}
    for name, fn in (("out", lambda: ac.check(got["out"], ref["out"], ref["out_scale"], "out")),
                     ("lse", lambda: ac.check_lse(got["lse"], ref["lse"])),
                     ("dq", lambda: ac.check(got["dq"], ref["dq"], ref["dq_scale"], "dq")),
                     ("dk", lambda: ac.check(got["dk"], ref["dk"], ref["dk_scale"], "dk")),
                     ("dv", lambda: ac.check(got["dv"], ref["dv"], ref["dv_scale"], "dv"))):
        try:
            fn()
            res[name] = None
        except AssertionError as e:
            res[name] = str(e)
    return res


@pytest.mark.parametrize("n_rep", [1, 4])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S", [65, 300])
def test_bound_accepts_the_kernels_rounding(S, hd, causal, n_rep):
    q, k, v, do = inputs(2, S, 2 * n_rep, 2, hd, seed=S + hd + n_rep)
    ref = ac.attn_ref(q, k, v, causal, do)
    res = compare(emulate(q, k, v, do, causal), ref)
    assert all(m is None for m in res.values()), res
    worst = ac.check(emulate(q, k, v, do, causal)["out"], ref["out"], ref["out_scale"], "out")
    assert worst > 0.02, f"out: the emulated rounding uses only {worst:.3g} of the bound (too loose to mean anything)"


# (mutation, the tensor that must reject it, causal settings where it applies).  Not applied:
#  * diag_excluded / past_diag without the mask (there is no diagonal);
#  * kv_sum at n_rep = 1: there is no second query head to leave out (every case below runs n_rep = 4).
MUTATIONS = [("drop_tile", "out", (True, False)), ("diag_excluded", "out", (True,)), ("past_diag", "out", (True,)),
             ("swap_heads", "out", (True, False)), ("kv_sum", "dk", (True, False)), ("lse", "lse", (True, False)),
             ("scale", "lse", (True, False)), ("zero_last_dv", "dv", (True, False))]


@pytest.mark.parametrize("S,hd", [(65, 64), (65, 128), (300, 64), (300, 128)])
@pytest.mark.parametrize("mut,caught_by,causal", [(m, t, c) for m, t, cs in MUTATIONS for c in cs])
def test_bound_rejects_kernel_bug_classes(mut, caught_by, causal, S, hd):
    q, k, v, do = inputs(2, S, 8, 2, hd, seed=7 * S + hd)
    ref = ac.attn_ref(q, k, v, causal, do)
    res = compare(emulate(q, k, v, do, causal, mut), ref)
    assert res[caught_by] is not None, f"{mut} (causal={causal}, S={S}, hd={hd}) passes the {caught_by} check: {res}"


def test_check_reports_the_first_failing_element():
    want = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    got = want.clone()
    got[1, 2, 3, 4] = 1.0
    got[1, 2, 3, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"2/120 elements out of bound; first at \(b=1, row=2, h=3, col=3\)"):
        ac.check(got, want, torch.ones_like(want), "t")
    assert ac.check(want + 2 * ac.U * 0.5, want, torch.ones_like(want), "t") == pytest.approx(0.5, rel=1e-3)


def test_rope_back_inverts_the_rotation():
    B, S, nh, hd = 2, 9, 3, 16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, S, nh, hd, generator=g)
    fc = ref_cpu.precompute_freqs_cis(hd, S)
    xr, _ = ref_cpu.apply_rotary_emb(x, x[:, :, :1], fc)
    assert torch.allclose(ac.rope_back(xr.double()), x.double(), atol=1e-5)
