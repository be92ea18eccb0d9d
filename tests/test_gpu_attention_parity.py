"""-m gpu: the bf16 prefill attention kernels (a3v_attn.hip forward, a3v_attn_bwd.hip backward, plain and packed) element by element
against the float64 oracle of oracle/attn_check.py, at the layouts production runs:

  1. the tile-rank-major block order of causal launches forced to G = 1 .. 16 heads per group (outputs bit-identical to G = 1);
  2. the library's default dispatch at the benchmark's shapes (7B, 13B, recipe length);
  3. ragged lengths around the 32-row / 64-key / 128-row tile edges, and causal Sq < Sk;
  4. production buffers: K / V^T pad rows and the qkv buffer around the backward's v poisoned with NaN or +-inf, every output
     inside a larger sentinel-filled buffer that must stay untouched outside the output's view;
  5. the packed backward (dq | dk | dv rotated back into the fused-qkv gradient) with a wide `out` and a wide `dqkv`.

Every case prints the largest err / bound of each tensor (run with -s to see them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from a3vlm_amd import lib, ops  # noqa: E402
from a3vlm_amd.model.LLM.llama_ens5 import precompute_cos_sin  # noqa: E402
from oracle import attn_check as ac  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SENT = -7777.0          # sentinel around every output view
WORST = {}              # family -> largest err / bound over its cases (printed at the end of the module)


def pad64(n):
    return (n + 63) // 64 * 64


def fwd_group(B, H, Sq, Sk, hd, causal, forced=0):
    """Mirror of the forward's block-order rule (a3v_attn.hip, attention_impl, the `p.head_group` block before the launch):
    causal, a 1-D grid of ceil(Sq / 128) * B * H blocks divisible by 8 and B * H divisible by 8; the largest power of two
    <= 16 whose K + V^T (G * Sk * hd * 4 bytes) fit 9 MiB, or A3V_ATTN_HEAD_GROUP; halved until it divides B * H / 8."""
    if not causal or (((Sq + 127) // 128) * B * H) % 8 or (B * H) % 8:
        return 1
    want = 16
    while want > 1 and want * Sk * hd * 4 > (9 << 20):
        want >>= 1
    G = max(forced if forced > 0 else want, 1)
    while G > 1 and ((B * H) // 8) % G:
        G >>= 1
    return G


def bwd_groups(B, S, H, Hkv, hd, causal, forced=0):
    """Mirror of the backward's rule (a3v_attn_bwd.hip, attention_bwd_mfma_impl, `group_of`): as the forward's, with a 4.5-MiB
    budget (Q + dO + K + V per head), for the dQ kernel over B * H heads and the dK / dV kernel over B * Hkv heads."""
    nqt = (S + 127) // 128

    def group_of(heads):
        if not causal or (nqt * heads) % 8 or heads % 8:
            return 1
        want = 16
        while want > 1 and want * S * hd * 4 > (9 << 19):
            want >>= 1
        G = max(forced if forced > 0 else want, 1)
        while G > 1 and (heads // 8) % G:
            G >>= 1
        return G
    return group_of(B * H), group_of(B * Hkv)


def inputs(B, Sq, Sk, H, Hkv, hd, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF)     # noqa: E731
    return mk(B, Sq, H, hd), mk(B, Sk, Hkv, hd), mk(B, Sk, Hkv, hd), mk(B, Sq, H, hd)


class Guarded:
    """A sentinel-filled device buffer and a view of it; ``untouched`` asserts that nothing outside the view changed."""

    def __init__(self, shape, dtype, region):
        self.buf = torch.full(shape, SENT, dtype=dtype, device=DEV)
        self.region = region
        self.view = self.buf[region]

    def untouched(self, what):
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        m[self.region] = False
        it = torch.int16 if self.buf.dtype == BF else torch.int32
        sent = torch.full((1,), SENT, dtype=self.buf.dtype, device=DEV).view(it)
        changed = int((self.buf.view(it)[m] != sent).sum())
        assert changed == 0, f"{what}: {changed} elements outside the output's view were written"


def run(q, k, v, do, causal, pad=float("nan"), bwd=True, packed=False, ld_extra=64, qkv_extra=0):
    """Forward (a3v_attention and a3v_attention_lse) and, with ``bwd``, the MFMA backward (plain or packed) of bf16 q [B,Sq,H,hd],
    k / v [B,Sk,Hkv,hd], do [B,Sq,H,hd] as production lays them out.  Returns the device results in the oracle's layouts."""
    B, Sq, H, hd = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    Smax = pad64(Sk)
    kc = torch.full((B, Hkv, Smax, hd), pad, dtype=BF, device=DEV)          # K cache, pad rows Sk..Smax poisoned
    vt = torch.full((B, Hkv, hd, Smax), pad, dtype=BF, device=DEV)          # V^T cache, pad columns poisoned
    kc[:, :, :Sk] = k.permute(0, 2, 1, 3).to(DEV)
    vt[:, :, :, :Sk] = v.permute(0, 2, 3, 1).to(DEV)
    qd = q.to(DEV).contiguous()
    ldo = H * hd + ld_extra
    res = {}
    for name in ("out", "out_lse"):
        og = Guarded((B * Sq + 8, ldo), BF, (slice(0, B * Sq), slice(0, H * hd)))
        st = (Sq * H * hd, H * hd, hd, Hkv * Smax * hd, Smax * hd, hd, Hkv * hd * Smax, hd * Smax, Smax, Sq * ldo, ldo, hd)
        if name == "out":
            ops.attention(qd, kc, vt, og.view, B, Sq, Sk, H, Hkv, hd, st, causal)
        else:
            lg = Guarded((B * H * Sq + 128,), torch.float32, slice(64, 64 + B * H * Sq))
            ops.attention_lse(qd, kc, vt, og.view, lg.view, B, Sq, Sk, H, Hkv, hd, st, causal)
            torch.cuda.synchronize()
            lg.untouched("lse")
            res["lse"] = lg.view.view(B, H, Sq).clone()
            o2d = og.view
        torch.cuda.synchronize()
        og.untouched(name)
        res[name] = og.view.view(B, Sq, H, hd).clone()
    if not bwd:
        return res
    assert Sq == Sk
    S = Sq
    N = (H + 2 * Hkv) * hd
    # v is the column slice of a qkv-shaped buffer (train.py: vrows = qkv[:, (H + Hkv) * hd:]); everything else in it is poison
    vbuf = torch.full((B * S + 64, N), pad, dtype=BF, device=DEV)
    vbuf[:B * S, (H + Hkv) * hd:] = v.reshape(B * S, Hkv * hd).to(DEV)
    vrows = vbuf[:B * S, (H + Hkv) * hd:]
    ldv = vbuf.stride(0)
    dod = do.to(DEV).contiguous()
    D = torch.empty(B, S, H, dtype=torch.float32, device=DEV)
    if packed:
        cs = precompute_cos_sin(hd, 2 * pad64(S), 10000.0, None).to(DEV)
        g = Guarded((B * S + 8, N + qkv_extra), BF, (slice(0, B * S), slice(0, N)))
        ops.attention_bwd_packed(qd, kc, Hkv * Smax * hd, Smax * hd, vrows, S * ldv, ldv, hd, o2d, dod, res["lse"], D, g.view, cs,
                                 B, S, H, Hkv, hd, causal, 0)
        torch.cuda.synchronize()
        g.untouched("dqkv")
        d = g.view.clone()
        res["dq"] = d[:, :H * hd].reshape(B, S, H, hd)
        res["dk"] = d[:, H * hd:(H + Hkv) * hd].reshape(B, S, Hkv, hd)
        res["dv"] = d[:, (H + Hkv) * hd:].reshape(B, S, Hkv, hd)
        return res
    ws = torch.empty(ops.attention_bwd_workspace_bytes(B, S, H, Hkv, hd), dtype=torch.uint8, device=DEV)
    gq = Guarded((B * S * H * hd + 512,), BF, slice(256, 256 + B * S * H * hd))
    gk = Guarded((B * Hkv * S * hd + 512,), BF, slice(256, 256 + B * Hkv * S * hd))
    gv = Guarded((B * Hkv * S * hd + 512,), BF, slice(256, 256 + B * Hkv * S * hd))
    dq, dk, dv = gq.view.view(B, S, H, hd), gk.view.view(B, Hkv, S, hd), gv.view.view(B, Hkv, S, hd)
    o_c = o2d.contiguous()                                   # (train.py: a K_ext `att` inside a wider buffer is made contiguous)
    ops.attention_bwd(qd, kc, Hkv * Smax * hd, Smax * hd, vrows, S * ldv, ldv, hd, o_c, dod, res["lse"], D, dq, dk, dv,
                      B, S, H, Hkv, hd, causal, workspace=ws)
    torch.cuda.synchronize()
    for gg, name in ((gq, "dq"), (gk, "dk"), (gv, "dv")):
        gg.untouched(name)
    res["dq"] = dq.clone()
    res["dk"] = dk.permute(0, 2, 1, 3).clone()
    res["dv"] = dv.permute(0, 2, 1, 3).clone()
    return res


def compare(got, q, k, v, do, causal, packed=False):
    """Every tensor of ``got``, every head, against attn_ref, one batch row at a time (bounded host memory).  The packed
    backward's dq / dk are compared with the oracle's rotated back (ac.rope_back).  Returns {tensor: largest err / bound}."""
    worst = {}
    for b in range(q.shape[0]):
        sel = lambda t: t[b:b + 1]                  # noqa: E731
        ref = ac.attn_ref(sel(q), sel(k), sel(v), causal, None if "dq" not in got else sel(do))
        tag = f"[b={b}]"
        r = {"out": ac.check(sel(got["out"]), ref["out"], ref["out_scale"], "out" + tag),
             "out_lse": ac.check(sel(got["out_lse"]), ref["out"], ref["out_scale"], "attention_lse out" + tag),
             "lse": ac.check_lse(sel(got["lse"]), ref["lse"], "lse" + tag)}
        if "dq" in got:
            wq, sq, wk, sk = ref["dq"], ref["dq_scale"], ref["dk"], ref["dk_scale"]
            if packed:
                wq, sq = ac.rope_back(wq, sq)
                wk, sk = ac.rope_back(wk, sk)
            r["dq"] = ac.check(sel(got["dq"]), wq, sq, "dq" + tag)
            r["dk"] = ac.check(sel(got["dk"]), wk, sk, "dk" + tag)
            r["dv"] = ac.check(sel(got["dv"]), ref["dv"], ref["dv_scale"], "dv" + tag)
        for n, x in r.items():
            worst[n] = max(worst.get(n, 0.0), x)
    return worst


def report(family, case, worst):
    print(f"\n[attn parity] {family} {case}: " + " ".join(f"{n}={x:.3f}" for n, x in worst.items()))
    fam = WORST.setdefault(family, {})
    for n, x in worst.items():
        fam[n] = max(fam.get(n, 0.0), x)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for fam, w in WORST.items():
        print(f"\n[attn parity] largest err/bound, {fam}: " + " ".join(f"{n}={x:.3f}" for n, x in w.items()))


# ------------------------------------------------------------------ 1. grouped block order, forced
@pytest.mark.parametrize("B,S,H,Hkv,hd", [(4, 300, 32, 32, 128), (4, 1091, 32, 32, 128), (4, 300, 32, 8, 128)])
def test_grouped_block_order_matches_oracle_and_head_major_order(B, S, H, Hkv, hd):
    q, k, v, do = inputs(B, S, S, H, Hkv, hd, seed=S + Hkv)
    base = None
    for G in (1, 2, 4, 8, 16):
        assert fwd_group(B, H, S, S, hd, True, G) == G
        gq, gkv = bwd_groups(B, S, H, Hkv, hd, True, G)
        assert gq == G and gkv == (G if Hkv == H else min(G, B * Hkv // 8))
        with lib.env(A3V_ATTN_HEAD_GROUP=G):
            got = run(q, k, v, do, True)
        report("1 grouped order", f"B={B} S={S} H={H} Hkv={Hkv} G={G} (dK/dV G={gkv})", compare(got, q, k, v, do, True))
        if base is None:
            base = got
            continue
        for n in base:
            assert torch.equal(got[n], base[n]), f"{n}: G={G} differs from the head-major order (G=1)"


# ------------------------------------------------------------------ 2. default dispatch at the benchmark's shapes
@pytest.mark.parametrize("name,B,S,H", [("7B", 8, 1091, 32), ("13B", 8, 1091, 40), ("recipe", 4, 2048, 32)])
def test_default_dispatch_at_benchmark_shapes(name, B, S, H):
    hd = 128
    q, k, v, do = inputs(B, S, S, H, H, hd, seed=len(name) * 1000 + S)
    G = fwd_group(B, H, S, S, hd, True)
    assert G == {"7B": 16, "13B": 8, "recipe": 8}[name]
    assert bwd_groups(B, S, H, H, hd, True) == {"7B": (8, 8), "13B": (8, 8), "recipe": (4, 4)}[name]
    got = run(q, k, v, do, True, packed=True, ld_extra=0)
    report("2 default dispatch", f"{name} B={B} S={S} H={H} G={G}", compare(got, q, k, v, do, True, packed=True))


# ------------------------------------------------------------------ 3. ragged edges
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S", [2, 31, 32, 63, 64, 65, 127, 128, 129, 255, 257, 1091])
def test_ragged_lengths_fwd_bwd(S, hd, causal, Hkv):
    q, k, v, do = inputs(2, S, S, 2, Hkv, hd, seed=S * 4 + hd + Hkv)
    got = run(q, k, v, do, causal)
    report("3 ragged", f"S={S} hd={hd} causal={causal} Hkv={Hkv}", compare(got, q, k, v, do, causal))


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("Sq", [65, 300])
@pytest.mark.parametrize("extra", [1, 63, 64, 65, 128])
def test_causal_forward_with_fewer_queries_than_keys(extra, Sq, hd):
    Sk = Sq + extra
    q, k, v, _ = inputs(2, Sq, Sk, 4, 2, hd, seed=Sq + extra + hd)
    got = run(q, k, v, None, True, bwd=False)
    report("3 ragged", f"Sq={Sq} Sk={Sk} hd={hd} causal", compare(got, q, k, v, None, True))


# ------------------------------------------------------------------ 4. production buffers and poison
@pytest.mark.parametrize("pad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("B,S,H,Hkv,hd,causal", [(2, 300, 4, 2, 128, True), (2, 129, 2, 2, 64, False), (1, 77, 4, 1, 128, False),
                                                 (2, 65, 4, 4, 64, True)])
def test_poisoned_pads_and_guarded_outputs(B, S, H, Hkv, hd, causal, pad):
    q, k, v, do = inputs(B, S, S, H, Hkv, hd, seed=S + hd)
    got = run(q, k, v, do, causal, pad=pad)
    report("4 poison", f"pad={pad} B={B} S={S} H={H} Hkv={Hkv} hd={hd} causal={causal}", compare(got, q, k, v, do, causal))


# ------------------------------------------------------------------ 5. packed backward against the oracle
@pytest.mark.parametrize("ld_extra,qkv_extra", [(0, 0), (64, 0), (0, 64), (64, 128)])
@pytest.mark.parametrize("B,S,H,Hkv,hd", [(2, 300, 4, 2, 128), (1, 77, 4, 2, 64), (2, 1091, 4, 4, 128), (2, 129, 8, 2, 64)])
def test_packed_backward_matches_oracle(B, S, H, Hkv, hd, ld_extra, qkv_extra):
    q, k, v, do = inputs(B, S, S, H, Hkv, hd, seed=S + H + hd)
    got = run(q, k, v, do, True, packed=True, ld_extra=ld_extra, qkv_extra=qkv_extra)
    report("5 packed", f"B={B} S={S} H={H} Hkv={Hkv} hd={hd} ld_out=H*hd+{ld_extra} ld_qkv=N+{qkv_extra}",
           compare(got, q, k, v, do, True, packed=True))
