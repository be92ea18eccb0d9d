"""-m gpu: the extend prefill kernels (include/a3vlm_hip.h, "Extend prefill").  Every check is an equality, bit for bit:
(a) the plain form gives, row by row, what a3v_attention gives at B = 1, Sq = nq[b], Sk = sk[b], causal, on that row's slice;
(b) the shared form gives the plain form's result on caches into which positions [0, S_b) of row src_row[b] were copied, while the
    row's own copy of those positions holds NaN;
(c) src_row == NULL is the plain call; (d) an idle row leaves its out rows untouched;
and the span write equals a3v_rope_kvcache per row with nothing outside the spans written (caches pre-filled with a sentinel)."""
import pytest
import torch

from a3vlm_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
H, HKV, SMAX = 4, 2, 256
# (nq, sk) per row, launched together: one query (a3v_attention's Sq == 1 route); a span that ends inside the second key tile; two
# query tiles with keys across 64 and 128; the idle row
ROWS = [(1, 65), (37, 101), (130, 200), (0, 0)]
B = len(ROWS)
NQ = [r[0] for r in ROWS]
SK = [r[1] for r in ROWS]
QOFF = [0, 1, 38, 168, 168]
M = QOFF[-1]


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _strides(hd, ldq=None):
    ldq = H * hd if ldq is None else ldq
    return (ldq, ldq, hd, HKV * SMAX * hd, SMAX * hd, hd, HKV * hd * SMAX, hd * SMAX, SMAX, H * hd, H * hd, hd)


def _scratch(hd, dtype, sk_max):
    if dtype == BF and hd in (64, 128):
        return torch.full((ops.attention_extend_rows_scratch_floats(B, H, hd, sk_max),), float("nan"), dtype=torch.float32, device=DEV)
    return None


_CACHE = {}


def _inputs(hd, dtype):
    """q, k, vt with NaN behind every row's keys, and the per-row a3v_attention reference (computed once, never changed)"""
    key = (hd, dtype)
    if key not in _CACHE:
        q = gen(M, H * hd, seed=hd).to(dtype).to(DEV)
        k = gen(B, HKV, SMAX, hd, seed=1).to(dtype).to(DEV)
        vt = gen(B, HKV, hd, SMAX, seed=2).to(dtype).to(DEV)
        for b, n in enumerate(SK):                         # the cache tail may hold anything
            k[b, :, n:] = float("nan")
            vt[b, :, :, n:] = float("nan")
        _CACHE[key] = (q, k, vt, _reference(q, k, vt, hd, dtype))
    return _CACHE[key]


def _reference(q, k, vt, hd, dtype):
    want = torch.full((M, H * hd), 7.0, dtype=dtype, device=DEV)          # 7.0: the sentinel an idle row must leave
    for b, (n, s) in enumerate(ROWS):
        if n <= 0:
            continue
        sc = None
        if n == 1 and dtype == BF and hd in (64, 128):
            sc = torch.empty(ops.attention_scratch_floats(1, H, hd, s), dtype=torch.float32, device=DEV)
        ops.attention(q[QOFF[b]:QOFF[b + 1]], k[b:b + 1], vt[b:b + 1], want[QOFF[b]:QOFF[b + 1]], 1, n, s, H, HKV, hd, _strides(hd), True, sc)
    return want


def _effective(src, shared):
    out = []
    for b in range(B):
        own = not 0 <= src[b] < B or src[b] == b
        out.append(0 if own else max(min(shared[b], SK[b]), 0) & ~63)
    return out


FORMS = [(BF, 64), (BF, 128), (torch.float32, 64), (torch.float32, 128), (torch.float32, 16), (BF, 32)]
FORM_IDS = ["bf16-hd64", "bf16-hd128", "fp32-hd64", "fp32-hd128", "fp32-hd16-generic", "bf16-hd32-generic"]


@pytest.mark.parametrize("dtype,hd", FORMS, ids=FORM_IDS)
def test_plain_form_equals_attention_per_row(dtype, hd):
    """(a), (c), (d)"""
    q, k, vt, want = _inputs(hd, dtype)
    got = torch.full_like(want, 7.0)
    sc = _scratch(hd, dtype, 200)
    ops.attention_extend_rows(q, k, vt, got, i32(QOFF), i32(SK), 130, 200, B, H, HKV, hd, _strides(hd), sc)
    assert torch.isfinite(got.float()).all(), "a NaN: a position behind a row's keys was read"
    for b in range(B):
        assert torch.equal(got[QOFF[b]:QOFF[b + 1]], want[QOFF[b]:QOFF[b + 1]]), (b, ROWS[b])
    # the idle row in the MIDDLE of the packing: its out rows (here: rows that belong to nobody) keep the sentinel
    qoff2 = [0, 1, 38, 38, 168]
    sk2, got2 = [65, 101, 0, 200], torch.full_like(want, 7.0)
    k2, vt2 = k.clone(), vt.clone()
    k2[3], vt2[3] = k[2], vt[2]
    ops.attention_extend_rows(q, k2, vt2, got2, i32(qoff2), i32(sk2), 130, 200, B, H, HKV, hd, _strides(hd), sc)
    assert torch.equal(got2, want)
    # a row that claims queries but has no keys, and one with keys but no queries, write nothing
    got3 = torch.full_like(want, 7.0)
    ops.attention_extend_rows(q, k, vt, got3, i32([0, 1, 38, 168, 168]), i32([0, 101, 200, 50]), 130, 200, B, H, HKV, hd, _strides(hd), sc)
    assert torch.equal(got3[:1], torch.full_like(got3[:1], 7.0)) and torch.equal(got3[1:], want[1:])


# (src_row, shared) per row; the row's sk is ROWS'
SHARED = {
    "shared-0": [(2, 0), (2, 0), (1, 0), (2, 0)],
    "shared-64": [(2, 64), (2, 64), (1, 64), (2, 64)],
    "shared-100-acts-as-64": [(2, 100), (2, 100), (1, 100), (2, 100)],
    "shared-128": [(2, 128), (2, 128), (1, 128), (2, 128)],              # rows 0 / 1 / 2: clamped by their own 65 / 101 / 200 keys
    "shared-above-sk": [(2, 4096), (2, 4096), (0, 4096), (2, 4096)],
    "src-self-and-out-of-range": [(0, 64), (-1, 64), (9, 128), (3, 64)],
}
EFF = {"shared-0": [0, 0, 0, 0], "shared-64": [64, 64, 64, 0], "shared-100-acts-as-64": [64, 64, 64, 0], "shared-128": [64, 64, 128, 0],
       "shared-above-sk": [64, 64, 192, 0], "src-self-and-out-of-range": [0, 0, 0, 0]}


@pytest.mark.parametrize("case", list(SHARED))
@pytest.mark.parametrize("dtype,hd", FORMS[:3] + FORMS[4:5], ids=FORM_IDS[:3] + FORM_IDS[4:5])
def test_shared_form_equals_plain_on_copied_caches(dtype, hd, case):
    """(b): the source rows here hold DIFFERENT keys than the own rows, and a source row shorter than S_b is filled up first"""
    q, k0, vt0, _ = _inputs(hd, dtype)
    src, shared = (list(x) for x in zip(*SHARED[case]))
    eff = _effective(src, shared)
    assert eff == EFF[case]
    k, vt = k0.clone(), vt0.clone()
    for b, e in enumerate(eff):                            # the source row holds real keys wherever a sibling reads them
        if e > 0 and e > SK[src[b]]:
            k[src[b], :, :e] = gen(HKV, e, hd, seed=90 + b).to(dtype).to(DEV)
            vt[src[b], :, :, :e] = gen(HKV, hd, e, seed=95 + b).to(dtype).to(DEV)
    kc, vc, kp, vp = k.clone(), vt.clone(), k.clone(), vt.clone()
    for b, e in enumerate(eff):
        if e > 0:
            kc[b, :, :e] = k[src[b], :, :e]
            vc[b, :, :, :e] = vt[src[b], :, :, :e]
    for b, e in enumerate(eff):
        if e > 0 and not any(src[o] == b and eff[o] > 0 for o in range(B)):     # (a row that is itself a source keeps its keys)
            kp[b, :, :e] = float("nan")
            vp[b, :, :, :e] = float("nan")
    sc = _scratch(hd, dtype, 200)
    want = torch.full((M, H * hd), 7.0, dtype=dtype, device=DEV)
    got = want.clone()
    ops.attention_extend_rows(q, kc, vc, want, i32(QOFF), i32(SK), 130, 200, B, H, HKV, hd, _strides(hd), sc)
    ops.attention_extend_rows(q, kp, vp, got, i32(QOFF), i32(SK), 130, 200, B, H, HKV, hd, _strides(hd), sc, i32(src), i32(shared))
    assert torch.isfinite(want.float()).all() and torch.isfinite(got.float()).all(), "a NaN: a poisoned position was read"
    assert torch.equal(got, want), (case, eff)
    if any(eff):                                           # sharing changed something: the own rows' keys differ from the sources'
        plain = torch.full_like(want, 7.0)
        ops.attention_extend_rows(q, k, vt, plain, i32(QOFF), i32(SK), 130, 200, B, H, HKV, hd, _strides(hd), sc)
        assert not torch.equal(plain, want)
    # one array without the other is an error, nothing launched
    rc = lib.load().a3v_attention_extend_rows(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), got.data_ptr(), i32(QOFF).data_ptr(),
                                              i32(SK).data_ptr(), i32(src).data_ptr(), None, 130, 200, B, H, HKV, hd,
                                              ops._Strides(*_strides(hd)), ops._p(sc), ops.dt(q), torch.cuda.current_stream().cuda_stream)
    assert rc != 0


@pytest.mark.parametrize("dtype,hd", FORMS[:2] + FORMS[4:5], ids=FORM_IDS[:2] + FORM_IDS[4:5])
def test_clamps_read_nothing_out_of_bounds(dtype, hd):
    """nq above nq_max is read as nq_max, sk above sk_max as sk_max: the result is a3v_attention's on the clamped row"""
    q, k, vt, _ = _inputs(hd, dtype)
    nq_max, sk_max = 100, 150
    got = torch.full((M, H * hd), 7.0, dtype=dtype, device=DEV)
    ops.attention_extend_rows(q, k, vt, got, i32(QOFF), i32(SK), nq_max, sk_max, B, H, HKV, hd, _strides(hd), _scratch(hd, dtype, sk_max))
    want = torch.full_like(got, 7.0)
    for b, (n, s) in enumerate(ROWS):
        n, s = min(n, nq_max), min(s, sk_max)
        if n <= 0:
            continue
        sc = torch.empty(ops.attention_scratch_floats(1, H, hd, s), dtype=torch.float32, device=DEV) if n == 1 and dtype == BF else None
        ops.attention(q[QOFF[b]:QOFF[b] + n], k[b:b + 1], vt[b:b + 1], want[QOFF[b]:QOFF[b] + n], 1, n, s, H, HKV, hd, _strides(hd), True, sc)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [64, 128])
def test_span_write_equals_rope_kvcache_per_row(hd, dtype):
    ld = (H + 2 * HKV) * hd
    qkv = gen(M, ld, seed=3).to(dtype).to(DEV)
    cs = torch.stack([torch.cos(gen(SMAX, hd // 2, seed=4)), torch.sin(gen(SMAX, hd // 2, seed=4))], dim=-1).contiguous().to(DEV)
    sent = 7.0
    wk = torch.full((B, HKV, SMAX, hd), sent, dtype=dtype, device=DEV)
    wv = torch.full((B, HKV, hd, SMAX), sent, dtype=dtype, device=DEV)
    wq = torch.full((M, H * hd), sent, dtype=dtype, device=DEV)
    for b, (n, s) in enumerate(ROWS):
        if n > 0:
            ops.rope_kvcache(qkv[QOFF[b]:QOFF[b + 1]], wq[QOFF[b]:QOFF[b + 1]], wk[b:b + 1], wv[b:b + 1], cs, 1, n, H, HKV, hd, s - n, s - n)
    gk, gv, gq = torch.full_like(wk, sent), torch.full_like(wv, sent), torch.full_like(wq, sent)
    ops.rope_kvcache_extend(qkv, gq, gk, gv, cs, i32(QOFF), i32(SK), 130, B, H, HKV, hd)
    assert torch.equal(gq, wq) and torch.equal(gk, wk) and torch.equal(gv, wv)
    for b, (n, s) in enumerate(ROWS):                      # the reference itself left everything outside the spans alone
        assert float((wk[b, :, :s - n].float() - sent).abs().max() if s - n else 0) == 0
        assert float((wk[b, :, s:].float() - sent).abs().max()) == 0 and float((wv[b, :, :, s:].float() - sent).abs().max()) == 0
    # in place on the qkv buffer, as the model calls it; a span that does not fit (sk > Smax, or longer than its keys) writes nothing
    q2 = qkv.clone()
    gk2, gv2 = torch.full_like(wk, sent), torch.full_like(wv, sent)
    ops.rope_kvcache_extend(q2, q2, gk2, gv2, cs, i32(QOFF), i32([65, SMAX + 1, 100, 0]), 130, B, H, HKV, hd)
    assert torch.equal(q2[:1, :H * hd], wq[:1]) and torch.equal(q2[1:], qkv[1:]), "rows 1 (past the cache) and 2 (130 queries, 100 keys) idle"
    assert torch.equal(gk2[0], wk[0]) and torch.equal(gv2[0], wv[0])
    assert float((gk2[1:].float() - sent).abs().max()) == 0 and float((gv2[1:].float() - sent).abs().max()) == 0
