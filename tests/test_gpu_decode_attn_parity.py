"""The decode-attention family on the GPU against tests/decode_attn_ref.py: for every table case, every form the case runs through and
every input family the output equals the expectation bit for bit, partial slots included (exact inputs), or lies inside the derived
bound (bounded and stress inputs).  q, both caches, the scales and the sk / pos / nq / src_row / shared vectors are views at a 16-byte
offset into NaN-filled (0x7F-filled) buffers, the bf16 caches with padded strides; cache positions a correct kernel never reads hold
NaN (0x7F bytes, inf scales); the output is a view into a sentinel-filled buffer whose surroundings must come back untouched; the
scratch is sized by the project's own *_scratch_floats, NaN-filled, and followed by a sentinel tail; the counters are zero before and
after; a second call gives the same bits.  tests/test_decode_attn_ref_cpu.py shows that a correct fp32 split walk passes these checks
on the same inputs and that wrong ones do not.  Run with -s for the ratios."""
import pytest
import torch

import decode_attn_ref as R
from a3vlm_amd import lib as L
from a3vlm_amd import ops
from test_gpu_gemm_parity import embedded, embedded1d, surroundings_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
TAIL = 256
FORMS = {"uniform": ("fused", "wave", "twophase", "rows"), "rows": ("rows", "shared0"), "shared": ("shared",),
         "fp8kv": ("fused", "standalone"), "verify": ("verify",)}
try:                                               # the table is placed from the library's plan: host code, no GPU needed to collect
    CASES = R.cases_for(ops.attention_decode_plan)
except RuntimeError:                               # collected before anything built the library
    import __graft_entry__ as _g
    _g.build()
    CASES = R.cases_for(ops.attention_decode_plan)
PARAMS = [(c.id, fam, form) for c in CASES for fam in R.FAMILIES for form in FORMS[c.kind]]
BY_ID = {c.id: c for c in CASES}
RATIOS = {}
_ops_cache = {}


def embed_cache(t):
    """t [B, Hkv, X, Y] -> (flat NaN-filled bf16 buffer, view into it at a 16-byte offset with padded row, head and batch strides)"""
    B, Hk, X, Y = t.shape
    ld = Y + 8
    sh = X * ld + 16
    sb = Hk * sh + 24
    flat = torch.full((8 + B * sb + 8,), NAN, dtype=BF, device=DEV)
    view = flat.as_strided((B, Hk, X, Y), (sb, sh, ld, 1), 8)
    view.copy_(t.to(BF).to(DEV))
    return flat, view


def _i32(x):
    return embedded1d(torch.tensor(list(x), dtype=torch.int32), 0x7F7F7F7F)


def operands(c, fam):
    """device views of the case's inputs, shared by the forms of one (case, family) -> dict; "flats": every input buffer"""
    key = (c.id, fam)
    if key in _ops_cache:
        return _ops_cache[key]
    _ops_cache.clear()
    inp = R.reference(c, fam)["inp"]
    d, flats = {}, []

    def keep(pair):
        flats.append(pair[0])
        return pair[1]
    d["q"] = keep(embedded(inp["q"].reshape(c.R, c.H * c.hd).to(BF), NAN))
    if c.kind == "fp8kv":
        for name in ("kq", "vtq"):
            d[name] = keep(embedded1d(inp[name].reshape(-1), R.NAN_BYTE)).view(inp[name].shape)
        for name in ("ks", "vs"):
            d[name] = keep(embedded1d(inp[name].reshape(-1), NAN)).view(inp[name].shape)
    else:
        d["k"] = keep(embed_cache(inp["k"]))
        d["vt"] = keep(embed_cache(inp["vt"]))
        k, v = d["k"], d["vt"]
        d["strides"] = lambda q, o: (q.stride(0), q.stride(0), c.hd, k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                                     o.stride(0), o.stride(0), c.hd)
    if c.kind == "verify":
        d["pos"], d["nq"] = keep(_i32(c.pos)), keep(_i32(c.nq))
    else:
        d["sk"] = keep(_i32(c.sk))
    if c.kind == "shared":
        d["src"], d["shared"] = keep(_i32(c.src)), keep(_i32(c.shared))
    if c.kind == "rows":                           # shared = 0 towards some other row: exactly the plain rows
        d["src"], d["shared"] = keep(_i32([(b + 1) % c.B for b in range(c.B)])), keep(_i32([0] * c.B))
    d["flats"] = flats
    d["before"] = [f.clone() for f in flats]
    _ops_cache[key] = d
    return d


def bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def call(c, form, d):
    """one call on a fresh output, scratch and counters -> (out [R, H, hd] bf16 on the CPU, partial slots or None, checks)"""
    R_, H, hd, B = c.R, c.H, c.hd, c.B
    oflat, out = embedded(torch.zeros(R_, H * hd, dtype=BF), R.SENT)
    out.fill_(R.SENT)
    if c.kind == "verify":
        n = ops.attention_verify_rows_scratch_floats(B, c.Q, H, hd, c.sk_max)
        nctr = 2 * B * H
    else:
        n = ops.attention_scratch_floats(B, H, hd, c.sk_max)
        nctr = B * H
    scratch = torch.full((n + TAIL,), NAN, dtype=torch.float32, device=DEV)
    scratch[n:] = R.SENT
    ctr = torch.zeros(nctr + 16, dtype=torch.int32, device=DEV)
    ns = c.nsplit2 if form == "twophase" else c.nsplit
    if c.kind == "fp8kv":
        ops.attention_decode_fp8kv(d["q"], d["kq"], d["vtq"], d["ks"], d["vs"], out, B, c.sk_max, H, c.Hkv, hd, scratch[:n],
                                   ctr if form == "fused" else None)
    else:
        st = d["strides"](d["q"], out)
        k, vt = d["k"], d["vt"]
        if form == "fused":
            ops.attention_decode_fused(d["q"], k, vt, out, B, c.sk_max, H, c.Hkv, hd, st, scratch[:n], ctr)
        elif form == "wave":
            with L.env(A3V_ATTN_DECODE_WAVE_STANDALONE="1"):
                ops.attention(d["q"], k, vt, out, B, 1, c.sk_max, H, c.Hkv, hd, st, False, scratch[:n])
        elif form == "twophase":
            ops.attention(d["q"], k, vt, out, B, 1, c.sk_max, H, c.Hkv, hd, st, False, scratch[:n])
        elif form == "rows":
            ops.attention_decode_rows(d["q"], k, vt, out, d["sk"], c.sk_max, B, H, c.Hkv, hd, st, scratch[:n], ctr)
        elif form in ("shared", "shared0"):
            ops.attention_decode_rows_shared(d["q"], k, vt, out, d["sk"], d["src"], d["shared"], c.sk_max, B, H, c.Hkv, hd, st, scratch[:n], ctr)
        elif form == "verify":
            ops.attention_verify_rows(d["q"], k, vt, out, d["pos"], d["nq"], c.sk_max, B, c.Q, H, c.Hkv, hd, st, scratch[:n], ctr)
        else:
            raise AssertionError(form)
    torch.cuda.synchronize()
    checks = [("output surroundings", surroundings_intact(oflat, out)),
              ("scratch tail", bool((scratch[n:] == R.SENT).all())),
              ("counters zero again", int(ctr.abs().sum()) == 0),
              ("inputs untouched", all(torch.equal(bits(f), bits(b)) for f, b in zip(d["flats"], d["before"])))]
    part = None
    if ns > 1:
        assert R_ * H * ns * (hd + 2) <= n
        part = scratch[:R_ * H * ns * (hd + 2)].view(R_, H, ns, hd + 2).cpu()
    return out.cpu().view(R_, H, hd), part, checks


@pytest.mark.parametrize("cid,fam,form", PARAMS)
def test_decode_attention(cid, fam, form):
    c = BY_ID[cid]
    ref = R.reference(c, fam, "twophase" if form == "twophase" else None)
    d = operands(c, fam)
    out, part, checks = call(c, form, d)
    assert all(ok for _, ok in checks), [name for name, ok in checks if not ok]
    ok, ratio, why = R.judge(c, fam, ref, out, part)
    if fam != "exact":
        key = (c.kind, form, fam)
        if ratio > RATIOS.get(key, (0.0, ""))[0]:
            RATIOS[key] = (ratio, c.id)
        print(f"{cid} {form} {fam} ({c.pattern if fam == 'stress' else '-'}; {c.nsplit2 if form == 'twophase' else c.nsplit} ranges): err / bound {ratio:.3f}")
    assert ok, why
    again, part2, _ = call(c, form, d)
    assert torch.equal(bits(again), bits(out)), "a second call on the same buffers gives other bits"
    # identities that hold bit for bit
    other = {("uniform", "wave"): "fused", ("uniform", "rows"): "fused", ("rows", "shared0"): "rows", ("fp8kv", "standalone"): "fused"}.get((c.kind, form))
    if other:
        base, bpart, _ = call(c, other, d)
        assert torch.equal(bits(base), bits(out)), f"{form} != {other}"
        if part is not None and bpart is not None:
            w = R.partial_rows_written(c)
            assert torch.equal(bits(part[w]), bits(bpart[w])), f"partial slots: {form} != {other}"
    if c.kind == "verify" and c.Q == 1:
        # The verify kernel walks 32-key tiles, the rows kernel 64-key tiles: their sums associate differently, so the outputs are the
        # same bits only where every sum is exact.  Asserted on the exact family; counted on the others.
        oflat, o2 = embedded(torch.zeros(c.R, c.H * c.hd, dtype=BF), R.SENT)
        n = ops.attention_scratch_floats(c.B, c.H, c.hd, c.sk_max)
        sk = _i32(c.keys())[1]
        ops.attention_decode_rows(d["q"], d["k"], d["vt"], o2, sk, c.sk_max, c.B, c.H, c.Hkv, c.hd, d["strides"](d["q"], o2),
                                  torch.full((n,), NAN, dtype=torch.float32, device=DEV), torch.zeros(c.B * c.H, dtype=torch.int32, device=DEV))
        o2 = o2.cpu().view(c.R, c.H, c.hd)
        if fam == "exact":
            assert torch.equal(bits(o2), bits(out)), "verify at Q = 1 != rows"
        else:
            print(f"{cid} {fam}: verify at Q = 1 against rows: {int((bits(o2) != bits(out)).sum())} of {out.numel()} elements differ (32- against 64-key tiles)")


def test_zz_largest_ratios():
    """printed last: the largest err / bound per (entry, form, family) of this run"""
    for key in sorted(RATIOS):
        print(f"largest err / bound, {key[0]:8s} {key[1]:10s} {key[2]:8s}: {RATIOS[key][0]:.3f}  ({RATIOS[key][1]})")
    print(f"{len(PARAMS)} parametrised cases over {len(CASES)} table cases")
