"""-m gpu: the forward row kernels of a3v_rowops.hip (norms, RoPE + KV-cache write, V^T pack, embedding / ViT assembly, im2col,
view split, argmax, cross entropy, generation step) in every dtype combination their entry points dispatch, element by element
against the fp64 references of tests/rowops_fwd_ref.py.

Every bound is rowops_ref.within with the relative term derived in rowops_fwd_ref's docstring (shown on the CPU to hold for a
correct fp32 implementation on these very inputs by tests/test_rowops_fwd_ref_cpu.py), or bit equality where the specified result
is a copy or one correctly rounded operation.  Every output is a view into a wider buffer pre-filled with a sentinel that must
come back untouched outside the view; every input that may be strided is.  Each test prints its worst error-to-bound ratio."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_fwd_ref as R  # noqa: E402
from a3vlm_amd import ops  # noqa: E402
from a3vlm_amd.model.LLM.llama_ens5 import precompute_cos_sin  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENT = R.SENT


def guarded(t, pad, extra_rows=2):
    """t on the device as the top-left view of a sentinel-filled buffer with ``pad`` more columns and ``extra_rows`` more rows"""
    r, c = t.shape
    wide = torch.full((r + extra_rows, c + pad), SENT, dtype=t.dtype, device=DEV)
    wide[:r, :c] = t.to(DEV)
    return wide, wide[:r, :c]


def intact(wide, view):
    r, c = view.shape
    return bool((wide[:r, c:] == SENT).all()) and bool((wide[r:] == SENT).all())


def strided(t, pad):
    return guarded(t, pad, extra_rows=0)[1]


def flat_guarded(shape, dtype, pad=256):
    """a contiguous sentinel-filled tensor of ``shape`` followed by ``pad`` sentinel elements -> (flat buffer, the tensor)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + pad,), SENT, dtype=dtype, device=DEV)
    return flat, flat[:n].view(*shape)


def tail_intact(flat, t):
    return bool((flat[t.numel():] == SENT).all())


def last_rows(t, S=3):
    """t [rows, dim] on the device as ``h.view(rows, S, dim)[:, -1]`` of a buffer S times as long: row stride S * dim"""
    rows, dim = t.shape
    h = torch.full((rows * S, dim), SENT, dtype=t.dtype, device=DEV)
    v = h.view(rows, S, dim)[:, -1]
    v.copy_(t)
    return v


# ------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("dim", R.RMS_DIMS)
@pytest.mark.parametrize("key", sorted(R.RMS_KEYS))
def test_rmsnorm(key, dim):
    """every dtype key at every dim (8: one lane; 2056: slot 1 live for thread 0 only; 8192: the cap), 1 / 3 / 37 rows with a zero
    row and rows scaled by 2^10 and 2^-10; x rows strided, ldy = dim + 8; in place where the dtypes allow"""
    xd, wd, yd = R.RMS_KEYS[key]
    worst = 0.0
    for rows in R.RMS_ROWS:
        d = R.rmsnorm_inputs(rows, dim, xd, wd)
        ref, mag = R.rmsnorm_ref(d["x"], d["w"])
        w = d["w"].to(DEV)
        y_wide, y = guarded(torch.zeros(rows, dim, dtype=yd), 8)
        ops.rmsnorm(last_rows(d["x"]), w, y, R.RMS_EPS)
        r = R.within(y, ref, mag, yd, rel=R.rmsnorm_rel(xd, yd))
        assert intact(y_wide, y), (rows, "sentinel")
        if rows > 1:
            assert bool((y[1] == 0).all())
        if xd == BF:                        # the rounding ORDER (x r to bf16, then the product): bit equality where fp32 cannot move it
            want, decided = R.rmsnorm_exact(d["x"], d["w"], yd)
            assert torch.equal(y.cpu()[decided], want[decided]), (rows, "rounding order")
        if xd == yd:
            x_wide, x = guarded(d["x"], 8)
            ops.rmsnorm(x, w, x, R.RMS_EPS)
            assert torch.equal(x, y) and intact(x_wide, x), (rows, "in place")
        worst = max(worst, r)
    print(f"rmsnorm key {key} dim {dim}: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dim", R.RMS_BAD_DIMS)
def test_rmsnorm_refuses(dim):
    d = R.rmsnorm_inputs(3, dim, BF, BF)
    pad = 8 if dim % 8 == 0 else 4                     # both row strides are multiples of 8: it is the dim that is refused
    x, w = strided(d["x"], pad), d["w"].to(DEV)
    y_wide, y = guarded(torch.zeros(3, dim, dtype=BF), pad)
    before = y_wide.clone()
    with pytest.raises(RuntimeError):
        ops.rmsnorm(x, w, y, R.RMS_EPS)
    with pytest.raises(RuntimeError):
        ops.rmsnorm(x, w, y, R.RMS_EPS, row_idx=torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(y_wide, before)


@pytest.mark.parametrize("wd", [BF, F32])
@pytest.mark.parametrize("n_src,dim,idx", R.RMS_IDX_CASES)
def test_rmsnorm_row_idx(n_src, dim, idx, wd):
    """repeated and descending indices: bit-equal to gather_rows followed by rmsnorm, and within the bound of fp64"""
    d = R.rmsnorm_inputs(n_src, dim, BF, wd)
    x, w = strided(d["x"], 8), d["w"].to(DEV)
    ridx = torch.tensor(idx, dtype=torch.int32, device=DEV)
    y_wide, y = guarded(torch.zeros(len(idx), dim, dtype=BF), 8)
    ops.rmsnorm(x, w, y, R.RMS_EPS, row_idx=ridx)
    gathered = torch.empty(len(idx), dim, dtype=BF, device=DEV)
    ops.gather_rows(x, ridx, gathered)
    two_step = torch.empty(len(idx), dim, dtype=BF, device=DEV)
    ops.rmsnorm(gathered, w, two_step, R.RMS_EPS)
    assert torch.equal(y, two_step) and intact(y_wide, y)
    ref, mag = R.rmsnorm_ref(d["x"][idx], d["w"])
    r = R.within(y, ref, mag, BF, rel=R.rmsnorm_rel(BF, BF))
    print(f"rmsnorm row_idx ({n_src}, {dim}) w {wd}: {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dim", R.LN_DIMS)
@pytest.mark.parametrize("key", sorted(R.LN_KEYS))
def test_layernorm(key, dim):
    """rows centred and 8 / 64 standard deviations off zero; rows= smaller than x.shape[0]; through row_map into twice the rows
    (the unmapped rows stay); in place where the dtypes allow"""
    xd, pd, yd = R.LN_KEYS[key]
    rows = R.LN_ROWS
    worst = 0.0
    for off in R.LN_OFFSETS:
        d = R.layernorm_inputs(rows, dim, off, xd, pd)
        ref, mag = R.layernorm_ref(d["x"][:rows], d["w"], d["b"])
        w, b = d["w"].to(DEV), d["b"].to(DEV)
        x = strided(d["x"], 8)
        y_wide, y = guarded(torch.zeros(rows + 2, dim, dtype=yd), 8)
        y[rows:] = SENT
        ops.layernorm(x, w, b, y, R.LN_EPS, rows=rows)
        r1 = R.within(y[:rows], ref, mag, yd)
        assert intact(y_wide, y[:rows]), (off, "rows=")
        big_wide, big = guarded(torch.full((2 * rows, dim), SENT, dtype=yd), 8)
        ops.layernorm(x, w, b, big, R.LN_EPS, row_map=d["row_map"].to(DEV), rows=rows)
        mapped = d["row_map"].long()
        assert torch.equal(big[mapped.to(DEV)], y[:rows]), (off, "row_map")
        untouched = torch.ones(2 * rows, dtype=torch.bool)
        untouched[mapped] = False
        assert bool((big[untouched.to(DEV)] == SENT).all()) and intact(big_wide, big), (off, "unmapped rows")
        if xd == yd:
            x_wide, xin = guarded(d["x"], 8)
            ops.layernorm(xin, w, b, xin, R.LN_EPS, rows=rows)
            assert torch.equal(xin[:rows], y[:rows]) and torch.equal(xin[rows:].cpu(), d["x"][rows:]) and intact(x_wide, xin), (off, "in place")
        worst = max(worst, r1)
    print(f"layernorm key {key} dim {dim}: {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ RoPE + KV-cache write
@functools.lru_cache(maxsize=None)
def cos_sin_table(hd):
    return precompute_cos_sin(hd, R.ROPE_TABLE, 10000.0, None)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("hd", R.ROPE_HD)
@pytest.mark.parametrize("S", R.ROPE_S)
def test_rope_kvcache(S, hd, dtype):
    """both kernels (S <= 4 / the 64-token tile), start_pos != rope_pos0, Smax 256 and 100 (the scalar V^T path), q in place and into
    a separate buffer with its own row stride, caches of B + 1 batch rows"""
    B, H, Hkv = R.ROPE_B, R.ROPE_H, R.ROPE_HKV
    cs = cos_sin_table(hd)
    cs_d = cs.to(DEV)
    qkv = R.rope_inputs(S, hd, dtype)
    nq, nqk = H * hd, (H + Hkv) * hd
    worst = 0.0
    for case, (start, rp, Smax) in enumerate(R.rope_cases(S)):
        ref, mag, v = R.rope_ref(qkv, cs, S, hd, rp)
        q_ref, q_mag = ref[:, :, :H].reshape(B * S, nq), mag[:, :, :H].reshape(B * S, nq)
        kc = torch.full((B + 1, Hkv, Smax, hd), SENT, dtype=dtype, device=DEV)
        vc = torch.full((B + 1, Hkv, hd, Smax), SENT, dtype=dtype, device=DEV)
        src_wide, src = guarded(qkv, 8)
        if case % 2 == 0:                   # in place
            ops.rope_kvcache(src, src, kc, vc, cs_d, B, S, H, Hkv, hd, start, rp)
            rq = R.within(src[:, :nq], q_ref, q_mag, dtype)
            assert torch.equal(src[:, nq:].cpu(), qkv[:, nq:]) and intact(src_wide, src), (start, rp, Smax, "k | v columns")
        else:                               # q_out of its own, ldq != ldqkv
            q_wide, q_out = guarded(torch.zeros(B * S, nq, dtype=dtype), 16)
            ops.rope_kvcache(src, q_out, kc, vc, cs_d, B, S, H, Hkv, hd, start, rp)
            rq = R.within(q_out, q_ref, q_mag, dtype)
            assert intact(q_wide, q_out) and torch.equal(src.cpu(), qkv) and intact(src_wide, src), (start, rp, Smax, "q_out")
        rk = R.within(kc[:B, :, start:start + S].permute(0, 2, 1, 3), ref[:, :, H:], mag[:, :, H:], dtype)
        want_v = torch.full((B + 1, Hkv, hd, Smax), SENT, dtype=dtype)
        want_v[:B, :, :, start:start + S] = v.permute(0, 2, 3, 1)
        assert torch.equal(vc.cpu(), want_v), (start, rp, Smax, "v^T cache: an exact copy, nothing else written")
        kc[:B, :, start:start + S] = SENT
        assert bool((kc == SENT).all()), (start, rp, Smax, "k cache outside the written positions")
        worst = max(worst, rq, rk)
        assert max(rq, rk) <= 1.0, (start, rp, Smax, rq, rk)
    print(f"rope_kvcache S {S} hd {hd} {dtype}: {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ V^T pack
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("hd", R.VT_HD)
@pytest.mark.parametrize("L,Lpad", R.VT_L)
def test_vt_pack(L, Lpad, hd, dtype):
    """the v third of a packed qkv (ldv = 3 H hd): an exact transposed copy, exact zeros in L .. Lpad, nothing past the last row"""
    qkv = R.vt_pack_inputs(L, hd, dtype)
    W = R.VT_H * hd
    flat, vt = flat_guarded((R.VT_N, R.VT_H, hd, Lpad), dtype)
    qd = qkv.to(DEV)
    ops.vt_pack(qd[:, 2 * W:], 3 * W, vt, R.VT_N, L, R.VT_H, hd, Lpad)
    assert torch.equal(vt.cpu(), R.vt_pack_ref(qkv, L, hd, Lpad)) and tail_intact(flat, vt)
    assert torch.equal(qd.cpu(), qkv)


# ------------------------------------------------------------------ embedding / ViT assembly
@pytest.mark.parametrize("W", R.EMBED_W)
@pytest.mark.parametrize("dim", R.EMBED_DIMS)
@pytest.mark.parametrize("table_dtype,h_dtype", R.DTYPE_PAIRS)
def test_embed_assemble(table_dtype, h_dtype, dim, W):
    """tokens as a column slice (ld_tok > T); -1 and V clamp to rows 0 and V - 1; the image-word rows keep the sentinel"""
    d = R.embed_inputs(dim, table_dtype)
    B, T = R.EMBED_B, R.EMBED_T
    tok_wide = torch.full((B, T + 3), 5, dtype=torch.int64, device=DEV)
    tok = tok_wide[:, 2:2 + T]
    tok.copy_(d["tokens"])
    flat, h = flat_guarded((B * (T + W), dim), h_dtype)
    ops.embed_assemble(tok, d["table"].to(DEV), h, B, T, W, dim)
    assert torch.equal(h.view(B, T + W, dim).cpu(), R.embed_ref(d["tokens"], d["table"], W, h_dtype)) and tail_intact(flat, h)


@pytest.mark.parametrize("src_dtype,dst_dtype", R.DTYPE_PAIRS)
def test_fill_rows(src_dtype, dst_dtype):
    tag = R._randn(R.FILL_DIM, seed=22000).to(src_dtype)
    wide, dst = guarded(torch.full((R.FILL_ROWS, R.FILL_DIM), SENT, dtype=dst_dtype), 8)
    ops.fill_rows(tag.to(DEV), dst, torch.tensor(R.FILL_IDX, dtype=torch.int32, device=DEV))
    want = torch.full((R.FILL_ROWS, R.FILL_DIM), SENT, dtype=dst_dtype)
    want[R.FILL_IDX] = tag.to(dst_dtype)
    assert torch.equal(dst.cpu(), want) and intact(wide, dst)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("T", R.VIT_T)
@pytest.mark.parametrize("width", R.VIT_WIDTHS)
def test_vit_embed(width, T, dtype):
    """the fp32 sum rounded once"""
    d = R.vit_embed_inputs(T, width, dtype)
    flat, x = flat_guarded((R.VIT_N * (T + 1), width), dtype)
    ops.vit_embed(d["patch"].to(DEV), d["cls"].to(DEV), d["pos"].to(DEV), x, R.VIT_N, T, width)
    assert torch.equal(x.view(R.VIT_N, T + 1, width).cpu(), R.vit_embed_ref(d["patch"], d["cls"], d["pos"], T)) and tail_intact(flat, x)


# ------------------------------------------------------------------ patch im2col
@pytest.mark.parametrize("gh,g", R.IM2COL_GRIDS)
@pytest.mark.parametrize("P", R.IM2COL_P)
@pytest.mark.parametrize("key", sorted(R.IM2COL_KEYS))
def test_patch_im2col(key, P, gh, g):
    """exact against the unfold order on a grid with Hi != Wi; the pad columns exactly zero"""
    in_dtype, out_dtype = R.IM2COL_KEYS[key]
    img = R.im2col_inputs(P, gh, g, in_dtype)
    img_d = img.to(DEV)
    for Kpad in R.im2col_kpads(P):
        flat, cols = flat_guarded((R.IM2COL_N * gh * g, Kpad), out_dtype)
        ops.patch_im2col(img_d, cols, P)
        assert torch.equal(cols.cpu(), R.im2col_ref(img, P, Kpad, out_dtype)) and tail_intact(flat, cols), Kpad


# ------------------------------------------------------------------ view split
@pytest.mark.parametrize("B,c", R.SPLIT_SHAPES)
@pytest.mark.parametrize("key", sorted(R.SPLIT_KEYS))
def test_split_views(key, B, c):
    in_dtype, out_dtype = R.SPLIT_KEYS[key]
    img = R.split_inputs(B, c, in_dtype)
    flat, out = flat_guarded((5 * B, 3, c, c), out_dtype)
    ops.split_views(img.to(DEV), out)
    assert torch.equal(out[B:].cpu(), R.split_quadrants_ref(img, out_dtype)) and tail_intact(flat, out)
    r = R.bicubic_within(out[:B], img, out_dtype)
    print(f"split_views key {key} ({B}, {c}): bicubic {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------ argmax
def gen_state_tensors(st, pad=2):
    """the python-list state on the device; tokens / text_mask as column slices (offset 1) of wider tensors"""
    B, total = len(st["tokens"]), len(st["tokens"][0])
    tok_wide = torch.full((B, total + pad + 1), 99, dtype=torch.int64, device=DEV)
    mask_wide = torch.ones((B, total + pad + 1), dtype=torch.bool, device=DEV)
    tok, mask = tok_wide[:, 1:1 + total], mask_wide[:, 1:1 + total]
    tok.copy_(torch.tensor(st["tokens"]))
    mask.copy_(torch.tensor(st["text_mask"]))
    return dict(tok_wide=tok_wide, mask_wide=mask_wide, tokens=tok, text_mask=mask,
                stopped=torch.tensor(st["stopped"], device=DEV), stop_pos=torch.tensor(st["stop_pos"], dtype=torch.int64, device=DEV),
                live=torch.tensor([st["live"]], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("extra_ld", [0, 1])
@pytest.mark.parametrize("V", R.ARGMAX_V)
def test_argmax_and_generate_step_argmax(V, extra_ld):
    """a3v_argmax and the argmax inside a3v_generate_step: the maximum at 0, at V - 1, in the scalar tail, in the last full vector; a
    tie (lowest index); an all-negative row; an all -inf row (both give 0); ld = V + 1 makes the rows of an odd V unaligned"""
    lg, want = R.argmax_inputs(V)
    rows = lg.shape[0]
    lg_d = strided(lg, extra_ld)
    assert lg_d.stride(0) == V + extra_ld
    flat = torch.full((rows + 8,), int(SENT), dtype=torch.int64, device=DEV)
    ops.argmax(lg_d, flat[:rows])
    assert flat[:rows].cpu().tolist() == want.tolist() and bool((flat[rows:] == int(SENT)).all())
    st = dict(tokens=[[0, 0] for _ in range(rows)], text_mask=[[False, False] for _ in range(rows)], stopped=[False] * rows,
              stop_pos=[1] * rows, live=rows)
    t = gen_state_tensors(st)
    ops.generate_step(lg_d, None, t["tokens"], t["text_mask"], 1, None, None, 0, t["stopped"], t["stop_pos"], t["live"])
    assert t["tokens"][:, 1].cpu().tolist() == want.tolist() and t["tokens"][:, 0].cpu().tolist() == [0] * rows
    assert t["stop_pos"].cpu().tolist() == [2] * rows and not bool(t["stopped"].any()) and int(t["live"]) == rows


# ------------------------------------------------------------------ cross entropy
def run_ce(d, dtype, scales, what):
    rows, V = d["logits"].shape
    lab = d["labels"].to(DEV)
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.count_valid(lab, nv)
    n_valid = R.ce_n_valid(d["labels"])
    assert int(nv.item()) == n_valid
    lg = strided(d["logits"], 8)
    worst = 0.0
    for scale in scales:
        loss_ref, mag_loss, dl_ref, mag_d, uf = R.ce_ref(d["logits"], d["labels"], scale, n_valid)
        loss_flat, loss = flat_guarded((rows,), F32, pad=8)
        dl_wide, dl = guarded(torch.full((rows, V), SENT, dtype=dtype), 8)
        ops.cross_entropy(lg, lab, loss, dl, nv, scale)
        r1, r2 = R.within(loss, loss_ref, mag_loss, F32), R.within(dl, dl_ref, mag_d, dtype, underflow=uf)
        print(f"cross_entropy {what} ({rows}, {V}) {dtype} scale {scale:.3f}: loss {r1:.3f} dlogits {r2:.3f}")
        assert tail_intact(loss_flat, loss) and intact(dl_wide, dl)
        invalid = ((d["labels"] <= 0) | (d["labels"] >= V)).to(DEV)
        assert float(loss[invalid].abs().sum()) == 0 and float(dl[invalid].float().abs().sum()) == 0
        worst = max(worst, r1, r2)
    loss_flat, loss2 = flat_guarded((rows,), F32, pad=8)
    ops.cross_entropy(lg, lab, loss2, None)                               # dlogits=None: the loss alone, the same bits
    assert torch.equal(loss2, loss) and tail_intact(loss_flat, loss2)
    assert torch.equal(lg.cpu(), d["logits"])
    return worst


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,V", R.CE_SHAPES)
def test_cross_entropy(rows, V, dtype):
    """ld = V + 8 for logits and dlogits, grad_scale 1 / 0.25 / 1/3, labels 1 and V - 1, an ignored row, a spike row (one logit 60
    above the rest), a flat row"""
    assert run_ce(R.ce_inputs(rows, V, dtype), dtype, R.CE_SCALES, "plain") <= 1.0


@pytest.mark.parametrize("dtype", [BF, F32])
def test_cross_entropy_label_rules(dtype):
    """labels -100, -1, 0, V, V + 5: zero loss, a zero gradient row; count_valid counts every non-zero label; one valid row"""
    for rows, V in ((7, 8), (9, 4100)):
        assert run_ce(R.ce_bad_label_inputs(rows, V, dtype), dtype, [0.25], "bad labels") <= 1.0
    assert run_ce(R.ce_one_valid_inputs(5, 255, dtype), dtype, [1.0], "one valid row") <= 1.0


# ------------------------------------------------------------------ generation step
def check_state(t, st, what):
    assert t["tokens"].cpu().tolist() == st["tokens"], what
    assert t["stopped"].cpu().tolist() == st["stopped"], what
    assert t["stop_pos"].cpu().tolist() == st["stop_pos"], what
    total = t["tokens"].shape[1]
    assert bool((t["tok_wide"][:, 0] == 99).all()) and bool((t["tok_wide"][:, 1 + total:] == 99).all()), what
    assert t["text_mask"].cpu().tolist() == st["text_mask"] and bool(t["mask_wide"][:, 0].all()) and bool(t["mask_wide"][:, 1 + total:].all()), what


@pytest.mark.parametrize("mode", ["logits", "sampled", "no_stops", "no_live"])
def test_generate_step(mode):
    """the scripted run of rowops_fwd_ref (forced rows, two stop sequences matching at one step, one longer than the sequence, a
    forced token completing a stop sequence, a match beginning inside the prompt, an already stopped row): after EVERY step the whole
    state equals the python reference; through the logits (argmax inside), through sampled ids, without stop sequences (null
    pointers), without the live counter"""
    stops = [] if mode == "no_stops" else R.GEN_STOPS
    table = R.gen_logits_table()
    table_d = table.to(DEV)
    st = R.gen_initial_state()
    t = gen_state_tensors(st)
    B = len(R.GEN_PROMPTS)
    stop_seq = torch.tensor([x for s in stops for x in s], dtype=torch.int64, device=DEV) if stops else None
    offs = [0]
    for s in stops:
        offs.append(offs[-1] + len(s))
    stop_off = torch.tensor(offs, dtype=torch.int32, device=DEV) if stops else None
    live = None if mode == "no_live" else t["live"]
    for cur in range(R.GEN_START, R.GEN_TOTAL):
        ids = torch.argmax(table[cur], dim=-1)
        R.generate_step_ref(st, ids.tolist(), cur, stops)
        if mode == "sampled":
            ops.generate_step(None, ids.to(DEV), t["tokens"], t["text_mask"], cur, stop_seq, stop_off, len(stops), t["stopped"], t["stop_pos"], live)
        else:
            ops.generate_step(table_d[cur], None, t["tokens"], t["text_mask"], cur, stop_seq, stop_off, len(stops), t["stopped"], t["stop_pos"], live)
        check_state(t, st, (mode, cur))
        assert int(t["live"]) == (B if live is None else st["live"]), (mode, cur)
    if live is not None:
        assert int(t["live"]) == B - int(t["stopped"].sum())
    if stops:
        assert st["stop_pos"] == [3, 8, 1, R.GEN_TOTAL, 3, 1]
