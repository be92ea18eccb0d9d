"""-m gpu: the optimizer step against a plain float64 reference, from the clip norm to the bf16 images.  a3v_adamw / a3v_adamw_scaled,
a3v_adamw_scaled_t, a3v_adamw_multi, a3v_adamw8_scaled, a3v_sumsq_partials and a3v_lora_refresh, each on inputs where every float32
operation is exact (bit for bit, any summation or contraction order) and on inputs where the arithmetic variants differ (element by
element inside the bounds derived in tests/optim_ref.py; no literal tolerance here).  Every buffer sits inside a sentinel-filled
allocation that must stay as it was around the data."""
import numpy as np
import pytest
import torch

import adam8_ref as R8
import optim_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                                   # sentinel elements on either side of every buffer (keeps the data 16-byte aligned)
SENT_F = -12345.678                        # float32 sentinel
SENT_I = 0xDEAD - 0x10000                  # bf16 images are held as int16 bit patterns: sentinel 0xDEAD
SENT_B = 0xA5                              # uint8 sentinel
ERR_SHAPE, ERR_ARG = -1, -3
WORST = {}


@pytest.fixture(scope="module")
def L():
    from a3vlm_amd import lib
    lib.load()
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sent(dtype):
    return {torch.float32: SENT_F, torch.int16: SENT_I, torch.uint8: SENT_B}[dtype]


class Guarded:
    """``data`` (1-D) in the middle of a sentinel-filled device buffer; ``untouched`` asserts that the surroundings still hold it."""

    def __init__(self, data, dtype=None, pad=PAD):
        if isinstance(data, int):
            data = torch.full((data,), _sent(dtype), dtype=dtype)
        elif isinstance(data, np.ndarray):
            data = torch.from_numpy(np.ascontiguousarray(data))
        self.n, self.pad = data.numel(), pad
        self.buf = torch.full((self.n + 2 * pad,), _sent(data.dtype), dtype=data.dtype, device=DEV)
        self.view = self.buf[pad:pad + self.n]
        self.view.copy_(data.reshape(-1))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def untouched(self, what):
        s = _sent(self.buf.dtype)
        ok = bool((self.buf[:self.pad] == s).all()) and bool((self.buf[self.pad + self.n:] == s).all())
        assert ok, f"{what}: the sentinels around the buffer were written"

    def host(self):
        return self.view.cpu().numpy()


def coef_dev(coef):
    return None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)


def _note(family, ratios):
    w = WORST.setdefault(family, [0.0, 0.0, 0.0])
    for i, r in enumerate(ratios):
        w[i] = max(w[i], r)


def _report(family):
    w = WORST.get(family)
    if w:
        print(f"\n[optim_parity] {family}: largest err/bound  p {w[0]:.3f}  m {w[1]:.3f}  v {w[2]:.3f}")


def check_bounded(family, got, inp, h, coef, what):
    """got = (p', m', v') numpy float32 of the device against the float64 reference of inp = (p, g, m, v) and the derived bounds."""
    ref = O.adamw_ref(*inp, h, coef)
    bounds = O.adamw_bounds(ref, h)
    ratios = [O.ratio(a, ref[k], b) for a, k, b in zip(got, "pmv", bounds)]
    _note(family, ratios)
    assert all(np.isfinite(a).all() for a in got), what
    assert max(ratios) <= 1.0, f"{what}: err/bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}"


def image_is_rounding_of(img_i16, p_f32, what):
    assert torch.equal(img_i16, O.bf16_bits_torch(p_f32)), f"{what}: the image is not the bf16 rounding of the device's own p'"


# ------------------------------------------------------------------------------------------------ a. a3v_adamw / a3v_adamw_scaled

def flat_step(L, inp, h, coef, image, entry="scaled"):
    """One launch on guarded copies of inp = (p, g, m, v) (numpy or torch) -> (P, G, M, V, IMG or None) Guarded."""
    P, G, M, V = (Guarded(a) for a in inp)
    IMG = Guarded(P.n, torch.int16) if image else None
    lib, gs = L.load(), coef_dev(coef)
    args = (P.ptr, G.ptr, M.ptr, V.ptr, P.n, h.lr, h.b1, h.b2, h.eps, h.wd, h.step, IMG.ptr if image else None)
    if entry == "plain":
        assert coef is None
        rc = lib.a3v_adamw(*args, _stream())
    else:
        rc = lib.a3v_adamw_scaled(*args, gs.data_ptr() if gs is not None else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b, name in zip((P, G, M, V, IMG), ("p", "g", "m", "v", "image")):
        if b is not None:
            b.untouched(name)
    return P, G, M, V, IMG


FLAT_N = [1, 3, 4, 5, 7, 1023, 1024, 1025, 4099, 262147]


@pytest.mark.parametrize("betas", O.BETAS, ids=lambda b: f"b{b[0]}_{b[1]}")
@pytest.mark.parametrize("n", FLAT_N)
def test_adamw_bounded(L, n, betas):
    """p', m', v' element by element against float64, for every step / decay / coefficient case, with and without the image."""
    k = 0
    for h in O.bounded_hypers():
        if (h.b1, h.b2) != betas:
            continue
        for coef in O.COEFS:
            k += 1
            inp = O.bounded_inputs(n, seed=k, eps=h.eps)
            P, G, M, V, IMG = flat_step(L, inp, h, coef, True, "plain" if (coef is None and k % 2) else "scaled")
            assert torch.equal(G.view.cpu(), torch.from_numpy(inp[1])), "the gradient was written"
            check_bounded("adamw", (P.host(), M.host(), V.host()), inp, h, coef, f"n={n} {h} coef={coef}")
            image_is_rounding_of(IMG.view, P.view, f"n={n} {h} coef={coef}")
            P2, _, M2, V2, _ = flat_step(L, inp, h, coef, False)
            assert torch.equal(P2.view, P.view) and torch.equal(M2.view, M.view) and torch.equal(V2.view, V.view), "with / without image differ"
    _report("adamw")


EXACT_N = FLAT_N + [O.CAP_N - 4, O.CAP_N, O.CAP_N + 4, O.CAP_N + 1027, 2 * O.CAP_N + 5]


@pytest.mark.parametrize("n", EXACT_N)
def test_adamw_exact(L, n):
    """Exact inputs: bit for bit the closed form, through the grid cap and the second and third trip of the grid-stride loop."""
    for wd in (0.0, 0.5):
        for st in (False, True):
            for coef in ((None, 0.5) if n <= 4099 or (wd, st) == (0.5, True) else (None,)):
                c = O.exact_case(n, wd, st, coef, device=DEV)
                P, G, M, V, IMG = flat_step(L, (c["p"], c["g"], c["m"], c["v"]), O.exact_hyper(wd), coef, True, "plain" if coef is None and st else "scaled")
                what = f"n={n} wd={wd} stationary={st} coef={coef}"
                assert torch.equal(P.view, c["p1"]), what + ": p"
                assert torch.equal(M.view, c["m1"]), what + ": m"
                assert torch.equal(V.view, c["v1"]), what + ": v"
                assert torch.equal(IMG.view, O.bf16_bits_torch(c["p1"])), what + ": image"


def test_adamw_position_independence(L):
    """Elements [0, 4k + r) as a whole tensor (the last r through the scalar tail) equal the same elements of a longer tensor (vector
    body), bit for bit, on inexact inputs: ZeRO-1 slices a flat master at arbitrary boundaries and promises the unsliced result."""
    for j, h in enumerate(O.bounded_hypers()[:12:2] + O.bounded_hypers()[21:24]):
        for coef in (None, 0.37):
            for n in (1, 2, 3, 7, 1025, 4098, 4099):
                inp = O.bounded_inputs(n + 9, seed=j, eps=h.eps)
                long = flat_step(L, inp, h, coef, True)
                short = flat_step(L, tuple(a[:n] for a in inp), h, coef, True)
                for a, b, name in zip(long, short, ("p", "g", "m", "v", "image")):
                    assert torch.equal(a.view[:n], b.view), f"{name}: n={n} {h} coef={coef}: the scalar tail and the vector body differ"


@pytest.mark.parametrize("coef", [-1.0, -1e-30, float("nan"), -0.0, float("-inf")])
def test_adamw_skip_coefficients_write_nothing(L, coef):
    for n in (7, 4099):
        inp = O.bounded_inputs(n, seed=3)
        P, G, M, V, IMG = flat_step(L, inp, O.Hyper(3e-3, 0.9, 0.95, 1e-8, 0.1, 2), coef, True)
        for b, a in zip((P, G, M, V), inp):
            assert np.array_equal(b.host().view(np.uint32), a.view(np.uint32))
        assert bool((IMG.view == SENT_I).all())


def test_adamw_refuses_and_writes_nothing(L):
    lib = L.load()
    inp = O.bounded_inputs(1032, seed=4)
    P, G, M, V = (Guarded(a) for a in inp)
    IMG = Guarded(1032, torch.int16)
    hp = (3e-3, 0.9, 0.95, 1e-8, 0.1)
    assert lib.a3v_adamw_scaled(P.ptr, G.ptr, M.ptr, V.ptr, 1032, *hp, 0, IMG.ptr, None, _stream()) == ERR_ARG          # step < 1
    assert lib.a3v_adamw(P.ptr, G.ptr, M.ptr, V.ptr, 1032, *hp, -3, IMG.ptr, _stream()) == ERR_ARG
    assert lib.a3v_adamw_scaled(P.ptr, G.ptr, M.ptr, V.ptr, 0, *hp, 1, IMG.ptr, None, _stream()) == ERR_ARG             # n <= 0
    assert lib.a3v_adamw_scaled(P.ptr, G.ptr, M.ptr, V.ptr, -8, *hp, 1, IMG.ptr, None, _stream()) == ERR_ARG
    for k in range(4):                                                                                                     # a misaligned pointer
        ptrs = [P.ptr, G.ptr, M.ptr, V.ptr]
        ptrs[k] += 4
        assert lib.a3v_adamw_scaled(*ptrs, 1024, *hp, 1, IMG.ptr, None, _stream()) == ERR_SHAPE
    assert lib.a3v_adamw_scaled(P.ptr, G.ptr, M.ptr, V.ptr, 1024, *hp, 1, IMG.ptr + 2, None, _stream()) == ERR_SHAPE
    assert lib.a3v_adamw_scaled(None, G.ptr, M.ptr, V.ptr, 1024, *hp, 1, IMG.ptr, None, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    for b, a in zip((P, G, M, V), inp):
        assert np.array_equal(b.host().view(np.uint32), a.view(np.uint32))
        b.untouched("refused call")
    assert bool((IMG.buf == SENT_I).all())


# ------------------------------------------------------------------------------------------------ b. a3v_adamw_scaled_t

def t_step(L, inp, rows, cols, h, coef, ldt, row0, image=True):
    """a3v_adamw_scaled_t on guarded copies; the transposed image is a [cols][ldt] guarded buffer written from column ``row0``."""
    P, G, M, V = (Guarded(a) for a in inp)
    IMG = Guarded(rows * cols, torch.int16) if image else None
    IMGT = Guarded(cols * ldt, torch.int16)
    gs = coef_dev(coef)
    rc = L.load().a3v_adamw_scaled_t(P.ptr, G.ptr, M.ptr, V.ptr, rows, cols, h.lr, h.b1, h.b2, h.eps, h.wd, h.step, IMG.ptr if image else None,
                                     IMGT.ptr + 2 * row0, ldt, gs.data_ptr() if gs is not None else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b, name in zip((P, G, M, V, IMG, IMGT), ("p", "g", "m", "v", "image", "image_t")):
        if b is not None:
            b.untouched(name)
    return P, G, M, V, IMG, IMGT


def check_image_t(IMGT, img_bits, rows, cols, ldt, row0, what):
    """Columns [row0, row0 + rows) of every row of the [cols][ldt] buffer = the forward image transposed; the rest untouched."""
    want = torch.full((cols, ldt), SENT_I, dtype=torch.int16, device=DEV)
    want[:, row0:row0 + rows] = img_bits.view(rows, cols).t()
    assert torch.equal(IMGT.view.view(cols, ldt), want), what + ": transposed image"


T_SHAPES = [(64, 64), (128, 64), (192, 128), (320, 192)]


def _t_layouts(rows):
    return [(rows, 0), (rows + 4, 4), (rows + 64, 0), (rows + 64, 64)]          # (ldt, row offset): ldt in {rows, rows + 4, rows + 64}


@pytest.mark.parametrize("rows,cols", T_SHAPES)
def test_adamw_t_bounded(L, rows, cols):
    n = rows * cols
    hs = O.bounded_hypers()
    for k, (h, coef) in enumerate([(hs[0], None), (hs[3], 0.37), (hs[12], 1.0), (hs[19], 0.37), (hs[24], 0.0), (hs[29], 0.37)]):
        ldt, row0 = _t_layouts(rows)[k % 4]
        inp = O.bounded_inputs(n, seed=k, eps=h.eps)
        P, G, M, V, IMG, IMGT = t_step(L, inp, rows, cols, h, coef, ldt, row0)
        what = f"{rows}x{cols} {h} coef={coef} ldt={ldt} row0={row0}"
        check_bounded("adamw_t", (P.host(), M.host(), V.host()), inp, h, coef, what)
        image_is_rounding_of(IMG.view, P.view, what)
        check_image_t(IMGT, IMG.view, rows, cols, ldt, row0, what)
        P2, _, M2, V2, _, IMGT2 = t_step(L, inp, rows, cols, h, coef, ldt, row0, image=False)          # bf16_image == NULL
        assert torch.equal(P2.view, P.view) and torch.equal(M2.view, M.view) and torch.equal(V2.view, V.view) and torch.equal(IMGT2.buf, IMGT.buf)
    _report("adamw_t")


@pytest.mark.parametrize("rows,cols", T_SHAPES + [(128, 64 * 2049), (64, 64 * 4097), (128, 64 * 4097)])
def test_adamw_t_exact(L, rows, cols):
    """Bit for bit the closed form; 2049 / 4097 tiles on 2048 blocks: block 0 walks two / three tiles and re-uses its first LDS patch."""
    n = rows * cols
    big = cols > 192
    for k, (wd, st, coef) in enumerate([(0.5, True, 0.5)] if big else [(0.0, False, None), (0.5, True, None), (0.5, True, 0.5), (0.0, True, None)]):
        ldt, row0 = _t_layouts(rows)[(k + 1) % 4]
        c = O.exact_case(n, wd, st, coef, device=DEV)
        P, G, M, V, IMG, IMGT = t_step(L, (c["p"], c["g"], c["m"], c["v"]), rows, cols, O.exact_hyper(wd), coef, ldt, row0)
        what = f"{rows}x{cols} wd={wd} stationary={st} coef={coef} ldt={ldt} row0={row0}"
        assert torch.equal(P.view, c["p1"]) and torch.equal(M.view, c["m1"]) and torch.equal(V.view, c["v1"]), what
        want = O.bf16_bits_torch(c["p1"])
        assert torch.equal(IMG.view, want), what + ": image"
        check_image_t(IMGT, want, rows, cols, ldt, row0, what)
    P, G, M, V, IMG, IMGT = t_step(L, (c["p"], c["g"], c["m"], c["v"]), rows, cols, O.exact_hyper(wd), -0.5, rows, 0)          # skipped
    assert torch.equal(P.view, c["p"]) and torch.equal(M.view, c["m"]) and torch.equal(V.view, c["v"])
    assert bool((IMG.view == SENT_I).all()) and bool((IMGT.view == SENT_I).all())


# ------------------------------------------------------------------------------------------------ c. a3v_adamw_multi

class Sink:
    """One bf16 destination of a table row: a guarded int16 buffer, the element offset of (0, 0) and the strides of (row, column)."""

    def __init__(self, size, off, sr, sc):
        self.g, self.off, self.sr, self.sc = Guarded(size, torch.int16), off, sr, sc

    def expect(self, bits, rows, cols):
        want = torch.full((self.g.n,), SENT_I, dtype=torch.int16, device=DEV)
        r = torch.arange(rows, device=DEV).view(-1, 1)
        c = torch.arange(cols, device=DEV).view(1, -1)
        want[(self.off + r * self.sr + c * self.sc).reshape(-1)] = bits.reshape(-1)
        return want


# (name, n, cols, sink form)
MULTI_TENSORS = [("n1", 1, 1, "none"), ("n3", 3, 3, "vec"), ("n4", 4, 4, "vec"), ("n7", 7, 7, "d2"), ("odd_cols", 780, 6, "same"),
                 ("lora_a", 65536, 4096, "two_a"), ("n65540", 65540, 65540, "vec"), ("lora_b", 176128, 16, "two_b"), ("big", 262147, 262147, "none"),
                 ("d1_strided", 780, 6, "d1")]


def _sinks(form, n, cols):
    rows = n // cols
    if form in ("vec", "same"):                     # a contiguous same-shape image: the vector path iff cols % 4 == 0
        return Sink(n, 0, cols, 1), None
    if form == "two_a":                             # lora_a [r, in]: rows col0.. of A [Rp, lda] and columns col0.. of At [in, Rp]
        lda, rp, col0 = cols + 8, 48, 16
        return Sink(rp * lda, col0 * lda, lda, 1), Sink(cols * rp, col0, 1, rp)
    if form == "two_b":                             # lora_b [nj, r]: B[row0 + t][col0 + i] of [N, ldb] and Bt[col0 + i][row0 + t] of [Rp, ldbt]
        ldb, ldbt, col0, row0 = 40, rows + 72, 16, 64
        return Sink((rows + 70) * ldb, row0 * ldb + col0, ldb, 1), Sink(48 * ldbt, col0 * ldbt + row0, 1, ldbt)
    if form == "d1":
        return Sink(rows * 10 + 8, 3, 10, 1), None
    if form == "d2":
        return None, Sink(n * 3 + 2, 1, 0, 3)
    return None, None


def multi_step(L, tensors, inputs, h, coef, max_n=None):
    """a3v_adamw_multi over a table built as optim.py builds it (12 int64 per row) -> per tensor (P, G, M, V, d1, d2)."""
    bufs, rows = [], []
    for (name, n, cols, form), inp in zip(tensors, inputs):
        P, G, M, V = (Guarded(a) for a in inp)
        d1, d2 = _sinks(form, n, cols)
        bufs.append((P, G, M, V, d1, d2))
        rows.append([P.ptr, G.ptr, M.ptr, V.ptr, n, cols,
                     d1.g.ptr + 2 * d1.off if d1 else 0, d1.sr if d1 else 0, d1.sc if d1 else 0,
                     d2.g.ptr + 2 * d2.off if d2 else 0, d2.sr if d2 else 0, d2.sc if d2 else 0])
    tab = Guarded(torch.tensor(rows, dtype=torch.int64).view(-1).view(torch.uint8).clone())
    gs = coef_dev(coef)
    rc = L.load().a3v_adamw_multi(tab.ptr, len(tensors), max_n or max(t[1] for t in tensors), h.lr, h.b1, h.b2, h.eps, h.wd, h.step,
                                  gs.data_ptr() if gs is not None else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    tab.untouched("table")
    for P, G, M, V, d1, d2 in bufs:
        for b in (P, G, M, V) + tuple(s.g for s in (d1, d2) if s):
            b.untouched("multi")
    return bufs


def check_multi_sinks(t, b, bits, what):
    name, n, cols, form = t
    for s in b[4:]:
        if s is not None:
            assert torch.equal(s.g.view, s.expect(bits, n // cols, cols)), f"{what} {name}: a bf16 sink"


MULTI_ORDERS = {"mixed": list(range(10)), "largest_first": [8, 0, 4, 5], "largest_last": [1, 2, 3, 9, 8], "one_tensor": [7], "one_small": [1]}


@pytest.mark.parametrize("order", list(MULTI_ORDERS))
def test_adamw_multi_bounded(L, order):
    tensors = [MULTI_TENSORS[i] for i in MULTI_ORDERS[order]]
    hs = O.bounded_hypers()
    for k, (h, coef) in enumerate([(hs[1], 0.37), (hs[14], None), (hs[26], 1.0), (hs[9], 0.0)] if order == "mixed" else [(hs[3], 0.37)]):
        inputs = [O.bounded_inputs(t[1], seed=10 * k + i, eps=h.eps) for i, t in enumerate(tensors)]
        bufs = multi_step(L, tensors, inputs, h, coef)
        for t, inp, b in zip(tensors, inputs, bufs):
            what = f"{order} {t[0]} {h} coef={coef}"
            assert torch.equal(b[1].view.cpu(), torch.from_numpy(inp[1])), what
            check_bounded("adamw_multi", (b[0].host(), b[2].host(), b[3].host()), inp, h, coef, what)
            check_multi_sinks(t, b, O.bf16_bits_torch(b[0].view), what)
    _report("adamw_multi")


@pytest.mark.parametrize("order", list(MULTI_ORDERS))
def test_adamw_multi_exact(L, order):
    tensors = [MULTI_TENSORS[i] for i in MULTI_ORDERS[order]]
    for wd, st, coef in [(0.5, True, 0.5), (0.0, False, None)]:
        cases = [O.exact_case(t[1], wd, st, coef, device=DEV, offset=1000 * i) for i, t in enumerate(tensors)]
        bufs = multi_step(L, tensors, [(c["p"], c["g"], c["m"], c["v"]) for c in cases], O.exact_hyper(wd), coef)
        for t, c, b in zip(tensors, cases, bufs):
            what = f"{order} {t[0]} wd={wd} stationary={st} coef={coef}"
            assert torch.equal(b[0].view, c["p1"]) and torch.equal(b[2].view, c["m1"]) and torch.equal(b[3].view, c["v1"]), what
            check_multi_sinks(t, b, O.bf16_bits_torch(c["p1"]), what)


@pytest.mark.parametrize("coef", [-1.0, float("nan"), -0.0])
def test_adamw_multi_skip_coefficients_write_nothing(L, coef):
    tensors = [MULTI_TENSORS[i] for i in (1, 4, 5, 8)]
    inputs = [O.bounded_inputs(t[1], seed=i) for i, t in enumerate(tensors)]
    bufs = multi_step(L, tensors, inputs, O.Hyper(3e-3, 0.9, 0.95, 1e-8, 0.1, 3), coef)
    for inp, b in zip(inputs, bufs):
        for k, j in enumerate((0, 1, 2, 3)):
            assert np.array_equal(b[j].host().view(np.uint32), inp[k].view(np.uint32))
        assert all(bool((s.g.view == SENT_I).all()) for s in b[4:] if s)


def test_adamw_multi_position_independence(L):
    """The scalar tail of a table row equals the vector body of a longer row, bit for bit (and both equal a3v_adamw_scaled)."""
    h = O.bounded_hypers()[2]
    for n in (1, 3, 7, 1027):
        inp = O.bounded_inputs(n + 9, seed=n, eps=h.eps)
        tensors = [("short", n, n, "none"), ("long", n + 9, n + 9, "none")]
        bufs = multi_step(L, tensors, [tuple(a[:n] for a in inp), inp], h, 0.37)
        flat = flat_step(L, inp, h, 0.37, False)
        for j in (0, 2, 3):
            assert torch.equal(bufs[0][j].view, bufs[1][j].view[:n]), f"n={n}: tail and body differ"
            assert torch.equal(bufs[1][j].view, flat[j].view), f"n={n}: multi and per-tensor launch differ"


# ------------------------------------------------------------------------------------------------ d. a3v_adamw8_scaled

@pytest.mark.parametrize("n", [256, 768, 256 * 4099])
def test_adamw8_fp64_anchor(L, n):
    """One step from a quantised state: p' within the float32 bound of the float64 reference evaluated on the dequantised moments; the
    stored moments within half an e4m3 step (adam8_ref.half_step_bound) of the float64 m' and sqrt(v').  Per-block magnitudes spread over
    2^-12 .. 2^12; inside a block within a factor of 8, so no quotient falls into the format's subnormals (the 0x01 rule has its own test)."""
    rs = np.random.RandomState(n % 1000)
    blk = np.repeat(np.exp2(rs.uniform(-12, 12, n // 256)), 256)
    g = (blk * rs.uniform(0.25, 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    m0 = (blk * rs.uniform(0.25, 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    v0 = ((blk * rs.uniform(0.25, 1.0, n)) ** 2).astype(np.float32)
    p = rs.randn(n).astype(np.float32)
    mq, ms, rq, rs_ = R8.quantize(m0, v0)
    md, vd = R8.dequantize(mq, ms, rq, rs_)
    h, coef = O.Hyper(1e-3, 0.9, 0.95, 1e-8, 0.02, 7), 0.37
    P, G, MQ, MS, RQ, RS = (Guarded(a) for a in (p, g, mq, ms, rq, rs_))
    IMG = Guarded(n, torch.int16)
    gs = coef_dev(coef)
    rc = L.load().a3v_adamw8_scaled(P.ptr, G.ptr, MQ.ptr, MS.ptr, RQ.ptr, RS.ptr, n, h.lr, h.b1, h.b2, h.eps, h.wd, h.step, IMG.ptr, gs.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b in (P, G, MQ, MS, RQ, RS, IMG):
        b.untouched("adamw8")
    ref = O.adamw_ref(p, g, md, vd, h, coef)
    Ep, _, _ = O.adamw_bounds(ref, h)
    rp = O.ratio(P.host(), ref["p"], Ep)
    m_new, r_new = R8.dequantize_m(MQ.host(), MS.host()), R8.dequantize_r(RQ.host(), RS.host())
    rm = O.ratio(m_new, ref["m"], R8.half_step_bound(ref["m"], MS.host()))
    rr = O.ratio(r_new, np.sqrt(ref["v"]), R8.half_step_bound(np.sqrt(ref["v"]), RS.host()))
    print(f"\n[optim_parity] adamw8 n={n}: err/bound p {rp:.3f}, stored m {rm:.3f}, stored sqrt(v) {rr:.3f}")
    assert rp <= 1.0 and rm <= 1.0 and rr <= 1.0, (rp, rm, rr)
    image_is_rounding_of(IMG.view, P.view, f"adamw8 n={n}")


# ------------------------------------------------------------------------------------------------ e. a3v_sumsq_partials

def sumsq(L, x):
    X = Guarded(x)
    out = Guarded(torch.full((O.SLOTS,), float("nan")))
    assert L.load().a3v_sumsq_partials(X.ptr, X.n, out.ptr, _stream()) == 0
    torch.cuda.synchronize()
    X.untouched("x")
    out.untouched("slots")
    return out.host().copy()


def sumsq_bounded_input(n, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randn(n) * np.exp2(rs.uniform(-8, 8, n))).astype(np.float32)


M1 = 1 << 20
SUMSQ_N = [1, 3, 4, 5, 1023, 1024, 1025, M1 - 4, M1, M1 + 4, M1 + 1027, 3 * M1 + 2]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_slots(L, n):
    """Every slot against its float64 sum (bounded) and bit for bit (integers); a slot without data is 0, never left as it was."""
    x = O.sumsq_exact_input(n, n)
    got = sumsq(L, x)
    assert np.array_equal(got.view(np.uint32), O.sumsq_ref(x).astype(np.float32).view(np.uint32)), n
    x = sumsq_bounded_input(n, n)
    got, ref = sumsq(L, x), O.sumsq_ref(x)
    r = O.ratio(got, ref, O.sumsq_bound(x, ref))
    w = WORST.setdefault("sumsq", [0.0])
    w[0] = max(w[0], r)
    print(f"\n[optim_parity] sumsq n={n}: largest err/bound per slot {r:.3f} (so far {w[0]:.3f})")
    assert np.isfinite(got).all() and r <= 1.0, (n, r)
    assert np.array_equal(got.view(np.uint32), O.emu_sumsq(x).view(np.uint32)), "the operation-for-operation emulation differs"


@pytest.mark.parametrize("blocks", [1, 3, 64, 1023])
def test_sumsq_narrow_grid_is_bit_identical(L, blocks):
    for n in (1025, M1 + 1027, 3 * M1 + 2):
        x = sumsq_bounded_input(n, blocks)
        want = sumsq(L, x)
        with L.env(A3V_SUMSQ_BLOCKS=blocks):
            got = sumsq(L, x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, blocks)


def _poison_positions(n):
    n4 = n // 4
    pos = {0, (n4 - 1) * 4 + 3} | set(range(n4 * 4, n))                          # element 0, the last full vector, each tail position
    if n4 > O.SLOTS * 256:
        pos |= {min(n4, 2 * O.SLOTS * 256) * 4 - 2}                               # the last vector of the second pass
    return sorted(pos)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_sumsq_non_finite_reaches_the_norm(L, bad):
    for n in (7, 1027, 2 * M1 + 3, M1 + 1027):
        x = Guarded(sumsq_bounded_input(n, 7))
        out = torch.empty(O.SLOTS, dtype=torch.float32, device=DEV)
        for pos in _poison_positions(n):
            keep = x.view[pos].clone()
            x.view[pos] = bad
            assert L.load().a3v_sumsq_partials(x.ptr, n, out.data_ptr(), _stream()) == 0
            assert not bool(torch.isfinite(out.sum().sqrt())), (n, pos, bad)
            x.view[pos] = keep
        assert L.load().a3v_sumsq_partials(x.ptr, n, out.data_ptr(), _stream()) == 0
        assert bool(torch.isfinite(out.sum().sqrt()))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("moments", ["fp32", "e4m3"])
def test_poisoned_gradient_never_reaches_the_masters(L, bad, moments):
    """The chain as engine_finetune.py composes it: norm = sqrt(sum of the partials), coef = where(bad, -1, clamp(max_norm / (norm + 1e-6),
    max = 1)), FusedAdamW.step(grad_scale=coef): one non-finite gradient element in a tail leaves parameters, moments and images as they were."""
    from a3vlm_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in (4096 + 256, 1027, 7, 300)]
    for p in params:
        p.grad = torch.zeros_like(p)
    imgs = {id(p): torch.zeros(p.shape, dtype=torch.bfloat16, device=DEV) for p in params}
    opt = FusedAdamW(params, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, image_of=lambda p: imgs[id(p)], moments=moments)
    opt.multi_threshold = 2048                                  # the first tensor alone is "big": its own launch (8-bit moments with e4m3)
    out = torch.empty(O.SLOTS, dtype=torch.float32, device=DEV)

    def clip_and_step():
        total = torch.zeros((), device=DEV)
        for p in params:
            L.check(L.load().a3v_sumsq_partials(p.grad.data_ptr(), p.grad.numel(), out.data_ptr(), _stream()), "sumsq")
            total = total + out.sum()
        norm = total.sqrt()
        isbad = ~torch.isfinite(norm)
        coef = torch.clamp(1.0 / (norm + 1e-6), max=1.0).to(torch.float32)
        opt.step(grad_scale=torch.where(isbad, -coef.new_ones(()), coef).reshape(1))
        return isbad

    for p in params:
        p.grad.copy_(torch.randn(p.shape, generator=gen).to(DEV))
    assert not bool(clip_and_step())
    assert ("exp_avg_q" in opt.state[params[0]]) == (moments == "e4m3")

    def snapshot():
        s = [p.detach().clone() for p in params] + [imgs[id(p)].clone() for p in params]
        for p in params:
            s += [t.clone() for k, t in sorted(opt.state[p].items()) if k != "step"]
        return s

    before = snapshot()
    for p in params:
        p.grad.copy_(torch.randn(p.shape, generator=gen).to(DEV))
    params[1].grad[-1] = bad                                    # the last of the three tail elements of the 1027-element gradient
    assert bool(clip_and_step())
    after = snapshot()
    assert len(before) == len(after) and all(a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, after))
    params[1].grad[-1] = 0.0
    assert not bool(clip_and_step())
    assert not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, snapshot()))


# ------------------------------------------------------------------------------------------------ f. a3v_lora_refresh

@pytest.mark.parametrize("r,in_f,nj", [(1, 1, 1), (8, 255, 257), (16, 256, 256), (16, 4096, 300), (3, 513, 64)])
def test_lora_refresh(L, r, in_f, nj):
    """A, At, B, Bt = the bf16 rounding of the masters at exactly the owned rows and columns; every other element untouched."""
    rs = np.random.RandomState(r + in_f)
    wa = (rs.randn(r, in_f) * np.exp2(rs.uniform(-6, 6, (r, in_f)))).astype(np.float32)
    wb = (rs.randn(nj, r) * np.exp2(rs.uniform(-6, 6, (nj, r)))).astype(np.float32)
    col0, row0 = 5, 37
    rp, n_tot = col0 + r + 3, row0 + nj + 11
    lda, ldat, ldb, ldbt = in_f + 7, rp + 5, rp + 9, n_tot + 13
    shapes = [(rp, lda), (in_f + 2, ldat), (n_tot, ldb), (rp, ldbt)]
    want = [np.full(s, 0xDEAD, np.uint16) for s in shapes]
    O.emu_lora_refresh(wa, wb, r, in_f, nj, *want, col0, row0)
    WA, WB = Guarded(wa), Guarded(wb)
    imgs = [Guarded(s[0] * s[1], torch.int16) for s in shapes]
    rc = L.load().a3v_lora_refresh(WA.ptr, WB.ptr, r, in_f, nj, imgs[0].ptr, lda, imgs[1].ptr, ldat, imgs[2].ptr, ldb, imgs[3].ptr, ldbt, col0, row0, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, g, w in zip(("A", "At", "B", "Bt"), imgs, want):
        g.untouched(name)
        assert np.array_equal(g.host().view(np.uint16), w.reshape(-1)), name
    assert np.array_equal(WA.host(), wa.reshape(-1)) and np.array_equal(WB.host(), wb.reshape(-1))
