"""CPU self-check of tests/optim_ref.py: the correct float32 emulations of the optimizer kernels stay inside the derived bounds on
every bounded case and are bit-equal to the closed form on every exact case, in the contracted and the uncontracted form; every
wrong variant of the list fails in at least one exact group and one bounded group where it applies; and the parameter-only bound of
test_fused_adamw_matches_torch_adamw lets some of them through on that test's own inputs."""
import numpy as np
import pytest
import torch

import optim_ref as O

FORMS = ("plain", "fma_a", "fma_b")
SENT = 0xDEAD
EXACT_GROUPS = [(wd, st, coef) for wd in (0.0, 0.5) for st in (False, True) for coef in (None, 0.5)] + [(0.5, True, -0.5)]
BOUNDED_GROUPS = [(h, coef) for h in O.bounded_hypers() for coef in O.COEFS] + [(O.bounded_hypers()[3], -0.37)]
# where a wrong variant cannot show: eps = 0 in the exact groups; a power-of-two coefficient makes the product exact
NOT_APPLICABLE = {("eps_before_bc", "exact"), ("coef_unrounded", "exact")}


def _np(case):
    return {k: t.numpy() for k, t in case.items()}


def _exact(n, wd, st, coef):
    """Inputs and expected (p, m, v, image bits) of an exact group; a negative coefficient: everything as it was."""
    c = _np(O.exact_case(n, wd, st, coef=abs(coef) if coef is not None else None))
    if coef is not None and coef < 0:
        return c, (c["p"], c["m"], c["v"], np.full(n, SENT, np.uint16))
    return c, (c["p1"], c["m1"], c["v1"], O.bf16_bits(c["p1"]))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def exact_group_passes(n, wd, st, coef, form="plain", mut=None):
    c, want = _exact(n, wd, st, coef)
    got = O.emu_adamw_flat(c["p"], c["g"], c["m"], c["v"], O.exact_hyper(wd), coef, form, mut, SENT)
    return all(_same(a, b) for a, b in zip(got, want))


def bounded_group(n, seed, h, coef, form="plain", mut=None):
    """-> (passes, (ratio p, ratio m, ratio v)) of the emulation against the float64 reference and the derived bounds."""
    p, g, m, v = O.bounded_inputs(n, seed, eps=h.eps)
    ref = O.adamw_ref(p, g, m, v, h, coef)
    Ep, Em, Ev = O.adamw_bounds(ref, h)
    pn, mn, vn, img = O.emu_adamw_flat(p, g, m, v, h, coef, form, mut, SENT)
    ratios = (O.ratio(pn, ref["p"], Ep), O.ratio(mn, ref["m"], Em), O.ratio(vn, ref["v"], Ev))
    want_img = np.full(n, SENT, np.uint16) if ref["skipped"] else O.bf16_bits(pn)      # the image: the rounding of the kernel's own p'
    ok = all(np.isfinite(a).all() for a in (pn, mn, vn)) and max(ratios) <= 1.0 and _same(img, want_img)
    return ok, ratios


@pytest.mark.parametrize("form", FORMS)
def test_correct_emulation_is_bit_equal_on_exact_inputs(form):
    for wd, st, coef in EXACT_GROUPS:
        assert exact_group_passes(100003, wd, st, coef, form), (wd, st, coef)


@pytest.mark.parametrize("form", FORMS)
def test_correct_emulation_is_inside_the_bounds(form):
    worst = [0.0, 0.0, 0.0]
    for i, (h, coef) in enumerate(BOUNDED_GROUPS):
        ok, ratios = bounded_group(4099, i, h, coef, form)
        assert ok, (h, coef, ratios)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    print(f"\n[optim_ref] {form}: largest err/bound over {len(BOUNDED_GROUPS)} cases: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert max(worst) > 0.05          # the bounds are of the size of the error, not orders above it


def test_zero_gradient_from_zero_state_is_a_zero_update():
    h = O.Hyper(3e-3, 0.9, 0.95, 1e-8, 0.0, 1)
    z = np.zeros(8, np.float32)
    p = np.arange(8, dtype=np.float32)
    ref = O.adamw_ref(p, z, z, z, h)
    assert np.array_equal(ref["p"], p) and not np.isnan(ref["p"]).any()
    assert all((b == 0).all() for b in O.adamw_bounds(ref, h))
    pn, mn, vn = O.emu_update(p, z, z, z, h)
    assert _same(pn, p) and not mn.any() and not vn.any()


ARITH = ["eps_before_bc", "bc2_missing", O.MUTATION_2B, "bc1_prev_step", "l2_decay", "decay_after_update", "coef_m_only", "coef_twice_in_v",
         "coef_unrounded", "neg_coef_abs"]
STRUCT = ["tail_skipped", "trip_last_vector_skipped", "lanes_rotated", "image_truncated", "image_pre_update"]


@pytest.mark.parametrize("mut", ARITH + STRUCT)
def test_wrong_update_fails(mut):
    assert mut == O.MUTATION_2B or mut in O.MUTATIONS.values()
    if (mut, "exact") not in NOT_APPLICABLE:
        failed = [g for g in EXACT_GROUPS if not exact_group_passes(4103, *g, mut=mut)]
        assert failed, f"{mut} passes every exact group"
    failed = [i for i, (h, coef) in enumerate(BOUNDED_GROUPS) if not bounded_group(1031, i, h, coef, mut=mut)[0]]
    assert failed, f"{mut} stays inside the bounds of every bounded group"
    print(f"\n[optim_ref] {mut}: fails {len(failed)} of {len(BOUNDED_GROUPS)} bounded groups")


def test_not_applicable_really_is():
    """The two exemptions are facts of the inputs, not gaps: with eps = 0 the eps placement is invisible, and a power-of-two
    coefficient makes the scaled gradient exact."""
    for mut, _ in NOT_APPLICABLE:
        assert all(exact_group_passes(4103, *g, mut=mut) for g in EXACT_GROUPS)


def _image_bits(kind, rows, cols):
    if kind == "exact":
        return O.bf16_bits(_np(O.exact_case(rows * cols, 0.5, True))["p1"])
    p, g, m, v = O.bounded_inputs(rows * cols, 5)
    return O.bf16_bits(O.emu_update(p, g, m, v, O.bounded_hypers()[0], 0.37)[0])


@pytest.mark.parametrize("mut", ["t_rc_swapped", "t_row_offset_dropped"])
@pytest.mark.parametrize("kind", ["exact", "bounded"])
def test_wrong_transposed_image_fails(mut, kind):
    hit = 0
    for rows, cols in ((64, 64), (128, 64), (192, 128), (320, 192)):
        bits = _image_bits(kind, rows, cols)
        want = np.full((cols, rows + 4), SENT, np.uint16)
        want[:, :rows] = bits.reshape(rows, cols).T                       # the plain statement: imgt[c][r] = img[r][c]
        assert _same(O.emu_image_t(bits, rows, cols, rows + 4, None, SENT), want)
        hit += not _same(O.emu_image_t(bits, rows, cols, rows + 4, mut, SENT), want)
    assert hit >= 2            # (64, 64) and (128, 64) are one tile row: a dropped row offset cannot show there


SUMSQ_N = [1, 3, 4, 5, 1023, 1024, 1025, 1027, 1048572, 1048576, 1048580, 1048576 + 1027]


def _sumsq_bounded_input(n, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randn(n) * np.exp2(rs.uniform(-8, 8, n))).astype(np.float32)


def test_sumsq_emulation_exact_and_bounded():
    worst = 0.0
    for n in SUMSQ_N:
        x = O.sumsq_exact_input(n, n)
        assert _same(O.emu_sumsq(x), O.sumsq_ref(x).astype(np.float32)), n
        x = _sumsq_bounded_input(n, n)
        ref = O.sumsq_ref(x)
        r = O.ratio(O.emu_sumsq(x), ref, O.sumsq_bound(x, ref))
        assert r <= 1.0, (n, r)
        worst = max(worst, r)
    print(f"\n[optim_ref] sumsq: largest err/bound per slot {worst:.3f}")
    total = sum(float(v) ** 2 for v in O.sumsq_exact_input(1027, 1))
    assert float(O.sumsq_ref(O.sumsq_exact_input(1027, 1)).sum()) == total


@pytest.mark.parametrize("mut", ["sumsq_tail_dropped", "sumsq_slot_to_neighbour"])
def test_wrong_sumsq_fails(mut):
    for n in (1027, 1048576 + 1027):
        x = O.sumsq_exact_input(n, 3)
        assert not _same(O.emu_sumsq(x, mut), O.sumsq_ref(x).astype(np.float32)), n
        x = _sumsq_bounded_input(n, 3)
        ref = O.sumsq_ref(x)
        assert O.ratio(O.emu_sumsq(x, mut), ref, O.sumsq_bound(x, ref)) > 1.0, n


def test_lora_refresh_emulation_writes_only_the_owned_rows_and_columns():
    r, in_f, nj, col0, row0 = 3, 9, 5, 2, 4
    rs = np.random.RandomState(0)
    wa, wb = rs.randn(r, in_f).astype(np.float32), rs.randn(nj, r).astype(np.float32)
    A, At, B, Bt = (np.full(s, SENT, np.uint16) for s in ((8, 12), (in_f + 1, 8), (12, 8), (8, 16)))
    O.emu_lora_refresh(wa, wb, r, in_f, nj, A, At, B, Bt, col0, row0)
    assert (A != SENT).sum() == r * in_f == (At != SENT).sum() and (B != SENT).sum() == r * nj == (Bt != SENT).sum()
    assert A[col0 + 1, 4] == O.bf16_bits(wa)[1, 4] == At[4, col0 + 1] and B[row0 + 2, col0] == O.bf16_bits(wb)[2, 0] == Bt[col0, row0 + 2]


def test_old_parameter_only_bound_lets_wrong_variants_through():
    """test_fused_adamw_matches_torch_adamw compares parameters only, with max|a - b| <= 2e-6 max|a| + 1e-7 per tensor, on four N(0, 1)
    tensors over five steps with lr 3e-3, betas (0.9, 0.95), eps 1e-8.  On those very inputs these wrong variants stay inside it
    (the moments are never looked at, and no coefficient is ever passed): the gap the parity tests close."""
    gen = torch.Generator().manual_seed(1)
    shapes = [(300, 257), (4096,), (7,), (64, 64)]
    p0 = [torch.randn(*s, generator=gen).numpy().reshape(-1) for s in shapes]
    grads = [[(torch.randn(*s, generator=gen) * (0.1 + it)).numpy().reshape(-1) for s in shapes] for it in range(5)]
    wds = [0.1, 0.1, 0.0, 0.0]

    def run(mut):
        state = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in p0]
        out = []
        for it in range(5):
            for k in range(4):
                p, m, v = state[k]
                state[k] = O.emu_update(p, grads[it][k], m, v, O.Hyper(3e-3, 0.9, 0.95, 1e-8, wds[k], it + 1), None, "plain", mut)
            out.append([s[0].copy() for s in state])
        return out

    good = run(None)
    through, not_exercised = [], []
    for mut in ARITH:
        bad = run(mut)
        if all(np.array_equal(a, b) for sa, sb in zip(good, bad) for a, b in zip(sa, sb)):
            not_exercised.append(mut)           # the test passes no coefficient: these variants compute the same there
        elif all(float(np.abs(a - b).max()) <= 2e-6 * float(np.abs(a).max()) + 1e-7 for sa, sb in zip(good, bad) for a, b in zip(sa, sb)):
            through.append(mut)
    print(f"\n[optim_ref] the old parameter-only bound lets through: {through}; never exercised by that test: {not_exercised}")
    assert "decay_after_update" in through and len(through) >= 1
    assert set(not_exercised) == {"coef_m_only", "coef_twice_in_v", "coef_unrounded", "neg_coef_abs"}
    # and the derived bounds do not, on the same inputs (first step, first tensor)
    h = O.Hyper(3e-3, 0.9, 0.95, 1e-8, 0.1, 1)
    z = np.zeros_like(p0[0])
    ref = O.adamw_ref(p0[0], grads[0][0], z, z, h)
    Ep, Em, Ev = O.adamw_bounds(ref, h)
    pn, mn, vn = O.emu_update(p0[0], grads[0][0], z, z, h, None, "plain", "decay_after_update")
    assert O.ratio(pn, ref["p"], Ep) > 1.0
