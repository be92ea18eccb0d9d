"""The one-launch gradient finish (a3v_grad_finish_multi) against the kernels it replaces, and the engine with and without it.

Bounds.  The plane jobs (PLANES, SCATTER) do, element for element, what a3v_splitk_reduce<float> (+ a3v_lora_gb_scatter) does:
bit-equal.  A column-sum job keeps colsum_add_kernel's chunking: 16 chunk sums, formed the same way and hence the same bits, land on
the destination as atomics in no fixed order -- in the old kernel as in the new one.  Two orders of adding the n = 17 terms
(destination + 16 chunk sums) differ by at most 2 (n - 1) u sum|terms|, u = 2^-24, and sum|terms| <= |dst0| + A with A the column's
sum of |partial row| -- so |new - old| <= 32 u (|dst0| + A) (first order; 1 % is added for the higher orders).  Over micro-steps
k = 1.. the same argument gives 32 u sum_k sum_{j <= k} A_j from a zero start.  Against an exact (fp64) column sum the bound is the
plain fp32 summation bound over the row count, (rows + 16) u (|dst0| + A).
"""
import ctypes

import pytest
import torch

from a3vlm_amd import grad_finish as gf
from a3vlm_amd import lib as _l
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5_peft as peft
from a3vlm_amd.train import TrainEngine
from a3vlm_amd.util import promote_trainable_params_to_fp32
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U = 2.0 ** -24
NJS = {(256, 1): (256,), (256, 2): (100, 156), (256, 3): (100, 92, 64), (384, 1): (384,), (384, 2): (200, 184), (384, 3): (200, 120, 64)}


def _reduce_old(planes, out, accumulate):
    S, R, N = planes.shape
    rc = _l.load().a3v_splitk_reduce(planes.data_ptr(), S, R, N, out.data_ptr(), out.stride(0), _l.F32, 1 if accumulate else 0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _l.check(rc, "a3v_splitk_reduce")


def _rand(g, *shape):
    return (torch.randn(*shape, generator=g) * 3.0).to(DEV)


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("N", [256, 384])
@pytest.mark.parametrize("mods", [1, 2, 3])
def test_mixed_table_equals_the_old_kernels(S, N, mods):
    """One table with every kind of job: dA-like planes accumulated into a strided destination and stored, R = 64 dB^T planes whose
    16 / 32 / 48 used rows are scattered into 1 - 3 modules of unequal width, a ragged plane job, and column sums -- run on a grid
    larger than the unit count and on one of 3 blocks."""
    g = torch.Generator().manual_seed(1000 * S + N + mods)
    r, njs = 16, NJS[(N, mods)]
    nr = r * mods
    row0s = [sum(njs[:j]) for j in range(mods)]
    pl_a, pl_s, pl_b, pl_r = _rand(g, S, nr, N), _rand(g, S, nr, N), _rand(g, S, 64, N), _rand(g, S, 20, 260)
    parts, parts5 = _rand(g, 37, 384), _rand(g, 5, 1280)                      # 37 rows: ragged chunks; 5 rows: most chunks empty
    d_a, d_s, d_r = _rand(g, nr, N + 8), torch.full((nr, N), float("nan"), device=DEV), _rand(g, 20, 264)
    d_b = [_rand(g, n, r) for n in njs]
    d_c, d_c5 = _rand(g, 384), _rand(g, 1280)
    # ---- the old kernels
    o_a, o_s, o_r, o_b = d_a.clone(), d_s.clone(), d_r.clone(), [d.clone() for d in d_b]
    _reduce_old(pl_a, o_a[:, :N], True)
    _reduce_old(pl_s, o_s, False)
    _reduce_old(pl_r, o_r[:, :260], True)
    gbt = torch.empty(64, N, device=DEV)
    _reduce_old(pl_b, gbt, False)
    ops.lora_gb_scatter(gbt, r, o_b, row0s)
    # ---- the table
    arena_parts = [pl_a, pl_s, pl_b, pl_r, parts, parts5]
    def run(max_blocks):
        n_a, n_s, n_r, n_b, n_c, n_c5 = d_a.clone(), d_s.clone(), d_r.clone(), [d.clone() for d in d_b], d_c.clone(), d_c5.clone()
        p = gf.FinishPlan(1 << 30)
        p.add_planes("a", nr, N, S, n_a.data_ptr(), n_a.stride(0), True)
        p.add_planes("s", nr, N, S, n_s.data_ptr(), N, False)
        p.add_scatter("b", 64, N, S, r, [d.data_ptr() for d in n_b], row0s, njs)
        p.add_planes("r", 20, 260, S, n_r.data_ptr(), 264, True)
        p.add_colsum("c", 37, 384, n_c.data_ptr())
        p.add_colsum("c5", 5, 1280, n_c5.data_ptr())
        f = gf.GradFinisher(1 << 30, 0)
        f.plan = p
        assert f.commit(DEV)
        for key, src in zip(("a", "s", "b", "r", "c", "c5"), arena_parts):
            f.slice_of(p.slots[key], src.numel()).copy_(src.reshape(-1))
        f.pending = {"a": S, "s": S, "b": S, "r": S, "c": 37, "c5": 5}
        units = p.rows(f.pending, f.arena.data_ptr())[1]
        f.launch(max_blocks)
        torch.cuda.synchronize()
        return units, n_a, n_s, n_r, n_b, n_c, n_c5

    for max_blocks in (0, 3):
        units, n_a, n_s, n_r, n_b, n_c, n_c5 = run(max_blocks)
        assert 3 < units < 4 * torch.cuda.get_device_properties(0).multi_processor_count       # fewer units than blocks / more than 3
        assert torch.equal(n_a, o_a) and torch.equal(n_s, o_s) and torch.equal(n_r, o_r)       # (padding columns untouched too)
        for j in range(mods):
            assert torch.equal(n_b[j], o_b[j]), f"module {j}"
        for new, d0, pr in ((n_c, d_c, parts), (n_c5, d_c5, parts5)):
            exact = d0.double() + pr.double().sum(0)
            bound = (pr.shape[0] + 16) * U * 1.01 * (d0.abs().double() + pr.abs().double().sum(0))
            err = (new.double() - exact).abs()
            print(f"S={S} N={N} mods={mods} blocks={max_blocks}: colsum rows {pr.shape[0]} max err/bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all())


@pytest.mark.parametrize("rows,dim,accumulate", [(46, 256, True), (200, 384, False), (1091, 4096, True)])
def test_norm_partials_plus_finish_equal_rmsnorm_bwd(rows, dim, accumulate):
    """a3v_rmsnorm_bwd_parts_bf16 + a COLSUM job against a3v_rmsnorm_bwd_bf16 (partial rows + colsum_add_kernel): dh bit-equal, dw within
    the atomic-order bound of the module docstring (A read from the partial rows)."""
    g = torch.Generator().manual_seed(rows + dim)
    x, dy, dh0 = (_rand(g, rows, dim).to(BF) for _ in range(3))
    w = (1.0 + 0.1 * torch.randn(dim, generator=g)).to(DEV)
    dw0 = _rand(g, dim) if accumulate else torch.zeros(dim, device=DEV)
    dh_o, dw_o = dh0.clone(), dw0.clone()
    ops.rmsnorm_bwd(x, w, dy, dh_o, dw_o, 1e-5)
    dh_n, dw_n = dh0.clone(), dw0.clone()
    nb = (rows + 7) // 8
    fin = gf.GradFinisher(1 << 30, 0)
    fin.plan.add_colsum("n", nb + 3, dim, dw_n.data_ptr())
    assert fin.commit(DEV)
    parts = fin.slice_of(fin.plan.slots["n"], nb * dim)
    ops.rmsnorm_bwd_parts(x, w, dy, dh_n, parts, 1e-5)
    fin.pending = {"n": nb}
    fin.launch()
    torch.cuda.synchronize()
    assert torch.equal(dh_n, dh_o)
    A = parts.view(nb, dim).abs().double().sum(0)
    bound = 32 * U * 1.01 * (dw0.abs().double() + A)
    err = (dw_n.double() - dw_o.double()).abs()
    print(f"rows {rows} dim {dim}: dw max |new - old| / bound = {float((err / bound).max()):.3f}, equal bits: {torch.equal(dw_n, dw_o)}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------- the engine with and without it
TINY = dict(dim=256, n_layers=2, n_heads=2, n_kv_heads=2, vocab_size=512, multiple_of=64, max_seq_len=512)
RANK, B, T = 16, 2, 100               # 200 rows: not a multiple of 64, four token slices per strip


@pytest.fixture(scope="module")
def tiny():
    args = peft.ModelArgs(**TINY, lora_rank=RANK, vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1)
    m = peft.Transformer(args, with_visual=True)
    oargs = ref_cpu.OracleArgs(**TINY)
    sd = ref_cpu.make_decoder_weights(oargs, seed=0, std=0.08)
    lsd = ref_cpu.make_lora_weights(oargs, RANK, seed=5, std_a=0.05, std_b=0.05)
    vsd = ref_cpu.make_vision_weights(TINY["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    m.load_state_dict({**sd, **lsd, **vsd}, strict=True)
    train = m.get_trainable_params()
    for n, p in m.named_parameters():
        p.requires_grad = n in train
    m.to(BF).to(DEV)
    promote_trainable_params_to_fp32(m)
    eng = TrainEngine(m, BF, recompute=False)
    gen = torch.Generator().manual_seed(11)
    micro = []
    for first in (T // 2, 31):                             # labels from here on: 98 and 136 labelled rows of 200
        ex = torch.randint(3, TINY["vocab_size"], (B, T), generator=gen)
        ex[:, 0] = 1
        lab = ex.clone()
        lab[:, :first] = 0
        micro.append((ex.to(DEV), lab.to(DEV)))
    return m, eng, micro


def _steps(m, eng, micro, defer, budget=gf.DEFAULT_BUDGET):
    """Gradients of a cycle over the micro-steps ``micro`` with the deferred finish on / off.  (An engine's first backward only plans
    the arena, so one un-measured backward goes first either way.)  Returns losses, named gradients, and per norm weight the bound
    32 u sum_k sum_{j <= k} A_j of the module docstring (deferred runs only)."""
    eng.finish_defer, eng.finish_budget, eng._fin = defer, budget, None
    eng.forward_loss(*micro[0])
    eng.backward(1.0)
    for p in m.parameters():
        p.grad = None
    losses, A_sum, bound = [], {}, {}
    for ex, lab in micro:
        losses.append(eng.forward_loss(ex, lab).clone())
        eng.backward(1.0 / len(micro))
        if eng._fin is not None and eng._fin.arena is not None:
            for key, slot in eng._fin.plan.slots.items():
                if slot.kind == gf.COLSUM:
                    rows = eng._fin.last_counts[key]
                    A = eng._fin.slice_of(slot, rows * slot.N).view(rows, slot.N).abs().double().sum(0)
                    A_sum[key] = A_sum.get(key, 0) + A
                    bound[key] = bound.get(key, 0) + 32 * U * 1.01 * A_sum[key]
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}
    return losses, grads, bound


def _norm_key(name):
    if name == "norm.weight":
        return "norm"
    _, i, sub, _ = name.split(".")
    return (int(i), sub)


def _compare(m, eng, micro):
    l0, g0, _ = _steps(m, eng, micro, defer=False)
    assert eng._fin is None
    l1, g1, bound = _steps(m, eng, micro, defer=True)
    fin = eng._fin
    assert fin is not None and fin.arena is not None and not fin.pending
    jobs = {k for k in fin.plan.slots}
    L = TINY["n_layers"]
    assert len(jobs) == L * (4 * 2 + 2) + 1               # per layer: four groups' dA and dB^T strips, two norms; the final norm
    assert set(fin.last_counts) == jobs                 # ... and every one of them ran through the finish launch
    assert g0.keys() == g1.keys()
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    n_norm = 0
    for name in g0:
        if "lora_" in name:
            assert torch.equal(g0[name], g1[name]), name
        elif name == "norm.weight" or (name.startswith("layers.") and name.endswith("norm.weight")):
            err = (g0[name].double() - g1[name].double()).abs()
            bd = bound[_norm_key(name)]
            print(f"{name}: max |defer - per-call| / bound = {float((err / bd.clamp_min(1e-300)).max()):.3f}, equal bits: {torch.equal(g0[name], g1[name])}")
            assert bool((err <= bd).all()), name
            n_norm += 1
    assert n_norm == 2 * L + 1
    return fin


def test_engine_step_equals_per_call_finish(tiny):
    m, eng, micro = tiny
    fin = _compare(m, eng, micro[:1])
    assert fin.tables_built == 1                          # the planning backward launches nothing; one step shape, one table


def test_engine_accumulation_equals_per_call_finish(tiny):
    m, eng, micro = tiny
    fin = _compare(m, eng, micro)
    assert fin.tables_built == 2                          # the two micro-steps label different row counts


def test_engine_falls_back_when_the_arena_exceeds_its_budget(tiny):
    m, eng, micro = tiny
    l0, g0, _ = _steps(m, eng, micro[:1], defer=False)
    l1, g1, _ = _steps(m, eng, micro[:1], defer=True, budget=1 << 16)
    assert eng._fin is not None and eng._fin.plan.closed and not eng._fin.plan.fits and eng._fin.arena is None
    assert eng._fin.plan.bytes > 1 << 16 and eng._fin.tables_built == 0
    assert torch.equal(l0[0], l1[0])
    for name in g0:
        if "lora_" in name:
            assert torch.equal(g0[name], g1[name]), name
    eng.finish_budget = gf.DEFAULT_BUDGET
