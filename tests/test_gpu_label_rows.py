"""The LoRA step with the last block's wo / FFN branch, the final norm, the head and the loss on the labelled rows only
(``TrainEngine.label_rows``) against the same step on every row (the switch off), in one process, and the kernels
underneath against torch indexing.

Tolerance of the step comparison.  Rows without a label contribute exact zeros, so on and off differ by fp32 summation order and by
bf16 roundings that fall differently (other row slices in the strip / TN planes, another GEMM plan at the smaller M).  The yardstick
is what the every-row path itself shows against the project's fp64 row-op reference (tests/rowops_ref.py) on that reference's own
inputs at this geometry's shape (rows = B S, dim 256): E = max |a3v_rmsnorm_bwd_bf16 - fp64| / max |fp64| over dh, the bf16 stream
gradient every gradient of the step is made from.  Tensors are compared with max |on - off| <= 2 E max |off|, the loss with
|on - off| <= 2 E |off|, and a bucket's sum of squares with |on - off| <= 2 E off.  E is measured in the test, on the switch-off
kernels, never on the new path.  Measured on MI355X (also in profiles/bench_notes.md): E = 2.81e-3 (dh, rows 182 x dim 256; dw
1.2e-7); worst |on - off| as a fraction of its bound, with the buckets at twice the bound used here: answer 0.007, two_segments
0.039, one_sample_empty 0.278, all_text / one_row / n17 / n33 0.000 (bit-identical gradients); the losses agree to 1e-6.
"""
import pytest
import torch

import rowops_ref as rr
from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5_peft as peft
from a3vlm_amd.train import TrainEngine, label_rows_ref
from a3vlm_amd.util import promote_trainable_params_to_fp32
from oracle import ref_cpu
from oracle.gen_golden import synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TINY = dict(dim=256, n_layers=2, n_heads=2, n_kv_heads=2, vocab_size=512, multiple_of=64, max_seq_len=512)
RANK, B, T = 8, 2, 24

def _labels(pattern, ex):
    """Labels [B, T] (before the shift: label p is read at text row p - 1) for a pattern of the issue."""
    lab = torch.zeros_like(ex)
    if pattern == "answer":                     # one contiguous answer per sample (the bench's pattern)
        lab[:, 9:] = ex[:, 9:]
    elif pattern == "two_segments":
        lab[0, 4:10] = ex[0, 4:10]
        lab[0, 15:] = ex[0, 15:]
        lab[1, 12:] = ex[1, 12:]
    elif pattern == "one_sample_empty":
        lab[1, 6:] = ex[1, 6:]
    elif pattern == "all_text":
        lab[:] = ex
    elif pattern == "one_row":
        lab[1, 7] = ex[1, 7]
    elif pattern == "n17":
        lab[0, 1:18] = ex[0, 1:18]
    elif pattern == "n33":
        lab[0, 1:] = ex[0, 1:]
        lab[1, 1:11] = ex[1, 1:11]
    elif pattern != "none":
        raise KeyError(pattern)
    return lab


PATTERNS = {"answer": 30, "two_segments": 27, "one_sample_empty": 18, "all_text": 46, "one_row": 1, "n17": 17, "n33": 33, "none": 0}


@pytest.fixture(scope="module")
def step():
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
    ex = torch.randint(3, TINY["vocab_size"], (B, T), generator=torch.Generator().manual_seed(11))
    ex[:, 0] = 1
    img = synth_image(B, size=112, seed=4).to(DEV)
    return m, eng, ex, img


@pytest.fixture(scope="module")
def parent_error(step):
    """E of the module docstring: the every-row path's own bf16 stream-gradient kernel against the fp64 reference, at rows = B S."""
    m = step[0]
    rows = B * (T + m.words_per_image)
    inp = rr.rmsnorm_bwd_inputs(rows, TINY["dim"])
    dh, dw = inp["dh0"].clone().to(DEV), inp["dw0"].clone().to(DEV)
    ops.rmsnorm_bwd(inp["x"].to(DEV), inp["w"].to(DEV), inp["dy"].to(DEV), dh, dw, rr.RMS_EPS)
    ref_dh, _, ref_dw, _ = rr.rmsnorm_bwd_ref(inp["x"], inp["w"], inp["dy"], inp["dh0"], inp["dw0"])
    e = float((dh.cpu().double() - ref_dh).abs().max() / ref_dh.abs().max())
    print(f"parent path vs fp64 (rmsnorm_bwd, rows {rows} x dim {TINY['dim']}): E_dh = {e:.3e}, "
          f"E_dw = {float((dw.cpu().double() - ref_dw).abs().max() / ref_dw.abs().max()):.3e}")
    assert 0 < e < 2.0 ** -7            # a bf16 result: about half an ulp of its largest element
    return e


def _run(eng, m, ex, lab, img, on):
    eng.label_rows = on
    for p in m.parameters():
        p.grad = None
    loss = eng.forward_loss(ex.to(DEV), lab.to(DEV), img)
    took = eng._saved["sel"] is not None
    eng.backward(1.0)
    flat = eng.flat_grads().detach().clone()
    sq = {b: float(flat[s:e].double().square().sum()) for b, s, e in eng.grad_ranges()}
    return float(loss), flat, sq, took


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_step_on_labelled_rows_matches_every_row(step, parent_error, pattern):
    m, eng, ex, img = step
    lab = _labels(pattern, ex)
    n = int((lab[:, 1:] != 0).sum())
    assert n == PATTERNS[pattern]
    loss0, flat0, sq0, took0 = _run(eng, m, ex, lab, img, False)
    loss1, flat1, sq1, took1 = _run(eng, m, ex, lab, img, True)
    assert not took0 and took1 == (n > 0)
    if n == 0:
        assert loss0 == 0.0 and loss1 == 0.0
        assert not bool(flat0.any()) and not bool(flat1.any())
        return
    tol = 2.0 * parent_error
    worst = abs(loss1 - loss0) / (tol * abs(loss0))
    print(f"{pattern}: n {n}  loss {loss0:.6f} / {loss1:.6f}  ratio to bound {worst:.3f}")
    assert worst <= 1.0
    assert float(flat0.abs().max()) > 0
    for name, p in m.get_trainable_params().items():
        o, _ = eng._offs[name]
        a, b = flat1[o:o + p.numel()], flat0[o:o + p.numel()]
        r = float((a - b).abs().max()) / (tol * float(b.abs().max()) + 1e-30)
        worst = max(worst, r)
        assert r <= 1.0, (pattern, name, r)
    for bucket in sq0:
        r = abs(sq1[bucket] - sq0[bucket]) / (tol * sq0[bucket] + 1e-30)
        worst = max(worst, r)
        assert r <= 1.0, (pattern, bucket, r)
    print(f"{pattern}: worst ratio to the bound over loss, {len(m.get_trainable_params())} gradients, {len(sq0)} buckets = {worst:.3f}")


# ------------------------------------------------------------------ the kernels against torch indexing
def _index(rows):
    """Ascending rows with gaps, from row 0 to the last row."""
    g = torch.Generator().manual_seed(rows)
    keep = torch.rand(rows, generator=g) < 0.4
    keep[0] = keep[rows - 1] = True
    keep[1:3] = False
    return torch.nonzero(keep).reshape(-1).to(torch.int32)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_label_rows_kernel_matches_nonzero(pattern):
    ex = torch.randint(3, 500, (B, T), generator=torch.Generator().manual_seed(2))
    lab = torch.zeros(B, T, dtype=torch.int64)
    lab[:, :T - 1] = _labels(pattern, ex)[:, 1:]
    W, S = 66, 66 + T
    outs = [torch.full((B * T,), -7, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.int64)]
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = ops.label_rows(lab.to(DEV), W, S, *outs, cnt)
    want = label_rows_ref(lab, W, S)
    pos = torch.nonzero(lab.reshape(-1)).reshape(-1)
    assert n == PATTERNS[pattern] == int(cnt) == pos.numel()
    assert torch.equal(want[1].long(), pos) and torch.equal(want[0].long(), (pos // T) * S + W + pos % T)
    for got, w in zip(outs, want):
        assert torch.equal(got[:n].cpu(), w)
        assert bool((got[n:] == -7).all())


def test_label_rows_kernel_longer_than_one_chunk():
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (5, 211), generator=g) * torch.randint(1, 900, (5, 211), generator=g)
    outs = [torch.zeros(5 * 211, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.int64)]
    n = ops.label_rows(lab.to(DEV), 3, 214, *outs, torch.zeros(1, dtype=torch.int32, device=DEV))
    want = label_rows_ref(lab, 3, 214)
    assert n == want[0].numel() > 256
    for got, w in zip(outs, want):
        assert torch.equal(got[:n].cpu(), w)


@pytest.mark.parametrize("rows,dim", [(37, 256), (300, 4096)])
def test_indexed_row_kernels_equal_the_plain_ones_on_gathered_rows(rows, dim):
    idx = _index(rows)
    n, li, di = idx.numel(), idx.long(), idx.to(DEV)
    inp = rr.rmsnorm_bwd_inputs(rows, dim)
    x, w, dh0, dw0 = inp["x"].to(DEV), inp["w"].to(DEV), inp["dh0"].to(DEV), inp["dw0"].to(DEV)
    dy = inp["dy"][:n].contiguous().to(DEV)
    # gather / scatter: bf16 and fp32, contiguous and inside a wider buffer
    for src in (x, x.float(), torch.cat([x, x[:, :64]], 1)[:, :dim]):
        got = ops.gather_rows(src, di, torch.empty(n, dim, dtype=src.dtype, device=DEV))
        assert torch.equal(got, src[li.to(DEV)])
        wide = torch.full((rows, dim + 64), float("nan"), dtype=src.dtype, device=DEV)
        ops.scatter_rows(got, di, wide[:, :dim])
        want = torch.zeros(rows, dim, dtype=src.dtype, device=DEV)
        want[li.to(DEV)] = got
        assert torch.equal(wide[:, :dim], want)                     # NaNs before: rows outside the list are zero now
        assert bool(torch.isnan(wide[:, dim:]).all())               # and nothing beyond the columns asked for was touched
    # rmsnorm on listed rows = rmsnorm of the gathered rows, bit for bit
    xg = x[li.to(DEV)].contiguous()
    y0 = ops.rmsnorm(xg, w, torch.empty(n, dim, dtype=BF, device=DEV), rr.RMS_EPS)
    y1 = ops.rmsnorm(x, w, torch.empty(n, dim, dtype=BF, device=DEV), rr.RMS_EPS, row_idx=di)
    assert torch.equal(y0, y1)
    # rmsnorm backward: compact dy, x and dh at the listed rows
    dh_c, dw_c = dh0[li.to(DEV)].contiguous(), dw0.clone()
    ops.rmsnorm_bwd(xg, w, dy, dh_c, dw_c, rr.RMS_EPS)
    dh_i, dw_i = dh0.clone(), dw0.clone()
    ops.rmsnorm_bwd(x, w, dy, dh_i, dw_i, rr.RMS_EPS, row_idx=di)
    # dh bit for bit.  dw: the same per-block partial rows, but a3v_rmsnorm_bwd's column sum adds its row chunks onto dw with atomics
    # in no fixed order, so two runs of the plain kernel may already differ in the last bits: both are held to the fp64 bound below,
    # and bit for bit where the order cannot matter -- one block (8 rows) onto dw = 0
    assert torch.equal(dh_i[li.to(DEV)], dh_c)
    one = [torch.zeros_like(dw0), torch.zeros_like(dw0)]
    ops.rmsnorm_bwd(xg[:8].contiguous(), w, dy[:8], dh0[li.to(DEV)][:8].contiguous(), one[0], rr.RMS_EPS)
    ops.rmsnorm_bwd(x, w, dy[:8], dh0.clone(), one[1], rr.RMS_EPS, row_idx=di[:8].contiguous())
    assert torch.equal(one[0], one[1]) and bool(one[0].any())
    rest = torch.ones(rows, dtype=torch.bool)
    rest[li] = False
    assert torch.equal(dh_i[rest.to(DEV)], dh0[rest.to(DEV)])       # rows outside the list keep their gradient
    ref_dh, mag_dh, ref_dw, mag_dw = rr.rmsnorm_bwd_ref(inp["x"][li], inp["w"], inp["dy"][:n], inp["dh0"][li], inp["dw0"])
    assert rr.within(dh_c, ref_dh, mag_dh, BF) <= 1.0
    assert rr.within(dw_c, ref_dw, mag_dw, torch.float32) <= 1.0 and rr.within(dw_i, ref_dw, mag_dw, torch.float32) <= 1.0
