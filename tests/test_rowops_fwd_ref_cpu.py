"""CPU: the fp64 references of tests/rowops_fwd_ref.py against the torch fp64 expression of the same op (a), every input set of
tests/test_gpu_rowops_fwd.py through an fp32 restatement of the kernel's formula (b) -- a correct fp32 implementation stays inside
the derived bounds on exactly these inputs, so a GPU failure there is the kernel's -- the cross-entropy bound against the
tolerances of tests/test_gpu_kernels.py::test_cross_entropy (c), and the generation-step reference against ref_cpu.generate_greedy (d)."""
from types import SimpleNamespace
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import rowops_fwd_ref as R
from a3vlm_amd.model.LLM.llama_ens5 import precompute_cos_sin
from oracle import ref_cpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max())


def oracle_in_fp64():
    """ref_cpu.rmsnorm / apply_rotary_emb compute in ``x.float()``: inside this context that is fp64"""
    return mock.patch.object(torch.Tensor, "float", lambda self: self.double())


def cos_sin_table(hd):
    return precompute_cos_sin(hd, R.ROPE_TABLE, 10000.0, None)


# ------------------------------------------------------------------ (a) the references are the torch fp64 ops
def test_rmsnorm_ref_is_oracle_fp64():
    d = R.rmsnorm_inputs(37, 136, BF, F32)
    with oracle_in_fp64():
        want = ref_cpu.rmsnorm(d["x"].to(F64), d["w"].to(F64), R.RMS_EPS)
    ref, mag = R.rmsnorm_ref(d["x"], d["w"])
    assert want.dtype == F64 and rel(ref, want) < 1e-12 and torch.equal(mag, ref.abs())
    assert bool((ref[1] == 0).all())
    assert R.rmsnorm_rel(BF, BF) == 2.0 ** -7 + 2.0 ** -16 and R.rmsnorm_rel(F32, BF) == 2.0 ** -8 and R.rmsnorm_rel(F32, F32) == 0.0


@pytest.mark.parametrize("offset_sd", R.LN_OFFSETS)
def test_layernorm_ref_is_torch_fp64(offset_sd):
    d = R.layernorm_inputs(R.LN_ROWS, 1032, offset_sd, BF, F32)
    x64 = d["x"].to(F64)
    want = F.layer_norm(x64, (1032,), d["w"].to(F64), d["b"].to(F64), R.LN_EPS)
    ref, mag = R.layernorm_ref(d["x"], d["w"], d["b"])
    assert rel(ref, want) < 1e-12 and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    off = (x64.mean(-1).abs() / x64.std(-1)).min()
    assert float(off) >= 0.9 * offset_sd                      # the rows are as far off zero as the case says (after the bf16 rounding)


@pytest.mark.parametrize("hd", R.ROPE_HD)
def test_rope_ref_is_oracle_fp64(hd):
    S, p0 = 5, 40
    B, H, Hkv = R.ROPE_B, R.ROPE_H, R.ROPE_HKV
    cs = cos_sin_table(hd)
    fc = ref_cpu.precompute_freqs_cis(hd, R.ROPE_TABLE)
    assert torch.equal(cs[..., 0], fc.real) and torch.equal(cs[..., 1], fc.imag)
    qkv = R.rope_inputs(S, hd, BF)
    t = qkv.to(F64).view(B, S, H + 2 * Hkv, hd)
    with oracle_in_fp64():
        oq, ok = ref_cpu.apply_rotary_emb(t[:, :, :H], t[:, :, H:H + Hkv], fc[p0:p0 + S])
    ref, mag, v = R.rope_ref(qkv, cs, S, hd, p0)
    assert oq.dtype == F64 and rel(ref[:, :, :H], oq) < 1e-12 and rel(ref[:, :, H:], ok) < 1e-12
    assert torch.equal(v, qkv.view(B, S, -1, hd)[:, :, H + Hkv:]) and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # the table row is rope_pos0 + s, whatever the cache position: another rope_pos0 gives another result
    assert rel(R.rope_ref(qkv, cs, S, hd, 5)[0], ref) > 1e-2


def test_copy_references_are_the_torch_ops():
    """vt_pack, embedding, vit_embed, im2col and the quadrant views, each against a second way to write it"""
    qkv = R.vt_pack_inputs(77, 80, BF)
    vt = R.vt_pack_ref(qkv, 77, 80, 128)
    v = qkv[:, 2 * R.VT_H * 80:].view(R.VT_N, 77, R.VT_H, 80)
    assert vt.shape == (R.VT_N, R.VT_H, 80, 128) and float(vt[..., 77:].abs().sum()) == 0
    assert all(torch.equal(vt[n, h, :, l], v[n, l, h]) for n in range(R.VT_N) for h in range(R.VT_H) for l in (0, 63, 64, 76))

    d = R.embed_inputs(8, F32)
    tok = d["tokens"]
    assert int(tok.min()) == -1 and int(tok.max()) == R.EMBED_V
    h = R.embed_ref(tok, d["table"], 7, BF)
    emb = F.embedding(tok.clamp(0, R.EMBED_V - 1), d["table"]).to(BF)
    assert torch.equal(h[:, 0], emb[:, 0]) and torch.equal(h[:, 8:], emb[:, 1:]) and bool((h[:, 1:8] == R.SENT).all())
    assert torch.equal(h[0, 8], d["table"][0].to(BF)) and torch.equal(h[1, 10], d["table"][R.EMBED_V - 1].to(BF))

    for dtype in (BF, F32):
        d = R.vit_embed_inputs(16, 64, dtype)
        want = torch.cat([d["cls"].expand(R.VIT_N, 1, 64), d["patch"].view(R.VIT_N, 16, 64)], dim=1) + d["pos"]      # torch's own add in dtype
        assert torch.equal(R.vit_embed_ref(d["patch"], d["cls"], d["pos"], 16), want)

    for P, (gh, g) in ((14, (2, 5)), (16, (2, 5)), (14, (16, 16))):
        img = R.im2col_inputs(P, gh, g, F32)
        K = 3 * P * P
        want = F.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, K)
        for Kpad in R.im2col_kpads(P):
            cols = R.im2col_ref(img, P, Kpad, F32)
            assert torch.equal(cols[:, :K], want) and float(cols[:, K:].abs().sum()) == 0
    assert R.im2col_kpads(14) == [588, 640] and R.im2col_kpads(16) == [768, 832]

    img = R.split_inputs(2, 7, F32)
    assert torch.equal(R.split_quadrants_ref(img, F32), ref_cpu.split_views(img, 7)[2:])


@pytest.mark.parametrize("B,c", R.SPLIT_SHAPES[:2])
def test_bicubic_ref_is_torch_fp64(B, c):
    img = R.split_inputs(B, c, F32)
    want = F.interpolate(img.half().to(F64), size=(c, c), mode="bicubic")
    ref, mag = R.bicubic_ref(img)
    assert rel(ref, want) < 1e-12 and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # and the oracle's fp16 evaluation is inside the bound of an fp32 output
    assert R.bicubic_within(ref_cpu.split_views(img, c)[:B], img, F32) <= 1.0


@pytest.mark.parametrize("V", R.ARGMAX_V)
def test_argmax_ref_is_torch(V):
    lg, want = R.argmax_inputs(V)
    assert torch.equal(torch.argmax(lg, dim=-1), want)


@pytest.mark.parametrize("rows,V", R.CE_SHAPES[:4])
def test_ce_ref_is_torch_fp64(rows, V):
    d = R.ce_inputs(rows, V, BF)
    lab = d["labels"]
    nv = R.ce_n_valid(lab)
    x = d["logits"].to(F64).requires_grad_(True)
    want = F.cross_entropy(x, lab, ignore_index=0, reduction="none")
    g = float(torch.tensor(1.0 / 3.0, dtype=F32)) / nv
    (want.sum() * g).backward()
    loss, mag_loss, dl, mag_d, _ = R.ce_ref(d["logits"], lab, 1.0 / 3.0, nv)
    assert rel(loss, want) < 1e-12 and rel(dl, x.grad) < 1e-12
    assert float(loss[2]) == 0.0 and float(dl[2].abs().sum()) == 0.0
    assert abs(float(loss[1]) - torch.log(torch.tensor(float(V), dtype=F64)).item()) < 1e-12         # the flat row
    assert float(loss[0]) > 50.0                                                                      # the spike row, labelled off the spike


def test_ce_ref_out_of_range_labels_are_ignored_rows():
    d = R.ce_bad_label_inputs(7, 8, F32)
    assert d["labels"][:5].tolist() == [-100, -1, 0, 8, 13]
    nv = R.ce_n_valid(d["labels"])
    assert nv == 6
    loss, mag_loss, dl, mag_d, _ = R.ce_ref(d["logits"], d["labels"], 1.0, nv)
    assert float(loss[:5].abs().sum()) == 0 and float(dl[:5].abs().sum()) == 0 and float(mag_d[:5].sum()) == 0
    assert bool((loss[5:] > 0).all())
    one = R.ce_one_valid_inputs(5, 255, F32)
    assert R.ce_n_valid(one["labels"]) == 1


# ------------------------------------------------------------------ (b) a correct fp32 implementation is inside the bounds
@pytest.mark.parametrize("key", sorted(R.RMS_KEYS))
def test_rmsnorm_fp32_emulation_within_bounds(key):
    xd, wd, yd = R.RMS_KEYS[key]
    worst = 0.0
    for dim in R.RMS_DIMS:
        for rows in R.RMS_ROWS:
            d = R.rmsnorm_inputs(rows, dim, xd, wd)
            ref, mag = R.rmsnorm_ref(d["x"], d["w"])
            worst = max(worst, R.within(R.emu_rmsnorm(d["x"], d["w"], yd), ref, mag, yd, rel=R.rmsnorm_rel(xd, yd)))
            if xd == BF:                       # the bits of the specified rounding order, where fp32 cannot move them
                want, decided = R.rmsnorm_exact(d["x"], d["w"], yd)
                assert torch.equal(R.emu_rmsnorm(d["x"], d["w"], yd)[decided], want[decided]) and float(decided.float().mean()) > 0.99
                xf = d["x"].float()
                one_rounding = (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + R.RMS_EPS) * d["w"].float()).to(yd)
                if dim >= 136:                 # a kernel without the intermediate rounding is inside the fp64 bound and is caught here
                    assert not torch.equal(one_rounding[decided], want[decided])
    for n_src, dim, idx in R.RMS_IDX_CASES:
        d = R.rmsnorm_inputs(n_src, dim, BF, wd)
        ref, mag = R.rmsnorm_ref(d["x"][idx], d["w"])
        worst = max(worst, R.within(R.emu_rmsnorm(d["x"][idx], d["w"], BF), ref, mag, BF, rel=R.rmsnorm_rel(BF, BF)))
    print(f"rmsnorm key {key}: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("key", sorted(R.LN_KEYS))
def test_layernorm_fp32_emulation_within_bounds(key):
    xd, pd, yd = R.LN_KEYS[key]
    worst = 0.0
    for dim in R.LN_DIMS:
        for off in R.LN_OFFSETS:
            d = R.layernorm_inputs(R.LN_ROWS, dim, off, xd, pd)
            ref, mag = R.layernorm_ref(d["x"], d["w"], d["b"])
            worst = max(worst, R.within(R.emu_layernorm(d["x"], d["w"], d["b"], yd), ref, mag, yd))
    print(f"layernorm key {key}: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("hd", R.ROPE_HD)
def test_rope_fp32_emulation_within_bounds(hd, dtype):
    cs = cos_sin_table(hd)
    worst = 0.0
    for S in R.ROPE_S:
        qkv = R.rope_inputs(S, hd, dtype)
        for rp in sorted({rp for _, rp, _ in R.rope_cases(S)}):
            ref, mag, _ = R.rope_ref(qkv, cs, S, hd, rp)
            worst = max(worst, R.within(R.emu_rope(qkv, cs, S, hd, rp), ref, mag, dtype))
    assert sum(sp != rp for sp, rp in R.ROPE_POS) >= 2 and all(len(R.rope_cases(S)) >= 5 for S in R.ROPE_S)
    print(f"rope hd {hd} {dtype}: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("key", sorted(R.SPLIT_KEYS))
def test_bicubic_fp32_emulation_within_bounds(key):
    in_dtype, out_dtype = R.SPLIT_KEYS[key]
    for B, c in R.SPLIT_SHAPES:
        img = R.split_inputs(B, c, in_dtype)
        r = R.bicubic_within(R.emu_bicubic(img, out_dtype), img, out_dtype)
        print(f"bicubic key {key} ({B}, {c}): {r:.3f}")
        assert r <= 1.0
    assert 5 * 3 * 3 * 224 * 224 > 8192 * 256


def ce_ratios(d, scale, dtype):
    nv = R.ce_n_valid(d["labels"])
    loss, mag_loss, dl, mag_d, uf = R.ce_ref(d["logits"], d["labels"], scale, nv)
    e_loss, e_dl = R.emu_ce(d["logits"], d["labels"], scale, nv)
    return R.within(e_loss, loss, mag_loss, F32), R.within(e_dl, dl, mag_d, dtype, underflow=uf)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_ce_fp32_emulation_within_bounds(dtype):
    worst = 0.0
    for rows, V in R.CE_SHAPES:
        for scale in R.CE_SCALES:
            worst = max(worst, *ce_ratios(R.ce_inputs(rows, V, dtype), scale, dtype))
    for rows, V in ((7, 8), (9, 4100)):
        worst = max(worst, *ce_ratios(R.ce_bad_label_inputs(rows, V, dtype), 0.25, dtype))
    worst = max(worst, *ce_ratios(R.ce_one_valid_inputs(5, 255, dtype), 1.0, dtype))
    print(f"cross entropy {dtype}: {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ (c) the derived CE bound is nowhere looser than the hand-picked one
@pytest.mark.parametrize("dtype", [BF, F32])
def test_ce_bound_is_not_looser_than_the_first_generation_tolerances(dtype):
    """the inputs of tests/test_gpu_kernels.py::test_cross_entropy; its tolerances: loss 1e-5 / 1e-5, fp32 gradient 1e-4 / 1e-8, bf16
    gradient 2^-7 / 1e-7 (rtol |ref| + atol)"""
    rows, V = 23, 32000
    lg = (torch.randn(rows, V, generator=torch.Generator().manual_seed(52)) * 3).to(dtype)
    lab = torch.randint(1, V, (rows,), generator=torch.Generator().manual_seed(3))
    lab[::5] = 0
    nv = R.ce_n_valid(lab)
    loss, mag_loss, dl, mag_d, uf = R.ce_ref(lg, lab, 1.0, nv)
    b_loss = R.EVAL_F32 * mag_loss + R.TINY[F32]
    assert bool((b_loss <= 1e-5 * loss.abs() + 1e-5).all())
    b_dl = (R.HALF_ULP_BF16 if dtype == BF else 0.0) * dl.abs() + R.EVAL_F32 * mag_d + R.TINY[dtype] + R.F32_MIN_NORMAL * uf
    rtol, atol = (2.0 ** -7, 1e-7) if dtype == BF else (1e-4, 1e-8)
    assert bool((b_dl <= rtol * dl.abs() + atol).all())
    print(f"ce bound / old tolerance, worst: loss {float((b_loss / (1e-5 * loss.abs() + 1e-5)).max()):.3g} "
          f"grad {float((b_dl / (rtol * dl.abs() + atol)).max()):.3g}")
    # and the bound is what `within` applies
    off = dl + 0.5 * b_dl
    assert R.within(off, dl, mag_d, dtype, underflow=uf) <= 0.5 + 1e-9


# ------------------------------------------------------------------ (d) the generation-step reference is ref_cpu.generate_greedy
class ScriptedDecoder:
    """forward_inference returns row cur_pos of the logits table; a trace entry is opened per step"""

    def __init__(self, table, trace):
        self.table, self.trace = table, trace
        self.args = SimpleNamespace(max_batch_size=len(R.GEN_PROMPTS), max_seq_len=R.GEN_TOTAL)

    def forward_inference(self, tokens, prev_pos, image_tokens=None):
        cur = prev_pos + tokens.shape[1]
        self.trace.append(dict(cur=cur, where=[], lor=[]))
        return self.table[cur]


def run_oracle(stops):
    """ref_cpu.generate_greedy over the script, recording what its torch.where / torch.logical_or calls return: the last of each in a
    step are stop_pos and stopped after that step"""
    trace = []
    dec = ScriptedDecoder(R.gen_logits_table(), trace)
    where0, lor0 = torch.where, torch.logical_or

    def where(*a):
        out = where0(*a)
        trace[-1]["where"].append(out.clone())
        return out

    def lor(*a):
        out = lor0(*a)
        trace[-1]["lor"].append(out.clone())
        return out

    max_gen = R.GEN_TOTAL - max(len(p) for p in R.GEN_PROMPTS)
    with mock.patch.object(torch, "where", where), mock.patch.object(torch, "logical_or", lor):
        tokens, outs = ref_cpu.generate_greedy(dec, [list(p) for p in R.GEN_PROMPTS], max_gen_len=max_gen, eos_id=stops[0][0],
                                               extra_stop=stops[1:])
    return tokens, outs, trace


def test_generate_step_ref_reproduces_the_oracle_loop():
    stops = R.GEN_STOPS
    tokens, outs, trace = run_oracle(stops)
    assert [t["cur"] for t in trace] == list(range(R.GEN_START, R.GEN_TOTAL))            # all ten steps ran
    table = R.gen_logits_table()
    st = R.gen_initial_state()
    for t in trace:
        cur = t["cur"]
        R.generate_step_ref(st, torch.argmax(table[cur], dim=-1).tolist(), cur, stops)
        assert t["lor"][-1].tolist() == st["stopped"], cur                               # mid-loop stopped / stop_pos
        assert t["where"][-1].tolist() == st["stop_pos"], cur
        assert st["live"] == len(st["stopped"]) - sum(st["stopped"])
    assert tokens.tolist() == st["tokens"]
    assert outs == [row[len(p):sp] for row, p, sp in zip(st["tokens"], R.GEN_PROMPTS, st["stop_pos"])]
    # the script drives what it says it drives
    assert st["stop_pos"] == [3, 8, 1, R.GEN_TOTAL, 3, 1] and st["stopped"] == [True, True, True, False, True, True]
    assert st["live"] == 1
    # a stop loop that took the LAST hit would end row 0 at 4 and row 2 at 2
    assert st["tokens"][0][3:6] == [5, 6, 7] and st["tokens"][2][1:4] == [5, 6, 7]
    # the forced 7 of row 1 completed [6, 7] and the forced positions ignored the scripted EOS
    assert st["tokens"][1][:6] == R.GEN_PROMPTS[1]


def test_generate_step_ref_without_stop_sequences():
    st = R.gen_initial_state()
    table = R.gen_logits_table()
    for cur in range(R.GEN_START, R.GEN_TOTAL):
        R.generate_step_ref(st, torch.argmax(table[cur], dim=-1).tolist(), cur, [])
    assert st["stopped"] == [False] * 6 and st["stop_pos"] == [R.GEN_TOTAL] * 6 and st["live"] == 6
