"""-m gpu: the LoRA merge -- the a3v_lora_merge kernel (exact inputs bit for bit, random inputs within the stated rounding bounds, NF4
base, windows, in-place use, refusals), ``llama_ens5_peft.Transformer.merge_adapters`` against the oracle with adapters and against a
base-plugin model holding the merged weights, ``MetaModel.merge_lora`` after an optimizer step, and the ``merge_lora`` command line."""
import json
import os
import types

import pytest
import torch

import lora_merge_ref as MR
from a3vlm_amd import lib, ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.LLM import llama_ens5_peft as peft
from a3vlm_amd.util import promote_trainable_params_to_fp32
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
NS = (1, 40, 200, 257)            # not tile multiples; 257 exceeds the 128-row workgroup tile (and 200 its 64-row pass)
KS_NF4 = (64, 192, 320)
KS = KS_NF4 + (72,)               # 72: a partial 64-column tile (bf16 base only: NF4 needs K % 64 == 0)
RS = (8, 24, 64, 256)             # 8 and 24: zero-filled fragment tails; 64 and 256: two and eight contraction steps
SENT = -7.0                       # exactly representable in bf16 and fp32
TK = dict(dim=128, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=192, multiple_of=64, max_seq_len=512)      # tests/test_gpu_lora.py
RANK = 8
LINEARS = (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight")


def _is_linear(k):
    return k.startswith("layers.") and k.endswith(LINEARS)


# ---------------------------------------------------------------------------------------------------------------- 1-5. the kernel
@pytest.mark.parametrize("R", RS)
def test_exact_inputs_bf16_bit_equal(R):
    for N in NS:
        for K in KS:
            base, B, A = MR.exact_inputs(N, K, R, seed=N + K + R)
            want = MR.merge_ref64(base, B, A).to(BF)               # fp64 -> bf16: ONE rounding, zero tolerance by derivation
            got = ops.lora_merge(base.to(DEV), B.to(DEV), A.to(DEV), out=torch.empty(N, K, dtype=BF, device=DEV))
            assert torch.equal(got.cpu(), want), (N, K, R, int((got.cpu() != want).sum()))


@pytest.mark.parametrize("R", RS)
def test_random_inputs_within_rounding_bounds(R):
    for dtype in (BF, torch.float32):
        for N in NS:
            for K in KS:
                base, B, A = MR.random_inputs(N, K, R, dtype, seed=3 * N + K + R)
                ref, mag = MR.merge_ref64(base, B, A), MR.abs_terms64(base, B, A)
                got = ops.lora_merge(base.to(DEV), B.to(DEV), A.to(DEV), out=torch.empty(N, K, dtype=dtype, device=DEV)).cpu().double()
                # one bf16 rounding of the result (2^-8 relative) + fp32 accumulation over R <= 256 terms (2^-18 of the magnitudes)
                bound = 2.0 ** -18 * mag + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0)
                excess = ((got - ref).abs() - bound).max()
                assert float(excess) <= 0.0, (dtype, N, K, R, float(excess))


@pytest.mark.parametrize("R", RS)
def test_nf4_base_bit_equal_to_merge_over_its_dequantised_matrix(R):
    for N in NS:
        for K in KS_NF4:
            w, B, A = MR.random_inputs(N, K, R, BF, seed=N + 2 * K + R)
            q, sc, _ = ops.quantize_nf4(w.to(DEV).contiguous())
            wd = ops.dequantize_nf4(q, sc, torch.empty(N, K, dtype=BF, device=DEV))
            B, A = B.to(DEV), A.to(DEV)
            over_wd = ops.lora_merge(wd, B, A, out=torch.empty(N, K, dtype=BF, device=DEV))
            over_q = ops.lora_merge((q, sc), B, A)
            assert over_q.dtype == BF and torch.equal(over_q, over_wd), (N, K, R)
            assert not torch.equal(over_wd, wd)                    # the adapters moved the matrix


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_windows_and_in_place(dtype):
    for N, K, R in ((40, 72, 24), (257, 192, 8), (200, 320, 64)):
        base, B, A = MR.random_inputs(N, K, R, dtype, seed=N)
        base, B, A = base.to(DEV), B.to(DEV), A.to(DEV)
        want = ops.lora_merge(base, B, A, out=torch.empty(N, K, dtype=dtype, device=DEV))
        # in place inside a wider image with a guard row: columns beyond K and the row after N keep their sentinel
        wide = torch.full((N + 1, K + 24), SENT, dtype=dtype, device=DEV)
        wide[:N, :K] = base
        ops.lora_merge(wide[:N, :K], B, A)
        assert torch.equal(wide[:N, :K], want), (N, K, R)
        assert bool((wide[:N, K:] == SENT).all()) and bool((wide[N] == SENT).all())
        # out of place: source window (ldw > K) and destination window (ldo > K) of different widths
        src = torch.full((N + 1, K + 8), SENT, dtype=dtype, device=DEV)
        src[:N, :K] = base
        dst = torch.full((N + 1, K + 16), SENT, dtype=dtype, device=DEV)
        ops.lora_merge(src[:N, :K], B, A, out=dst[:N, :K])
        assert torch.equal(dst[:N, :K], want) and torch.equal(src[:N, :K], base)
        assert bool((dst[:N, K:] == SENT).all()) and bool((dst[N] == SENT).all())
    # NF4 base into a window
    N, K, R = 40, 192, 24
    w, B, A = MR.random_inputs(N, K, R, BF, seed=5)
    q, sc, _ = ops.quantize_nf4(w.to(DEV).contiguous())
    dst = torch.full((N + 1, K + 16), SENT, dtype=BF, device=DEV)
    ops.lora_merge((q, sc), B.to(DEV), A.to(DEV), out=dst[:N, :K])
    assert torch.equal(dst[:N, :K], ops.lora_merge((q, sc), B.to(DEV), A.to(DEV)))
    assert bool((dst[:N, K:] == SENT).all()) and bool((dst[N] == SENT).all())


def test_refusals_leave_the_output_untouched():
    L = lib.load()
    N, K, R = 40, 128, 16
    S, A_, D = -1, -3, -2                                             # A3V_ERR_SHAPE, A3V_ERR_ARG, A3V_ERR_DTYPE
    t = {"W": torch.zeros(N + 1, K + 8, dtype=BF, device=DEV), "B": torch.zeros(N + 1, 264 + 8, dtype=BF, device=DEV),
         "A": torch.zeros(264 + 1, K + 8, dtype=BF, device=DEV), "out": torch.full((N + 1, K + 8), SENT, dtype=BF, device=DEV),
         "q": torch.zeros(N + 1, K // 2, dtype=torch.uint8, device=DEV), "scales": torch.zeros(N + 1, K // 64, dtype=torch.float32, device=DEV)}
    good = dict(W=t["W"].data_ptr(), ldw=K + 8, q=None, scales=None, B=t["B"].data_ptr(), ldb=272, A=t["A"].data_ptr(), lda=K + 8,
                out=t["out"].data_ptr(), ldo=K + 8, N=N, K=K, R=R, dtype=lib.BF16)
    nf4 = dict(good, W=None, ldw=0, q=t["q"].data_ptr(), scales=t["scales"].data_ptr())

    def call(a):
        return L.a3v_lora_merge(a["W"], a["ldw"], a["q"], a["scales"], a["B"], a["ldb"], a["A"], a["lda"], a["out"], a["ldo"], a["N"],
                                a["K"], a["R"], a["dtype"], torch.cuda.current_stream().cuda_stream)
    cases = [
        ("R % 8", dict(good, R=12), S), ("R < 8", dict(good, R=0), S), ("R > 256", dict(good, R=264), S),
        ("K % 8, bf16 base", dict(good, K=124), S), ("K % 64, NF4 base", dict(nf4, K=72), S),
        ("ldw % 8", dict(good, ldw=K + 4), S), ("ldo % 8", dict(good, ldo=K + 4), S), ("lda % 8", dict(good, lda=K + 4), S),
        ("ldb % 8", dict(good, ldb=R + 4), S),
        ("W alignment", dict(good, W=good["W"] + 8), S), ("B alignment", dict(good, B=good["B"] + 8), S),
        ("A alignment", dict(good, A=good["A"] + 8), S), ("out alignment", dict(good, out=good["out"] + 8), S),
        ("q alignment", dict(nf4, q=nf4["q"] + 8), S), ("scales alignment", dict(nf4, scales=nf4["scales"] + 8), S),
        ("W and q", dict(good, q=nf4["q"], scales=nf4["scales"]), A_), ("neither W nor q", dict(good, W=None), A_),
        ("q without scales", dict(nf4, scales=None), A_), ("fp32 form over NF4", dict(nf4, dtype=lib.F32), A_),
        ("NULL B", dict(good, B=None), A_), ("NULL A", dict(good, A=None), A_), ("NULL out", dict(good, out=None), A_),
        ("dtype", dict(good, dtype=7), D),
    ]
    for what, a, code in cases:
        assert call(a) == code, what
        torch.cuda.synchronize()
        assert bool((t["out"] == SENT).all()), what
    assert call(good) == 0 and call(nf4) == 0                         # the unmodified arguments are accepted
    torch.cuda.synchronize()
    assert bool((t["out"][:N, :K] == 0).all()) and bool((t["out"][:N, K:] == SENT).all())
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.lora_merge(torch.zeros(8, 64, dtype=BF), torch.zeros(8, 8, dtype=BF), torch.zeros(8, 64, dtype=BF))


# ---------------------------------------------------------------------------------------------------------------- 6-8. the plugin
def _weights(cfg=TK, seed=0, std=0.08):
    oargs = ref_cpu.OracleArgs(**cfg)
    sd = ref_cpu.make_decoder_weights(oargs, seed=seed, std=std)
    lsd = ref_cpu.make_lora_weights(oargs, RANK, seed=5, std_a=0.05, std_b=0.05)
    return oargs, sd, lsd


def _peft_model(cfg, sd, lsd, dtype):
    m = peft.Transformer(peft.ModelArgs(**cfg, lora_rank=RANK), with_visual=False)
    m.load_state_dict({**sd, **lsd}, strict=True)
    train = m.get_trainable_params()
    for n, p in m.named_parameters():
        p.requires_grad = n in train
    return m.to(dtype).to(DEV)


def _base_model(cfg, sd, dtype):
    m = plugin.Transformer(plugin.ModelArgs(**cfg))
    m.load_state_dict(sd, strict=True)
    return m.to(dtype).to(DEV)


def _logits(m, ex):
    """forward, prefill of 17 tokens, 4 cached decode steps"""
    out = [m(ex).float().clone(), m.forward_inference(ex[:, :17], 0).float().clone()]
    out += [m.forward_inference(ex[:, t:t + 1], t).float().clone() for t in range(17, 21)]
    return out


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (BF, 4e-2)])
def test_merged_model_vs_oracle_and_vs_base_plugin(dtype, tol):
    oargs, sd, lsd = _weights()
    m = _peft_model(TK, sd, lsd, dtype)
    g = torch.Generator().manual_seed(3)
    ex = torch.randint(3, 192, (3, 21), generator=g)
    ex[:, 0] = 1
    cast = (lambda t: t.to(BF)) if dtype == BF else (lambda t: t)
    dec = ref_cpu.OracleDecoder(oargs, {k: cast(v) for k, v in {**sd, **lsd}.items()})
    want = [dec.forward(ex).float(), dec.forward_inference(ex[:, :17], 0).float()]
    want += [dec.forward_inference(ex[:, t:t + 1], t).float() for t in range(17, 21)]
    base_only = ref_cpu.OracleDecoder(oargs, {k: cast(v) for k, v in sd.items()}).forward(ex).float()
    scale = float(want[0].abs().max())
    assert float((want[0] - base_only).abs().max()) > tol * scale       # the adapters matter

    m.merge_adapters()
    assert not any("lora_" in n for n, _ in m.named_modules()) and not any("lora_" in k for k in m.state_dict())
    fresh = plugin.Transformer(plugin.ModelArgs(**TK))
    assert list(m.state_dict()) == list(fresh.state_dict())
    assert m.is_peft is False and not hasattr(m, "_per_kernel_decode") and type(m.args) is plugin.ModelArgs
    assert set(m.get_trainable_params()) == set(fresh.get_trainable_params())
    with pytest.raises(RuntimeError):
        m.merge_adapters()
    with pytest.raises(RuntimeError):
        m.quantize_base_weights("nf4")

    got = _logits(m, ex.to(DEV))
    for i, (a, w) in enumerate(zip(got, want)):
        err = float((a.cpu() - w).abs().max()) / scale
        print(f"merged {dtype} logits[{i}] vs oracle with adapters: {err:.3e}")
        assert err < tol, (i, err)
        if dtype == torch.float32 and i >= 2:
            assert (a.argmax(-1).cpu() == w.argmax(-1)).all(), i
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.to(dtype).to(DEV)
    for i, (a, b) in enumerate(zip(got, _logits(fresh, ex.to(DEV)))):
        assert torch.equal(a, b), i                                      # the same code on the same weights


def _wd_state(sd):
    """bf16 state dict with Wd = bf16(NF4[q] * s_b) in the seven linears of every layer and the head (the library's own round trip)"""
    out = {}
    for k, v in sd.items():
        v = v.to(BF)
        if k == "output.weight" or _is_linear(k):
            q, sc, _ = ops.quantize_nf4(v.to(DEV).contiguous())
            v = ops.dequantize_nf4(q, sc, torch.empty(v.shape, dtype=BF, device=DEV)).cpu()
        out[k] = v
    return out


@pytest.fixture(scope="module")
def qlora_merged():
    """(merged QLoRA model, merged bf16 model on Wd, the Wd state) on the tiny config"""
    oargs, sd, lsd = _weights()
    mq = _peft_model(TK, sd, lsd, BF)
    mq.quantize_base_weights("nf4")
    mq.merge_adapters()
    wd = _wd_state(sd)
    md = _peft_model(TK, wd, lsd, BF)
    md.merge_adapters()
    return mq, md, wd


def test_qlora_base_merge_equals_merge_over_wd(qlora_merged):
    mq, md, wd = qlora_merged
    assert mq._q4 is None and not hasattr(mq.output, "q4") and not hasattr(mq.layers[0].attention.wq, "q4")
    sq, sdd = mq.state_dict(), md.state_dict()
    assert list(sq) == list(plugin.Transformer(plugin.ModelArgs(**TK)).state_dict()) == list(sdd)
    for k in sq:
        assert sq[k].dtype == BF and torch.equal(sq[k], sdd[k]), k
    assert torch.equal(sq["output.weight"].cpu(), wd["output.weight"])
    assert not torch.equal(sq["layers.0.attention.wq.weight"].cpu(), wd["layers.0.attention.wq.weight"])


NF4CFG = dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)       # tests/test_gpu_nf4.py (vocabulary: the tokenizer's)


def _meta(llama_type, cfg, max_seq_len, dtype=BF):
    from a3vlm_amd.model.meta import MetaModel
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(DEV):
            mm = MetaModel(llama_type, [cfg], os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=max_seq_len)
    finally:
        torch.set_default_dtype(old)
    return mm.eval()


@pytest.mark.parametrize("mode", ["nf4", "fp8"])
def test_quantising_a_merged_model(mode):
    oargs, sd, lsd = _weights(dict(NF4CFG, vocab_size=192, max_seq_len=192), seed=11, std=0.05)
    mp = _meta("llama_ens5_peft", dict(NF4CFG, lora_rank=RANK), 192)
    mp.llma.load_state_dict({k: v.to(BF) for k, v in {**sd, **lsd}.items()}, strict=True)
    with pytest.raises(NotImplementedError):
        mp.llma.quantize_decode_weights("nf4")                           # not merged: still refused
    mp.merge_lora()
    merged = {k: v.clone() for k, v in mp.llma.state_dict().items()}
    mb = _meta("llama_ens5", NF4CFG, 192)
    mb.llma.load_state_dict(merged, strict=True)
    mp.llma.quantize_decode_weights(mode)
    mb.llma.quantize_decode_weights(mode)
    assert mp.llma.weight_format == mode and mb.llma.weight_format == mode
    prompts = ["Detect all manipulable object parts.", "the quick brown fox"]
    _, ids_p = mp.generate(prompts, None, max_gen_len=12, temperature=0, return_ids=True)
    _, ids_b = mb.generate(prompts, None, max_gen_len=12, temperature=0, return_ids=True)
    assert ids_p == ids_b and any(len(i) > 0 for i in ids_p)


# ---------------------------------------------------------------------------------------------------------------- 9-10. façade, CLI
def _tiny_meta_cfg():
    return {k: v for k, v in TK.items() if k not in ("vocab_size", "max_seq_len")}


def test_facade_merges_the_stepped_adapters():
    from a3vlm_amd.optim import FusedAdamW
    oargs, sd, lsd = _weights()
    mm = _meta("llama_ens5_peft", dict(_tiny_meta_cfg(), lora_rank=RANK), 64)
    mm.llma.load_state_dict({k: v.to(BF) for k, v in {**sd, **lsd}.items()}, strict=True)
    mm._set_default_trainability()
    promote_trainable_params_to_fp32(mm)
    mm.train()
    before = {n: p.detach().clone() for n, p in mm.llma.named_parameters()}
    g = torch.Generator().manual_seed(7)
    ex = torch.randint(3, 192, (2, 24), generator=g)
    ex[:, 0] = 1
    lab = ex.clone()
    lab[:, :5] = 0
    opt = FusedAdamW([p for p in mm.parameters() if p.requires_grad], lr=1e-2, betas=(0.9, 0.95))
    loss, _ = mm(ex.to(DEV), lab.to(DEV))
    loss.backward()
    opt.step()
    assert getattr(mm, "_engine", None) is not None
    n0 = "layers.0.attention.wq"
    stepped = dict(mm.llma.named_parameters())
    assert not torch.equal(stepped[n0 + ".lora_b.weight"], before[n0 + ".lora_b.weight"])
    # the merge the test computes itself from the POST-step adapters (cast to the base dtype first)
    want = {}
    for k in before:
        if _is_linear(k):
            p = k[:-len("weight")]
            want[k] = ops.lora_merge(before[k], stepped[p + "lora_b.weight"].detach().to(BF).contiguous(),
                                     stepped[p + "lora_a.weight"].detach().to(BF).contiguous(), out=torch.empty_like(before[k]))
    mm.merge_lora()
    assert mm.llama_type == "llama_ens5" and mm.is_peft is False and getattr(mm, "_engine", None) is None
    sdm = mm.state_dict()
    assert list(sdm) == ["llma." + k for k in plugin.Transformer(plugin.ModelArgs(**TK)).state_dict()]
    for k, w in want.items():
        assert torch.equal(sdm["llma." + k], w), k
        assert not torch.equal(w, before[k]), k
    assert all(p.requires_grad for n, p in mm.llma.named_parameters())    # the base plugin trains everything but the encoders
    with pytest.raises(RuntimeError):
        mm.merge_lora()
    with pytest.raises(RuntimeError):
        _meta("llama_ens5", _tiny_meta_cfg(), 64).merge_lora()


@pytest.mark.parametrize("quant_base", [False, True])
def test_merge_lora_cli(tmp_path, quant_base, qlora_merged):
    from a3vlm_amd import checkpoint as ck, merge_lora
    from a3vlm_amd.model.meta import MetaModel
    oargs, sd, lsd = _weights()
    mm = _meta("llama_ens5_peft", dict(_tiny_meta_cfg(), lora_rank=RANK), 512)
    mm.llma.load_state_dict({k: v.to(BF) for k, v in {**sd, **lsd}.items()}, strict=True)
    ckdir = ck.save_checkpoint(str(tmp_path / "ck"), types.SimpleNamespace(precision="bf16", only_save_trainable=False), mm, None, None, None, epoch=0)
    out = str(tmp_path / "merged")
    merged = merge_lora.main(["--pretrained_path", ckdir, "--output_dir", out, "--no_visual", "--max_seq_len", "512"]
                             + (["--quant_base"] if quant_base else []))
    assert json.load(open(os.path.join(out, "meta.json"))) == {"llama_type": "llama_ens5"}
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert "lora_rank" not in cfg and "bias_tuning" not in cfg and cfg["dim"] == TK["dim"]
    assert {"consolidated.00-of-01.model.pth", "tokenizer.model"} <= set(os.listdir(out))
    with _no_mismatch_warning():
        back = MetaModel.from_pretrained(out, with_visual=False, max_seq_len=512)
    assert back.llama_type == "llama_ens5" and type(back.llma) is plugin.Transformer and not back.is_peft
    assert list(back.state_dict()) == list(merged.state_dict())
    for k, v in back.state_dict().items():
        assert torch.equal(v, merged.state_dict()[k]), k
    g = torch.Generator().manual_seed(3)
    ex = torch.randint(3, 192, (3, 21), generator=g).to(DEV)
    ex[:, 0] = 1
    for i, (a, b) in enumerate(zip(_logits(back.llma, ex), _logits(merged.llma, ex))):
        assert torch.equal(a, b), i
    if quant_base:                                                       # the weights of the QLoRA merge above
        mq = qlora_merged[0].state_dict()
        for k, v in mq.items():
            assert torch.equal(back.state_dict()["llma." + k], v), k
    else:
        mref = _peft_model(TK, sd, lsd, BF)
        mref.merge_adapters()
        for k, v in mref.state_dict().items():
            assert torch.equal(back.state_dict()["llma." + k], v), k


class _no_mismatch_warning:
    """from_pretrained warns when the checkpoint and the model differ in keys: that warning must not appear"""

    def __enter__(self):
        import warnings
        self.cm = warnings.catch_warnings(record=True)
        self.rec = self.cm.__enter__()
        warnings.simplefilter("always")
        return self

    def __exit__(self, *exc):
        self.cm.__exit__(*exc)
        assert not [w for w in self.rec if "mismatch" in str(w.message)], [str(w.message) for w in self.rec]
        return False
