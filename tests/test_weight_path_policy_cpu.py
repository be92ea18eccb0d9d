"""CPU: the path policy of the decode weight formats (a3vlm_amd/model/LLM/weight_formats.py layer_path / head_path), the format table
and the record ``Transformer._weights``.  The expected paths are written out here by hand from the rules the formats were merged with;
nothing below is computed by calling the code under test."""
import dataclasses
import itertools

import pytest
import torch

from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.LLM import weight_formats as wf

ROWS = (1, 16, 17, 32, 33, 64)
ANY = None

# (fmt, prefill, decode [S == 1], dim, bf16 stream, ragged) -> the path at each of ROWS; ANY matches every value.  head_dim = 128.
LAYER_RULES = [
    # bf16 weights: nothing else to run on
    (("bf16", ANY, ANY, ANY, ANY, ANY),       "bf16 bf16 bf16 bf16 bf16 bf16"),
    # fp8: W8A8 above 16 rows of a bf16 stream when asked for, never in the ragged step; everything else on the bf16 weights
    (("fp8", False, ANY, ANY, ANY, ANY),      "bf16 bf16 bf16 bf16 bf16 bf16"),
    (("fp8", True, ANY, ANY, False, ANY),     "bf16 bf16 bf16 bf16 bf16 bf16"),
    (("fp8", True, ANY, ANY, True, True),     "bf16 bf16 bf16 bf16 bf16 bf16"),
    (("fp8", True, ANY, ANY, True, False),    "bf16 bf16 w8a8 w8a8 w8a8 w8a8"),
    # mxfp4: decode steps of at most 32 rows on the GEMV whatever prefill says; the rest W4A8 if asked for, else on the dequantised layer
    (("mxfp4", False, True, ANY, ANY, ANY),   "gemv gemv gemv gemv dequant dequant"),
    (("mxfp4", False, False, ANY, ANY, ANY),  "dequant dequant dequant dequant dequant dequant"),
    (("mxfp4", True, True, ANY, ANY, ANY),    "gemv gemv gemv gemv w4a8 w4a8"),
    (("mxfp4", True, False, ANY, ANY, ANY),   "w4a8 w4a8 w4a8 w4a8 w4a8 w4a8"),
    # nf4: at most 16 rows on the GEMV at any S (a 10-token prefill too) if dim >= 512; prefill means nothing
    (("nf4", ANY, ANY, 512, ANY, ANY),        "gemv gemv dequant dequant dequant dequant"),
    (("nf4", ANY, ANY, 256, ANY, ANY),        "dequant dequant dequant dequant dequant dequant"),
]

# (fmt, prefill, decode [S == 1 and B <= 32], fp32 stream) -> the LM head's path
HEAD_RULES = [
    ((ANY, ANY, ANY, True),                   "gemm_nt"),
    (("bf16", ANY, ANY, False),               "linear"),
    (("fp8", ANY, ANY, False),                "linear"),
    (("nf4", ANY, ANY, False),                "gemv"),
    (("mxfp4", ANY, True, False),             "gemv"),
    (("mxfp4", True, False, False),           "w4a8"),
    (("mxfp4", False, False, False),          "dequant"),
]


def _expected(rules, case):
    hits = [want for pat, want in rules if all(p is ANY or p == c for p, c in zip(pat, case))]
    assert len(hits) == 1, (case, hits)          # the hand-written table covers every case exactly once
    return hits[0]


def test_layer_path_of_every_format_and_shape():
    n = 0
    for case in itertools.product(("bf16", "fp8", "nf4", "mxfp4"), (False, True), (True, False), (256, 512), (True, False), (False, True)):
        fmt, prefill, decode, dim, bf16, ragged = case
        if ragged and not decode:
            continue                              # the ragged step is a decode step
        want = _expected(LAYER_RULES, case).split()
        for rows, w in zip(ROWS, want):
            assert wf.layer_path(fmt, prefill, rows, decode, dim, 128, bf16, ragged) == w, (case, rows)
            n += 1
    assert n == 4 * 2 * 3 * 2 * 2 * len(ROWS)


@pytest.mark.parametrize("head_dim,want", [(64, "w8a8"), (128, "w8a8"), (32, "bf16"), (96, "bf16"), (256, "bf16")])
def test_w8a8_needs_head_dim_64_or_128(head_dim, want):
    assert wf.layer_path("fp8", True, 24, False, 512, head_dim, True) == want
    assert wf.layer_path("fp8", True, 16, False, 512, head_dim, True) == "bf16"


def test_head_path_of_every_format():
    for case in itertools.product(("bf16", "fp8", "nf4", "mxfp4"), (False, True), (True, False), (False, True)):
        assert wf.head_path(*case) == _expected(HEAD_RULES, case), case


def test_format_table():
    F = wf.FORMATS
    assert set(F) == {"bf16", "fp8", "nf4", "mxfp4"}
    assert [F[k].step_code for k in ("bf16", "fp8", "nf4", "mxfp4")] == [0, 1, 2, None]
    assert [F[k].frees_weights for k in ("bf16", "fp8", "nf4", "mxfp4")] == [False, False, True, True]
    assert (F["nf4"].gemv_rows, F["nf4"].gemv_max_rows) == (16, 16) and (F["mxfp4"].gemv_rows, F["mxfp4"].gemv_max_rows) == (16, 32)
    assert F["bf16"].gemv is None and F["fp8"].gemv is None, "Python runs no GEMV on fp8 images: the C step does"
    for k in ("nf4", "mxfp4"):
        assert all(callable(getattr(F[k], f)) for f in ("check", "quantize", "dequantize", "gemv", "gemv_ws_bytes")), k
    assert F["nf4"].step_fields == ("_n4", "_n4s") and F["fp8"].step_fields == ("_q", "_s") and F["mxfp4"].step_fields is None
    assert wf.WeightImage._fields == ("q", "s") and wf.LAYER_KEYS == ("wqkv", "wo", "w13", "w2")
    q, s = wf.WeightImage(1, 2)                   # tuple unpacking, as ops calls take it
    assert (q, s) == (1, 2)


def _toy(dtype=torch.float32):
    torch.manual_seed(0)
    return plugin.Transformer(plugin.ModelArgs(dim=256, n_layers=2, n_heads=2, vocab_size=64, multiple_of=256, max_seq_len=64)).to(dtype)


def test_fresh_model_is_bf16_format_without_attribute_fallbacks():
    m = _toy()
    assert m.__dict__["_weights"] is None and "_layer_tab_key" in m.__dict__
    assert m.weight_format == "bf16" and m._step_format_code() == 0
    for old in ("_q8", "_fp8_prefill", "_n4", "_mx4", "_mx4_prefill"):
        assert not hasattr(m, old), old


def test_cpu_model_refusals_keep_their_text():
    m = _toy()
    with pytest.raises(ValueError, match=r"^NF4 weights need a bf16 model on the GPU \(quantise after \.to\(device\)\)$"):
        m.quantize_decode_weights("nf4")
    with pytest.raises(ValueError, match=r"^MXFP4 weights need a bf16 model, this one is torch\.float32 \(fp32 models are refused\)$"):
        m.quantize_decode_weights("mxfp4")
    with pytest.raises(ValueError, match=r"^fp8 decode weights need bf16 parameters and dim, ffn, n_heads\*head_dim multiples of 256$"):
        m.quantize_decode_weights("fp8")
    with pytest.raises(ValueError, match=r"^only weight-only 'fp8' \(OCP e4m3fn\) is implemented$"):
        m.quantize_decode_weights("int4")
    mb = _toy(torch.bfloat16)
    with pytest.raises(ValueError, match=r"^NF4 weights need a bf16 model on the GPU \(quantise after \.to\(device\)\)$"):
        mb.quantize_decode_weights("nf4")
    with pytest.raises(ValueError, match=r"^MXFP4 weights need the model on the GPU \(quantise after \.to\(device\)\)$"):
        mb.quantize_decode_weights("mxfp4", prefill=True)
    assert m.weight_format == "bf16" and mb.weight_format == "bf16" and hasattr(mb.output, "weight")


def _fake_format(monkeypatch, fmt):
    """The real walk of quantize_decode_weights on the CPU: the format's row with the device check off and a torch stand-in for its
    quantiser (codes = the low byte of every other element, one scale per row)."""
    def quantize(w, ws):
        return w.view(torch.uint8)[:, ::4].contiguous(), w.float().abs().amax(1)
    monkeypatch.setitem(wf.FORMATS, fmt, dataclasses.replace(wf.FORMATS[fmt], check=lambda m: None, quantize=quantize, quantize_ws_bytes=None))


@pytest.mark.parametrize("fmt,prefill", [("nf4", False), ("nf4", True), ("mxfp4", False), ("mxfp4", True)])
def test_4bit_record(monkeypatch, fmt, prefill):
    _fake_format(monkeypatch, fmt)
    m = _toy(torch.bfloat16)
    w1, w3 = m.layers[1].feed_forward.w1.weight.data.clone(), m.layers[1].feed_forward.w3.weight.data.clone()
    m.quantize_decode_weights(fmt, prefill=prefill)
    w = m._weights
    assert m.weight_format == fmt == w.fmt and w.prefill is (prefill and fmt == "mxfp4") and w.version is None
    assert set(w.images) == {f"{k}.{i}" for k in wf.LAYER_KEYS for i in range(2)} | {"output"}
    assert all(type(img) is wf.WeightImage for img in w.images.values())
    hd, F = m.head_dim, m.ffn
    assert w.images["wqkv.0"].q.shape[0] == 3 * 2 * hd and w.images["w13.1"].q.shape[0] == 2 * F and w.images["output"].s.shape == (64,)
    # w1 | w3 in 16-row blocks, codes and scales alike
    s13 = w.images["w13.1"].s.view(F // 16, 2, 16)
    assert torch.equal(s13[:, 0].reshape(-1), w1.float().abs().amax(1)) and torch.equal(s13[:, 1].reshape(-1), w3.float().abs().amax(1))
    sd = m.state_dict()
    assert "output.weight" not in sd and not any(".attention.w" in k or ".feed_forward.w" in k for k in sd), "the bf16 weights are freed"
    assert not any(k.startswith(("wqkv.", "w13.")) for k in m._pack()), "and never packed again"
    assert m._step_format_code() == {"nf4": 2, "mxfp4": None}[fmt]
    name = {"nf4": "NF4", "mxfp4": "MXFP4"}[fmt]
    for mode in ("fp8", "nf4", "mxfp4", None):
        with pytest.raises(RuntimeError, match=rf"^this model holds {name} weights: quantize_decode_weights\('{fmt}'\) freed its bf16 decoder weights "
                                               r"and cannot be undone or combined with another mode; reload the checkpoint instead$"):
            m.quantize_decode_weights(mode)


def test_fp8_record(monkeypatch):
    _fake_format(monkeypatch, "fp8")
    m = _toy(torch.bfloat16)
    for prefill in (False, True):
        m.quantize_decode_weights("fp8", prefill=prefill)
        w = m._weights
        assert m.weight_format == "fp8" and w.prefill is prefill and m._step_format_code() == 1
        assert set(w.images) == {f"{k}.{i}" for k in wf.LAYER_KEYS for i in range(2)}, "no 'output': the head stays bf16"
        assert w.version is not None and w.version == m._packed_version
        assert "output.weight" in m.state_dict() and "wqkv.0" in m._pack(), "the bf16 weights stay"
        assert w.images["w13.0"].q.shape[0] == m._pack()["w13.0"].shape[0] and w.images["wo.1"].s.shape == (256,)
    m.quantize_decode_weights(None)
    assert m._weights is None and m.weight_format == "bf16" and m._layer_tab_key is None


def test_meta_reads_the_property():
    import inspect
    from a3vlm_amd.model.meta import MetaModel
    src = inspect.getsource(MetaModel.train_engine)
    assert "weight_format" in src and "getattr(self.llma" not in src
