"""MXFP4 without a GPU: the entries exist in header, library and ctypes table; argument refusals; the plan query; parsers and
signatures; properties of the numpy restatement of the format (tests/mx4_ref.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mx4_ref as R
from a3vlm_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_quantize_mxfp4", "a3v_dequantize_mxfp4", "a3v_gemm_skinny_mxfp4", "a3v_gemm_skinny_mxfp4_ws_bytes", "a3v_mx4_gemv_plan")
SHAPE, ARG = -1, -3
P = 4096            # a dummy, 16-B aligned, never dereferenced: every refusal comes before any launch


def test_entries_in_header_library_and_table():
    header = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    assert "MXFP4 weights" in header
    L = lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES and getattr(L, name) is not None


def test_quantiser_and_dequantiser_refusals():
    L = lib.load()
    assert L.a3v_quantize_mxfp4(None, 128, P, 64, P, 16, 128, None) == ARG
    assert L.a3v_quantize_mxfp4(P, 128, None, 64, P, 16, 128, None) == ARG
    assert L.a3v_quantize_mxfp4(P, 128, P, 64, None, 16, 128, None) == ARG
    assert L.a3v_quantize_mxfp4(P, 96, P, 48, P, 16, 96, None) == SHAPE           # K % 128
    assert L.a3v_quantize_mxfp4(P, 128, P, 32, P, 16, 128, None) == SHAPE         # ldq < K / 2
    assert L.a3v_quantize_mxfp4(P, 128, P, 72, P, 16, 128, None) == SHAPE         # ldq % 16
    assert L.a3v_quantize_mxfp4(P + 2, 128, P, 64, P, 16, 128, None) == SHAPE     # alignment
    assert L.a3v_quantize_mxfp4(P, 128, P, 64, P, 0, 128, None) == SHAPE
    assert L.a3v_dequantize_mxfp4(None, 64, P, P, 128, 16, 128, None) == ARG
    assert L.a3v_dequantize_mxfp4(P, 64, P, None, 128, 16, 128, None) == ARG
    assert L.a3v_dequantize_mxfp4(P, 64, P, P, 120, 16, 128, None) == SHAPE       # ldo < K
    assert L.a3v_dequantize_mxfp4(P, 64, P, P + 8, 128, 16, 128, None) == SHAPE
    assert L.a3v_dequantize_mxfp4(P, 64, P, P, 128, 16, 64, None) == SHAPE


def test_gemv_refusals():
    L = lib.load()

    def call(A=P, lda=256, q=P, ldq=128, s=P, C=P, ldc=32, M=4, N=32, K=256, res=None, ldr=0, epi=0, ws=P):
        return L.a3v_gemm_skinny_mxfp4(A, lda, q, ldq, s, C, ldc, M, N, K, res, ldr, epi, ws, None)
    for kw in (dict(A=None), dict(q=None), dict(s=None), dict(C=None), dict(ws=None), dict(epi=ops.EPI_RESIDUAL)):
        assert call(**kw) == ARG, kw
    for kw in (dict(M=0), dict(M=17), dict(N=24), dict(N=0), dict(K=192), dict(K=0), dict(K=32768), dict(N=65536 + 16), dict(lda=128),
               dict(lda=260), dict(ldq=64), dict(ldq=136), dict(ldc=16), dict(ldc=34), dict(A=P + 8), dict(q=P + 8), dict(C=P + 8),
               dict(ws=P + 4), dict(s=P + 1), dict(epi=ops.EPI_SWIGLU, N=48), dict(epi=ops.EPI_SWIGLU | ops.EPI_OUT_F32),
               dict(epi=ops.EPI_GELU), dict(epi=ops.EPI_RESIDUAL, res=P, ldr=16), dict(epi=ops.EPI_RESIDUAL, res=P + 4, ldr=32)):
        assert call(**kw) == SHAPE, kw
    assert L.a3v_gemm_skinny_mxfp4_ws_bytes(17, 32, 256) == 0 and L.a3v_gemm_skinny_mxfp4_ws_bytes(4, 32, 192) == 0
    assert L.a3v_gemm_skinny_mxfp4_ws_bytes(4, 32, 256) >= 65536 + 8 * 4 * 64 * 16


DECODE = {"7B": dict(dim=4096, ffn=11008, vocab=32000), "13B": dict(dim=5120, ffn=13824, vocab=32000)}


@pytest.mark.parametrize("name", list(DECODE))
def test_plan_on_decode_shapes(name):
    g = DECODE[name]
    for N, K, epi in ((3 * g["dim"], g["dim"], 0), (g["dim"], g["dim"], ops.EPI_RESIDUAL), (2 * g["ffn"], g["dim"], ops.EPI_SWIGLU),
                      (g["dim"], g["ffn"], ops.EPI_RESIDUAL), (g["vocab"], g["dim"], ops.EPI_OUT_F32)):
        rc, (grid, block, S, rows, lds, nun, tgs, maxun) = ops.mx4_gemv_plan(8, N, K, epi, 256)
        assert rc == 0, (N, K)
        assert block == 256 and rows == 64 and tgs == -(-N // 64) and nun == -(-K // 512)
        assert 1 <= S <= min(8, nun) and maxun == -(-nun // S) and maxun <= 4
        assert grid == -(-tgs // 8) * 8 * S and grid >= 256, "every CU gets a block"
        assert lds == maxun * 8448 + 4 * 3 * 4352 and lds + 2048 <= 160 * 1024
        assert ops.gemm_skinny_mxfp4_ws_bytes(8, N, K) >= 65536 + tgs * S * 4 * 64 * 16


def test_plan_slices_and_refusals():
    assert ops.mx4_gemv_plan(1, 16, 128)[1][2] == 1 and ops.mx4_gemv_plan(16, 4112, 128)[1][2] == 1      # one slice: K is one unit
    assert ops.mx4_gemv_plan(5, 48, 384)[1][2] == 1
    assert ops.mx4_gemv_plan(5, 16, 4096)[1][2] == 8 and ops.mx4_gemv_plan(5, 48, 11008)[1][2] == 8      # split: N alone fills nothing
    assert ops.mx4_gemv_plan(8, 16, 16384)[0] == 0
    for M, N, K, epi in ((0, 16, 128, 0), (17, 16, 128, 0), (8, 24, 128, 0), (8, 16, 64, 0), (8, 16, 16384 + 128, 0), (8, 65552, 128, 0),
                         (8, 48, 128, ops.EPI_SWIGLU), (8, 32, 128, ops.EPI_SWIGLU | ops.EPI_RESIDUAL), (8, 32, 128, ops.EPI_BIAS)):
        assert ops.mx4_gemv_plan(M, N, K, epi)[0] == SHAPE, (M, N, K, epi)
    assert lib.load().a3v_mx4_gemv_plan(8, 16, 128, 0, 256, None) == ARG
    assert ops.mx4_gemv_plan(8, 16, 128, 0, 0)[0] == SHAPE
    # the bf16 / fp8 / NF4 planner knows no fourth format
    plan = (ctypes.c_int32 * 13)()
    assert lib.load().a3v_gemv_plan(8, 4096, 4096, 0, 3, 0, 0, 0, 1, 256, plan) < 0


def test_parsers_and_signatures():
    from a3vlm_amd import eval_affordance_with_quant as ev
    from a3vlm_amd.model.meta import MetaModel
    from a3vlm_amd.model.LLM import llama_ens5, llama_ens5_peft, weight_formats
    p = ev.get_parser()
    base = ["--llama_config", "c.json", "--tokenizer_path", "t.model"]
    req = [a for a in p._actions if a.required]
    argv = []
    for a in req:
        argv += [a.option_strings[0], "x"]
    assert p.parse_args(argv + ["--quant"]).quant_format == "nf4", "--quant alone is what it was"
    assert p.parse_args(argv + ["--quant", "--quant_format", "mxfp4"]).quant_format == "mxfp4"
    with pytest.raises(SystemExit):
        p.parse_args(argv + ["--quant_format", "int4"])
    assert "quant" in inspect.signature(MetaModel.from_pretrained).parameters
    assert "mxfp4" in inspect.getsource(MetaModel.from_pretrained)
    assert "mxfp4" in inspect.getsource(llama_ens5_peft.Transformer.quantize_decode_weights)
    assert hasattr(llama_ens5.Transformer, "_quantize_4bit") and weight_formats.WeightImage._fields == ("q", "s")
    assert weight_formats.FORMATS["mxfp4"].quantize is not None and weight_formats.FORMATS["mxfp4"].frees_weights
    for name in ("quantize_mxfp4", "dequantize_mxfp4", "gemm_skinny_mxfp4"):
        assert callable(getattr(ops, name))


def test_fp32_model_is_refused_before_any_launch():
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    m = plugin.Transformer(plugin.ModelArgs(dim=256, n_layers=1, n_heads=4, vocab_size=64, multiple_of=256, max_seq_len=64))
    with pytest.raises(ValueError, match="fp32"):
        m.quantize_decode_weights("mxfp4")


# ------------------------------------------------------------------ the restated format
def _bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


def test_round_trip_of_codes_is_exact():
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, size=(8, 64), dtype=np.uint8)
    q[(q & 15) == 8] &= 0xF0                                       # -0 is never written
    q[(q >> 4) == 8] &= 0x0F
    s = rng.integers(1, 250, size=(8, 4), dtype=np.uint8)
    # a block whose largest code is below 4 would be re-scaled: give every block one code 6 or 7 (|v| >= 4)
    q[:, ::16] = (q[:, ::16] & 0xF0) | 7
    wd = R.dequantize(q, s)
    assert np.array_equal(_bf16(wd), wd.astype(np.float32)), "Wd is exact in bf16"
    q2, s2 = R.quantize(wd)
    assert np.array_equal(q2, q) and np.array_equal(s2, s)


def test_grid_values_zero_blocks_saturation_and_ties():
    grid = np.concatenate([R.E2M1, -R.E2M1[1:]])
    w = np.zeros((2, 64))
    w[0, :15] = grid * 2.0 ** -5
    w[1, 32:47] = grid * 2.0 ** 9
    q, s = R.quantize(w)
    assert np.array_equal(R.dequantize(q, s), w), "values on the grid round-trip exactly"
    assert s[0, 1] == 127 and s[1, 0] == 127 and not q[0, 16:].any() and not q[1, :16].any(), "zero blocks: byte 127, codes 0"
    assert s[0, 0] == 127 + 2 - 5 - 2 and s[1, 1] == 127 + 2 + 9 - 2
    # max 7.5 -> E = 0: 7.5 and 7 saturate to 6; ties 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4; -0 -> +0
    w = np.zeros((1, 32))
    w[0, :12] = [7.5, -7.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.0, -5.0]
    q, s = R.quantize(w)
    assert s[0, 0] == 127
    assert np.array_equal(R.dequantize(q, s)[0, :12], [6, -6, 0, 1, 1, 2, 2, 4, 4, 0, 0, -4])
    assert (q[0, 4] >> 4) == 0 and (q[0, 5] & 0x0F) == 0,"-0.25 -> +0 and -0 -> +0: no sign bit on a zero code"
    assert not (R.quantize(np.full((1, 32), 2.0 ** 127))[1] == 255).any() and R.quantize(np.full((1, 32), 2.0 ** -133))[1][0, 0] == 0


def test_activation_rule():
    a = np.zeros((1, 96))
    a[0, :4] = [3.0, -8.0, 1.0, 0.5]                               # max 8 -> E = 3 - 8
    a[0, 32:35] = [500.0, 449.0, -17.0]                            # max 500 -> E = 0: 500 saturates at 448; 449 -> 448; 17 -> 16 (tie to even)
    aq, ea = R.quant_act_mxfp8(a)
    assert list(ea[0]) == [-5, 0, 0] and np.array_equal(aq[0, :4], [96, -256, 32, 16])
    assert np.array_equal(aq[0, 32:35], [448, 448, -16]) and not aq[0, 64:].any()
    assert np.array_equal(R.fake_quant_act(a)[0, :4], a[0, :4])


def test_quality_on_gaussian_weights():
    """Relative Frobenius error of RTN MXFP4 on seeded N(0, 0.02) bf16 256 x 4096 (NF4 by tests/nf4_ref.py on the same matrix: 0.092)."""
    w = (torch.randn(256, 4096, generator=torch.Generator().manual_seed(0)) * 0.02).bfloat16().float().numpy()
    q, s = R.quantize(w)
    err = float(np.linalg.norm(R.dequantize(q, s) - w) / np.linalg.norm(w))
    print(f"MXFP4 relative Frobenius error {err:.4f}")
    assert err <= 0.125
