"""The W4A8 GEMM on MXFP4 images without a GPU: the restatement (tests/mx4_gemm_ref.py) against hand-computed blocks; the three entries in
header, library and ctypes table; every plan of a3v_mx4_gemm_plan self-consistent; refusals before any launch; the --quant_prefill rules."""
import argparse
import inspect
import os
import re

import numpy as np
import pytest

import mx4_gemm_ref as G
import mx4_ref as R
from a3vlm_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("a3v_quantize_rows_mxfp8", "a3v_gemm_nt_mxfp4", "a3v_mx4_gemm_plan")
SHAPE, ARG = -1, -3
P = 4096            # a dummy, 16-B aligned, never dereferenced: every refusal comes before any launch


# ------------------------------------------------------------------ the restatement against hand-computed blocks
def test_rows_zero_block_ties_saturation_and_subnormals():
    a = np.zeros((2, 128))
    a[0, 32:36] = [-0.0, 0.0, -0.0, 0.0]                            # block 1 of row 0: zeros of either sign
    # block 2: max 288 -> E = 8 - 8 = 0.  e4m3 steps: 16 in [128, 256), 32 in [256, 512): ties 136 -> 128, 152 -> 160, 272 -> 256
    a[0, 64:70] = [288.0, 136.0, 152.0, 272.0, -136.0, 17.0]
    # block 3: max 500 -> E = 0: 500, 449 and 464.5 (beyond 448) saturate at 448, -480 at -448
    a[0, 96:100] = [500.0, 449.0, -480.0, 464.5]
    # row 1 block 0: max 256 -> E = 0; the e4m3 subnormal range is below 2^-6 with step 2^-9: 2^-9 is the smallest code, 2^-10 is a tie
    # to even (0), 3 * 2^-10 and 5 * 2^-10 are ties to even (both 2 * 2^-9), 2^-6 - 2^-10 is a tie that goes up to the smallest normal 2^-6
    a[1, :7] = [256.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10, -(2.0 ** -11), 5 * 2.0 ** -10]
    # row 1 block 1: a block of one small power of two: max 2^-20 -> E = -28, the element becomes 256
    a[1, 40] = 2.0 ** -20
    aq, ea = G.quant_rows(a)
    assert list(ea[0]) == [0, 0, 0, 0] and not aq[0, :64].any(), "zero blocks: exponent 0 (byte 127), codes 0"
    assert np.array_equal(aq[0, 64:70], [288, 128, 160, 256, -128, 16]), "ties go to the even code"
    assert np.array_equal(aq[0, 96:100], [448, 448, -448, 448]), "saturation at 448"
    assert np.array_equal(aq[1, :7], [256, 2.0 ** -9, 0, 2 * 2.0 ** -9, 2.0 ** -6, -0.0, 2 * 2.0 ** -9]), "the subnormal range: step 2^-9, ties to even"
    assert ea[1, 1] == -28 and aq[1, 40] == 256 and list(ea[1, [0, 2, 3]]) == [0, 0, 0]
    b = G.e4m3_bytes(aq)
    assert not b[0, :64].any() and b[0, 64] == 0x79 and b[0, 96] == 0x7E and b[0, 98] == 0xFE, "288 = 1.125 * 2^8: 0x79; 448 = 1.75 * 2^8: 0x7E"
    assert b[1, 1] == 0x01 and b[1, 4] == 0x08 and b[1, 5] == 0x80, "2^-9 is code 1, 2^-6 code 8; a negative that rounds to zero keeps its sign"
    assert (ea + 127 >= 0).all() and (ea + 127 <= 254).all()


def test_rows_of_the_rmsnorm_prologue():
    rng = np.random.default_rng(0)
    x = G.rbf(rng.standard_normal((3, 256)) * 3.0)
    w = G.rbf(1.0 + 0.1 * rng.standard_normal(256))
    y = G.rmsnorm_bf16(x, w, 1e-5)
    assert np.array_equal(G.rbf(y), y), "the norm's output is bf16"
    assert abs(float((y / w[None, :]) .std()) - 1.0) < 0.05
    aq, ea = G.quant_rows(x, w, 1e-5)
    aq2, ea2 = R.quant_act_mxfp8(y)
    assert np.array_equal(aq, aq2) and np.array_equal(ea, ea2)


def test_product_and_epilogues_on_a_hand_block():
    # one 32-k block per operand: a = k / 2 for k = 1..16, w on the e2m1 grid times 2
    a = np.zeros((1, 128))
    a[0, :16] = np.arange(1, 17) * 0.5                               # max 8 -> E = -5: the elements become 16 k, four significant bits at most
    w = np.zeros((32, 128))
    w[0, :16] = 2.0 * np.array([6, -6, 4, -4, 3, -3, 2, -2, 1.5, -1.5, 1, -1, 0.5, -0.5, 0, 6])     # gate row 0
    w[16, :16] = 2.0                                                                               # up row 0 (rows 16..31 of the pair)
    q, s = R.quantize(w)
    assert np.array_equal(R.dequantize(q, s), w)
    aq, ea = G.quant_rows(a)
    assert np.array_equal(R.dequant_act(aq, ea), a)
    acc = a @ w.T
    want00 = float((a[0, :16] * w[0, :16]).sum())
    r = G.reference(aq, ea, q, s, 0)
    assert r["ref"][0, 0] == want00 == acc[0, 0] and r["bits"][0, 0] == G.rbf(np.array([[want00]]))[0, 0]
    res = np.full((1, 32), 0.375)
    r = G.reference(aq, ea, q, s, G.EPI_RESIDUAL, res)
    assert r["bits"][0, 0] == G.rbf(G.rbf(np.array([[want00]])) + 0.375)[0, 0] and r["bits"][0, 5] == 0.375
    r = G.reference(aq, ea, q, s, G.EPI_OUT_F32)
    assert r["bits"][0, 16] == acc[0, 16] == 2.0 * a.sum()
    r = G.reference(aq, ea, q, s, G.EPI_SWIGLU)
    g, u = acc[0, 0], acc[0, 16]
    assert r["ref"].shape == (1, 16) and abs(r["ref"][0, 0] - g / (1 + np.exp(-g)) * u) < 1e-12 and r["bits"] is None
    assert G.ratio(G.swiglu_on_exact(acc), r) <= 1.0, "the sequence on an exact accumulator lies inside the bound"
    assert G.ratio(r["ref"] * (1 + 2.0 ** -5), r) > 1.0, "and four bf16 steps away does not"


def test_bound_holds_for_fp32_accumulation_in_two_orders():
    rng = np.random.default_rng(1)
    M, N, K = 5, 32, 1024
    a = G.rbf(rng.standard_normal((M, K)))
    q, s = R.quantize(G.rbf(rng.standard_normal((N, K)) * 0.02))
    aq, ea = G.quant_rows(a)
    A, W = R.dequant_act(aq, ea).astype(np.float32), R.dequantize(q, s).astype(np.float32)
    fwd = np.zeros((M, N), dtype=np.float32)
    bwd = np.zeros((M, N), dtype=np.float32)
    for k in range(K):
        fwd += A[:, k:k + 1] * W[:, k][None, :]
        bwd += A[:, K - 1 - k:K - k] * W[:, K - 1 - k][None, :]
    res = G.rbf(rng.standard_normal((M, N)))
    for epi in (0, G.EPI_OUT_F32, G.EPI_RESIDUAL):
        r = G.reference(aq, ea, q, s, epi, res if epi == G.EPI_RESIDUAL else None)
        for acc in (fwd, bwd):
            out = G.rbf(acc)
            if epi == G.EPI_RESIDUAL:
                out = G.rbf((out.astype(np.float32) + res.astype(np.float32)).astype(np.float64))
            assert G.ratio(out, r) <= 1.0, epi
        assert G.ratio(r["ref"] + 2.0 ** -6 * np.abs(r["ref"]) + 1e-2, r) > 1.0, "two bf16 steps and ten times the accumulation allowance are outside"


# ------------------------------------------------------------------ entries, plans, refusals
def test_entries_in_header_library_and_table():
    """Fails before the W4A8 GEMM exists: the three symbols are in the built library, the header and the ctypes table."""
    header = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    L = lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES and getattr(L, name) is not None
    for name in ("quantize_rows_mxfp8", "gemm_nt_mxfp4", "mx4_gemm_plan"):
        assert callable(getattr(ops, name))


SHAPES = {"7B": dict(dim=4096, ffn=11008, vocab=32000), "13B": dict(dim=5120, ffn=13824, vocab=32000)}


def _five(g):
    return ((3 * g["dim"], g["dim"], 0), (g["dim"], g["dim"], ops.EPI_RESIDUAL), (2 * g["ffn"], g["dim"], ops.EPI_SWIGLU),
            (g["dim"], g["ffn"], ops.EPI_RESIDUAL), (g["vocab"], g["dim"], ops.EPI_OUT_F32))


def _check_plan(M, N, K, epi):
    rc, (rows, cols, stage, grid, block, lds, slices, stages) = ops.mx4_gemm_plan(M, N, K, epi, 256)
    assert rc == 0, (M, N, K, epi)
    assert rows in (16, 32, 64, 128) and rows % 16 == 0 and cols % 16 == 0 and block % 64 == 0 and 0 < block <= 1024
    assert cols % 32 == 0 or not (epi & ops.EPI_SWIGLU), "a SwiGLU tile holds whole gate | up pairs"
    mt, nt = -(-M // rows), -(-N // cols)
    assert grid == mt * nt and mt * rows >= M and nt * cols >= N, "grid x tile covers M x N"
    assert (mt - 1) * rows < M and (nt - 1) * cols < N, "and no tile is empty"
    assert rows >= min(M, 128), "up to 128 rows the image is streamed once"
    assert 0 <= lds <= 160 * 1024
    assert stage % 128 == 0 and slices >= 1 and stages >= 1
    assert slices * stages * stage >= K > slices * (stages - 1) * stage, "K slices x stages x stage covers K, no stage empty"
    return rows, cols, stage, slices


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_plan_is_self_consistent(name):
    seen = set()
    for N, K, epi in _five(SHAPES[name]):
        for M in range(1, 601):
            seen.add(_check_plan(M, N, K, epi)[0])
    assert seen == {16, 32, 64, 128}


def test_plans_of_small_and_large_shapes():
    for M, N, K, epi in ((1, 16, 128, 0), (33, 48, 640, 0), (129, 80, 1536, ops.EPI_RESIDUAL), (40, 32, 512, ops.EPI_SWIGLU),
                         (5, 65536, 16384, ops.EPI_OUT_F32), (100000, 65536, 128, 0)):
        _check_plan(M, N, K, epi)
    assert ops.mx4_gemm_plan(2048, 4096, 4096)[1] == ops.mx4_gemm_plan(2048, 4096, 4096, 0, 8)[1], "today's plan does not depend on cus"


def test_plan_refusals():
    for M, N, K, epi in ((0, 16, 128, 0), (-1, 16, 128, 0), (8, 24, 128, 0), (8, 0, 128, 0), (8, 16, 64, 0), (8, 16, 192, 0), (8, 16, 0, 0),
                         (8, 16, 16384 + 128, 0), (8, 65536 + 16, 128, 0), (8, 48, 128, ops.EPI_SWIGLU),
                         (8, 32, 128, ops.EPI_SWIGLU | ops.EPI_RESIDUAL), (8, 32, 128, ops.EPI_SWIGLU | ops.EPI_OUT_F32), (8, 32, 128, ops.EPI_BIAS),
                         (8, 32, 128, ops.EPI_GELU), (2 ** 31 - 1, 65536, 128, 0)):
        assert ops.mx4_gemm_plan(M, N, K, epi)[0] == SHAPE, (M, N, K, epi)
    assert lib.load().a3v_mx4_gemm_plan(8, 16, 128, 0, 256, None) == ARG
    assert ops.mx4_gemm_plan(8, 16, 128, 0, 0)[0] == SHAPE


def test_gemm_refusals_come_before_any_launch():
    L = lib.load()

    def call(A=P, lda=256, ea=P, q=P, ldq=128, s=P, C=P, ldc=32, M=40, N=32, K=256, res=None, ldr=0, epi=0):
        return L.a3v_gemm_nt_mxfp4(A, lda, ea, q, ldq, s, C, ldc, M, N, K, res, ldr, epi, None)
    for kw in (dict(A=None), dict(ea=None), dict(q=None), dict(s=None), dict(C=None), dict(epi=ops.EPI_RESIDUAL)):
        assert call(**kw) == ARG, kw
    for kw in (dict(M=0), dict(N=24), dict(N=0), dict(K=192), dict(K=0), dict(K=32768), dict(N=65536 + 16), dict(lda=128), dict(lda=264),
               dict(ldq=64), dict(ldq=136), dict(ldc=16), dict(ldc=34), dict(A=P + 8), dict(q=P + 8), dict(C=P + 4),
               dict(C=P + 8, epi=ops.EPI_OUT_F32), dict(epi=ops.EPI_SWIGLU, N=48), dict(epi=ops.EPI_SWIGLU | ops.EPI_OUT_F32),
               dict(epi=ops.EPI_GELU), dict(epi=ops.EPI_RESIDUAL, res=P, ldr=16), dict(epi=ops.EPI_RESIDUAL, res=P + 4, ldr=32)):
        assert call(**kw) == SHAPE, kw


def test_row_quantiser_refusals_come_before_any_launch():
    L = lib.load()

    def call(x=P, ldx=256, w=None, q=P, ldq=256, e=P, rows=4, K=256):
        return L.a3v_quantize_rows_mxfp8(x, ldx, w, 1e-5, q, ldq, e, rows, K, None)
    for kw in (dict(x=None), dict(q=None), dict(e=None)):
        assert call(**kw) == ARG, kw
    for kw in (dict(rows=0), dict(K=0), dict(K=192), dict(K=16384 + 128, ldx=32768, ldq=32768), dict(ldx=128), dict(ldx=260), dict(ldq=128),
               dict(ldq=260), dict(x=P + 8), dict(w=P + 8), dict(q=P + 4)):
        assert call(**kw) == SHAPE, kw


# ------------------------------------------------------------------ parsers and signatures
def test_quant_prefill_parser_rules():
    from a3vlm_amd import eval_affordance_with_quant as ev
    from a3vlm_amd.model.meta import MetaModel
    import dataclasses
    from a3vlm_amd.model.LLM import llama_ens5, weight_formats
    p = ev.get_parser()
    argv = []
    for a in (a for a in p._actions if a.required):
        argv += [a.option_strings[0], "x"]
    assert p.parse_args(argv + ["--quant"]).quant_prefill is False, "off by default"
    ok = p.parse_args(argv + ["--quant", "--quant_format", "mxfp4", "--quant_prefill"])
    assert ok.quant_prefill is True
    ev.check_args(ok)
    for bad in (["--quant", "--quant_prefill"], ["--quant", "--quant_format", "nf4", "--quant_prefill"], ["--quant_prefill"],
                ["--quant_format", "mxfp4", "--quant_prefill"]):
        with pytest.raises(SystemExit, match="MXFP4 option"):
            ev.check_args(p.parse_args(argv + bad))
    ev.check_args(p.parse_args(argv + ["--quant"]))
    sig = inspect.signature(MetaModel.from_pretrained).parameters
    assert sig["quant_prefill"].default is False
    with pytest.raises(ValueError, match="MXFP4 option"):
        MetaModel.from_pretrained("/nonexistent", quant="nf4", quant_prefill=True)
    assert "prefill" in inspect.signature(llama_ens5.Transformer.quantize_decode_weights).parameters
    assert "prefill" in inspect.getsource(llama_ens5.Transformer._quantize_4bit)
    assert "prefill" in [f.name for f in dataclasses.fields(weight_formats.DecodeWeights)]
    assert isinstance(p, argparse.ArgumentParser)
