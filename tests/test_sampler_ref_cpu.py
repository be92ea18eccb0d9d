"""CPU: tests/sampler_ref.py (the checker of a3v_sample_top_k_p) on rows whose kept sets are written out by hand, against
oracle/ref_cpu.py with top-k and min-p off, against HF's warpers where ``transformers`` is installed; and the interface of the
feature (header, lib.py, built library, generate signatures, validator, eval flags)."""
import ctypes
import inspect
import os

import pytest
import torch

import sampler_ref as S
from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sorted: 3.0 (5), 2.0 (0), 1.0 (2), 1.0 (3), 0.5 (6), 0.0 (1), -1.0 (4), -2.0 (7)
#   e = exp(z - 3):  1, .3679, .1353, .1353, .0821, .0498, .0183, .0067       Z = 1.7955
#   p:               .5570, .2049, .0754, .0754, .0457, .0277, .0102, .0038   mass before: 0, .5570, .7619, .8373, .9126, .9584, .9861, .9963
ROW = torch.tensor([[2.0, 0.0, 1.0, 1.0, -1.0, 3.0, 0.5, -2.0]])
ALL = set(range(8))


@pytest.mark.parametrize("k,p,m,want", [
    (1, 1.0, 0.0, {5}),
    (2, 1.0, 0.0, {5, 0}),
    (3, 1.0, 0.0, {5, 0, 2, 3}),            # the 3rd value is tied with the 4th: both kept
    (4, 1.0, 0.0, {5, 0, 2, 3}),
    (8, 1.0, 0.0, ALL),                     # k = V
    (11, 1.0, 0.0, ALL),                    # k = V + 3
    (0, 1.0, 0.0, ALL),
    (0, 1.0, 1.0, {5}),                     # min-p 1: the arg-max alone
    (0, 1.0, 0.1, {5, 0, 2, 3}),            # .1353 >= .1 > .0821
    (0, 0.8, 0.0, {5, 0, 2}),               # top-p binding: cuts inside the tie, lower index first (.7619 <= .8 < .8373)
    (2, 0.99, 0.01, {5, 0}),                # top-k binding
    (5, 0.99, 0.2, {5, 0}),                 # min-p binding: K = {5, 0, 2, 3, 6}, all within top-p .99 of Z_K; e >= .2 leaves two
    (5, 0.8, 0.05, {5, 0, 2}),              # top-p binding inside K: Z_K = 1.7206, mass before: 0, .5812, .7950, .8737, .9523
    (2, 0.7, 0.0, {5}),                     # top-p sees K renormalised: .7311 > .7 (over the whole row token 0 sits behind .5570 <= .7)
])
def test_kept_sets_written_out_by_hand(k, p, m, want):
    assert S.kept_sets(ROW, 1.0, k, p, m) == [want]


def test_temperature_comes_first_and_the_draw_is_the_inverse_cdf():
    # T = 0.5: e = exp(2 (z - 3)) = 1, .1353, .0183 (x2), .0067, ...: min-p .1 now keeps two tokens, not four
    assert S.kept_sets(ROW, 0.5, 0, 1.0, 0.1) == [{5, 0}]
    # K = {5, 0} renormalised: .7311, .2689
    ps, idx = S.nucleus(ROW, 1.0, 2, 1.0, 0.0)
    assert idx[0, :2].tolist() == [5, 0] and torch.allclose(ps[0, :2], torch.tensor([0.7311, 0.2689]), atol=1e-4) and float(ps[0, 2:].sum()) == 0
    for u, want in ((0.0, 5), (0.5, 5), (0.73, 5), (0.74, 0), (0.99999994, 0)):
        assert int(S.sample_at(ROW, 1.0, 2, 1.0, 0.0, torch.tensor([u]))) == want, u
    # an all-tied row: k = 3 keeps everything; a row with -inf entries: they are never kept
    assert S.kept_sets(torch.full((1, 6), 0.25), 1.0, 3, 1.0, 0.0) == [set(range(6))]
    z = torch.tensor([[1.0, float("-inf"), 0.0, float("-inf"), 2.0, -1.0]])
    assert S.kept_sets(z, 1.0, 5, 1.0, 0.0) == [{0, 2, 4, 5}] and S.kept_sets(z, 1.0, 2, 1.0, 0.0) == [{0, 4}]


@pytest.mark.parametrize("T,p", [(0.1, 0.75), (1.0, 0.9), (0.7, 1.0)])
def test_filters_off_is_the_oracles_nucleus(T, p):
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(4, 1003, generator=g) * 2.5).bfloat16().float()
    probs = torch.softmax(z / T, dim=-1)
    want_ps, want_idx = ref_cpu.top_p_nucleus(probs, p)
    for k in (0, 1003, 1008):
        ps, idx = S.nucleus(z, T, k, p, 0.0)
        assert torch.equal(ps, want_ps) and torch.equal(idx, want_idx)
        u = torch.rand(4, generator=g)
        assert torch.equal(S.sample_at(z, T, k, p, 0.0, u), ref_cpu.sample_top_p_at(probs, p, u))


def test_kept_sets_equal_hf_warpers():
    try:
        from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper
    except Exception as e:                    # not installed here: nothing to compare with
        pytest.skip(f"transformers does not import: {e!r}")
    # every pair of neighbouring values 0.37 apart (and two exact ties): no threshold of either library falls on a rounding edge
    g = torch.Generator().manual_seed(9)
    V = 40
    vals = torch.arange(V, dtype=torch.float32) * 0.37 - 6.0
    vals[11] = vals[10]
    vals[30] = vals[29]
    z = torch.stack([vals[torch.randperm(V, generator=g)] for _ in range(3)])
    ids = torch.zeros(3, 1, dtype=torch.long)
    for T in (0.7, 1.0):
        for k in (1, 2, 10, 11, 12, V - 1, V, V + 3):
            hf = TopKLogitsWarper(top_k=k)(ids, TemperatureLogitsWarper(T)(ids, z.clone()))
            assert [set(torch.nonzero(r > float("-inf")).flatten().tolist()) for r in hf] == S.kept_sets(z, T, k, 1.0, 0.0), (T, k)
        e = torch.sort(S.e_values(z[:1], T)[0], descending=True).values
        for a in (0, 3, 9, 10, 20, V - 2):
            if float(e[a]) == float(e[a + 1]):
                continue
            m = float(torch.sqrt(e[a].double() * e[a + 1].double()))            # between two neighbouring e values
            for k in (0, 12):
                x = TemperatureLogitsWarper(T)(ids, z.clone())
                if k:
                    x = TopKLogitsWarper(top_k=k)(ids, x)
                hf = MinPLogitsWarper(min_p=m)(ids, x)
                assert [set(torch.nonzero(r > float("-inf")).flatten().tolist()) for r in hf] == S.kept_sets(z, T, k, 1.0, m), (T, a, k)


# ---------------------------------------------------------------- interface
def test_entry_is_declared_bound_and_exported():
    from a3vlm_amd import lib
    assert "int a3v_sample_top_k_p(const float* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p, float min_p," in \
        open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    I, F, P, L = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
    assert lib.SIGNATURES["a3v_sample_top_k_p"] == (I, [P, L, I, I, F, I, F, F, P, P, P])
    fn = lib.load().a3v_sample_top_k_p
    # argument errors come back before anything is launched (no device is needed to see them)
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    assert fn(a, 8, 1, 8, 1.0, -1, 0.9, 0.0, a, a, None) == -3
    assert fn(a, 8, 1, 8, 1.0, 0, 0.9, 1.5, a, a, None) == -3
    assert fn(a, 8, 1, 8, 1.0, 0, 0.9, -0.1, a, a, None) == -3
    assert fn(a, 8, 1, 8, 1.0, 0, 0.9, float("nan"), a, a, None) == -3
    assert fn(None, 8, 1, 8, 1.0, 2, 0.9, 0.1, a, a, None) == -3
    assert fn(a, 8, 1, 8, 0.0, 2, 0.9, 0.1, a, a, None) == -1 and fn(a, 70000, 1, 70000, 1.0, 2, 0.9, 0.1, a, a, None) == -1
    assert buf.raw == b"\0" * 64


def test_generate_methods_and_validator():
    from a3vlm_amd import ops
    from a3vlm_amd.model import genctl
    from a3vlm_amd.model.meta import MetaModel
    assert callable(ops.sample_top_k_p)
    for name in ("generate", "generate_many", "stream_generate"):
        sig = inspect.signature(getattr(MetaModel, name))
        assert sig.parameters["top_k"].default == 0 and sig.parameters["min_p"].default == 0.0, name
    assert genctl.check_filters(0, 0.0) == (0, 0.0) and genctl.check_filters(50, 1) == (50, 1.0)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            genctl.check_filters(bad, 0.0)
    for bad in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            genctl.check_filters(0, bad)


def test_eval_parsers_accept_the_flags():
    from a3vlm_amd import eval_affordance_v2, eval_affordance_with_quant
    p = eval_affordance_v2.get_args_parser()
    assert p.get_default("top_k") == 0 and p.get_default("min_p") == 0.0
    a = p.parse_args(["--top_k", "50", "--min_p", "0.05"])
    assert a.top_k == 50 and a.min_p == 0.05
    a = eval_affordance_with_quant.get_parser().parse_args(["--top_k", "7", "--min_p", "0.5"])
    assert a.top_k == 7 and a.min_p == 0.5
