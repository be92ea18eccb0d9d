"""Generation controls, no GPU: the restatement (tests/genctl_ref.py) against plain torch and against an independent loop over the
HF rule, the entry's flags, the keyword defaults of the three generators and the refusal of a non-positive penalty."""
import inspect
import math
import os

import pytest
import torch

import genctl_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def _rows(B, V, seed):
    z = torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 2.0
    z[:, 1], z[:, 2] = 0.0, -0.0
    return z


@pytest.mark.parametrize("V", [33, 640, 32000])
def test_logprob_restatement_against_fp64_log_softmax(V):
    z = _rows(3, V, V)
    z[1, 5] = -math.inf
    tok = torch.tensor([0, V - 1, 7])
    want = torch.log_softmax(z.double(), dim=-1).gather(-1, tok[:, None]).squeeze(-1)
    got = G.logprob32(z, tok)
    # the restated fp32 form is itself a max-subtracted sum: inside the bound derived for the device's order, with the depth of a
    # pairwise / sequential fp32 sum of V terms in place of the kernel's (V u relative, the textbook worst case)
    tol = G.lse_bound(z) + V * G.U32 + G.U32 * z.gather(-1, tok[:, None]).squeeze(-1).abs().double()
    assert bool(((got.double() - want).abs() <= tol).all()), (got, want, tol)
    assert torch.equal(G.lse32(torch.full((1, V), -math.inf)), torch.tensor([-math.inf]))
    assert float(G.lse_bound(z).max()) < 1e-4, "the bound is a few dozen ulps, not a tolerance"


def test_penalty_restatement_against_a_loop_over_the_hf_rule():
    V, p = 97, 1.3
    z = _rows(2, V, 1)
    z[0, 9], z[1, 11] = math.inf, -math.inf
    ids = [[0, 1, 2, 31, 32, 96, 96, 9, 200, -4], [11, 64, 3]]
    bm = G.seen_bitmap(ids, V)
    mask = G.seen_mask(bm, V)
    got = G.penalise(z, mask, p)
    want = z.clone()
    for b, row in enumerate(ids):                        # HF: score = gather(scores, input_ids); where(score < 0, score * p, score / p); scatter
        for t in set(row):
            if not 0 <= t < V:
                continue
            s = z[b, t]
            want[b, t] = s * torch.tensor(p) if s < 0 else s / torch.tensor(p)
    assert torch.equal(got, want)                        # (+-0 take either branch to the same bits' value: 0 / p == 0 * p)
    assert got[0, 9] == math.inf and got[1, 11] == -math.inf
    assert int(mask.sum()) == len({0, 1, 2, 31, 32, 96, 9}) + 3
    assert torch.equal(G.penalise(z, mask, 1.0), z)
    # bitmap layout: bit t & 31 of word t >> 5
    assert int(bm[0, 0]) == (1 << 0) | (1 << 1) | (1 << 2) | (1 << 31) | (1 << 9) and int(bm[0, 1]) == 1 and int(bm[0, 3]) == 1


def test_generate_record_restatement_by_hand():
    V = 40
    z = _rows(3, V, 2)
    lse = G.lse32(z)
    tokens = torch.tensor([[1, 5, 39, 0], [1, 7, 0, 0], [1, 2, 3, 4]])
    lp = torch.full((3, 3), 9.0)
    bm = torch.zeros(3, 2, dtype=torch.int64)
    G.generate_record(z, lse, tokens, bm, lp, V, col=2, prompt_len=torch.tensor([2, 1, 3]))
    assert lp[0, 0] == z[0, 39] - lse[0] and lp[1, 1] == z[1, 0] - lse[1] and torch.equal(lp[2], torch.full((3,), 9.0))
    assert bm.tolist() == [[0, 1 << 7], [1, 0], [0, 0]]
    G.generate_record(z, lse, tokens, bm, lp, V, cur=torch.tensor([2, 0, 4]), stopped_before=torch.tensor([0, 0, 1]), prompt_len=torch.tensor([1, 1, 1]))
    assert lp[0, 0] == z[0, 5] - lse[0] and bm.tolist() == [[1 << 5, 1 << 7], [1, 0], [0, 0]]


def test_parser_flags_and_defaults():
    from a3vlm_amd.eval_affordance_v2 import get_args_parser
    from a3vlm_amd.eval_affordance_with_quant import get_parser
    import argparse
    for p in (argparse.ArgumentParser(parents=[get_args_parser()]), get_parser()):
        a = p.parse_args([])
        assert a.repetition_penalty == 1.0 and a.save_scores is False
        a = p.parse_args(["--repetition_penalty", "1.3", "--save_scores"])
        assert a.repetition_penalty == 1.3 and a.save_scores is True


def test_generator_keyword_defaults():
    from a3vlm_amd.model.meta import MetaModel
    for fn in (MetaModel.generate, MetaModel.generate_many, MetaModel.stream_generate):
        ps = inspect.signature(fn).parameters
        assert ps["repetition_penalty"].default == 1.0 and ps["return_logprobs"].default is False, fn


def test_non_positive_penalty_is_refused_before_any_device_use():
    from a3vlm_amd.model.meta import MetaModel
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=64)
    for p in (0, 0.0, -1.5, float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            mm.generate(["Lid?"], None, max_gen_len=2, repetition_penalty=p)
        with pytest.raises(ValueError, match="repetition_penalty"):
            mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=2, repetition_penalty=p)
        with pytest.raises(ValueError, match="repetition_penalty"):
            next(mm.stream_generate("Lid?", None, max_gen_len=2, repetition_penalty=p))
