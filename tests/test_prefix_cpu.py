"""Prefix sharing without a GPU: ragged.prefix_groups / PrefixScheduler against tests/prefix_ref.py on hand cases, the two mutants,
the refusals of extend_rows / generate_many / the eval entry, the new C symbols and the parser flag."""
import os
import types

import pytest

from a3vlm_amd.model import ragged
from tests import prefix_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _drive(lens, limits, R, W, groups, finish_order):
    s = ragged.PrefixScheduler(lens, limits, R, W, groups)
    log, row_of = [], {}

    def admit():
        for lead, P, new, members in s.refill():
            for k, (r, i) in enumerate(members):
                row_of[i] = r
                log.append((i, r, lead if P else None, (new and k == 0) if P else None))
    admit()
    for i in finish_order:
        s.advance()
        s.release(row_of.pop(i))
        admit()
    assert s.done()
    return log


def T(common, tail):
    return [1] + [7] * (common - 1) + list(tail)


CASES = {
    # a common prefix that ends exactly on a 64 boundary: C = 128, every member has its own tail
    "ends-on-boundary": ([T(128, [9, 9]), T(128, [10]), T(128, [11, 12, 13])], [0, 0, 0], 0, [([0, 1, 2], 128)]),
    # a member that is itself a prefix of another: P = min(C, shortest - 1) keeps one token of its own
    "member-is-a-prefix": ([T(128, []), T(128, [5, 6])], ["a", "a"], 0, [([0, 1], 64)]),
    "one-short-of-two-tiles": ([T(129, []), T(129, [5])], ["a", "a"], 0, [([0, 1], 128)]),
    # images: W words in front; a different image cuts the run; mixed runs and single prompts
    "mixed": ([T(40, [2]), T(40, [3]), T(40, [4]), T(3, [8]), T(40, [5]), T(40, [6])], ["a", "a", "b", "b", "c", "c"], 30,
              [([0, 1], 64), ([2], 0), ([3], 0), ([4, 5], 64)]),
    # the image words cannot be cut: P = 64 < W + 1 counts as 0
    "prefix-inside-the-image": ([T(5, [2]), T(5, [3])], ["a", "a"], 100, [([0], 0), ([1], 0)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_runs_and_shared_length(case):
    toks, keys, W, want = CASES[case]
    assert ragged.prefix_groups(toks, keys, W) == want
    assert ref.runs(toks, keys, W) == want
    for members, P in want:
        assert P % 64 == 0 and all(P <= W + len(toks[i]) - 1 for i in members if P)


def test_mutant_unrounded_p_is_caught():
    toks, keys, W, want = CASES["member-is-a-prefix"]
    assert ref.runs(toks, keys, W, round_p=False) == [([0, 1], 127)] != want


SCRIPTS = {
    # a run larger than batch_rows: members 3, 4 wait; member 3 goes to the first row that frees, 4 onto the LEADER row itself
    "run-of-5-in-3-rows": ([70] * 5 + [10], [80] * 6, 3, [([0, 1, 2, 3, 4], 64), ([5], 0)], [1, 0, 3, 2, 4, 5]),
    # the leader finishes first: its row is held, prompt 3 (another run) must take another row
    "held-leader": ([70, 70, 70, 70, 70], [80] * 5, 3, [([0, 1, 2], 64), ([3, 4], 64)], [0, 1, 2, 3, 4]),
    "singles-only": ([5, 6, 7, 8], [9] * 4, 2, [([0], 0), ([1], 0), ([2], 0), ([3], 0)], [1, 0, 2, 3]),
    "finished-at-once-member": ([70, 70, 70], [80, 70, 80], 2, [([0, 1, 2], 64)], [0, 2]),
}


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_admission_order_and_held_rows(name):
    lens, limits, R, groups, fin = SCRIPTS[name]
    got = _drive(lens, limits, R, 0, groups, fin)
    assert got == ref.simulate(lens, limits, R, groups, fin), name
    if name == "run-of-5-in-3-rows":
        assert got == [(0, 0, 0, True), (1, 1, 0, False), (2, 2, 0, False), (3, 1, 0, False), (4, 0, 0, False), (5, 1, None, None)]
    if name == "held-leader":
        assert got[3] == (3, 1, 1, True), "row 0 holds the first run's prefix while members 1 and 2 run: prompt 3 waits for row 1"
    if name == "singles-only":
        s = ragged.RowScheduler(lens, limits, R, 0)
        assert [(i, r) for i, r, _, _ in got[:2]] == [(i, r) for r, i in s.refill()]


def test_mutant_refilled_held_row_is_caught():
    lens, limits, R, groups, fin = SCRIPTS["held-leader"]
    bad = ref.simulate(lens, limits, R, groups, fin, hold=False)
    assert bad[3][:2] == (3, 0), "the mutant hands the held leader row to the next run"
    assert bad != _drive(lens, limits, R, 0, groups, fin)


# ------------------------------------------------------------------ refusals (nothing here touches a device)
def test_c_symbols_in_header_and_library():
    hdr = open(os.path.join(ROOT, "include", "a3vlm_hip.h")).read()
    from a3vlm_amd import lib
    for sym in ("a3v_attention_extend_rows", "a3v_attention_extend_rows_scratch_floats", "a3v_rope_kvcache_extend"):
        assert sym + "(" in hdr and sym in lib._SIGNATURES if hasattr(lib, "_SIGNATURES") else sym + "(" in hdr
    so = os.path.join(ROOT, "a3vlm_amd", "liba3vlm_hip.so")
    if os.path.isfile(so):
        data = open(so, "rb").read()
        for sym in (b"a3v_attention_extend_rows", b"a3v_rope_kvcache_extend"):
            assert sym in data
    assert "a3v_extend.hip" in open(os.path.join(ROOT, "a3vlm_amd", "csrc", "Makefile")).read()


def _args(**kw):
    base = dict(share_image_prefix=True, continuous_rows=4, num_samples=1, lookup_decoding=0, num_beams=0, kv_quant=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_eval_entry_flag_and_refusals():
    from a3vlm_amd import eval_affordance_v2 as ev
    from a3vlm_amd import eval_affordance_with_quant as evq
    for mod in (ev, evq):
        p = mod.get_args_parser()
        assert "--share_image_prefix" in p.format_help()
    assert ev.check_share_image_prefix(_args()) is True
    assert ev.check_share_image_prefix(_args(share_image_prefix=False, continuous_rows=0)) is False
    for kw, word in ((dict(continuous_rows=1), "--continuous_rows"), (dict(num_samples=2), "--num_samples 1"),
                     (dict(lookup_decoding=3), "--lookup_decoding 0"), (dict(num_beams=2), "--num_beams 0"), (dict(kv_quant="fp8"), "--kv_quant")):
        with pytest.raises(SystemExit, match=word):
            ev.check_share_image_prefix(_args(**kw))


def test_model_refusals_before_any_allocation():
    import torch
    from a3vlm_amd.model.LLM import llama_ens5 as plugin
    from a3vlm_amd.model.meta import MetaModel
    m = plugin.Transformer(plugin.ModelArgs(dim=64, n_layers=1, n_heads=2, vocab_size=64, multiple_of=64, max_seq_len=128))
    m._kv_quant, m._kv_rows = "fp8", True
    with pytest.raises(RuntimeError, match="quantize_kv_cache\\(None\\)"):
        m.extend_rows([0], [torch.tensor([1])], [64])
    m._kv_rows = False
    with pytest.raises(RuntimeError, match="fp8"):
        m.extend_rows([0], [torch.tensor([1])], [64])
    m._kv_quant = None
    with pytest.raises(ValueError, match="together"):
        m.extend_rows([0], [torch.tensor([1])], [64], src_row=[0])
    with pytest.raises(ValueError, match="allocate_rows"):
        m.extend_rows([0], [torch.tensor([1])], [64])
    assert not m._k_cache, "nothing was allocated"
    mm = MetaModel.__new__(MetaModel)
    for kw, word in ((dict(n=2, temperature=0.5), "n=1"), (dict(lookup=2), "lookup=0")):
        with pytest.raises(ValueError, match=word):
            MetaModel.generate_many(mm, ["a"], None, batch_rows=4, prefix_sharing=True, **kw)
    with pytest.raises(ValueError, match="prefix_sharing=False"):
        MetaModel.beam_search(mm, ["a"], None, num_beams=2, batch_rows=4, prefix_sharing=True)
