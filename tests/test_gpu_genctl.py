"""-m gpu: generation controls (a3v_genctl.hip, model/genctl.py, MetaModel.generate / generate_many with repetition_penalty and
return_logprobs, the eval entry's --repetition_penalty / --save_scores) against the restatement of tests/genctl_ref.py: the bitmap
and the penalised rows bit for bit, the log-sum-exp inside the bound derived there from the kernel's reduction shape, the record
bit for bit, the model level against an oracle replay that applies the rule on the CPU."""
import functools
import json
import math
import os
import subprocess
import sys
import types

import pytest
import torch

import genctl_ref as G
from a3vlm_amd import ops
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
CANARY = 0x5A5A5A5A
SHAPES = [(V, B) for V in (33, 640, 32000) for B in (1, 3)]


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(V, B):
    """Logits N(0, 4) with exact 0.0 / -0.0, the (finite) maximum at two indices and one -inf; seen ids 0, 31, 32, V - 1, a duplicate,
    ids out of range; row 1 (B = 3) has lens = 0.  The bitmap rows start with bit 3 set and end in a canary word."""
    z = torch.randn(B, V, generator=torch.Generator().manual_seed(V + B)) * 2.0
    z[:, 1], z[:, 2], z[:, 7] = 0.0, -0.0, -math.inf
    mx = z.max(dim=-1).values + 1.0
    z[:, 5], z[:, V - 3] = mx, mx
    ids = [[0, 31, 32, V - 1, 5, 5, 1, 2, V + 5, -3, 10 + b, V] for b in range(B)]
    lens = [len(r) for r in ids]
    if B > 1:
        lens[1] = 0
    wpr = G.words(V)
    start = torch.zeros(B, wpr + 1, dtype=torch.int64)
    start[:, 0], start[:, wpr] = 1 << 3, CANARY
    tok = torch.full((B, 16), 9, dtype=torch.int64)           # (the columns past lens hold an id that must NOT be marked)
    for b, r in enumerate(ids):
        tok[b, :len(r)] = torch.tensor(r)
    want = G.seen_bitmap([r[:n] for r, n in zip(ids, lens)], V, wpr + 1, start=start)
    return z, tok, lens, start, want


def dev_bitmap(words64):
    """int64 words -> the device's int32 storage."""
    return words64.to(torch.int64).where(words64 < 2 ** 31, words64 - 2 ** 32).to(torch.int32).to(DEV)


# ------------------------------------------------------------------ 1. the seen set
@pytest.mark.parametrize("V,B", SHAPES)
def test_seen_mark_is_the_restated_bitmap(V, B):
    z, tok, lens, start, want = case(V, B)
    seen = dev_bitmap(start)
    ops.seen_mark(tok.to(DEV), i32(lens), seen, V)
    got = G.as_u32(seen)
    assert torch.equal(got, want), "bit for bit, the canary word and the out-of-range ids included"
    assert int(got[0, 0]) & 1 and int(got[0, G.words(V) - 1]) >> ((V - 1) & 31) & 1 and int(got[0, 0]) >> 9 & 1 == 0
    if B > 1:
        assert torch.equal(got[1], start[1]), "lens = 0"
    before = seen.clone()
    ops.seen_mark(tok.to(DEV), i32([0] * B), seen, V)
    ops.seen_mark(tok.to(DEV), i32([-4] * B), seen, V)
    assert torch.equal(seen, before), "lens <= 0 leaves every row alone"
    # clearing rows through a device row list: the listed rows only, not the canary word behind them, not an entry out of range
    ops.seen_clear_rows(seen[:, :G.words(V)], i32([B - 1, B + 7, -1]))
    got = G.as_u32(seen)
    want = want.clone()
    want[B - 1, :G.words(V)] = 0
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 2. logits_prepare
@pytest.mark.parametrize("pad", [0, 1], ids=["dense", "ld+1"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_logits_prepare_penalty_bits_and_lse_bound(V, B, pad):
    """out: torch.equal with where(seen, where(z > 0, z / p, z * p), z) in fp32.  lse: against fp64 logsumexp of the same fp32 inputs
    inside genctl_ref.lse_bound -- per-element exp error (own exponential 2 u, argument roundings u D), summation depth ((4 k + 31) u
    from k folds per thread, the wave and the block stage), the final log and add (2 u |log S| + u |lse|); derived in the docstring
    of tests/genctl_ref.py from the reduction order in include/a3vlm_hip.h, not tuned.  ld = V + 1 makes every other row start off a
    16-byte boundary (the element walk); V = 33 does so without padding."""
    z, tok, lens, start, want_bm = case(V, B)
    wpr = G.words(V)
    mask = G.seen_mask(want_bm[:, :wpr], V)
    zd_full = torch.full((B, V + pad), 3.0, device=DEV)
    zd_full[:, :V] = z.to(DEV)
    zd = zd_full[:, :V]
    raw = zd_full.clone()
    seen = dev_bitmap(want_bm)
    bound = G.lse_bound(z)
    ref64 = G.lse64(z)
    lses = []
    for p in (1.0, 1.3, 0.5):
        out_full = torch.full((B, V + pad + 4), 77.0, device=DEV)
        lse = torch.full((B + 1,), 55.0, device=DEV)
        ops.logits_prepare(zd, seen, p, out_full[:, :V], lse)
        assert torch.equal(out_full[:, :V].cpu(), G.penalise(z, mask, p)), p
        assert bool((out_full[:, V:] == 77.0).all()) and float(lse[B]) == 55.0, "canaries"
        assert torch.equal(zd_full, raw), "the raw logits stay intact"
        assert torch.equal(G.as_u32(seen), want_bm)
        lses.append(lse[:B].cpu())
    # no bitmap: out is not written, the lse is the same number
    out_full = torch.full((B, V), 77.0, device=DEV)
    lse = torch.full((B,), 55.0, device=DEV)
    ops.logits_prepare(zd, None, 1.0, out_full, lse)
    assert bool((out_full == 77.0).all())
    lses.append(lse.cpu())
    # a bitmap and no lse
    out2 = torch.full((B, V), 77.0, device=DEV)
    ops.logits_prepare(zd, seen, 1.3, out2, None)
    assert torch.equal(out2.cpu(), G.penalise(z, mask, 1.3))
    for l in lses[1:]:
        assert torch.equal(l, lses[0]), "penalty and bitmap do not enter the raw log-sum-exp"
    err = (lses[0].double() - ref64).abs()
    print(f"V {V} B {B} pad {pad}: max |lse - fp64| = {float(err.max()):.3e}, bound {float(bound.min()):.3e} .. {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), (err, bound)


def test_logits_prepare_special_rows():
    """NaN and +-inf pass through: a row of -inf has lse -inf, a +inf makes it +inf, a NaN makes it NaN (torch.logsumexp's values)."""
    V = 640
    z = torch.randn(4, V, generator=torch.Generator().manual_seed(4))
    z[0] = -math.inf
    z[1, 100] = math.inf
    z[2, 5] = math.nan
    lse = torch.empty(4, device=DEV)
    seen = dev_bitmap(G.seen_bitmap([[100, 5, 3]] * 4, V))
    out = torch.empty(4, V, device=DEV)
    ops.logits_prepare(z.to(DEV), seen, 1.3, out, lse)
    got, want = lse.cpu(), torch.logsumexp(z, dim=-1)
    assert got[0] == -math.inf and got[1] == math.inf and math.isnan(got[2]) and abs(float(got[3] - want[3])) < 1e-5
    o = out.cpu()
    assert o[1, 100] == math.inf and math.isnan(o[2, 5]) and o[0, 3] == -math.inf


# ------------------------------------------------------------------ 3. generate_record
@pytest.mark.parametrize("mode", ["col", "cur"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_generate_record_is_the_restatement(V, B, mode):
    """lp bit-equal to z[tok] - lse[b] in fp32 from the GPU's own lse, the bit set; a row stopped before the step, an idle row
    (cur < 0) and a teacher-forced position leave the lp canary and the bitmap alone; both addressings."""
    z, _, _, start, _ = case(V, B)
    wpr = G.words(V)
    zd = z.to(DEV)
    lse = torch.empty(B, device=DEV)
    ops.logits_prepare(zd, None, 1.0, None, lse)
    W, L = 6, 4
    tokens = torch.zeros(B, W, dtype=torch.int64)
    chosen = [32, 5, V - 1]
    tokens[:, 3] = torch.tensor(chosen[:B])
    tokens[:, 1] = torch.tensor([V - 3, 0, 31][:B])
    runs = []
    if mode == "col":        # column 3: row 0 at generated index 1, row 1 teacher-forced (prompt of 4), row 2 at index 3
        runs.append(dict(col=3, prompt_len=[2, 4, 0][:B]))
        runs.append(dict(col=3, prompt_len=[2, 4, 0][:B], stopped_before=[True, False, False][:B]))
        runs.append(dict(col=1, prompt_len=[0, 0, 0][:B], stopped_before=[False, True, False][:B]))
    else:                    # cur is the step kernel's, already advanced: the id sits at cur - 1
        runs.append(dict(cur=[4, 4, 4][:B], prompt_len=[1, 3, 0][:B]))
        runs.append(dict(cur=[4, -1, 0][:B], prompt_len=[3, 0, 0][:B]))                                  # idle rows
        runs.append(dict(cur=[2, 4, W + 1][:B], prompt_len=[1, 0, 0][:B], stopped_before=[False, True, False][:B]))
        runs.append(dict(cur=[6, 6, 6][:B], prompt_len=[0, 1, 2][:B]))             # generated index 5, 4 (past the lp row: marked only), 3
    for kw in runs:
        for with_seen, with_lp in ((True, True), (True, False), (False, True)):
            lp = torch.full((B, L + 1), 7.0)
            lp_d = lp.to(DEV)
            bm = start.clone()
            seen = dev_bitmap(start)
            dkw = {k: (v if k == "col" else (torch.tensor(v, device=DEV) if k == "stopped_before" else i32(v))) for k, v in kw.items()}
            ops.generate_record(zd, lse if with_lp else None, tokens.to(DEV), seen if with_seen else None, lp_d[:, :L] if with_lp else None, **dkw)
            G.generate_record(z, lse.cpu(), tokens, bm if with_seen else None, lp[:, :L] if with_lp else None, V,
                              **{k: (v if k == "col" else torch.tensor(v)) for k, v in kw.items()})
            assert torch.equal(lp_d.cpu(), lp), (kw, with_seen, with_lp)
            assert torch.equal(G.as_u32(seen), bm), (kw, with_seen, with_lp)
            sb = kw.get("stopped_before", [False] * B)
            for b in range(B):
                idle = "cur" in kw and not 0 < kw["cur"][b] <= W
                if sb[b] or idle:
                    assert bool((lp_d[b] == 7.0).all()) and torch.equal(G.as_u32(seen)[b], start[b]), (kw, b)
    # the first run wrote something (the restatement is not vacuous): row 0's value and bit
    lp_d = torch.full((B, L), 7.0, device=DEV)
    seen = dev_bitmap(start)
    kw = runs[0]
    ops.generate_record(zd, lse, tokens.to(DEV), seen, lp_d, col=kw.get("col", 0), cur=i32(kw["cur"]) if "cur" in kw else None,
                        prompt_len=i32(kw["prompt_len"]))
    g0 = 3 - kw["prompt_len"][0]
    assert float(lp_d[0, g0]) == float(z[0, 32] - lse.cpu()[0]) and int(G.as_u32(seen)[0, 1]) & 1


# ------------------------------------------------------------------ 4. model level
PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
GEN = 8
PEN = 1.3
REL = 1e-3                  # the fp32 model bound of tests/test_gpu_model.py: logits within 1e-3 of max |logit|


def _tiny_meta(dtype=torch.float32, max_seq_len=96):
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=max_seq_len)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(dtype).to(DEV)
    dec = ref_cpu.OracleDecoder(ref_cpu.OracleArgs(vocab_size=V, **{**TINY, "max_seq_len": max_seq_len}), sd)
    return mm, dec


@pytest.fixture(scope="module")
def text_case():
    """The oracle's answers, computed once: per prompt alone (generate_many's semantics) with and without the penalty, and what a
    refilled row would give if it inherited the seen set of the prompt before it."""
    mm, dec = _tiny_meta()
    eos = mm.tokenizer.eos_id
    pt = [mm.tokenizer.encode(p, bos=True, eos=False) for p in PROMPTS]
    plain = [G.oracle_replay(ref_cpu, dec, [t], GEN, eos, 1.0) for t in pt]
    pen = [G.oracle_replay(ref_cpu, dec, [t], GEN, eos, PEN) for t in pt]
    assert any(a[0] != b[0] for a, b in zip(plain, pen)), "the penalty changes a token of the oracle's own answers"
    inherit = [G.oracle_replay(ref_cpu, dec, [pt[i]], GEN, eos, PEN, extra_seen=set(pt[i - 1]) | set(pen[i - 1][0][0]))[0][0] for i in range(1, len(pt))]
    assert all(a != b[0][0] for a, b in zip(inherit, pen[1:])), "inheriting the previous prompt's seen set would change every refilled answer"
    # the scale of the logits (for the model tolerance of a log-prob: two logit errors, z[tok] and the lse)
    scale = float(dec.forward_inference(torch.tensor([pt[1]]), 0).abs().max())
    return mm, dec, pt, plain, pen, scale


def _check_scores(scores, ids, want_lps, scale, V):
    for sc, t, w in zip(scores, ids, want_lps):
        assert len(sc["logprobs"]) == len(t) == len(w)
        assert sc["sum"] == float(sum(sc["logprobs"]))
        # the model tolerance on z[tok] and on the lse (a soft maximum of the logits: no further off than they are), plus lse_bound at
        # this row size (k = 2 folds, D <= max d_i <= 2 scale, log S <= log V, |lse| <= scale + log V) and the subtraction's rounding
        tol = 2 * REL * scale + G.U32 * (1.01 * (4 * 2 + 33 + 2 * scale) + 2 * math.log(V) + (scale + math.log(V)) + (2 * scale + math.log(V)))
        err = max((abs(a - b) for a, b in zip(sc["logprobs"], w)), default=0.0)
        print(f"max |lp - oracle fp64| = {err:.3e} (tolerance {tol:.3e}, {len(t)} tokens)")
        assert err <= tol, (sc["logprobs"], w)
        assert all(x <= 0 for x in sc["logprobs"])


def test_generate_unequal_prompts_penalty_and_logprobs_equal_the_oracle_replay(text_case):
    mm, dec, pt, _, _, scale = text_case
    V = mm.tokenizer.n_words
    eos = mm.tokenizer.eos_id
    sel = [0, 2, 4]                                          # prompts of 9, 5 and 6 tokens: rows 0 and 2 are teacher-forced at first
    assert len({len(pt[i]) for i in sel}) == 3
    want_ids, want_lps = G.oracle_replay(ref_cpu, dec, [pt[i] for i in sel], GEN, eos, PEN)
    greedy_ids, _ = G.oracle_replay(ref_cpu, dec, [pt[i] for i in sel], GEN, eos, 1.0)
    assert want_ids != greedy_ids
    texts, ids, scores = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, repetition_penalty=PEN, return_logprobs=True, return_ids=True)
    assert ids == want_ids, (ids, want_ids)
    assert texts == [mm.tokenizer.decode(t) for t in want_ids]
    _check_scores(scores, ids, want_lps, scale, V)
    # without return_ids: (texts, scores); log-probs alone do not change the answer, and score the greedy tokens
    t2, s2 = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, repetition_penalty=PEN, return_logprobs=True)
    assert t2 == texts and s2 == scores
    t3, i3, s3 = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, return_logprobs=True, return_ids=True)
    assert i3 == greedy_ids
    _check_scores(s3, i3, G.oracle_replay(ref_cpu, dec, [pt[i] for i in sel], GEN, eos, 1.0)[1], scale, V)
    # the penalty alone: a plain list of strings
    t4 = mm.generate([PROMPTS[i] for i in sel], None, max_gen_len=GEN, repetition_penalty=PEN)
    assert isinstance(t4, list) and t4 == texts


@pytest.mark.parametrize("rows", [1, 2])
def test_generate_many_penalty_and_logprobs_equal_the_oracle_per_prompt(text_case, rows):
    """More prompts than rows: a refilled row must not inherit the seen set of the prompt that ran in it before (text_case asserts on
    the CPU that inheriting would change every refilled answer)."""
    mm, dec, pt, plain, pen, scale = text_case
    V = mm.tokenizer.n_words
    texts, ids, scores = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, repetition_penalty=PEN, return_logprobs=True,
                                          return_ids=True)
    assert ids == [p[0][0] for p in pen], (rows, ids)
    assert texts == [mm.tokenizer.decode(t) for t in ids]
    _check_scores(scores, ids, [p[1][0] for p in pen], scale, V)
    t2, s2 = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_logprobs=True, poll_every=3)
    assert t2 == [mm.tokenizer.decode(p[0][0]) for p in plain]
    _check_scores(s2, [p[0][0] for p in plain], [p[1][0] for p in plain], scale, V)


def test_stream_generate_penalty_and_logprobs(text_case):
    mm, dec, pt, plain, pen, scale = text_case
    last = None
    for last in mm.stream_generate(PROMPTS[0], None, max_gen_len=GEN, repetition_penalty=PEN, return_logprobs=True):
        pass
    assert last["end_of_content"] and last["text"] == mm.tokenizer.decode(pen[0][0][0])
    _check_scores([{"logprobs": last["logprobs"], "sum": float(sum(last["logprobs"]))}], [pen[0][0][0]], [pen[0][1][0]], scale, mm.tokenizer.n_words)
    plain_last = list(mm.stream_generate(PROMPTS[0], None, max_gen_len=GEN))[-1]
    assert set(plain_last) == {"text", "end_of_content"}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_defaults_are_a_no_op(dtype, text_case):
    """Defaults: the same type and strings as before; return_logprobs alone (penalty 1.0) leaves the strings identical."""
    mm = text_case[0] if dtype == torch.float32 else _tiny_meta(dtype)[0]
    P3 = [PROMPTS[i] for i in (0, 2, 4)]
    base = mm.generate(P3, None, max_gen_len=GEN)
    assert isinstance(base, list) and all(isinstance(t, str) for t in base)
    if dtype == torch.float32:
        want = ref_cpu.generate_greedy(text_case[1], [text_case[2][i] for i in (0, 2, 4)], max_gen_len=GEN, eos_id=mm.tokenizer.eos_id)[1]
        assert base == [mm.tokenizer.decode(t) for t in want]
    texts, scores = mm.generate(P3, None, max_gen_len=GEN, return_logprobs=True, repetition_penalty=1.0)
    assert texts == base and len(scores) == 3 and all(set(s) == {"logprobs", "sum"} for s in scores)
    for T in (0.0, 0.7):
        U = torch.rand(GEN + 40, 3, generator=torch.Generator().manual_seed(5))
        a = mm.generate(P3, None, max_gen_len=GEN, temperature=T, top_p=0.75, sample_uniforms=U)
        b, _ = mm.generate(P3, None, max_gen_len=GEN, temperature=T, top_p=0.75, sample_uniforms=U, return_logprobs=True)
        assert a == b, T
    many = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN)
    assert isinstance(many, list) and mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, return_logprobs=True)[0] == many


# ------------------------------------------------------------------ 5. the eval entry
def test_eval_entry_save_scores_adds_two_keys_and_nothing_else(tmp_path):
    from a3vlm_amd import checkpoint as ck
    vit = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({**{k: v for k, v in TINY.items() if k != "max_seq_len"}, **vit}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, **TINY), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(64, width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    ckdir = ck.save_checkpoint(str(tmp_path / "ck"), types.SimpleNamespace(precision="tf32", only_save_trainable=False), mm, None, None, None, epoch=0)
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_v2", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2", "--num_workers", "0",
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "10", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32"]
    for flag, extra in (("plain", []), ("scores", ["--save_scores"])):
        r = subprocess.run(cmd + ["--addition_flag", flag] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    plain = json.load(open(tmp_path / "logs" / "plain" / "demo.json"))
    keys = {"answer", "format_answer", "annotation", "question", "image", "fail"}
    assert len(plain) == 3 and all(set(r) == keys for r in plain), "without the flag: today's record, no logprob_sum, no logprobs"
    recs = json.load(open(tmp_path / "logs" / "scores" / "demo.json"))
    assert len(recs) == 3
    for r, p in zip(recs, plain):
        assert set(r) == keys | {"logprob_sum", "logprobs"}
        assert {k: r[k] for k in keys} == p, "otherwise identical"
        assert len(r["logprobs"]) > 0 and r["logprob_sum"] == float(sum(r["logprobs"])) and r["logprob_sum"] < 0
