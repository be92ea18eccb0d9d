"""-m gpu: constrained decoding (a3v_constrain.hip, model/constrain.py, MetaModel.generate / generate_many(constraint=...)) -- the two
kernels bit for bit against the integer restatements of tests/constrain_ref.py, the samplers on masked rows, the generation loops
against a host loop that masks with the reference, and the eval entry."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
from a3vlm_amd import ops
from a3vlm_amd.model import constrain as C
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")


def dev_bits(x):
    """uint32 numpy [B, ld] -> fp32 device tensor with the same bits"""
    return torch.from_numpy(x.view(np.int32).copy()).to(DEV).view(torch.float32)


def bits_of(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. a3v_constrain_logits
@pytest.mark.parametrize("V", [1, 7, 8, 9, 511, 32000, 32003])
def test_constrain_logits_is_bit_equal_to_the_reference(V):
    """B in {1, 3, 32} x ld in {V, V + 3} x in place / out of place (the out buffer once on the logits' 16-byte phase, once a
    column off it: the scalar form).  Odd V and ld put the rows and the int16 table rows on every alignment."""
    for B in (1, 3, 32):
        for ld in (V, V + 3):
            x, trans, state = CR.logits_case(B, V, ld, seed=V + B)
            t_dev = torch.from_numpy(trans).to(DEV)
            s_dev = torch.from_numpy(state).to(DEV)
            for mode, ld_out in (("in place", ld), ("out", ld), ("out, other phase", ld + 1)):
                buf = dev_bits(x)
                before = x if mode == "in place" else np.full((B, ld_out), 0x12345678, dtype=np.uint32)
                obuf = buf if mode == "in place" else dev_bits(before)
                got = ops.constrain_logits(buf[:, :V], t_dev, s_dev, obuf[:, :V])
                assert got.data_ptr() == obuf.data_ptr()
                want = CR.constrain_logits_ref(x, V, trans, state, before)
                assert np.array_equal(bits_of(obuf), want), (B, ld, mode)
                if mode != "in place":
                    assert np.array_equal(bits_of(buf), x), "the logits are not written"


def test_constrain_logits_argument_errors_launch_nothing():
    from a3vlm_amd import lib
    x = torch.zeros(2, 8, device=DEV)
    t = torch.zeros(2, 8, dtype=torch.int16, device=DEV)
    s = torch.zeros(2, dtype=torch.int32, device=DEV)
    f = lib.load().a3v_constrain_logits
    st = torch.cuda.current_stream().cuda_stream
    assert f(x.data_ptr(), 8, t.data_ptr(), 8, 2, s.data_ptr(), x.data_ptr(), 8, 2, st) == 0
    for args in ((None, 8, t.data_ptr(), 8, 2, s.data_ptr(), x.data_ptr(), 8, 2, st),
                 (x.data_ptr(), 7, t.data_ptr(), 8, 2, s.data_ptr(), x.data_ptr(), 8, 2, st),
                 (x.data_ptr(), 8, t.data_ptr(), 0, 2, s.data_ptr(), x.data_ptr(), 8, 2, st),
                 (x.data_ptr(), 8, t.data_ptr(), 8, 0, s.data_ptr(), x.data_ptr(), 8, 2, st),
                 (x.data_ptr(), 8, t.data_ptr(), 8, 40000, s.data_ptr(), x.data_ptr(), 8, 2, st),
                 (x.data_ptr(), 8, t.data_ptr(), 8, 2, s.data_ptr(), x.data_ptr(), 8, 0, st)):
        assert f(*args) == -3, args


# ------------------------------------------------------------------ 2. a3v_constrain_advance
def test_constrain_advance_is_bit_equal_to_the_reference_in_both_forms():
    forms = set()
    for case in CR.advance_cases():
        want = CR.constrain_advance_ref(**case)
        state = torch.from_numpy(case["state"].copy()).to(DEV)
        cur = None if case["cur"] is None else torch.from_numpy(case["cur"]).to(DEV)
        sb = None if case["stopped_before"] is None else torch.from_numpy(case["stopped_before"]).to(DEV)
        ops.constrain_advance(torch.from_numpy(case["tokens"]).to(DEV), torch.from_numpy(case["trans"]).to(DEV), state,
                              torch.from_numpy(case["first"]).to(DEV), col=case["col"], cur=cur, stopped_before=sb)
        assert np.array_equal(state.cpu().numpy(), want), case["col"]
        forms.add((cur is None, sb is None))
    assert len(forms) == 4


# ------------------------------------------------------------------ 3. the samplers and the argmax on masked rows
def test_samplers_and_argmax_never_return_a_masked_id():
    V, N = 512, 2000
    rng = np.random.default_rng(5)
    trans = np.full((3, V), -1, dtype=np.int16)
    for s, k in enumerate((1, 2, 37)):
        trans[s, rng.choice(V, size=k, replace=False)] = 0
    allowed = torch.from_numpy(trans >= 0).to(DEV)
    state = torch.arange(3 * N, dtype=torch.int32, device=DEV) % 3
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(3 * N, V, generator=g) * 4).to(DEV)
    z = ops.constrain_logits(logits, torch.from_numpy(trans).to(DEV), state, torch.empty_like(logits))
    assert bool((torch.isinf(z) & (z < 0)).eq(~allowed[state.long()]).all())
    u = torch.rand(3 * N, generator=g).to(DEV)
    u[:6] = torch.tensor([0.0, 0.0, 0.0, 0.99999994, 0.99999994, 0.99999994])
    out = torch.empty(3 * N, dtype=torch.long, device=DEV)
    only = torch.from_numpy(np.flatnonzero(trans[0] >= 0)).to(DEV)
    draws = {}
    for T in (1.0, 0.1):                                  # 0.1: most allowed masses underflow to 0 as the masked ones do
        for top_p in (0.75, 1.0):
            draws[("top_p", T, top_p)] = ops.sample_top_p(z, T, top_p, u, out).clone()
            draws[("top_k_p", T, top_p)] = ops.sample_top_k_p(z, T, 50, top_p, 0.02, u, out).clone()      # 50 > 37: the k-th value is -inf
        draws[("top_k", T)] = ops.sample_top_k_p(z, T, 5, 0.9, 0.0, u, out).clone()
        draws[("min_p", T)] = ops.sample_top_k_p(z, T, 0, 0.9, 0.3, u, out).clone()
    draws["argmax"] = ops.argmax(z, out).clone()
    for name, ids in draws.items():
        assert bool(((ids >= 0) & (ids < V)).all()), name
        assert bool(allowed[state.long(), ids].all()), f"{name}: a masked id was returned"
        assert bool((ids[0::3] == only).all()), f"{name}: the one allowed token"
    assert len(set(draws[("top_p", 1.0, 1.0)][2::3].tolist())) > 10, "the 37-token rows really sample"
    assert bool((draws["argmax"] == torch.where(allowed[state.long()], logits, torch.full_like(logits, float("-inf"))).argmax(-1)).all())


# ------------------------------------------------------------------ 4. the generation loops against a host loop
PROMPTS = ["Detect the lid", "Where is the drawer handle of the cabinet, and which way does it open?", "Open", "Find the door of the microwave",
           "Lid?"]
PATTERN = r"\[[01]\.\d{2}(,[01]\.\d{2}){3}\]"             # at most 21 characters + the optional space: every answer ends within 23 tokens
GEN = 26


@pytest.fixture(scope="module")
def tiny():
    """the tiny fp32 text model of tests/test_gpu_ragged.py"""
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=96)
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=mm.tokenizer.n_words, **TINY), seed=0, std=0.08)
    mm.llma.load_state_dict(sd)
    mm.to(torch.float32).to(DEV)
    A = mm.constraint_automaton(PATTERN)
    assert mm.constraint_automaton(PATTERN) is A, "compiled once per pattern"
    return mm, A


def host_loop(mm, A, prompts, max_gen_len, choose):
    """MetaModel.generate restated on the host: ``forward_inference`` step by step at the batch size of ``prompts``, the row masked by
    constrain_logits_ref, ``choose(row index, generated index, masked fp32 row) -> id``, the state advanced by the table; teacher-forced
    prompt positions leave the state alone.  Returns the generated id lists (cut in front of EOS)."""
    tok, V = mm.tokenizer, mm.llma.args.vocab_size
    pt = [tok.encode(p, bos=True, eos=False) for p in prompts]
    B, lo, hi = len(pt), min(map(len, pt)), max(map(len, pt))
    total = min(mm.llma.args.max_seq_len, max_gen_len + hi)
    tokens = torch.zeros((B, total), dtype=torch.long)
    for b, t in enumerate(pt):
        tokens[b, :len(t)] = torch.tensor(t)
    trans = A.trans.numpy()
    state = np.full(B, A.start, dtype=np.int32)
    stop = [None] * B
    prev = 0
    for cur in range(lo, total):
        logits = mm.llma.forward_inference(tokens[:, prev:cur].to(DEV), prev).float().cpu().numpy()
        bits = logits.view(np.uint32)
        masked = CR.constrain_logits_ref(bits, V, trans, state, bits).view(np.float32)
        for b in range(B):
            if cur < len(pt[b]):
                continue                                 # teacher forcing: the prompt token stays, the automaton has not started
            nxt = int(choose(b, cur - len(pt[b]), masked[b]))
            tokens[b, cur] = nxt
            if 0 <= state[b] < trans.shape[0]:
                state[b] = trans[state[b], nxt]
            if stop[b] is None and nxt == tok.eos_id:
                stop[b] = cur
        prev = cur
        if all(s is not None for s in stop):
            break
    return [tokens[b, len(pt[b]):(stop[b] if stop[b] is not None else total)].tolist() for b in range(B)]


def greedy(b, g, row):
    return np.argmax(row)                                 # first index on ties, as a3v_argmax


def test_generate_greedy_equals_the_host_loop(tiny):
    mm, A = tiny
    want = host_loop(mm, A, PROMPTS, GEN, greedy)
    texts, ids = mm.generate(PROMPTS, None, max_gen_len=GEN, temperature=0, return_ids=True, constraint=A)
    assert ids == want, (ids, want)
    assert mm.generate(PROMPTS, None, max_gen_len=GEN, temperature=0, return_ids=True, constraint=PATTERN)[1] == want, "a pattern string"
    for t, i in zip(texts, ids):
        assert len(i) < GEN and re.fullmatch(PATTERN, t), t
    # with a repetition penalty and log-probs: the penalised row is masked in place, the scores are the raw model's
    t2, i2, sc = mm.generate(PROMPTS, None, max_gen_len=GEN, temperature=0, return_ids=True, constraint=A, repetition_penalty=1.3,
                             return_logprobs=True)
    for t, i, s in zip(t2, i2, sc):
        assert re.fullmatch(PATTERN, t) and len(s["logprobs"]) == len(i) and all(np.isfinite(s["logprobs"])), (t, s)
    _, i3, sc3 = mm.generate(PROMPTS, None, max_gen_len=GEN, temperature=0, return_ids=True, constraint=A, return_logprobs=True)
    assert i3 == want
    # scores are the UNCONSTRAINED model's: log-softmax of the raw logits at the chosen ids (teacher-forced replay of row 2 alone)
    row = 2
    pt = mm.tokenizer.encode(PROMPTS[row], bos=True, eos=False)
    full = torch.tensor([pt + want[row]], device=DEV)
    lp = []
    for k in range(len(want[row])):
        lg = mm.llma.forward_inference(full[:, :len(pt) + k] if k == 0 else full[:, len(pt) + k - 1:len(pt) + k], 0 if k == 0 else len(pt) + k - 1)
        lp.append(float(torch.log_softmax(lg.double()[0], -1)[want[row][k]]))
    alone = mm.generate([PROMPTS[row]], None, max_gen_len=GEN, temperature=0, return_ids=True, constraint=A, return_logprobs=True)
    assert alone[1][0] == want[row]
    assert np.allclose(alone[2][0]["logprobs"], lp, rtol=0, atol=1e-4), (alone[2][0]["logprobs"], lp)


def test_generate_many_equals_the_host_loop_and_refill_resets_the_state(tiny):
    mm, A = tiny
    want = [host_loop(mm, A, [p], GEN, greedy)[0] for p in PROMPTS]
    for rows in (2, 1, 4):
        texts, ids = mm.generate_many(PROMPTS, None, batch_rows=rows, max_gen_len=GEN, return_ids=True, constraint=A)
        assert ids == want, (rows, ids, want)
        assert all(re.fullmatch(PATTERN, t) for t in texts), texts
    assert mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=GEN, return_ids=True, constraint=A, poll_every=1)[1] == want


def test_generate_many_n2_equals_the_host_loop_fed_the_same_uniforms(tiny):
    mm, A = tiny
    T, p, n = 1.0, 0.9, 2
    U = torch.rand(len(PROMPTS), n, GEN + 2, generator=torch.Generator().manual_seed(23))
    want = []
    for i, prompt in enumerate(PROMPTS):
        per = []
        for s in range(n):
            def choose(b, g, row, i=i, s=s):
                probs = torch.softmax(torch.from_numpy(row.copy())[None] / T, dim=-1)
                return int(ref_cpu.sample_top_p_at(probs, p, U[i, s, g:g + 1])[0])
            per.append(host_loop(mm, A, [prompt], GEN, choose)[0])
        want.append(per)
    assert any(a != b for a, b in want), "the two samples of a prompt differ somewhere"
    texts, ids = mm.generate_many(PROMPTS, None, batch_rows=4, max_gen_len=GEN, temperature=T, top_p=p, n=n, sample_uniforms=U,
                                  return_ids=True, constraint=A)
    assert ids == want, (ids, want)
    assert all(re.fullmatch(PATTERN, t) for per in texts for t in per), texts


def test_the_constraint_bites(tiny):
    """Sampled at temperature 1 (seed 3): every answer that ended on EOS is a full match, every answer cut by the length limit is a
    viable prefix; without the constraint the random-weight model produces no box at all."""
    mm, A = tiny
    U = torch.rand(len(PROMPTS), GEN + 2, generator=torch.Generator().manual_seed(3))
    kw = dict(batch_rows=3, temperature=1.0, top_p=0.95, sample_uniforms=U, return_ids=True)
    texts, ids = mm.generate_many(PROMPTS, None, max_gen_len=GEN, constraint=A, **kw)
    for t, i in zip(texts, ids):
        assert len(i) < GEN, "the pattern is finite: the answer ended on EOS"
        assert re.fullmatch(PATTERN, t) and A.accepts(t), t
    assert len(set(texts)) > 1
    short, sids = mm.generate_many(PROMPTS, None, max_gen_len=4, constraint=A, **kw)
    for t, i in zip(short, sids):                          # this vocabulary needs at least 5 tokens for a box: 4 never reach a match
        assert len(i) == 4 and A.viable_prefix(t) and not re.fullmatch(PATTERN, t), t
    free = mm.generate_many(PROMPTS, None, max_gen_len=GEN, constraint=None, **kw)[0]
    assert sum(re.fullmatch(PATTERN, t) is None for t in free) >= 1, free
    free_g = mm.generate(PROMPTS, None, max_gen_len=GEN, temperature=0)
    assert sum(re.fullmatch(PATTERN, t) is None for t in free_g) >= 1, free_g


def test_an_automaton_that_allows_everything_changes_nothing(tiny):
    mm, _ = tiny
    A1 = C.TokenAutomaton.allow_all(mm.llma.args.vocab_size, mm.tokenizer.eos_id)
    assert A1.n_states == 1 and bool((A1.trans == 0).all())
    U = torch.rand(GEN + 30, len(PROMPTS), generator=torch.Generator().manual_seed(4))
    for kw in (dict(temperature=0), dict(temperature=0.8, top_p=0.9, sample_uniforms=U), dict(temperature=0, repetition_penalty=1.2)):
        a = mm.generate(PROMPTS, None, max_gen_len=8, return_ids=True, return_logprobs=True, **kw)
        b = mm.generate(PROMPTS, None, max_gen_len=8, return_ids=True, return_logprobs=True, constraint=A1, **kw)
        assert a == b, kw                                  # texts, ids and every log-prob (floats compared exactly)
    Um = U.t().contiguous()
    for kw in (dict(temperature=0), dict(temperature=0.8, top_p=0.9, sample_uniforms=Um, top_k=20, min_p=0.01)):
        a = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=8, return_ids=True, return_logprobs=True, **kw)
        b = mm.generate_many(PROMPTS, None, batch_rows=2, max_gen_len=8, return_ids=True, return_logprobs=True, constraint=A1, **kw)
        assert a == b, kw


# ------------------------------------------------------------------ 5. refusals
def test_refusals_raise_before_any_launch():
    """On a model that never left the CPU: a launch would raise something else (the ops refuse host tensors)."""
    mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=96)
    with pytest.raises(ValueError, match=r"lookup=0"):
        mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=4, lookup=2, constraint=PATTERN)
    with pytest.raises(ValueError, match=r"no streaming form"):
        next(mm.stream_generate("Lid?", None, max_gen_len=4, constraint=PATTERN))
    with pytest.raises(ValueError, match="anchor"):
        mm.generate(["Lid?"], None, max_gen_len=4, constraint=r"^\d+$")
    with pytest.raises(ValueError, match="dead end"):
        mm.generate_many(["Lid?"], None, batch_rows=1, max_gen_len=4, constraint=r"\{\d+\}")      # the vocabulary has no braces
    with pytest.raises(ValueError, match="compiled for 7 tokens"):
        mm.generate(["Lid?"], None, max_gen_len=4, constraint=C.TokenAutomaton.allow_all(7))
    with pytest.raises(ValueError, match="TokenAutomaton or a pattern string"):
        mm.generate(["Lid?"], None, max_gen_len=4, constraint=5)
    assert mm.llma._cache_shape is None, "nothing was allocated"
    from a3vlm_amd.eval_affordance_v2 import check_answer_regex
    with pytest.raises(SystemExit, match="--lookup_decoding 0"):
        check_answer_regex(types.SimpleNamespace(answer_regex=r"\d", lookup_decoding=2))
    with pytest.raises(SystemExit, match="anchor"):
        check_answer_regex(types.SimpleNamespace(answer_regex=r"^\d", lookup_decoding=0))
    assert check_answer_regex(types.SimpleNamespace(answer_regex=None, lookup_decoding=3)) is None


# ------------------------------------------------------------------ 6. the eval entry
def test_eval_entry_answer_regex_writes_matching_records(tmp_path):
    """The demo fixture of tests/test_gpu_eval_entry.py.  postprocess_answer drops every '.', so the pattern has none: four integers."""
    from a3vlm_amd import checkpoint as ck
    pattern = r"\[\d{1,3}(,\d{1,3}){3}\]"
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
           "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224", "--max_gen_len", "20", "--max_seq_len", "512",
           "--temperature", "0", "--image_root", os.path.join(GD, "demo"), "--output_root", str(tmp_path / "logs"), "--precision", "tf32",
           "--addition_flag", "rx", "--answer_regex", pattern]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = json.load(open(tmp_path / "logs" / "rx" / "demo.json"))
    assert len(recs) == 3
    for rec in recs:
        assert re.fullmatch(pattern, rec["answer"]), rec["answer"]
        assert len(rec["format_answer"]) == 4
