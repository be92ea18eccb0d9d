"""-m gpu: prefix sharing at model level -- Transformer.extend_rows and generate_many(prefix_sharing=True) on the tiny bf16 models
of the other GPU model tests (hd 64 and hd 128), with an image in front of every prompt."""
import os

import pytest
import torch

from a3vlm_amd import ops
from a3vlm_amd.model.LLM import llama_ens5 as plugin
from a3vlm_amd.model.meta import MetaModel
from oracle import ref_cpu
from oracle.gen_golden import synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
GEOM = {64: dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256),
        128: dict(dim=512, n_layers=2, n_heads=4, n_kv_heads=4, multiple_of=256)}
STEM = "Where is the drawer handle of the cabinet, and which way does it open? " * 2       # 85 tokens in front of every question
QUESTIONS = [STEM + q for q in ("Detect the lid", "Open", "Find the door of the microwave", "Find the axis", "Which way does the lid turn")]
IMAGE_OF = [0, 0, 0, 1, 1]                  # 5 questions over 2 images; batch_rows = 3: one member of the first run has to wait
ROWS, GEN = 3, 6
# Per-token |log-prob of generate_many's decode step - log-prob of a teacher-forced prefill_row| of the PLAIN loop
# (prefix_sharing=False, the path of the parent commit) on these models, prompts and images, maximum over every returned token:
# profiles/prefix_extend.md.  The sharing path is held to twice that.
PARENT_DIFF = {64: 0.015830, 128: 0.028377}


_MODELS = {}


def _meta(hd):
    if hd not in _MODELS:
        mm = MetaModel("llama_ens5", os.path.join(GD, "tiny_params.json"), os.path.join(GD, "tokenizer.model"), with_visual=False, max_seq_len=256)
        V = mm.tokenizer.n_words
        g = GEOM[hd]
        m = plugin.Transformer(plugin.ModelArgs(vocab_size=V, max_seq_len=256, max_batch_size=4, **g, vit_width=64, vit_layers=2, vit_heads=4,
                                                vit_crop=112, n_views=1), with_visual=True)
        sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=256, **g), seed=0, std=0.05)
        vsd = ref_cpu.make_vision_weights(g["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
        m.load_state_dict({**sd, **vsd})
        mm.llma = m.to(BF).to(DEV)
        imgs = synth_image(2, size=112, seed=3).to(DEV)
        _MODELS[hd] = (mm, imgs)
    return _MODELS[hd]


def _teacher_forced(mm, prompt_ids, ids, image):
    out = []
    for t in range(len(ids)):
        z = mm.llma.prefill_row(0, torch.tensor([prompt_ids + ids[:t]], dtype=torch.long, device=DEV), image)[0].double()
        out.append(float((z - torch.logsumexp(z, -1))[ids[t]]))
    return out


def logprob_difference(hd, sharing):
    """max |returned per-token log-prob - teacher-forced prefill_row log-prob| over the greedy answers of the five questions"""
    mm, imgs = _meta(hd)
    images = [imgs[k] for k in IMAGE_OF]
    kw = dict(prefix_sharing=True, image_ids=IMAGE_OF) if sharing else {}
    _, ids, sc = mm.generate_many(QUESTIONS, torch.stack(images), batch_rows=ROWS, max_gen_len=GEN, return_ids=True, return_logprobs=True, **kw)
    worst = 0.0
    for q, k, i, s in zip(QUESTIONS, IMAGE_OF, ids, sc):
        assert len(i) > 0 and len(s["logprobs"]) == len(i)
        tf = _teacher_forced(mm, mm.tokenizer.encode(q, bos=True, eos=False), i, imgs[k:k + 1])
        worst = max([worst] + [abs(a - b) for a, b in zip(s["logprobs"], tf)])
    return worst


@pytest.mark.parametrize("hd", [64, 128])
def test_extend_rows_equals_the_entries_by_hand_and_the_whole_prefill(hd):
    mm, imgs = _meta(hd)
    m = mm.llma
    W = m.image_words
    pt = [mm.tokenizer.encode(q, bos=True, eos=False) for q in QUESTIONS[:3]]
    C = W + min(len(os.path.commonprefix([pt[0], t])) for t in pt)
    P = min(C, W + min(map(len, pt)) - 1) & ~63
    assert P >= 128 and P >= W + 1, (P, W, C)
    whole = []
    m.allocate_rows(4)
    for t in pt:                                              # the reference: the whole prompt through prefill_row (row 3)
        whole.append(m.prefill_row(3, torch.tensor([t], device=DEV), imgs[:1])[0].clone())
    m.prefill_row(1, torch.tensor([pt[0][:P - W]], device=DEV), imgs[:1])
    for i in range(m.n_layers):                               # the members' own rows hold NaN wherever the prefix would be
        for r in (0, 2):
            m._k_cache[i][r] = float("nan")
            m._vt_cache[i][r] = float("nan")
    rows = [2, 1, 0]                                          # not in row order: the logits come back in the order of the call
    sfx = [torch.tensor(t[P - W:], device=DEV) for t in pt]
    before = [(k.clone(), v.clone()) for k, v in zip(m._k_cache, m._vt_cache)]
    got = m.extend_rows(rows, sfx, [P] * 3, src_row=[1] * 3, shared=[P] * 3).clone()
    assert torch.isfinite(got).all()
    bound = 3e-2                                              # tests/test_gpu_model.py: two bf16 paths, relative to max |logit|
    for j in range(3):
        err = float((got[j] - whole[j]).abs().max() / whole[j].abs().max())
        print(f"hd {hd} member {j}: extend vs whole prefill {err:.3e}")
        assert err < bound, (j, err)
    # by hand: the same public entries, kernel by kernel, on the caches as they were
    for (k, v), kc, vc in zip(before, m._k_cache, m._vt_cache):
        kc.copy_(k)
        vc.copy_(v)
    a, H, Hkv = m.args, m.n_heads, m.n_kv_heads
    order = sorted(range(3), key=lambda j: rows[j])
    lens = [len(sfx[j]) for j in order]
    q_off = [0, lens[0], lens[0] + lens[1], sum(lens), sum(lens)]
    sk = [P + n for n in lens] + [0]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    M = sum(lens)
    h = torch.empty(M, a.dim, dtype=BF, device=DEV)
    ops.embed_assemble(torch.cat([sfx[j] for j in order]).view(M, 1), m.tok_embeddings.weight, h, M, 1, 0, a.dim)
    xn, att = torch.empty_like(h), torch.empty(M, H * hd, dtype=BF, device=DEV)
    qkv = torch.empty(M, (H + 2 * Hkv) * hd, dtype=BF, device=DEV)
    act = torch.empty(M, m.ffn, dtype=BF, device=DEV)
    sc = torch.empty(ops.attention_extend_rows_scratch_floats(4, H, hd, 256), dtype=torch.float32, device=DEV)
    cs = m._cos_sin_dev()
    ld = qkv.stride(0)
    st = (ld, ld, hd, Hkv * 256 * hd, 256 * hd, hd, Hkv * hd * 256, hd * 256, 256, H * hd, H * hd, hd)
    for i in range(m.n_layers):
        kc, vc = m._k_cache[i], m._vt_cache[i]
        m._layer(i, "bf16", h, (xn, qkv, att, act),
                 lambda: ops.rope_kvcache_extend(qkv, qkv, kc, vc, cs, i32(q_off), i32(sk), max(lens), 4, H, Hkv, hd),
                 lambda: ops.attention_extend_rows(qkv, kc, vc, att, i32(q_off), i32(sk), max(lens), max(sk), 4, H, Hkv, hd, st, sc,
                                                   i32([1, 1, 1, 3]), i32([P, P, P, 0])))
    last = [q_off[r + 1] - 1 for r in range(3)]
    xl = torch.empty(3, a.dim, dtype=BF, device=DEV)
    ops.rmsnorm(h, m.norm.weight, xl, a.norm_eps, row_idx=i32(last))
    hand = torch.empty(3, a.vocab_size, dtype=torch.float32, device=DEV)
    m._lm_head_last(xl, hand, False)
    for j in range(3):
        assert torch.equal(got[j], hand[rows[j]]), j
    for r in (0, 2):                                          # a member's own row: written from P on, NaN below
        assert torch.isnan(m._k_cache[0][r][:, :P].float()).all() and torch.isfinite(m._k_cache[0][r][:, P:sk[r]].float()).all()
    with pytest.raises(ValueError, match="empty suffix"):
        m.extend_rows([0], [torch.tensor([], dtype=torch.long)], [P])
    with pytest.raises(ValueError, match="cache length"):
        m.extend_rows([0], [torch.tensor([1, 2, 3])], [254])


@pytest.mark.parametrize("hd", [64, 128])
def test_generate_many_prefix_sharing_logprobs_and_one_encode_per_run(hd):
    mm, imgs = _meta(hd)
    calls = []
    orig = mm.llma.encode_image_into

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    mm.llma.encode_image_into = counted
    try:
        images = torch.stack([imgs[k] for k in IMAGE_OF])
        mm.generate_many(QUESTIONS, images, batch_rows=ROWS, max_gen_len=GEN, prefix_sharing=True, image_ids=IMAGE_OF)
        assert len(calls) == 2, "one image encode per run: 5 questions over 2 images"
        del calls[:]
        mm.generate_many(QUESTIONS, images, batch_rows=ROWS, max_gen_len=GEN)
        assert len(calls) == 5
    finally:
        del mm.llma.encode_image_into
    diff = logprob_difference(hd, sharing=True)
    print(f"hd {hd}: sharing path vs teacher-forced {diff:.6f}; plain loop {PARENT_DIFF[hd]}")
    assert PARENT_DIFF[hd] is not None, "the plain loop's deviation is measured and written down first"
    assert diff <= 2 * PARENT_DIFF[hd], (diff, PARENT_DIFF[hd])


def test_a_list_without_repeated_images_is_the_plain_call():
    mm, imgs = _meta(64)
    qs, images = QUESTIONS[:2], imgs[:2]
    want = mm.generate_many(qs, images, batch_rows=2, max_gen_len=GEN, return_ids=True)
    assert mm.generate_many(qs, images, batch_rows=2, max_gen_len=GEN, return_ids=True, prefix_sharing=True) == want
    assert mm.generate_many(qs, images, batch_rows=2, max_gen_len=GEN, return_ids=True, prefix_sharing=True, image_ids=["a", "b"]) == want
