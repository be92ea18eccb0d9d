"""-m gpu: the NF4 mode through its user-facing entry points -- MetaModel.from_pretrained(quant="nf4") on a checkpoint folder in the
reference layout, and the eval_affordance_with_quant --quant batch-inference flow (the demo of test_gpu_eval_entry.py)."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import nf4_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden")
DEC = dict(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, multiple_of=256, norm_eps=1e-5, rope_theta=10000.0)
VIT = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=5)
QUANT = (".wq.weight", ".wk.weight", ".wv.weight", ".wo.weight", ".w1.weight", ".w2.weight", ".w3.weight")


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from a3vlm_amd import checkpoint as ck
    from a3vlm_amd.model.meta import MetaModel
    from oracle import ref_cpu
    tmp = tmp_path_factory.mktemp("nf4ck")
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps({**DEC, **VIT}))
    mm = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    V = mm.tokenizer.n_words
    sd = ref_cpu.make_decoder_weights(ref_cpu.OracleArgs(vocab_size=V, max_seq_len=512, **DEC), seed=0, std=0.08)
    vsd = ref_cpu.make_vision_weights(DEC["dim"], width=64, layers=2, patch=14, grid=8, seed=1, std=0.05)
    mm.llma.load_state_dict({**sd, **vsd})
    args = types.SimpleNamespace(precision="tf32", only_save_trainable=False)
    ckdir = ck.save_checkpoint(str(tmp / "ck"), args, mm, None, None, None, epoch=0)
    return cfgp, ckdir, {**sd, **vsd}, tmp


def _wd_model(cfgp, sd):
    """bf16 MetaModel holding Wd = bf16(NF4[q] * s_b) in every quantised module (the CPU restatement of the format)"""
    from a3vlm_amd.model.meta import MetaModel
    sdq = {}
    for k, v in sd.items():
        v = v.to(torch.bfloat16)
        if k == "output.weight" or (k.startswith("layers.") and k.endswith(QUANT)):
            nib, sc, _ = R.quantize(v)
            v = R.dequantize(nib, sc)
        sdq[k] = v
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            md = MetaModel("llama_ens5", str(cfgp), os.path.join(GD, "tokenizer.model"), with_visual=True, max_seq_len=512)
    finally:
        torch.set_default_dtype(old)
    md.llma.load_state_dict(sdq)
    md.eval()
    return md


def test_from_pretrained_nf4_greedy_ids_match_the_bf16_model_on_wd(ckpt):
    from a3vlm_amd.model.meta import MetaModel
    cfgp, ckdir, sd, _ = ckpt
    mq = MetaModel.from_pretrained(ckdir, llama_type="llama_ens5", llama_config=[str(cfgp)], tokenizer_path=os.path.join(GD, "tokenizer.model"),
                                   with_visual=True, max_seq_len=512, quant="nf4")
    assert mq.llma.weight_format == "nf4" and mq.llma._weights.images
    names = mq.state_dict()
    assert "llma.layers.0.attention.wq.weight" not in names and "llma.output.weight" not in names
    assert "llma.layers.0.attention_norm.weight" in names
    with pytest.raises(RuntimeError, match="NF4"):
        mq.train_engine()
    md = _wd_model(cfgp, sd)
    prompts = ["Detect all manipulable object parts.", "the quick brown fox"]
    _, ids_q = mq.generate(prompts, None, max_gen_len=12, temperature=0, return_ids=True)
    _, ids_d = md.generate(prompts, None, max_gen_len=12, temperature=0, return_ids=True)
    # decided positions: the Wd model's top-1 / top-2 logit gap exceeds the NF4-vs-Wd deviation (measured ~1-2e-2 of max|logit|,
    # test_gpu_nf4.py); the ids must agree up to the first position that is not decided
    decided_any = 0
    for b, p in enumerate(prompts):
        tok = mq.tokenizer.encode(p, bos=True, eos=False)
        seq = torch.tensor([tok + ids_d[b]], device="cuda")
        lg = md.llma.forward_inference(seq[:, :len(tok)], 0).float()
        n_ok = 0
        for j in range(len(ids_d[b])):
            top = lg[0].topk(2).values
            if float(top[0] - top[1]) < 5e-2 * float(lg.abs().max()):
                break
            assert ids_q[b][j] == ids_d[b][j], (b, j, ids_q[b], ids_d[b])
            n_ok += 1
            if j + 1 < len(ids_d[b]):
                lg = md.llma.forward_inference(seq[:, len(tok) + j:len(tok) + j + 1], len(tok) + j).float()
        decided_any += n_ok
    assert decided_any > 0


def test_eval_affordance_with_quant_demo(ckpt):
    cfgp, ckdir, _, tmp = ckpt
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "a3vlm_amd.eval_affordance_with_quant", "--llama_type", "llama_ens5", "--llama_config", str(cfgp),
           "--tokenizer_path", os.path.join(GD, "tokenizer.model"), "--pretrained_path", ckdir, "--batch_size", "2",
           "--num_workers", "0", "--dataset", os.path.join(GD, "demo", "demo.json"), "--input_size", "224",
           "--max_gen_len", "10", "--max_seq_len", "512", "--temperature", "0", "--image_root", os.path.join(GD, "demo"),
           "--output_root", str(tmp / "logs"), "--precision", "bf16"]
    r = subprocess.run(cmd + ["--addition_flag", "q", "--quant"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "'missing_keys': [], 'unexpected_keys': []" in r.stdout
    recs = json.load(open(tmp / "logs" / "q" / "demo.json"))
    assert len(recs) == 3 and set(recs[0]) == {"answer", "format_answer", "annotation", "question", "image", "fail"}
    assert recs[0]["answer"] == recs[1]["answer"]          # the three demo items share image and question
    # --quant with the fp32 parity path is refused up front
    r2 = subprocess.run(cmd[:-1] + ["tf32", "--addition_flag", "f", "--quant"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r2.returncode != 0 and "--precision bf16" in (r2.stdout + r2.stderr)
