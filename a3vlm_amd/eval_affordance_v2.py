#!/usr/bin/env python3
"""Batch inference entry point with the CLI surface of the reference's ``eval_affordance_v2.py`` (:236-259 as used by
scripts/a3vlm_infer.sh:37-44), on DP replicas: every rank takes a contiguous shard of the request list (the reference's
dormant InferenceSampler, :182-205) and runs ``MetaModel.generate`` on it; results are gathered on rank 0 and written
to ``vqa_logs/{addition_flag}/{dataset}.json`` in the reference's record format (:363-370).

The reference broadcasts every batch from rank 0 to its tensor-parallel peers (:333-334, 378-380); there are no
TP peers here, so there is no data-path collective.  ``--temperature/--top_p`` default to the reference's 0.1 / 0.75
(:46-49); ``--temperature 0`` gives the greedy (bit-exact) path.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import random
import re

import torch
import torch.distributed as dist
from PIL import Image

from .checkpoint import load_tensor_parallel_model_list
from .data.conversation import default_conversation
from .data.transform import GpuPaddedResize, T_decode_rgb, T_padded_resize
from .model.meta import MetaModel


def normalize_number(x: float) -> float:
    """eval_affordance_v2.py:207-215"""
    if x > 100:
        return x / 1000
    if x > 10:
        return x / 100
    if x >= 1:
        return x / 10
    return x


def format_bounding_box(answer: str):
    """eval_affordance_v2.py:217-232: digits and commas only, a dot before the last three digits of every 4+ digit run,
    then per-number magnitude normalisation."""
    cleaned = re.sub(r"[^\d,]", "", answer.replace(" ", ""))
    formatted = re.sub(r"\d{4,}", lambda m: m.group(0)[:-3] + "." + m.group(0)[-3:], cleaned)
    return [normalize_number(float(n)) for n in formatted.split(",") if n]


def postprocess_answer(answer: str) -> str:
    """eval_affordance_v2.py:343-357"""
    answer = answer.split("###")[0]
    answer = answer.replace(".", "").strip()
    if "answer is" in answer:
        try:
            ext = re.findall(r"answer is[ ]*[a-zA-Z0-9.]+", answer)[0]
            answer = re.sub("answer is", "", ext).strip()
        except Exception:
            answer = answer.strip()
    return answer


class VQADataset(torch.utils.data.Dataset):
    """eval_affordance_v2.py:109-180 (without the resample-on-corrupt-image fallback's undefined-field access)."""

    def __init__(self, test: str, img_size: int = 224, sampled_num: int = 5000, result=None, image_root: str = "", decode_only: bool = False):
        with open(test, "r") as f:
            self.test = json.load(f)
        if len(self.test) > sampled_num:
            random.shuffle(self.test)
            self.test = self.test[:sampled_num]
        if result is not None:
            done = {r["image"] for r in result}
            self.test = [t for t in self.test if t["image"] not in done]
        # decode_only: the worker hands over the decoded pixels (uint8 HWC); pad / resize / normalise run on the device per batch
        self.transform_val = T_decode_rgb(img_size) if decode_only else T_padded_resize(img_size)
        self.image_root = image_root
        self.cache_last = False            # --share_image_prefix: records of one image are adjacent, the image is loaded once
        self._last = (None, None)

    def __len__(self):
        return len(self.test)

    def __getitem__(self, idx):
        data = self.test[idx]
        path = data["image"]
        local = path if os.path.isfile(path) or not self.image_root else os.path.join(self.image_root, os.path.basename(path))
        if self.cache_last and self._last[0] == local:
            image = self._last[1]
        else:
            image = self.transform_val(Image.open(local).convert("RGB"))
            if self.cache_last:
                self._last = (local, image)
        conv = default_conversation()
        conv.load_qas([[data["conversations"][0]["value"], None]])
        return {"question": conv.get_prompt(), "question_id": idx, "annotation": data["conversations"][1]["value"],
                "image": image, "image_path": path}


def collate_fn(batches):
    images = [b["image"] for b in batches]
    if images[0].dtype != torch.uint8:
        images = torch.stack(images)          # CPU transform: [B, 3, size, size]; decode-only: a list of uint8 HWC images
    return (images, [b["question_id"] for b in batches], [b["question"] for b in batches],
            [b["annotation"] for b in batches], [b["image_path"] for b in batches])


def shard_range(total: int, world: int, rank: int) -> range:
    """InferenceSampler._get_local_indices, eval_affordance_v2.py:191-199."""
    size, left = total // world, total % world
    sizes = [size + int(r < left) for r in range(world)]
    return range(sum(sizes[:rank]), min(sum(sizes[:rank + 1]), total))


def get_args_parser():
    p = argparse.ArgumentParser("A3VLM batch inference on MI355X (DP replicas)", add_help=False)
    p.add_argument("--llama_type", default="llama_ens5", type=str)
    p.add_argument("--llama_config", type=str, default=None, nargs="*")
    p.add_argument("--tokenizer_path", type=str, default="../tokenizer.model")
    p.add_argument("--pretrained_path", default=[], type=str, nargs="*")
    p.add_argument("--device", default="cuda")
    p.add_argument("--model_parallel_size", default=1, type=int)
    p.add_argument("--batch_size", default=4, type=int)
    p.add_argument("--num_workers", default=4, type=int)
    p.add_argument("--seed", default=1, type=int)
    p.add_argument("--dataset", default="path_to_eval_json", type=str)
    p.add_argument("--input_size", type=int, default=224)
    p.add_argument("--addition_flag", default=None, type=str)
    p.add_argument("--remove_space", action="store_true", default=False)
    p.add_argument("--sampled_num", type=int, default=200)
    p.add_argument("--max_gen_len", type=int, default=2048)
    p.add_argument("--max_seq_len", type=int, default=4096)
    p.add_argument("--temperature", type=float, default=0.1)
    p.add_argument("--top_p", type=float, default=0.75)
    p.add_argument("--image_root", type=str, default="", help="directory to look images up by basename (demo.json paths are absolute)")
    p.add_argument("--output_root", type=str, default="vqa_logs")
    p.add_argument("--precision", type=str, choices=["bf16", "tf32"], default="bf16", help="tf32 = fp32 parity path")
    p.add_argument("--preprocess", type=str, choices=["gpu", "cpu"], default="gpu",
                   help="gpu: workers decode only, PadToSquare / bicubic resize / normalise run on the device per batch (a3v_preprocess_batch, "
                        "bit-identical to the PIL transform); cpu: the PIL transform in the workers (data/transform.py:59-68)")
    p.add_argument("--merge_lora", action="store_true", default=False,
                   help="a LoRA model (--llama_type llama_ens5_peft): fold the adapters into the base weights after loading (MetaModel.merge_lora), "
                        "so that decoding takes the single-call step (and --quant of eval_affordance_with_quant applies)")
    p.add_argument("--kv_quant", type=str, choices=["fp8"], default=None,
                   help="keep the KV cache in fp8 e4m3 with per-position scales (Transformer.quantize_kv_cache): half the cache memory and half "
                        "the cache bytes per decode step; independent of --quant, applied after --merge_lora.  With --continuous_rows N "
                        "it is the fp8 cache of the per-row decode path (quantize_kv_cache('fp8', rows=True)); not with "
                        "--lookup_decoding or --num_beams")
    p.add_argument("--continuous_rows", type=int, default=0,
                   help="N > 0: answers come from MetaModel.generate_many on N KV-cache rows (every row at its own position, a finished "
                        "row is refilled with the next prompt); the loader then hands over 4 N samples at a time and --batch_size is "
                        "not used.  0 (default): generate() per batch.  Not with an unmerged LoRA model; with --kv_quant fp8 the rows "
                        "decode over the fp8 cache")
    p.add_argument("--repetition_penalty", type=float, default=1.0,
                   help="HF repetition penalty over the prompt text and everything generated so far, applied on the device before "
                        "temperature / top-p (1.0 = off, the default; > 1 discourages loops in long answers)")
    p.add_argument("--top_k", type=int, default=0,
                   help="sample among the k largest logits only (ties at the k-th kept; 0 = off, the default); applied on the device "
                        "after temperature and before top-p, as HF generate does")
    p.add_argument("--min_p", type=float, default=0.0,
                   help="drop tokens whose probability is below min_p times the most likely token's (0 = off, the default); applied on "
                        "the device after top-p")
    p.add_argument("--save_scores", action="store_true", default=False,
                   help="every record gains \"logprob_sum\" and \"logprobs\": the model's own log-probability of the answer's tokens "
                        "(raw logits, temperature 1), a confidence for AP-style evaluation")
    p.add_argument("--share_image_prefix", action="store_true",
                   help="several questions about one image pay for its prefill once (MetaModel.generate_many(prefix_sharing=True)): the "
                        "records are ordered stably so that equal image paths are adjacent, each image is loaded once, questions that "
                        "share the image and the leading prompt tokens read those keys from one KV-cache row; the output file keeps the "
                        "record order and format it had.  Needs --continuous_rows >= 2; not with --num_samples > 1, --lookup_decoding, "
                        "--num_beams or --kv_quant")
    p.add_argument("--num_samples", type=int, default=1,
                   help="N > 1: draw N answers per (image, question) from ONE prefill (MetaModel.generate_many(n=N): the image is "
                        "encoded once and the prompt's keys are stored once) and keep the most confident well-formed box; every record "
                        "gains \"samples\".  Needs --continuous_rows >= N and --temperature > 0")
    p.add_argument("--lookup_decoding", type=int, default=0,
                   help="D > 0: lookup decoding (MetaModel.generate_many(lookup=D)): every decode step verifies up to D tokens drafted "
                        "from the row's own earlier tokens; the answers are the greedy ones, every record gains \"accepted_per_step\" "
                        "(accepted drafts per row step of the generate_many call that produced it).  Needs --continuous_rows R with "
                        "R * (D + 1) <= 32 and --temperature 0")
    p.add_argument("--answer_regex", type=str, default=None,
                   help="constrained decoding (MetaModel.generate(constraint=PATTERN)): every step may only choose tokens that can still "
                        "lead to a full match of PATTERN (literals, escapes, '.', '\\d', [...] classes, groups, '|', '?', '*', '+', "
                        "'{m}', '{m,n}'), and EOS only where the answer matches; an answer cut by --max_gen_len is a prefix of a match "
                        "and keeps its \"fail\" flag.  Not with --lookup_decoding, unless --lookup_verify choice")
    p.add_argument("--lookup_verify", type=str, choices=["argmax", "choice"], default="argmax",
                   help="how --lookup_decoding verifies its drafts.  argmax (default): against the greedy choice.  choice: sample and "
                        "match (MetaModel.generate_many(lookup_verify='choice')): every query's token is chosen as the plain loop would "
                        "choose it -- penalty, --answer_regex mask, temperature / top-k / top-p / min-p with the uniform of its generated "
                        "index -- and a draft is kept when the choice equals it; allows --temperature > 0, --answer_regex, "
                        "--repetition_penalty and --save_scores beside --lookup_decoding (still --num_samples 1)")
    p.add_argument("--num_beams", type=int, default=0,
                   help="K > 0: beam search (MetaModel.beam_search(num_beams=K)): K beams per (image, question) from ONE prefill, the "
                        "best finished hypothesis is the answer; every record gains \"beam_score\" (sum of log-probs over "
                        "length ** --length_penalty) and \"logprob_sum\".  0 (default): the path as it was.  Needs --continuous_rows >= K "
                        "and --temperature 0; combines with --answer_regex; not with --num_samples > 1, --lookup_decoding or "
                        "--repetition_penalty != 1")
    p.add_argument("--length_penalty", type=float, default=1.0,
                   help="--num_beams: a hypothesis of n tokens scores sum / n ** length_penalty (1.0, the default: the mean log-prob)")
    p.add_argument("--beam_early_stopping", action="store_true", default=False,
                   help="--num_beams: a prompt ends as soon as K hypotheses are finished (default: when no live beam can still beat "
                        "the worst of them)")
    return p


def check_num_beams(args) -> int:
    k = int(getattr(args, "num_beams", 0) or 0)
    if k == 0:
        return 0
    if k < 0 or k > 8:
        raise SystemExit(f"--num_beams {k}: 0 (off) .. 8 beams per prompt")
    if getattr(args, "continuous_rows", 0) < k:
        raise SystemExit(f"--num_beams {k} decodes the {k} beams of a prompt in {k} KV-cache rows at once: add --continuous_rows R with R >= {k}")
    if args.temperature > 0:
        raise SystemExit(f"--num_beams {k} is deterministic: set --temperature 0, or use --num_samples for best-of-n sampling")
    if int(getattr(args, "num_samples", 1)) > 1:
        raise SystemExit(f"--num_beams {k} and --num_samples {args.num_samples} are two ways to the same end: use --num_samples 1, or --num_beams 0")
    if int(getattr(args, "lookup_decoding", 0) or 0):
        raise SystemExit(f"--num_beams {k}: lookup decoding verifies drafts against one greedy continuation: set --lookup_decoding 0, or --num_beams 0")
    if float(getattr(args, "repetition_penalty", 1.0)) != 1.0:
        raise SystemExit(f"--num_beams {k} scores beams by raw log-probs: set --repetition_penalty 1.0, or --num_beams 0")
    return k


def check_kv_quant(args) -> bool:
    """True: the fp8 KV cache of the per-row decode path (--kv_quant fp8 with --continuous_rows N).  What has no fp8 form ends the
    run before the model is built."""
    if not getattr(args, "kv_quant", None):
        return False
    if int(getattr(args, "lookup_decoding", 0) or 0):
        raise SystemExit(f"--lookup_decoding {args.lookup_decoding} has no fp8 KV-cache form (there is no fp8 verify attention): set "
                         "--lookup_decoding 0, or drop --kv_quant")
    if int(getattr(args, "num_beams", 0) or 0):
        raise SystemExit(f"--num_beams {args.num_beams} has no fp8 KV-cache form (the tail permute of beam search is bf16): set "
                         "--num_beams 0, or drop --kv_quant")
    return int(getattr(args, "continuous_rows", 0) or 0) > 0


def check_answer_regex(args):
    pattern = getattr(args, "answer_regex", None)
    if pattern is not None and int(getattr(args, "lookup_decoding", 0) or 0) and getattr(args, "lookup_verify", "argmax") != "choice":
        raise SystemExit(f"--answer_regex changes the choice lookup decoding verifies its drafts against: set --lookup_decoding 0 "
                         f"(or drop --answer_regex), or add --lookup_verify choice")
    if pattern is not None:
        from .model.constrain import parse_regex
        try:
            parse_regex(pattern)           # a pattern outside the subset ends the run before the model is built
        except ValueError as e:
            raise SystemExit(f"--answer_regex: {e}")
    return pattern


def check_lookup(args) -> int:
    d = int(getattr(args, "lookup_decoding", 0) or 0)
    if d < 0 or d > 7:
        raise SystemExit(f"--lookup_decoding {d}: 0 (off) .. 7 drafted tokens per step")
    if d and getattr(args, "continuous_rows", 0) <= 0:
        raise SystemExit(f"--lookup_decoding {d} runs on the per-row decode path: add --continuous_rows R")
    choice = getattr(args, "lookup_verify", "argmax") == "choice"
    if d and args.temperature > 0 and not choice:
        raise SystemExit(f"--lookup_decoding {d} verifies drafts against the greedy choice: set --temperature 0, or add --lookup_verify choice")
    if d and int(getattr(args, "num_samples", 1)) > 1:
        raise SystemExit(f"--lookup_decoding {d} " + ("has no parallel-sampling form" if choice else "is greedy") + ": use --num_samples 1")
    if d and getattr(args, "continuous_rows", 0) * (d + 1) > 32:
        raise SystemExit(f"--lookup_decoding {d} with --continuous_rows {args.continuous_rows}: rows * (D + 1) must be <= 32")
    return d


def make_record(answer: str, score=None) -> dict:
    """answer / format_answer / fail of one generated text, with its logprob_sum if a score is given"""
    answer = postprocess_answer(answer)
    box = format_bounding_box(answer)
    rec = {"answer": answer, "format_answer": box, "fail": len(box) != 4 or box[0] > box[2] or box[1] > box[3]}
    if score is not None:
        rec["logprob_sum"] = score["sum"]
    return rec


def select_sample(samples) -> int:
    """Best-of-n: the index of the sample with the largest ``logprob_sum`` among those with ``fail == False``; if every sample
    failed, the largest ``logprob_sum`` overall.  Ties go to the first."""
    pool = [k for k, s in enumerate(samples) if not s["fail"]] or list(range(len(samples)))
    return max(pool, key=lambda k: (samples[k]["logprob_sum"], -k))


def check_share_image_prefix(args) -> bool:
    """--share_image_prefix and what it cannot be combined with: every refusal ends the run here, before the model is built."""
    if not getattr(args, "share_image_prefix", False):
        return False
    if int(getattr(args, "continuous_rows", 0) or 0) < 2:
        raise SystemExit("--share_image_prefix runs the questions of an image in several KV-cache rows that read one prefix: add "
                         "--continuous_rows R with R >= 2")
    if int(getattr(args, "num_samples", 1)) > 1:
        raise SystemExit(f"--share_image_prefix shares one level only and --num_samples {args.num_samples} already shares the prompt "
                         "among its samples: use --num_samples 1, or drop --share_image_prefix")
    if int(getattr(args, "lookup_decoding", 0) or 0):
        raise SystemExit("--share_image_prefix has no verify step over a shared prefix: set --lookup_decoding 0, or drop --share_image_prefix")
    if int(getattr(args, "num_beams", 0) or 0):
        raise SystemExit(f"--share_image_prefix: the beams of --num_beams {args.num_beams} already read their leader's row: set "
                         "--num_beams 0, or drop --share_image_prefix")
    if getattr(args, "kv_quant", None):
        raise SystemExit("--share_image_prefix has no fp8 KV-cache form (no prefill attention reads fp8 keys): drop --kv_quant, or "
                         "--share_image_prefix")
    return True


def check_num_samples(args) -> int:
    n = int(getattr(args, "num_samples", 1))
    if n < 1:
        raise SystemExit(f"--num_samples {n}: at least 1")
    if n > 1 and getattr(args, "continuous_rows", 0) < n:
        raise SystemExit(f"--num_samples {n} decodes the {n} answers of a prompt in {n} KV-cache rows at once: add --continuous_rows R with R >= {n}")
    if n > 1 and not args.temperature > 0:
        raise SystemExit(f"--num_samples {n} with --temperature 0 would draw the same greedy answer {n} times: set --temperature > 0 "
                         "(the recipe's 0.1), or --num_samples 1")
    return n


def main(args):
    num_beams = check_num_beams(args)          # before the model is built
    num_samples = check_num_samples(args)
    lookup = check_lookup(args)
    answer_regex = check_answer_regex(args)
    kv_rows = check_kv_quant(args)
    share_prefix = check_share_image_prefix(args)
    distributed = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if args.model_parallel_size != 1:
        raise SystemExit("tensor parallelism is not part of this build (DP replicas only): use --model_parallel_size 1")
    if os.environ.get("A3V_ONE_DEVICE") == "1":      # tests: several ranks on a single-GPU box (with A3V_DIST_BACKEND=gloo)
        local = 0
    torch.cuda.set_device(local)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("A3V_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    dev = torch.device("cuda", local)
    cfg = args.llama_config or []
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16 if args.precision == "bf16" else torch.float32)   # model.bfloat16().cuda(), :282
    with torch.device(dev):
        model = MetaModel(args.llama_type, cfg, args.tokenizer_path, with_visual=True, max_seq_len=args.max_seq_len)
    torch.set_default_dtype(old)
    if args.pretrained_path:
        print(f"load pretrained from {args.pretrained_path}:", load_tensor_parallel_model_list(model, args.pretrained_path))
    if getattr(args, "merge_lora", False):
        model.merge_lora()
    if getattr(args, "quant", False):     # eval_affordance_with_quant.py --quant: 4-bit decoder linears + LM head, NF4 or --quant_format mxfp4 (bf16 weights freed)
        model.llma.quantize_decode_weights(getattr(args, "quant_format", "nf4"), prefill=getattr(args, "quant_prefill", False))
    if getattr(args, "kv_quant", None):
        model.llma.quantize_kv_cache(args.kv_quant, rows=kv_rows)
    model.eval()

    name = os.path.basename(args.dataset).split(".")[0]
    save_dir = os.path.join(args.output_root, str(args.addition_flag))
    os.makedirs(save_dir, exist_ok=True)
    results_file = os.path.join(save_dir, f"{name}.json")
    result = json.load(open(results_file)) if os.path.exists(results_file) else None
    random.seed(args.seed)
    on_gpu = getattr(args, "preprocess", "gpu") == "gpu"
    dataset = VQADataset(args.dataset, img_size=args.input_size, sampled_num=args.sampled_num, result=result, image_root=args.image_root,
                         decode_only=on_gpu)
    pre = GpuPaddedResize(args.input_size, dev, torch.float32) if on_gpu else None
    idx = list(shard_range(len(dataset), world, rank))
    rows = getattr(args, "continuous_rows", 0)
    if share_prefix:       # equal image paths adjacent (stable: the questions of an image keep their order); written back in record order
        idx.sort(key=lambda k: dataset.test[k]["image"])
        dataset.cache_last = True
    order = []
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, idx), batch_size=4 * rows if rows > 0 else args.batch_size, shuffle=False,
                                         num_workers=args.num_workers, pin_memory=True, drop_last=False, collate_fn=collate_fn)
    outputs = []
    # the sampled recipe (default: temperature 0.1 / top-p 0.75) draws its uniform numbers from torch's device generator inside
    # generate(): seeded here, per rank, so that a run with the same --seed reproduces its answers (the reference seeds only the
    # dataset shuffle, :304; its sampling stream is whatever the process left in the generator)
    torch.manual_seed(args.seed + rank)
    save_scores = getattr(args, "save_scores", False)
    controls = dict(repetition_penalty=getattr(args, "repetition_penalty", 1.0), return_logprobs=save_scores or num_samples > 1)
    if getattr(args, "top_k", 0) or getattr(args, "min_p", 0.0):      # opt-in: with the defaults the calls below are what they were
        controls.update(top_k=args.top_k, min_p=args.min_p)
    if answer_regex is not None:      # compiled against the model's vocabulary once (MetaModel keeps it by pattern); refusals end the run here
        try:
            model.constraint_automaton(answer_regex)
        except ValueError as e:
            raise SystemExit(f"--answer_regex: {e}")
        controls.update(constraint=answer_regex)
    with torch.no_grad():
        for image, qids, prompts, annotations, paths in loader:
            image = pre.batch(image) if isinstance(image, list) else image.to(dev)
            if num_beams:          # beam search: the best finished hypothesis of every prompt, with its two scores
                answers, scores = model.beam_search(prompts, image, num_beams=num_beams, batch_rows=rows, max_gen_len=args.max_gen_len,
                                                    length_penalty=args.length_penalty, early_stopping=args.beam_early_stopping,
                                                    constraint=answer_regex, return_scores=True)
                for answer, sc, annotation, question, path in zip(answers, scores, annotations, prompts, paths):
                    rec = make_record(answer)
                    outputs.append({"answer": rec["answer"], "format_answer": rec["format_answer"], "annotation": annotation,
                                    "question": question, "image": path, "fail": rec["fail"], "beam_score": sc["score"],
                                    "logprob_sum": sc["sum"]})
                continue
            if num_samples > 1:    # best-of-n: n answers per prompt from one prefill, the most confident well-formed one is the record's
                answers, scores = model.generate_many(prompts, image, batch_rows=rows, max_gen_len=args.max_gen_len,
                                                      temperature=args.temperature, top_p=args.top_p, n=num_samples, **controls)
                for texts, scs, annotation, question, path in zip(answers, scores, annotations, prompts, paths):
                    samples = [make_record(t, sc) for t, sc in zip(texts, scs)]
                    best = select_sample(samples)
                    b = samples[best]
                    outputs.append({"answer": b["answer"], "format_answer": b["format_answer"], "annotation": annotation,
                                    "question": question, "image": path, "fail": b["fail"], "samples": samples})
                    if save_scores:
                        outputs[-1].update(logprob_sum=scs[best]["sum"], logprobs=scs[best]["logprobs"])
                continue
            order.extend(qids)
            if rows > 0:           # a chunk of a few batches at a time: the loader's workers stay ahead of the decode
                answers = model.generate_many(prompts, image, batch_rows=rows, max_gen_len=args.max_gen_len, temperature=args.temperature,
                                              top_p=args.top_p, **controls, **({"lookup": lookup} if lookup else {}),
                                              **({"prefix_sharing": True, "image_ids": list(paths)} if share_prefix else {}),
                                              **({"lookup_verify": "choice"} if lookup and getattr(args, "lookup_verify", "argmax") == "choice" else {}))
            else:
                answers = model.generate(prompts, image, max_gen_len=args.max_gen_len, temperature=args.temperature, top_p=args.top_p,
                                         **controls)
            answers, scores = answers if save_scores else (answers, [None] * len(prompts))
            for answer, annotation, question, path, sc in zip(answers, annotations, prompts, paths, scores):
                answer = postprocess_answer(answer)
                box = format_bounding_box(answer)
                fail = len(box) != 4 or box[0] > box[2] or box[1] > box[3]
                outputs.append({"answer": answer, "format_answer": box, "annotation": annotation, "question": question,
                                "image": path, "fail": fail})
                if lookup:
                    st = model.last_lookup_stats
                    outputs[-1]["accepted_per_step"] = st["accepted"] / max(st["steps"], 1)
                if sc is not None:     # the scores of the generated tokens (the text above may be cut further by postprocess_answer)
                    outputs[-1].update(logprob_sum=sc["sum"], logprobs=sc["logprobs"])
    if share_prefix:       # back to the order of the records
        outputs = [o for _, o in sorted(zip(order, outputs), key=lambda x: x[0])]
    if distributed:
        gathered = [None] * world
        dist.all_gather_object(gathered, outputs)
        outputs = list(itertools.chain.from_iterable(gathered))
    if rank == 0:
        if result:
            outputs.extend(result)
        with open(results_file, "w") as f:
            json.dump(outputs, f, ensure_ascii=False)
        print(f"{len(outputs)} records -> {results_file}")
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    return outputs


if __name__ == "__main__":
    main(argparse.ArgumentParser(parents=[get_args_parser()]).parse_args())
