"""``MetaModel`` with the interface of the reference's ``accessory.model.meta.MetaModel``
(reference: model/accessory/model/meta.py:20-597), driving the MI355X-native plugin.

Kept: constructor signature, plugin discovery by ``llama_type`` (meta.py:30-32), the params-json
merge (:34-47), ``forward -> (loss, {})`` with the trailing-pad trim and the all-zero-label
guard (:234-263), batched ``generate`` with shortest-prompt start, teacher forcing of longer
prompts, multi-token stop strings and left truncation (:379-485), ``stream_generate``,
``compute_logits``, ``evaluate_examples``, ``sample_top_p``, ``get_trainable_params`` etc.

Changed on purpose: no fairscale / torch.distributed requirement for a single process, tensors
are created on the model's device instead of ``.cuda()``, the loss and the
argmax run in HIP kernels (a3v_cross_entropy / a3v_argmax) instead of torch ops.
"""
from __future__ import annotations

import dataclasses
import importlib
import inspect
import json
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn

from .. import ops
from . import constrain, genctl
from .LLM.weight_formats import FORMATS
from .tokenizer import Tokenizer, probe_tokenizer_path_from_pretrained  # noqa: F401

# llama_type -> module; extend to plug further model files (same contract as accessory.model.LLM.*)
_PLUGIN_PACKAGE = "a3vlm_amd.model.LLM"


class MetaModel(nn.Module):
    def __init__(self, llama_type: str, llama_config, tokenizer_path: str, with_visual: bool = False,
                 max_seq_len: int = 4096, pretrain_stage: bool = False) -> None:
        super().__init__()
        self.llama_type = llama_type
        self.with_visual = with_visual
        model_module = importlib.import_module(f"{_PLUGIN_PACKAGE}.{llama_type}")
        ModelArgs, Transformer = model_module.ModelArgs, model_module.Transformer

        llama_args = {}
        if isinstance(llama_config, str):
            llama_config = [llama_config]
        for cfg in llama_config or []:
            if isinstance(cfg, dict):
                llama_args.update(cfg)
            else:
                with open(cfg, "r") as f:
                    llama_args.update(json.loads(f.read()))
        llama_args["max_seq_len"] = max_seq_len
        llama_args["max_batch_size"] = 32
        tokenizer = Tokenizer(model_path=tokenizer_path)
        llama_args["vocab_size"] = tokenizer.n_words
        known = {f.name for f in dataclasses.fields(ModelArgs)}
        unknown = set(llama_args) - known
        if unknown:
            raise TypeError(f"unknown ModelArgs fields in config: {sorted(unknown)}")
        args = ModelArgs(**llama_args)

        if "tokenizer" in inspect.signature(Transformer.__init__).parameters:
            model = Transformer(args, tokenizer, with_visual=with_visual)
            self.tokenizer = model.tokenizer
        else:
            model = Transformer(args, with_visual=with_visual)
            self.tokenizer = tokenizer
        self.llma = model
        self.criterion = torch.nn.CrossEntropyLoss(ignore_index=0)  # kept as an attribute (meta.py:67)
        self._set_default_trainability(pretrain_stage)
        self.is_peft = getattr(model, "is_peft", False)
        self._constraints: Dict[str, constrain.TokenAutomaton] = {}      # pattern -> automaton over this model's vocabulary

    # ------------------------------------------------------------------ construction from a checkpoint folder
    @classmethod
    def from_pretrained(cls, pretrained_path, llama_type: Optional[str] = None, llama_config=None,
                        tokenizer_path: Optional[str] = None, with_visual: bool = False, max_seq_len: int = 4096,
                        mp_group=None, dtype=torch.bfloat16, device="cuda", quant=False, kv_quant: Optional[str] = None,
                        quant_prefill: bool = False, kv_rows: bool = False) -> "MetaModel":
        """Build the model a checkpoint folder describes and load it (reference: model/meta.py:88-222).

        What is not given is looked up in the LAST folder of ``pretrained_path``: ``llama_type`` in ``meta.json``,
        ``llama_config`` in ``config.json`` (absent: ModelArgs defaults), the tokenizer as ``tokenizer.model`` or an HF pair.
        Folders are loaded in order (``consolidated`` / ``meta_ori`` override, ``consolidated_diff`` adds).  Differences to the
        reference, all forced by the DP-replica design: no process group is created (``mp_group`` must be None or of size 1;
        TP-sharded folders are merged on load), ``hf://`` ids need a network and are refused, and ``quant=True`` selects this
        package's weight-only fp8 decoder images (``Transformer.quantize_decode_weights("fp8")``) instead of bitsandbytes NF4.
        ``quant="nf4"`` is the reference's 4-bit mode (meta.py:197-219, util/quant.py:95-163): the bf16 checkpoint is loaded,
        then every decoder linear and the LM head is quantised to NF4 layer by layer and its bf16 weight freed
        (``Transformer.quantize_decode_weights("nf4")``; inference only, irreversible).
        ``quant="mxfp4"`` is the same flow in the chip's own 4-bit format (OCP MXFP4 on the scaled MFMA,
        ``Transformer.quantize_decode_weights("mxfp4")``; no reference counterpart).  ``quant_prefill=True`` with it runs prefill and
        decode steps of more than 32 rows W4A8 on the images (``prefill=True`` there); with fp8 it is that mode's W8A8 prefill; with
        ``quant="nf4"`` it is refused.
        ``kv_quant="fp8"`` (no reference counterpart) keeps the KV cache of ``generate`` in fp8 e4m3 with per-position scales
        (``Transformer.quantize_kv_cache``); independent of ``quant``.  ``kv_rows=True`` (needs ``kv_quant="fp8"``) makes it the fp8
        cache of the ragged path as well (``quantize_kv_cache("fp8", rows=True)``: ``generate_many`` over fp8 rows)."""
        import os
        import warnings
        from ..checkpoint import load_tensor_parallel_model_list
        paths = [pretrained_path] if isinstance(pretrained_path, str) else list(pretrained_path or [])
        if not paths:
            raise ValueError("pretrained_path should be specified")
        if quant_prefill and quant == "nf4":
            raise ValueError("quant_prefill is an MXFP4 option (quant='mxfp4': the W4A8 GEMM on the images; with fp8 it selects the W8A8 "
                             "prefill): NF4 has no quantised-activation form")
        if quant_prefill and not quant:
            raise ValueError("quant_prefill needs quant='mxfp4' (or fp8)")
        if kv_rows and kv_quant != "fp8":
            raise ValueError("kv_rows is the ragged form of the fp8 KV cache: it needs kv_quant='fp8'")
        for path in paths:
            if path.startswith("hf://"):
                raise NotImplementedError(f"{path}: downloading from the hub is not available here; pass a local folder")
        if mp_group is not None:
            import torch.distributed as dist
            if dist.get_world_size(mp_group) != 1:
                raise NotImplementedError("model parallel size > 1 is replaced by DP replicas; TP-sharded folders are merged on load")
        last = paths[-1]
        if llama_type is None:
            meta_file = os.path.join(last, "meta.json")
            if not os.path.exists(meta_file):
                raise ValueError("Cannot determine llama_type")
            with open(meta_file) as f:
                llama_type = json.load(f)["llama_type"]
        if llama_config is None:
            cfg_file = os.path.join(last, "config.json")
            llama_config = [cfg_file] if os.path.exists(cfg_file) else []
        if tokenizer_path is None:
            tokenizer_path = probe_tokenizer_path_from_pretrained(last)
            if tokenizer_path is None:
                raise FileNotFoundError("No tokenizer available")
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            with torch.device(device):
                model = cls(llama_type, llama_config, tokenizer_path, with_visual, max_seq_len)
        finally:
            torch.set_default_dtype(old)
        print(f"Loading pretrained weights from {paths} ...")
        load_result = load_tensor_parallel_model_list(model, paths)
        if load_result != {"missing_keys": [], "unexpected_keys": []}:
            warnings.warn(f"checkpoint and model mismatch: \n{load_result}")
        else:
            print("all params match perfectly!")
        if quant == "mxfp4":
            model.llma.quantize_decode_weights(quant, prefill=bool(quant_prefill))
        elif quant == "nf4":
            model.llma.quantize_decode_weights(quant)
        elif quant:
            model.llma.quantize_decode_weights("fp8", prefill=bool(quant_prefill))
        if kv_quant is not None:
            model.llma.quantize_kv_cache(kv_quant, rows=bool(kv_rows))
        model.eval()
        return model

    # ------------------------------------------------------------------ trainability
    def get_trainable_params(self, pretrain_stage: bool = False):
        return {"llma." + n: p for n, p in self.llma.get_trainable_params(pretrain_stage).items()}

    def _set_default_trainability(self, pretrain_stage: bool = False) -> None:
        for _, v in self.named_parameters():
            v.requires_grad = False
        for _, v in self.get_trainable_params(pretrain_stage=pretrain_stage).items():
            v.requires_grad = True

    @property
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    # ------------------------------------------------------------------ loss
    @staticmethod
    def _trim(examples: torch.Tensor, labels: torch.Tensor):
        """meta.py:235-249: cut the batch after the last column that holds any label."""
        nz = torch.count_nonzero(labels, dim=0).tolist()
        pos = len(nz) - 1
        while pos >= 0 and nz[pos] == 0:
            pos -= 1
        if pos == -1:
            pos = 2
        return examples[:, :pos + 1], labels[:, :pos + 1]

    def loss_from_logits(self, output: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """meta.py:256-262 on logits [B,T,V] and UNshifted labels [B,T]: mean CE over labels != 0."""
        B, T, V = output.shape
        lab = labels[:, 1:].contiguous().view(-1)
        if int(lab.sum()) == 0:
            return torch.zeros((), dtype=torch.float32, device=output.device)
        dev = output.device
        row_loss = torch.empty(B, T - 1, dtype=torch.float32, device=dev)
        for b in range(B):     # logits rows [b, 0:T-1] are contiguous per sample
            ops.cross_entropy(output[b, :T - 1], lab[b * (T - 1):(b + 1) * (T - 1)], row_loss[b])
        n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.count_valid(lab, n_valid)
        # final scalar reduction of B*(T-1) fp32 values: plumbing, not the hot path
        return row_loss.sum() / n_valid.to(torch.float32)[0]

    def train_engine(self, compute_dtype: torch.dtype = None, zero1_world: int = 0):
        """The HIP forward/backward engine of the plugin (a3vlm_amd/train.py).  compute dtype: bf16
        ("autocast") unless the model is all-fp32 (parity path)."""
        from ..train import TrainEngine
        fmt = FORMATS[self.llma.weight_format]
        if fmt.frees_weights:
            raise RuntimeError(f"this model holds {fmt.name} weights (inference only): training needs the bf16 checkpoint")
        if getattr(self, "_engine", None) is None:
            if compute_dtype is None:
                frozen = [p for p in self.llma.parameters() if not p.requires_grad]
                compute_dtype = frozen[0].dtype if frozen else torch.bfloat16
                if getattr(self, "train_compute_dtype", None) is not None:
                    compute_dtype = self.train_compute_dtype
            self._engine = TrainEngine(self.llma, compute_dtype, zero1_world=zero1_world)
            self._anchor = torch.zeros((), dtype=torch.float32, device=self._device, requires_grad=True)
        return self._engine

    def _sync_engine(self):
        eng = getattr(self, "_engine", None)
        if eng is not None:
            eng.sync_optimizer()

    def merge_lora(self) -> None:
        """Fold the LoRA adapters into the base matrices (``Transformer.merge_adapters``: W' = W + lora_b . lora_a, one rounding) and
        become a plain ``llama_ens5`` model: ``llama_type`` and ``is_peft`` say so, ``save_checkpoint`` writes a folder that
        ``from_pretrained`` loads without a ``llama_type``, and every inference path of the base plugin (the single-call decode
        step, ``quantize_decode_weights``) applies.  A live ``TrainEngine`` is joined first, so the adapters merged are the ones the
        last optimizer step wrote, and dropped (its weight images describe the adapter model).  In place and irreversible."""
        if not self.is_peft or not hasattr(self.llma, "merge_adapters"):
            raise RuntimeError(f"merge_lora needs a model with LoRA adapters; this is a {self.llama_type} model without any")
        self._sync_engine()
        self._engine = None
        self.llma.merge_adapters()
        self.llama_type = "llama_ens5"
        self.is_peft = False
        self._set_default_trainability()

    def zero_grad(self, set_to_none: bool = True):
        """``set_to_none=False`` WRITES the gradients: an overlapped optimizer step (``FusedAdamW.step(overlap=True)``) may still
        be reading them on its own stream, so it is joined first (``set_to_none=True`` only drops references)."""
        if not set_to_none:
            self._sync_engine()
        return super().zero_grad(set_to_none=set_to_none)

    def state_dict(self, *args, **kwargs):
        self._sync_engine()            # checkpoints read the parameters on the current stream
        return super().state_dict(*args, **kwargs)

    def forward(self, examples, labels, images=None, depth_imgs=None, trimmed: bool = False):
        """``trimmed=True`` (not in the reference's signature): the caller already cut the batch after its last labelled column
        (``MetaModel._trim`` on the CPU batch, as ``engine_finetune.train_one_epoch`` does) -- skips the host read of the
        per-column label counts that the trim needs on device tensors."""
        if not trimmed:
            with torch.no_grad():
                examples, labels = self._trim(examples, labels)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.llma.parameters()):
            # training: loss and gradients through the HIP backward (loss.backward() fills param.grad)
            from ..train import step_loss
            eng = self.train_engine()
            return step_loss(eng, self._anchor, examples, labels, images), {}
        output = self.llma(examples, images)
        additional_loss = {}
        if isinstance(output, tuple):
            output, additional_loss = output
        return self.loss_from_logits(output, labels), additional_loss

    # ------------------------------------------------------------------ logits / eval
    @torch.no_grad()
    def compute_logits(self, examples, images=None, bos=True, eos=False) -> List[torch.Tensor]:
        if isinstance(examples, str):
            raise ValueError(f"{self.__class__}.generate expects a batched LIST of prompts, but str is given")
        if isinstance(examples[0], str):
            examples = [self.tokenizer.encode(x, bos, eos) for x in examples]
        dev = self._device
        if images is not None:
            images = images.to(dev)
        lens = [len(x) for x in examples]
        tok = torch.zeros((len(examples), max(lens)), dtype=torch.long, device=dev)
        for i, t in enumerate(examples):
            tok[i, :len(t)] = torch.tensor(t, dtype=torch.long)
        out = self.llma(tok, images)
        logits = out[0] if isinstance(out, tuple) else out
        return [lg[:n].float() for lg, n in zip(logits, lens)]

    @torch.no_grad()
    def evaluate_examples(self, examples, contexts=None, images=None, bos=True, eos=False) -> Dict[str, List]:
        """meta.py:306-377."""
        if isinstance(examples, str):
            raise ValueError(f"{self.__class__}.generate expects a batched LIST of prompts, but str is given")
        if isinstance(examples[0], str):
            examples = [self.tokenizer.encode(x, bos, eos) for x in examples]
            if contexts is not None:
                contexts = [self.tokenizer.encode(x, bos, False) for x in contexts]
        if contexts is not None:
            assert all(e[:len(c)] == c for e, c in zip(examples, contexts))
        logits = self.compute_logits(examples, images)
        res = {"log_likelihood": [], "ppl": [], "max_equal": [], "non_context_logits": []}
        for i, lg in enumerate(logits):
            start = 0 if contexts is None else len(contexts[i]) - 1
            assert start >= 0
            lg = lg[start:-1].contiguous()
            lab = torch.tensor(examples[i][start + 1:], dtype=torch.long, device=lg.device)
            row = torch.empty(lg.shape[0], dtype=torch.float32, device=lg.device)
            ops.cross_entropy(lg, lab, row)
            res["log_likelihood"].append(-row.sum().item())
            res["ppl"].append(row.mean().item())
            am = torch.empty(lg.shape[0], dtype=torch.long, device=lg.device)
            ops.argmax(lg, am)
            res["max_equal"].append(bool((am == lab).all().item()))
            res["non_context_logits"].append(lg)
        return res

    # ------------------------------------------------------------------ generation
    def constraint_automaton(self, constraint) -> Optional[constrain.TokenAutomaton]:
        """The ``constraint`` argument of ``generate`` / ``generate_many`` as a ``TokenAutomaton``: a pattern string is compiled
        against this model's tokenizer (``model/constrain.py``: regex -> DFA -> int16 table over the vocabulary) and kept by pattern.
        Host work only; every refusal (unsupported construct, dead end under the vocabulary, too many states) is a ``ValueError``."""
        constrain.check_constraint(constraint)
        V = self.llma.args.vocab_size
        if isinstance(constraint, str):
            if constraint not in self._constraints:
                pieces = list(self.tokenizer.pieces())[:V]
                pieces += [None] * (V - len(pieces))             # ids the tokenizer does not know contribute no text
                self._constraints[constraint] = constrain.compile_constraint(constraint, pieces, self.tokenizer.eos_id)
            constraint = self._constraints[constraint]
        if constraint is not None and constraint.vocab_size != V:
            raise ValueError(f"constraint: the automaton was compiled for {constraint.vocab_size} tokens, the model has {V}")
        return constraint

    @torch.no_grad()
    def generate(self, prompts: List[str], images: Optional[torch.Tensor] = None,
                 depth_images: Optional[torch.Tensor] = None, max_gen_len: int = 512,
                 temperature: float = 0.0, top_p: float = 0.95,
                 additional_stop_symbols: Iterable[str] = (), return_ids: bool = False, poll_every: int = 4,
                 sample_uniforms: Optional[torch.Tensor] = None, repetition_penalty: float = 1.0,
                 return_logprobs: bool = False, top_k: int = 0, min_p: float = 0.0, constraint=None) -> List[str]:
        """meta.py:379-485.  ``return_ids`` additionally returns the generated id lists (the
        arguments of tokenizer.decode at :482-484) for bit-exact parity checks.
        ``temperature > 0`` (the eval script's default recipe, T 0.1 / top-p 0.75): the nucleus draw of :456-459 / :568-583 runs on
        the device (``a3v_sample_top_p``: no full-vocabulary sort, no host-visible op per token); its one random ingredient is a
        uniform number per row and step, drawn up front from torch's device generator (``torch.manual_seed`` reproduces a run) or
        handed in as ``sample_uniforms`` [steps, bsz] (parity tests replay the oracle with the same numbers).
        ``poll_every``: the all-rows-stopped flag lives on the device and is read back (a host sync) only every
        ``poll_every`` steps instead of every step (:478-479); steps taken after every row has stopped write past
        ``stop_pos`` and are discarded, so the outputs are identical for any value (1 = the reference's cadence).
        ``repetition_penalty`` (HF's rule over the prompt text and everything generated so far, applied before temperature and
        top-p; 1.0 = off) and ``return_logprobs`` (the return gains ``scores``: per answer ``{"logprobs": [...], "sum": ...}``, the
        model's own log-probability of every kept token, from the raw logits at temperature 1) are opt-in and run on the device
        inside the step (model/genctl.py); with the defaults nothing of them is allocated or launched.
        ``top_k`` / ``min_p`` (opt-in, ``temperature > 0`` only; 0 = off): HF's two other filters on the device, in HF's order
        temperature, top-k, top-p, min-p (``a3v_sample_top_k_p``); they see the penalised row.  With the defaults the sampler is
        ``a3v_sample_top_p`` as before.
        ``constraint`` (opt-in; a ``TokenAutomaton`` or a regex pattern string, see ``constraint_automaton``): constrained decoding.
        Every step's choice is restricted to the tokens that can still lead to a full match of the pattern, and EOS to the places
        where the text so far is one: the row's automaton state lives on the device, ``a3v_constrain_logits`` masks the (penalised)
        row in front of the sampler / argmax and ``a3v_constrain_advance`` moves the state behind the token write, no host read.
        An answer that ends on EOS matches the pattern; one that reaches ``max_gen_len`` first is a viable PREFIX of a match, not a
        match.  Scores (``return_logprobs``) stay the UNCONSTRAINED model's log-probabilities of the chosen tokens (raw logits), and
        the repetition penalty is applied before the mask.  With ``constraint=None`` nothing of it is allocated or launched."""
        if isinstance(prompts, str):
            raise ValueError(f"{self.__class__}.generate expects a batched LIST of prompts, but str is given")
        controls = genctl.wanted(repetition_penalty, return_logprobs)      # ValueError before any device use
        top_k, min_p = genctl.check_filters(top_k, min_p)
        automaton = self.constraint_automaton(constraint)
        dev = self._device
        if images is not None:
            images = images.to(dev)
        if depth_images is not None:
            depth_images = depth_images.to(dev)
        bsz = len(prompts)
        args = self.llma.args
        assert bsz <= args.max_batch_size, (bsz, args.max_batch_size)
        prompt_tokens = [self.tokenizer.encode(x, bos=True, eos=False) for x in prompts]
        min_prompt = min(len(t) for t in prompt_tokens)
        max_prompt = max(len(t) for t in prompt_tokens)
        max_seq_len = args.max_seq_len
        if images is not None:
            max_seq_len -= self.llma.image_words
        total_len = min(max_seq_len, max_gen_len + max_prompt)
        prompt_tokens = [t[-(max_seq_len - max_gen_len):] for t in prompt_tokens]

        tokens_cpu = torch.zeros((bsz, total_len), dtype=torch.long)
        mask_cpu = torch.zeros((bsz, total_len), dtype=torch.bool)
        for k, t in enumerate(prompt_tokens):
            tokens_cpu[k, :len(t)] = torch.tensor(t, dtype=torch.long)
            mask_cpu[k, :len(t)] = True
        tokens = tokens_cpu.to(dev)
        text_mask = mask_cpu.to(dev)
        start_pos, prev_pos = min_prompt, 0

        # stop sequences: EOS, then each extra stop string tokenised as a word-initial and as a word-internal piece (:438-444)
        l_stop = [[self.tokenizer.eos_id]]
        l_stop += [self.tokenizer.encode_segment(s) for s in additional_stop_symbols]
        l_stop += [self.tokenizer.encode_wo_prefix_space(s) for s in additional_stop_symbols]
        offs = [0]
        for st in l_stop:
            offs.append(offs[-1] + len(st))
        stop_seq = torch.tensor([t for st in l_stop for t in st], dtype=torch.long, device=dev)
        stop_off = torch.tensor(offs, dtype=torch.int32, device=dev)
        stopped = torch.zeros(bsz, dtype=torch.bool, device=dev)
        stop_pos = torch.full((bsz,), start_pos + 1, dtype=torch.long, device=dev)
        live = torch.full((1,), bsz, dtype=torch.int32, device=dev)      # rows still generating (device counter)
        uni = sampled = None
        if temperature > 0:
            n_steps = max(total_len - start_pos, 1)
            uni = (torch.rand(n_steps, bsz, device=dev, dtype=torch.float32) if sample_uniforms is None
                   else sample_uniforms.to(device=dev, dtype=torch.float32).contiguous())
            assert uni.shape[0] >= total_len - start_pos and uni.shape[1] == bsz, tuple(uni.shape)
            sampled = torch.empty(bsz, dtype=torch.long, device=dev)
        gc = None
        if controls:       # teacher-forced prompt positions are marked here, up front, and never scored (generated index < 0)
            gc = genctl.GenControls(bsz, args.vocab_size, total_len - start_pos, repetition_penalty, return_logprobs, dev)
            gc.prompt_len.copy_(torch.tensor([len(t) for t in prompt_tokens], dtype=torch.int32))
            gc.mark_prompts(tokens)
        cs = None
        if automaton is not None:      # every row starts in the automaton's start state; its first generated id sits behind its prompt
            cs = constrain.ConstraintState(automaton, bsz, args.vocab_size, dev)
            cs.first.copy_(torch.tensor([len(t) for t in prompt_tokens], dtype=torch.int32))

        # One iteration = the model step (one C call for a decode step) + ONE launch of a3v_generate_step, which does everything
        # meta.py:456-477 does with a dozen small torch ops: argmax, teacher forcing of longer prompts, the tokens[:, cur_pos]
        # write, stop_pos / stopped bookkeeping and the multi-token stop match.  The host only reads `live` every poll_every steps.
        for cur_pos in range(start_pos, total_len):
            if depth_images is not None:                     # two-image plugin (meta.py:447-451)
                if prev_pos == 0:
                    logits = self.llma.forward_inference(tokens[:, prev_pos:cur_pos], prev_pos, images, depth_images)
                else:
                    logits = self.llma.forward_inference(tokens[:, prev_pos:cur_pos], prev_pos)
            else:
                logits = self.llma.forward_inference(tokens[:, prev_pos:cur_pos], prev_pos,
                                                     images if prev_pos == 0 else None)
            z = gc.prepare(logits) if gc is not None else logits       # the choice reads the penalised row, the score the raw one
            if cs is not None:         # ... under the automaton's mask (a teacher-forced step is masked too: its choice is discarded)
                z = cs.mask(z, logits)
            if temperature > 0:
                self._sample_into(z, temperature, top_p, uni[cur_pos - start_pos], sampled, top_k, min_p)
            ops.generate_step(z, sampled, tokens, text_mask, cur_pos, stop_seq, stop_off, len(l_stop), stopped, stop_pos, live)
            if gc is not None:         # a stopped row keeps writing past its stop_pos, as its tokens do: cut below
                gc.record(logits, tokens, col=cur_pos)
            if cs is not None:         # a stopped row sits in DONE (only EOS allowed) or keeps walking: cut below as well
                cs.advance(tokens, col=cur_pos)
            if ((cur_pos - start_pos) % poll_every == poll_every - 1 or cur_pos == total_len - 1) and int(live.item()) == 0:
                break
            prev_pos = cur_pos

        decoded, ids = [], []
        sp = stop_pos.tolist()
        for i, t in enumerate(tokens.tolist()):
            t = t[len(prompt_tokens[i]):sp[i]]
            ids.append(t)
            decoded.append(self.tokenizer.decode(t))
        ret = (decoded, ids) if return_ids else decoded
        if return_logprobs:            # the device array, read back once
            scores = [genctl.score(row[:len(t)]) for row, t in zip(gc.lp.tolist(), ids)]
            ret = ret + (scores,) if return_ids else (decoded, scores)
        return ret

    @torch.no_grad()
    def generate_many(self, prompts: List[str], images: Optional[torch.Tensor] = None, *, batch_rows: int,
                      max_gen_len=512, temperature: float = 0.0, top_p: float = 0.95,
                      additional_stop_symbols: Iterable[str] = (), return_ids: bool = False, poll_every: int = 4,
                      sample_uniforms: Optional[torch.Tensor] = None, repetition_penalty: float = 1.0,
                      return_logprobs: bool = False, top_k: int = 0, min_p: float = 0.0, n: int = 1,
                      lookup: Optional[int] = None, lookup_ngram: int = 3, lookup_drafter=None, constraint=None,
                      lookup_verify: str = "argmax", prefix_sharing: bool = False, image_ids=None):
        """Any number of prompts through ``batch_rows`` KV-cache rows (no reference counterpart; opt-in): every row decodes at its
        own position, and a row whose answer is finished is prefilled with the next prompt while the others keep decoding, so a
        short answer does not hold its row until the longest answer of a batch is done.  Answers come back in input order.

        ``max_gen_len``: an int, or one int per prompt.  Per prompt the truncation and the length limit are ``generate``'s for a
        batch of one (prompt cut to its last ``max_seq_len - max_gen_len`` tokens, ``max_seq_len`` less the image words; at most
        ``min(max_seq_len, max_gen_len + len(prompt))`` tokens in all); generation starts behind the truncated prompt.
        ``images`` [N, ...]: one image per prompt, or None.  ``temperature > 0``: uniforms are indexed [prompt, generated index]
        (drawn up front, or ``sample_uniforms`` [N, >= max steps]), so an answer does not depend on ``batch_rows`` or on the row it
        ran in.  ``stopped`` is read back every ``poll_every`` steps; a stopped row is not touched by later steps.
        ``repetition_penalty`` / ``return_logprobs``: as in ``generate``; the seen set belongs to the cache row and is cleared and
        re-marked when the row is refilled, a finished row's log-probs are read back with its ids.  ``top_k`` / ``min_p``: as in
        ``generate``.
        ``n > 1`` (parallel sampling; needs ``temperature > 0`` and ``n <= batch_rows``): n answers per prompt from ONE prefill.  A
        prompt is admitted when n rows are free (``GroupScheduler``); the lowest is the leader: it is prefilled and runs sample 0,
        its logits start every sample, and the siblings read the prompt's keys below the last 64 boundary from the leader's row
        (``share_prefix``: the image is encoded once and most of the prompt is stored once).  Uniforms are indexed [prompt, sample,
        generated index] (``sample_uniforms`` [N, n, >= max steps]; [N, >= max steps] is still taken when n == 1), so sample s of a
        prompt is the answer of that prompt alone with that row of uniforms.  Every per-prompt element of the return (text, ids,
        scores) becomes a list of n, in sample order.  With ``n == 1`` the call is the one it was.
        ``lookup=D`` (1..7; greedy only; 0 / None: the loop as it was): lookup decoding.  Every step drafts up to D tokens per row
        by prompt lookup -- the continuation of the latest earlier occurrence of the row's last ``lookup_ngram``-gram (then shorter
        ones) in its own tokens -- feeds the last token and the drafts through ONE decode step (``forward_verify_rows``) and keeps
        the longest prefix the model itself produces: the answers are the plain loop's.  draft -> verify -> accept run without a
        host read; ``batch_rows * (D + 1) <= 32``.  Afterwards ``self.last_lookup_stats`` holds ``steps`` (row steps), ``tokens``,
        ``drafted`` and ``accepted``.  ``lookup_drafter`` (tests): a callable ``(tokens, cur, limit, pos, stopped, next_tok, x, nq)``
        that fills x / nq in place of the lookup kernel.
        ``constraint``: as in ``generate`` (a ``TokenAutomaton`` or a pattern string; scores stay the unconstrained model's).  The
        state belongs to the cache row and is set back to the start at every refill, for every sibling row when ``n > 1``.  Not with
        ``lookup`` (verification compares against the unconstrained argmax): use ``lookup=0``.
        ``lookup_verify`` (``"argmax"``, the default: everything above; ``"choice"``, opt-in): sample and match.  Every query of a
        verify step is prepared as the plain loop would prepare it had the drafts in front of it been emitted (penalty over the
        seen set and those drafts, the constraint's mask in the state behind them: ``a3v_verify_prepare``), its token is drawn with
        the uniform of its generated index (or is the argmax at temperature 0), and a draft is accepted if and only if the draw
        equals it (``a3v_accept_rows_chosen``): the answers are the plain loop's for the same ``sample_uniforms``.  It lifts the
        refusals of ``lookup`` for ``temperature > 0`` (with ``top_p`` / ``top_k`` / ``min_p``), ``repetition_penalty``,
        ``return_logprobs`` and ``constraint``; ``n > 1`` is still refused (use ``n=1``, or ``lookup=0``).
        ``prefix_sharing=True`` (opt-in; several questions about one image): prompts that are ADJACENT in the list, carry the same
        image (``image_ids[i] == image_ids[j]``; without ``image_ids``: the same object of a list of images, or no image at all) and
        start with the same tokens form a run (``ragged.prefix_groups``).  With C = 1 + image words + common text tokens and
        P = min(C, shortest member - 1) & ~63, the first P positions are prefilled ONCE, in the row of the run's first member (the
        image is encoded once, those logits are discarded), every member then runs its own suffix over them in one packed pass
        (``Transformer.extend_rows``) and decodes with the shared-prefix step.  Members that find no free row wait and are extended
        over the prefix later; the row that holds it takes no other run's prompt until the last member is done
        (``ragged.PrefixScheduler``).  Order and format of the results are the plain call's; a run of one, or P == 0, takes the
        plain path.  One level of sharing only: not with ``n > 1`` (use ``n=1``), ``lookup`` (use ``lookup=0``), ``beam_search`` or
        the fp8 KV cache (each raises, naming the way out).
        Not for the fp8 KV cache, LoRA models before ``merge_lora()`` or the two-image plugin (each raises, naming the way out)."""
        from .ragged import GroupScheduler, LookupBound, PrefixScheduler, RowScheduler, prefix_groups
        if isinstance(prompts, str):
            raise ValueError(f"{self.__class__}.generate_many expects a LIST of prompts, but str is given")
        controls = genctl.wanted(repetition_penalty, return_logprobs)      # ValueError before any device use
        top_k, min_p = genctl.check_filters(top_k, min_p)
        n = int(n)
        if n < 1:
            raise ValueError(f"generate_many: n = {n} samples per prompt; n >= 1")
        if n > 1 and not temperature > 0:
            raise ValueError(f"generate_many: n = {n} samples per prompt need temperature > 0 (at temperature 0 all {n} are the same "
                             "greedy answer); use n=1")
        if n > int(batch_rows):
            raise ValueError(f"generate_many: n = {n} samples per prompt need n cache rows at once: batch_rows = {batch_rows} < n")
        D = int(lookup or 0)
        if prefix_sharing:                 # refusals of prefix sharing, before any device use
            if n > 1:
                raise ValueError(f"generate_many: prefix_sharing shares one level only, n = {n} samples already read their leader's "
                                 "prompt: use n=1, or prefix_sharing=False")
            if D:
                raise ValueError(f"generate_many: prefix_sharing has no verify step over a shared prefix, lookup = {D}: use lookup=0, "
                                 "or prefix_sharing=False")
            if image_ids is not None and len(image_ids) != len(prompts):
                raise ValueError(f"generate_many: image_ids has {len(image_ids)} entries for {len(prompts)} prompts")
        if lookup_verify not in ("argmax", "choice"):
            raise ValueError(f"generate_many: lookup_verify = {lookup_verify!r}; 'argmax' (greedy verification, the default) or 'choice' "
                             "(sample and match)")
        if D and lookup_verify == "choice":
            return self._generate_many_choice(prompts, images, batch_rows=batch_rows, max_gen_len=max_gen_len, temperature=temperature,
                                              top_p=top_p, additional_stop_symbols=additional_stop_symbols, return_ids=return_ids,
                                              poll_every=poll_every, sample_uniforms=sample_uniforms, repetition_penalty=repetition_penalty,
                                              return_logprobs=return_logprobs, top_k=top_k, min_p=min_p, n=n, D=D, lookup_ngram=lookup_ngram,
                                              lookup_drafter=lookup_drafter, constraint=constraint)
        if D and constraint is not None:
            raise ValueError("generate_many: lookup decoding verifies drafts against the unconstrained argmax, a constraint changes the "
                             "choice: use lookup=0, or constraint=None, or lookup_verify='choice'")
        automaton = self.constraint_automaton(constraint)
        if D:                              # refusals of lookup decoding, before any device use
            if D < 0 or D > 7:
                raise ValueError(f"generate_many: lookup = {D} drafted tokens per step; 1 .. 7 (a step has at most 8 query positions per row)")
            if temperature > 0:
                raise ValueError("generate_many: lookup decoding verifies drafts against the greedy choice: use temperature=0, or lookup=0, "
                                 "or lookup_verify='choice'")
            if n > 1:
                raise ValueError(f"generate_many: lookup decoding is greedy, n = {n} samples need temperature > 0: use n=1, or lookup=0")
            if controls:
                raise ValueError("generate_many: lookup decoding has no repetition-penalty / log-prob form (several tokens per step): "
                                 "use repetition_penalty=1.0 and return_logprobs=False, or lookup=0, or lookup_verify='choice'")
            if int(batch_rows) * (D + 1) > 32:
                raise ValueError(f"generate_many: batch_rows * (lookup + 1) = {int(batch_rows) * (D + 1)} > 32 rows of one decode step: "
                                 f"use batch_rows <= {32 // (D + 1)} or lookup <= {max(32 // int(batch_rows) - 1, 0)}")
            if int(lookup_ngram) < 1:
                raise ValueError(f"generate_many: lookup_ngram = {lookup_ngram}; >= 1")
        llma = self.llma
        llma._ragged_check("lookup decoding" if D else "extend_rows" if prefix_sharing else None)  # before anything is allocated or launched
        dev = self._device
        N = len(prompts)
        args = llma.args
        R = int(batch_rows)
        assert 0 < R <= args.max_batch_size, (R, args.max_batch_size)
        mgl = [int(max_gen_len)] * N if isinstance(max_gen_len, int) else [int(x) for x in max_gen_len]
        assert len(mgl) == N, (len(mgl), N)
        image_keys = list(image_ids) if image_ids is not None else None
        if isinstance(images, (list, tuple)):          # a list of per-prompt images: the same object is the same image
            if image_keys is None:
                image_keys = [id(x) for x in images]
            images = torch.stack(list(images)) if len(images) else None
        if image_keys is None:                         # a stacked tensor says nothing about equal rows; no image at all is one image
            image_keys = list(range(N)) if images is not None else [None] * N
        if images is not None:
            images = images.to(dev)
            assert images.shape[0] == N, (tuple(images.shape), N)
        max_seq_len = args.max_seq_len - (llma.image_words if images is not None else 0)
        W = llma.image_words if images is not None else 0
        prompt_tokens, limits = [], []
        for x, mg in zip(prompts, mgl):
            t = self.tokenizer.encode(x, bos=True, eos=False)
            limits.append(min(max_seq_len, mg + len(t)))
            prompt_tokens.append(t[-(max_seq_len - mg):])
        lens = [len(t) for t in prompt_tokens]
        if N == 0:
            ret = ([], []) if return_ids else []
            return (ret + ([],) if return_ids else ([], [])) if return_logprobs else ret

        l_stop = [[self.tokenizer.eos_id]]
        l_stop += [self.tokenizer.encode_segment(s) for s in additional_stop_symbols]
        l_stop += [self.tokenizer.encode_wo_prefix_space(s) for s in additional_stop_symbols]
        offs = [0]
        for st in l_stop:
            offs.append(offs[-1] + len(st))
        stop_seq = torch.tensor([t for st in l_stop for t in st], dtype=torch.long, device=dev)
        stop_off = torch.tensor(offs, dtype=torch.int32, device=dev)

        width = max(max(limits), max(lens), 1)
        tokens = torch.zeros((R, width), dtype=torch.long, device=dev)
        cur = torch.zeros(R, dtype=torch.int32, device=dev)
        limit = torch.zeros(R, dtype=torch.int32, device=dev)
        stopped = torch.ones(R, dtype=torch.bool, device=dev)            # an empty row is a stopped row: no step touches it
        stop_pos = torch.zeros(R, dtype=torch.long, device=dev)
        next_tok = torch.zeros(R, dtype=torch.long, device=dev)
        pos = torch.full((R,), -1, dtype=torch.int32, device=dev)
        logits = torch.zeros((R, args.vocab_size), dtype=torch.float32, device=dev)
        uni = sampled = ubase = None
        if temperature > 0:
            n_steps = max(max(lim - ln for lim, ln in zip(limits, lens)), 1)
            uni = (torch.rand(N, n, n_steps, device=dev, dtype=torch.float32) if sample_uniforms is None
                   else sample_uniforms.to(device=dev, dtype=torch.float32).contiguous())
            if n == 1 and uni.dim() == 2:
                uni = uni[:, None]
            assert uni.dim() == 3 and tuple(uni.shape[:2]) == (N, n) and uni.shape[2] >= n_steps, (tuple(uni.shape), N, n, n_steps)
            n_uni = uni.shape[2]
            uni = uni.reshape(-1)
            sampled = torch.zeros(R, dtype=torch.long, device=dev)
            ubase = torch.zeros(R, dtype=torch.long, device=dev)         # index of the row's uniform at scheduler step 0

        gc = None
        if controls:
            gc = genctl.GenControls(R, args.vocab_size, max(lim - ln for lim, ln in zip(limits, lens)), repetition_penalty,
                                    return_logprobs, dev)
        cs = constrain.ConstraintState(automaton, R, args.vocab_size, dev) if automaton is not None else None
        # answers are kept per (prompt, sample) at index i * n + s
        runs = prefix_groups(prompt_tokens, image_keys, W) if prefix_sharing else []
        share = any(P > 0 for _, P in runs)            # no run of several prompts: the plain call, untouched
        if share:
            sched = PrefixScheduler(lens, limits, R, W, runs)
        else:
            sched = RowScheduler(lens, limits, R, W) if n == 1 else GroupScheduler(lens, limits, R, W, n)
        ids: List[Optional[List[int]]] = [None] * (N * n)
        lps: List[List[float]] = [[] for _ in range(N * n)]
        llma.allocate_rows(R)
        src_row = shared = None
        if n > 1 or share:                 # shared prompt keys: row r reads its keys below shared[r] from cache row src_row[r]
            src_row = torch.arange(R, dtype=torch.int32, device=dev)
            shared = torch.zeros(R, dtype=torch.int32, device=dev)
        sample_of = [0] * R
        if D:
            Q = D + 1
            xq = torch.zeros((R, Q), dtype=torch.long, device=dev)
            nq = torch.ones(R, dtype=torch.int32, device=dev)
            vlogits = torch.zeros((R * Q, args.vocab_size), dtype=torch.float32, device=dev)
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            bound = LookupBound(R, Q)
            smax = llma._k_cache[0].shape[2]
            emitted = it = 0
            while True:
                for row, i in sched.refill():
                    t = torch.tensor(prompt_tokens[i], dtype=torch.long, device=dev)
                    vlogits[row * Q].copy_(llma.prefill_row(row, t[None], None if images is None else images[i:i + 1])[0])
                    tokens[row].zero_()
                    tokens[row, :lens[i]] = t
                    cur[row], limit[row], stopped[row], stop_pos[row], nq[row] = lens[i], limits[i], False, lens[i] + 1, 1
                    bound.start(row, W + lens[i], W + limits[i] - 1)      # the first generated id lands behind the prompt
                for i in sched.finished_at_once:
                    ids[i] = []
                sched.finished_at_once.clear()
                if not sched.occupied():
                    break
                # a refilled row has nq = 1 and its prefill logits in query 0: the plain token step
                ops.accept_rows(vlogits, xq, nq, tokens, cur, limit, W, stop_seq, stop_off, len(l_stop), stopped, stop_pos, next_tok, pos, stats)
                it += 1
                if it % poll_every == 0:                     # the one host read: stopped, and cur to re-synchronise the position bound
                    st, cu, sp = stopped.tolist(), cur.tolist(), stop_pos.tolist()
                    for r, i in sched.occupied():
                        if st[r]:
                            ids[i] = tokens[r, lens[i]:sp[r]].tolist()
                            emitted += cu[r] - lens[i]
                            sched.release(r)
                            bound.release(r)
                        else:
                            bound.resync(r, W + cu[r] - 1)
                    if not sched.occupied():
                        continue                                         # refill (or leave) before another step
                if lookup_drafter is not None:
                    lookup_drafter(tokens, cur, limit, pos, stopped, next_tok, xq, nq)
                else:
                    ops.lookup_draft_rows(tokens, cur, limit, pos, stopped, next_tok, D, int(lookup_ngram), smax, xq, nq)
                llma.forward_verify_rows(xq, pos, nq, bound.step(), out=vlogits)
            drafted, accepted = (int(v) for v in stats.tolist())
            self.last_lookup_stats = {"steps": emitted - accepted, "tokens": emitted, "drafted": drafted, "accepted": accepted}
            decoded = [self.tokenizer.decode(t) for t in ids]
            return (decoded, ids) if return_ids else decoded
        while True:
            if share:                      # prefix sharing: plain refills as below; a run's members extend over the prefix in its leader row
                admitted = []
                for lead, P, new, members in sched.refill():
                    if P == 0:
                        admitted.append((members[0][1], [lead], True))
                        src_row[lead], shared[lead] = lead, 0
                        continue
                    i0 = members[0][1]
                    if new:                # the first P positions, once: BOS, the image words, the common text (logits discarded)
                        t = torch.tensor(prompt_tokens[i0][:P - W], dtype=torch.long, device=dev)
                        llma.prefill_row(lead, t[None], None if images is None else images[i0:i0 + 1])
                    rws = [r for r, _ in members]
                    sfx = [torch.tensor(prompt_tokens[i][P - W:], dtype=torch.long, device=dev) for _, i in members]
                    lg = llma.extend_rows(rws, sfx, [P] * len(rws), src_row=[lead] * len(rws), shared=[P] * len(rws))
                    for j, (r, i) in enumerate(members):
                        logits[r].copy_(lg[j])
                        src_row[r], shared[r] = lead, P
                        admitted.append((i, [r], False))
            else:
                admitted = [(i, rows, True) for i, rows in ([(i, [row]) for row, i in sched.refill()] if n == 1 else sched.refill())]
            for i, rows, prefill in admitted:
                lead = rows[0]
                t = torch.tensor(prompt_tokens[i], dtype=torch.long, device=dev)
                if prefill:
                    logits[lead].copy_(llma.prefill_row(lead, t[None], None if images is None else images[i:i + 1])[0])
                if n > 1:                  # one prefill per group: the siblings start from the leader's logits and read its prefix
                    src_row[lead], shared[lead] = lead, 0
                    sib = torch.tensor(rows[1:], dtype=torch.long, device=dev)
                    for r in rows[1:]:
                        logits[r].copy_(logits[lead])
                    src_row[sib] = lead
                    shared[sib] = llma.share_prefix(lead, sib.to(torch.int32), W + lens[i])
                for s, row in enumerate(rows):
                    sample_of[row] = s
                    tokens[row].zero_()
                    tokens[row, :lens[i]] = t
                    cur[row], limit[row], stopped[row], stop_pos[row] = lens[i], limits[i], False, lens[i] + 1
                    if gc is not None:     # the row's seen set is its new prompt alone; the first id (prefill logits) is recorded below
                        gc.prompt_len[row] = lens[i]
                        gc.mark_prompts(tokens, row)
                    if ubase is not None:
                        ubase[row] = (i * n + s) * n_uni - sched.steps
                    if cs is not None:     # a refilled row (every sibling of a group) starts over
                        cs.reset(row, lens[i])
            for i in sched.finished_at_once:
                for s in range(n):
                    ids[i * n + s] = []
            sched.finished_at_once.clear()
            if not sched.occupied():
                break
            z = logits
            if gc is not None:
                z = gc.prepare(logits)
                gc.snapshot(stopped)       # a row that is stopped on entry is not touched by the step, nor by the record
            if cs is not None:
                z = cs.mask(z, logits)
                cs.stopped_before.copy_(stopped)               # as gc.snapshot: a row stopped on entry is not advanced
            if temperature > 0:
                u = uni[(ubase + sched.steps).clamp_(0, uni.numel() - 1)]
                self._sample_into(z, temperature, top_p, u, sampled, top_k, min_p)
            ops.generate_step_rows(z, sampled, tokens, cur, limit, W, stop_seq, stop_off, len(l_stop), stopped, stop_pos, None,
                                   next_tok, pos)
            if gc is not None:
                gc.record(logits, tokens, cur=cur, stopped_before=gc.stopped_before)
            if cs is not None:
                cs.advance(tokens, cur=cur, stopped_before=cs.stopped_before)
            pos_max = sched.advance()
            if sched.steps % poll_every == 0 or all(sched.generated[r] >= limits[i] - lens[i] for r, i in sched.occupied()):
                st = stopped.tolist()
                fin = [(r, i) for r, i in sched.occupied() if st[r]]
                if fin:
                    sp = stop_pos.tolist()
                    for r, i in fin:
                        j = i * n + sample_of[r]
                        ids[j] = tokens[r, lens[i]:sp[r]].tolist()
                        if return_logprobs:
                            lps[j] = gc.lp[r, :len(ids[j])].tolist()
                        sched.release(r)
                    if not sched.occupied():
                        continue                                         # refill (or leave) before another step
            if n == 1 and not share:
                llma.forward_inference_rows(next_tok, pos, pos_max, out=logits)
            else:
                llma.forward_inference_rows(next_tok, pos, pos_max, out=logits, src_row=src_row, shared=shared)
        decoded = [self.tokenizer.decode(t) for t in ids]
        scores = [genctl.score(x) for x in lps] if return_logprobs else None
        if n > 1:                          # per prompt: a list of n, sample order
            decoded, ids = ([x[i * n:(i + 1) * n] for i in range(N)] for x in (decoded, ids))
            if scores is not None:
                scores = [scores[i * n:(i + 1) * n] for i in range(N)]
        ret = (decoded, ids) if return_ids else decoded
        if return_logprobs:
            ret = ret + (scores,) if return_ids else (decoded, scores)
        return ret

    def _generate_many_choice(self, prompts, images, *, batch_rows, max_gen_len, temperature, top_p, additional_stop_symbols, return_ids,
                              poll_every, sample_uniforms, repetition_penalty, return_logprobs, top_k, min_p, n, D, lookup_ngram,
                              lookup_drafter, constraint):
        """``generate_many(lookup=D, lookup_verify="choice")``: the lookup loop with sample and match in place of the greedy
        accept.  Per step: draft -> ``forward_verify_rows`` -> ``a3v_verify_prepare`` -> sampler or argmax over the R * Q prepared
        rows -> ``a3v_accept_rows_chosen``; no host read outside the poll.  Afterwards ``last_lookup_stats`` as in the greedy
        loop and ``last_lookup_state``: the final seen bitmap and automaton states of the cache rows (None where not used)."""
        from .ragged import LookupBound, RowScheduler
        controls = genctl.wanted(repetition_penalty, return_logprobs)      # every refusal: a ValueError before any device use
        if D < 1 or D > 7:
            raise ValueError(f"generate_many: lookup = {D} drafted tokens per step; 1 .. 7 (a step has at most 8 query positions per row)")
        if n > 1:
            raise ValueError(f"generate_many: lookup decoding has no shared-prefix verify step, n = {n} samples per prompt cannot use it: "
                             "use n=1, or lookup=0")
        if int(batch_rows) * (D + 1) > 32:
            raise ValueError(f"generate_many: batch_rows * (lookup + 1) = {int(batch_rows) * (D + 1)} > 32 rows of one decode step: "
                             f"use batch_rows <= {32 // (D + 1)} or lookup <= {max(32 // int(batch_rows) - 1, 0)}")
        if int(lookup_ngram) < 1:
            raise ValueError(f"generate_many: lookup_ngram = {lookup_ngram}; >= 1")
        automaton = self.constraint_automaton(constraint)
        llma = self.llma
        llma._ragged_check("lookup decoding")                 # before anything is allocated or launched
        dev = self._device
        N = len(prompts)
        args = llma.args
        R, Q, V = int(batch_rows), D + 1, args.vocab_size
        assert 0 < R <= args.max_batch_size, (R, args.max_batch_size)
        mgl = [int(max_gen_len)] * N if isinstance(max_gen_len, int) else [int(x) for x in max_gen_len]
        assert len(mgl) == N, (len(mgl), N)
        if images is not None:
            images = images.to(dev)
            assert images.shape[0] == N, (tuple(images.shape), N)
        max_seq_len = args.max_seq_len - (llma.image_words if images is not None else 0)
        W = llma.image_words if images is not None else 0
        prompt_tokens, limits = [], []
        for x, mg in zip(prompts, mgl):
            t = self.tokenizer.encode(x, bos=True, eos=False)
            limits.append(min(max_seq_len, mg + len(t)))
            prompt_tokens.append(t[-(max_seq_len - mg):])
        lens = [len(t) for t in prompt_tokens]
        if N == 0:
            ret = ([], []) if return_ids else []
            return (ret + ([],) if return_ids else ([], [])) if return_logprobs else ret

        l_stop = [[self.tokenizer.eos_id]]
        l_stop += [self.tokenizer.encode_segment(s) for s in additional_stop_symbols]
        l_stop += [self.tokenizer.encode_wo_prefix_space(s) for s in additional_stop_symbols]
        offs = [0]
        for st in l_stop:
            offs.append(offs[-1] + len(st))
        stop_seq = torch.tensor([t for st in l_stop for t in st], dtype=torch.long, device=dev)
        stop_off = torch.tensor(offs, dtype=torch.int32, device=dev)

        width = max(max(limits), max(lens), 1)
        max_new = max(max(lim - ln for lim, ln in zip(limits, lens)), 1)
        tokens = torch.zeros((R, width), dtype=torch.long, device=dev)
        cur = torch.zeros(R, dtype=torch.int32, device=dev)
        limit = torch.zeros(R, dtype=torch.int32, device=dev)
        stopped = torch.ones(R, dtype=torch.bool, device=dev)            # an empty row is a stopped row: no step touches it
        stop_pos = torch.zeros(R, dtype=torch.long, device=dev)
        next_tok = torch.zeros(R, dtype=torch.long, device=dev)
        pos = torch.full((R,), -1, dtype=torch.int32, device=dev)
        uni, n_uni = None, 0
        if temperature > 0:            # indexed [prompt, generated index], as the plain loop's
            uni = (torch.rand(N, max_new, device=dev, dtype=torch.float32) if sample_uniforms is None
                   else sample_uniforms.to(device=dev, dtype=torch.float32).contiguous())
            if uni.dim() == 3 and uni.shape[1] == 1:
                uni = uni[:, 0]
            assert uni.dim() == 2 and uni.shape[0] == N and uni.shape[1] >= max_new, (tuple(uni.shape), N, max_new)
            n_uni = uni.shape[1]
            uni = uni.reshape(-1)
        gc = genctl.GenControls(R, V, max_new, repetition_penalty, return_logprobs, dev) if controls else None
        cs = constrain.ConstraintState(automaton, R, V, dev) if automaton is not None else None
        vc = genctl.VerifyControls(R, Q, V, dev, gc=gc, cs=cs, sampling=uni is not None)
        sched = RowScheduler(lens, limits, R, W)
        ids: List[Optional[List[int]]] = [None] * N
        lps: List[List[float]] = [[] for _ in range(N)]
        llma.allocate_rows(R)
        xq = torch.zeros((R, Q), dtype=torch.long, device=dev)
        nq = torch.ones(R, dtype=torch.int32, device=dev)
        vlogits = torch.zeros((R * Q, V), dtype=torch.float32, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        bound = LookupBound(R, Q)
        smax = llma._k_cache[0].shape[2]
        emitted = it = 0
        while True:
            for row, i in sched.refill():
                t = torch.tensor(prompt_tokens[i], dtype=torch.long, device=dev)
                vlogits[row * Q].copy_(llma.prefill_row(row, t[None], None if images is None else images[i:i + 1])[0])
                tokens[row].zero_()
                tokens[row, :lens[i]] = t
                cur[row], limit[row], stopped[row], stop_pos[row], nq[row] = lens[i], limits[i], False, lens[i] + 1, 1
                pos[row] = W + lens[i] - 1                    # query 0 of a refilled row is live: the prefill logits of its last prompt token
                vc.prompt_len[row] = lens[i]
                vc.row_base[row] = i * n_uni
                if gc is not None:                            # the row's seen set is its new prompt alone
                    gc.mark_prompts(tokens, row)
                if cs is not None:
                    cs.reset(row, lens[i])
                bound.start(row, W + lens[i], W + limits[i] - 1)
            for i in sched.finished_at_once:
                ids[i] = []
            sched.finished_at_once.clear()
            if not sched.occupied():
                break
            z = vc.prepare(vlogits, xq, nq, pos)              # a refilled row has nq = 1 and its prefill logits in query 0
            if uni is not None:
                self._sample_into(z, temperature, top_p, vc.uniforms(uni, cur), vc.chosen, top_k, min_p)
            else:
                ops.argmax(z, vc.chosen)
            vc.accept(vlogits, xq, nq, tokens, cur, limit, W, stop_seq, stop_off, len(l_stop), stopped, stop_pos, next_tok, pos, stats)
            it += 1
            if it % poll_every == 0:                          # the one host read: stopped, and cur to re-synchronise the position bound
                st, cu, sp = stopped.tolist(), cur.tolist(), stop_pos.tolist()
                for r, i in sched.occupied():
                    if st[r]:
                        ids[i] = tokens[r, lens[i]:sp[r]].tolist()
                        if return_logprobs:
                            lps[i] = gc.lp[r, :len(ids[i])].tolist()
                        emitted += cu[r] - lens[i]
                        sched.release(r)
                        bound.release(r)
                    else:
                        bound.resync(r, W + cu[r] - 1)
                if not sched.occupied():
                    continue                                  # refill (or leave) before another step
            if lookup_drafter is not None:
                lookup_drafter(tokens, cur, limit, pos, stopped, next_tok, xq, nq)
            else:
                ops.lookup_draft_rows(tokens, cur, limit, pos, stopped, next_tok, D, int(lookup_ngram), smax, xq, nq)
            llma.forward_verify_rows(xq, pos, nq, bound.step(), out=vlogits)
        drafted, accepted = (int(v) for v in stats.tolist())
        self.last_lookup_stats = {"steps": emitted - accepted, "tokens": emitted, "drafted": drafted, "accepted": accepted}
        self.last_lookup_state = {"seen": gc.seen if gc is not None else None, "state": cs.state if cs is not None else None}
        decoded = [self.tokenizer.decode(t) for t in ids]
        ret = (decoded, ids) if return_ids else decoded
        if return_logprobs:
            scores = [genctl.score(x) for x in lps]
            ret = ret + (scores,) if return_ids else (decoded, scores)
        return ret

    @torch.no_grad()
    def beam_search(self, prompts: List[str], images: Optional[torch.Tensor] = None, *, num_beams: int, batch_rows: int,
                    max_gen_len=512, length_penalty: float = 1.0, early_stopping: bool = True, num_return_sequences: int = 1,
                    constraint=None, return_ids: bool = False, return_scores: bool = False, poll_every: int = 4,
                    additional_stop_symbols: Iterable[str] = (), temperature: float = 0.0, repetition_penalty: float = 1.0, lookup=None,
                    prefix_sharing: bool = False):
        """Beam search over ``batch_rows // num_beams`` prompts at a time (no reference counterpart; opt-in; ``model/beam.py``): the
        most probable answers by the sum of raw log-probs over ``len ** length_penalty``, HF ``num_beams`` semantics
        (``tests/beam_ref.py`` is the contract).  1 <= ``num_beams`` <= 8 consecutive cache rows per prompt, ONE prefill per prompt
        (the siblings read the leader's prompt keys, ``share_prefix``); a finished group is refilled with the next prompt, in input
        order.  Truncation and limits per prompt are ``generate_many``'s.  Only the EOS id ends a hypothesis.  ``early_stopping``:
        a prompt ends when ``num_beams`` hypotheses are finished; False: when no live beam can still beat the worst of them.
        ``constraint``: as in ``generate_many`` (scores stay the unconstrained model's).  Returns per prompt the best text (a list of
        ``num_return_sequences`` when that is > 1); with ``return_ids`` the ids, with ``return_scores``
        ``{"sum": sum of log-probs, "score": sum / len ** length_penalty}``.  Every step moves the generated keys of re-parented
        beams, which grows linearly with the answer's length: made for the short structured answers of this task.
        ``additional_stop_symbols``, ``temperature > 0``, ``repetition_penalty != 1`` and ``lookup`` are refused, as are the fp8 KV
        cache, LoRA models before ``merge_lora()`` and the two-image plugin (each raises, naming the way out), and
        ``prefix_sharing`` (the beams of a prompt already read their leader's row; sharing goes one level only)."""
        if prefix_sharing:
            raise ValueError("beam_search: the beams of a prompt already share their leader's prompt keys and sharing goes one level "
                             "only: use prefix_sharing=False, or generate_many(prefix_sharing=True) for greedy / sampled answers")
        from . import beam
        return beam.beam_search(self, prompts, images, num_beams=num_beams, batch_rows=batch_rows, max_gen_len=max_gen_len,
                                length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                                constraint=constraint, return_ids=return_ids, return_scores=return_scores, poll_every=poll_every,
                                additional_stop_symbols=additional_stop_symbols, temperature=temperature,
                                repetition_penalty=repetition_penalty, lookup=lookup)

    @torch.no_grad()
    def stream_generate(self, prompt: str, image: Optional[torch.Tensor] = None, max_gen_len: int = 512,
                        temperature: float = 0.0, top_p: float = 0.95,
                        additional_stop_symbols: Iterable[str] = (), repetition_penalty: float = 1.0,
                        return_logprobs: bool = False, top_k: int = 0, min_p: float = 0.0, constraint=None):
        """meta.py:487-566.  ``repetition_penalty`` / ``return_logprobs`` as in ``generate``; with ``return_logprobs`` every yielded
        dict also carries ``"logprobs"``: one value per token generated so far (the text may be cut inside the last ones by a stop
        string).  ``top_k`` / ``min_p`` as in ``generate``.  ``constraint`` is refused: constrained decoding has no streaming form
        (use ``generate`` / ``generate_many``)."""
        if constraint is not None:
            raise ValueError("stream_generate: constrained decoding has no streaming form: use generate(constraint=...) or "
                             "generate_many(constraint=...), or constraint=None")
        controls = genctl.wanted(repetition_penalty, return_logprobs)      # ValueError before any device use
        top_k, min_p = genctl.check_filters(top_k, min_p)
        args = self.llma.args
        dev = self._device
        prompt_tokens = self.tokenizer.encode(prompt, bos=True, eos=False)
        max_seq_len = args.max_seq_len
        if image is not None:
            max_seq_len -= self.llma.image_words
            if image.dim() == 4:
                assert image.shape[0] == 1
            else:
                assert image.dim() == 3
                image = image.unsqueeze(0)
            image = image.to(dev)
        prompt_tokens = prompt_tokens[-(max_seq_len - max_gen_len):]
        prompt_size = len(prompt_tokens)
        total_len = min(max_seq_len, max_gen_len + prompt_size)
        tokens = torch.zeros(total_len, dtype=torch.long, device=dev)
        tokens[:prompt_size] = torch.tensor(prompt_tokens, dtype=torch.long)
        start_pos, prev_pos, generate_until = prompt_size, 0, prompt_size
        nt_buf = torch.empty(1, dtype=torch.long, device=dev)
        gc = None
        if controls:
            gc = genctl.GenControls(1, args.vocab_size, total_len - start_pos, repetition_penalty, return_logprobs, dev)
            gc.prompt_len.fill_(prompt_size)
            gc.mark_prompts(tokens[None])

        def out(text, end):
            d = {"text": text, "end_of_content": end}
            if return_logprobs:
                d["logprobs"] = gc.lp[0, :generate_until - start_pos].tolist()
            return d

        for cur_pos in range(start_pos, total_len):
            logits = self.llma.forward_inference(tokens[None, prev_pos:cur_pos], prev_pos,
                                                 image if prev_pos == 0 else None)
            z = gc.prepare(logits) if gc is not None else logits
            if temperature > 0:
                nt = self._sample_into(z, temperature, top_p, torch.rand(1, device=dev), nt_buf, top_k, min_p)
            else:
                nt = ops.argmax(z, nt_buf)
            nt = int(nt.reshape(-1)[0].item())
            if nt == self.tokenizer.eos_id:
                break
            tokens[cur_pos] = nt
            if gc is not None:
                gc.record(logits, tokens[None], col=cur_pos)
            prev_pos = cur_pos
            generate_until = cur_pos + 1
            generated = self.tokenizer.decode(tokens[start_pos:generate_until].tolist())
            for s in additional_stop_symbols:
                sp = generated.find(s)
                if sp != -1:
                    yield out(generated[:sp], True)
                    return
            yield out(generated, False)
        generated = self.tokenizer.decode(tokens[start_pos:generate_until].tolist())
        yield out(generated, True)

    def _sample_into(self, logits: torch.Tensor, temperature: float, top_p: float, uniforms: torch.Tensor, out: torch.Tensor,
                     top_k: int = 0, min_p: float = 0.0) -> torch.Tensor:
        """One top-p draw per row into ``out``: the device kernel where it applies (V <= 65536, 0 < top_p), otherwise the reference's
        sort / cumsum / multinomial recipe (meta.py:456-458, 568-583) -- larger vocabularies must keep working as they do there.
        ``top_k`` / ``min_p`` set: ``a3v_sample_top_k_p`` under the same condition, otherwise the same three rules in torch."""
        filters = top_k > 0 or min_p > 0
        if logits.shape[-1] <= 65536 and top_p > 0:
            if filters:
                return ops.sample_top_k_p(logits, temperature, top_k, top_p, min_p, uniforms, out)
            return ops.sample_top_p(logits, temperature, top_p, uniforms, out)
        z = logits.float()
        if 0 < top_k < z.shape[-1]:                       # on the logits' own values: ties at the k-th one are kept
            z = z.masked_fill(z < z.topk(top_k, dim=-1).values[..., -1:], float("-inf"))
        probs = torch.softmax(z / temperature, dim=-1)
        out.copy_(self.sample_top_p(probs, top_p, min_p).reshape(-1))
        return out

    def sample_top_p(self, probs: torch.Tensor, p: float, min_p: float = 0.0) -> torch.Tensor:
        """meta.py:568-583, kept for callers of the reference's method (torch ops; ``generate`` itself draws on the device with
        ``a3v_sample_top_p``, same nucleus, explicit uniforms)."""
        ranked, order = probs.sort(dim=-1, descending=True)
        before = ranked.cumsum(dim=-1) - ranked                 # mass ranked ahead of each token
        kept = ranked.masked_fill(before > p, 0.0)
        if min_p > 0:                                     # p_i >= min_p * p_max (ranked[..., 0] is the maximum)
            kept = kept.masked_fill(ranked < min_p * ranked[..., :1], 0.0)
        draw = torch.multinomial(kept / kept.sum(dim=-1, keepdim=True), num_samples=1)
        return order.gather(-1, draw)

    def get_image_words(self) -> int:
        return self.llma.image_words

    def get_quant_blocklist(self) -> List[str]:
        if hasattr(self.llma, "get_quant_blocklist"):
            return ["llma." + x for x in self.llma.get_quant_blocklist()]
        return []

    def get_basic_block_classes(self):
        if hasattr(self.llma, "get_basic_block_classes"):
            return self.llma.get_basic_block_classes()
        return [type(self.llma.layers[0])]
