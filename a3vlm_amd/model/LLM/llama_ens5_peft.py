"""LoRA variant of the ``llama_ens5`` plugin (BASELINE config 3: LoRA fine-tune of the same backbone).

The reference snapshot ships the adapter layers (``model/peft.py``: ``y = W x (+ b) + lora_b(lora_a(x))``, no alpha / rank
scaling, ``lora_a ~ trunc_normal(0.02)``, ``lora_b = 0``, state-dict keys ``<linear>.lora_a.weight`` / ``.lora_b.weight``)
and the façade hooks (``MetaModel.is_peft`` meta.py:72, whole-model FSDP wrap when PEFT main_finetune.py:246) but no plugin
that instantiates them (``llama_peft`` is absent, ``LLM/__init__.py:3``).  This plugin puts adapters on the seven decoder
linears of every block -- the upstream LLaMA2-Accessory ``llama_peft`` arrangement -- on top of the ``llama_ens5``
multimodal stack, with the same key names, so a checkpoint of base + adapters loads by name.

Trainable: adapters, RMSNorm weights, the vision->language projectors and the image tags (everything the base plugin
trains that is not a frozen backbone matrix).  Base matrices, embeddings and the LM head are frozen.

Kernels: the three (two) adapters that share an input are fused -- ``t = x . [A_q; A_k; A_v]^T`` (one GEMM, rank padded to
a 64 multiple) and ``y += t . blockdiag(B_q, B_k, B_v)^T`` (one GEMM with the residual epilogue: ``bf16(acc) + y``, the
reference's rounding order) -- so an adapter group costs two skinny-N / skinny-K MFMA GEMMs instead of six.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, Optional

import torch
import torch.nn as nn

from ... import ops
from ... import lib as _lib
from ...train_images import GROUPS, group_modules
from . import llama_ens5 as base
from .llama_ens5 import _W


@dataclass
class ModelArgs(base.ModelArgs):
    lora_rank: int = 16
    bias_tuning: bool = False          # the Llama linears carry no bias (llama_ens5.py:63-90); kept for config compatibility


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def base_shape(mod) -> tuple:
    """(out, in) of a decoder linear's base matrix, also after ``quantize_base_weights`` freed its bf16 ``weight``."""
    q4 = getattr(mod, "q4", None)
    if q4 is not None:
        return q4[2]
    q8 = getattr(mod, "q8_shape", None)
    return tuple(mod.weight.shape) if q8 is None else q8


def merged_args(args: ModelArgs) -> base.ModelArgs:
    """The base plugin's ModelArgs of a merged model: the peft-only fields (``lora_rank``, ``bias_tuning``) are dropped, since the base
    ``ModelArgs`` -- and ``MetaModel`` reading a ``config.json`` for it -- rejects fields it does not know."""
    return base.ModelArgs(**{f.name: getattr(args, f.name) for f in fields(base.ModelArgs)})


class Transformer(base.Transformer):
    is_peft = True

    def __init__(self, args: ModelArgs, with_visual: bool = False):
        super().__init__(args, with_visual=with_visual)
        if args.bias_tuning:
            raise NotImplementedError("bias_tuning: the decoder linears of llama_ens5 have no bias terms")
        r = args.lora_rank
        assert r > 0 and r % 8 == 0, "lora_rank must be a positive multiple of 8"
        self.lora_rank = r
        for lyr in self.layers:
            for mod in (lyr.attention.wq, lyr.attention.wk, lyr.attention.wv, lyr.attention.wo,
                        lyr.feed_forward.w1, lyr.feed_forward.w2, lyr.feed_forward.w3):
                out_f, in_f = mod.weight.shape
                mod.lora_a = _W(r, in_f, init="normal")
                nn.init.trunc_normal_(mod.lora_a.weight, std=0.02)      # peft.py:72-74
                mod.lora_b = _W(out_f, r, init="normal")
                nn.init.zeros_(mod.lora_b.weight)                       # peft.py:76
        self._per_kernel_decode = True       # the single-call decode step has no adapter hooks
        self._lora_img: Dict[str, torch.Tensor] = {}
        self._lora_ver = None
        self._q4: Optional[Dict[str, tuple]] = None      # quantize_base_weights: module name -> (nibbles, scales, (N, K))
        self._q8base: Optional[Dict[str, tuple]] = None  # quantize_base_weights("fp8"): "<kind>.<layer>" -> (Wq, sw, WqT) of the fused group
        self._merged = False                             # merge_adapters: from then on every override below defers to the base class

    def quantize_decode_weights(self, mode: str = "fp8", prefill: bool = False) -> None:
        if self._merged:
            return super().quantize_decode_weights(mode, prefill)
        if mode == "nf4":
            # the reference keeps the LoRA adapters unquantised beside the NF4 base (llama_ens5.py:541-550, QLoRA): a follow-up
            raise NotImplementedError("NF4 decode weights beside LoRA adapters are not implemented: merge_adapters() first")
        if mode == "mxfp4":
            raise NotImplementedError("MXFP4 decode weights beside LoRA adapters are not implemented: merge_adapters() first")
        super().quantize_decode_weights(mode, prefill)

    def _ragged_check(self, what: Optional[str] = None) -> None:
        if not self._merged:
            # the ragged step has no adapter hooks: it would silently decode with the base weights alone
            raise NotImplementedError("ragged decode (prefill_row / forward_inference_rows / generate_many) is not implemented beside "
                                      "LoRA adapters: merge_adapters() first (MetaModel.merge_lora / --merge_lora), or use generate()")
        super()._ragged_check(what)

    def quantize_kv_cache(self, mode: Optional[str] = "fp8", rows: bool = False) -> None:
        if mode is not None and not self._merged:
            # decode beside adapters runs kernel by kernel with the adapter hooks (no fused step): the fp8 cache is not wired into it
            raise NotImplementedError("the fp8 KV cache is not implemented beside LoRA adapters: merge_adapters() first "
                                      "(MetaModel.merge_lora / --merge_lora), then quantize_kv_cache('fp8')")
        super().quantize_kv_cache(mode, rows)

    def quantize_base_weights(self, mode: str = "nf4") -> None:
        """QLoRA (the reference's ``main_finetune.py --quant``: bf16 model, checkpoint, ``quantize(model, nf4)``, then train what is left
        trainable; util/quant.py:95-163 skips every ``lora`` module).  The seven decoder linears of every layer and ``output`` are
        quantised by a3v_quantize_nf4 -- one ORIGINAL module at a time, rows in module order -- and each bf16 ``weight`` is freed
        (gone from ``state_dict()``; irreversible).  ``(nibbles, scales, (N, K))`` is kept per module (``self._q4[name]`` and
        ``module.q4``).  Adapters, norms, embeddings, projectors and tags are untouched and train as before.

        Training: ``TrainEngine`` dequantises one layer at a time into a reused scratch (a3v_dequantize_nf4_images) and runs the bf16
        LoRA step on it.  Inference (``forward``, ``forward_inference``, ``generate``) works for every row count the same way: a
        layer's Wd in a reused scratch, then the bf16 kernels plus adapters of the unquantised plugin -- bit-identical to the bf16 model
        holding Wd, but every decode step dequantises every layer again: decode speed on this path is not a goal.

        Needs bf16 base matrices on the GPU and K % 64 == 0 for every module (the format); none of the NF4 decode GEMV's limits.

        ``mode="fp8"``: the frozen base as OCP e4m3fn bytes for the LoRA step's base GEMMs.  Each fused GEMM group of a
        layer (``GROUPS``: wq|wk|wv, wo, w1|w3, w2; rows in image order) is quantised per output row by a3v_quantize_rows_fp8 into
        ``Wq`` [N, K] bytes and ``sw`` [N] fp32, and ``WqT`` [K, N padded to 128] is the byte transpose of Wq (zero pad; not a second
        quantisation) for the input gradient; ``self._q8base["<kind>.<layer>"] = (Wq, sw, WqT)``.  The bf16 ``weight`` of the seven
        linears is freed as above; ``output``, norms, embeddings, projectors, tags and adapters are untouched.  Training runs the base
        products on a3v_gemm_nt_fp8 (``TrainEngine``); inference dequantises a layer's Wd = bf16(Wq * sw) into the reused scratch and
        runs the unquantised plugin's kernels -- bit-identical to the bf16 model holding Wd.  Needs bf16 base matrices on the GPU,
        K % 128 == 0 for every decoder linear (the fp8 MFMA's K step) and head_dim 64 or 128."""
        if mode not in ("nf4", "fp8"):
            raise ValueError("only 'nf4' and 'fp8' base weights are implemented")
        if self._merged:
            raise RuntimeError("the adapters are merged: this is a plain llama_ens5 model now (quantize_decode_weights quantises it for inference)")
        if self._q4 is not None:
            raise RuntimeError("the base weights are already NF4")
        if self._q8base is not None:
            raise RuntimeError("the base weights are already fp8")
        if mode == "fp8":
            return self._quantize_base_fp8()
        named = []
        for i, lyr in enumerate(self.layers):
            at, f = lyr.attention, lyr.feed_forward
            named += [(f"layers.{i}.attention.{n}", getattr(at, n)) for n in ("wq", "wk", "wv", "wo")]
            named += [(f"layers.{i}.feed_forward.{n}", getattr(f, n)) for n in ("w1", "w3", "w2")]
        named.append(("output", self.output))
        for name, mod in named:
            w = mod.weight
            if w.dtype != torch.bfloat16 or w.device.type != "cuda":
                raise ValueError(f"NF4 base weights need a bf16 model on the GPU (quantise after .to(device)); {name}.weight is {w.dtype} on {w.device}")
            if w.shape[1] % 64:
                raise ValueError(f"NF4 base weights need K % 64 == 0 for every module; {name}.weight is {tuple(w.shape)}")
        ws = torch.empty((max(int(_lib.load().a3v_quantize_nf4_ws_bytes(*mod.weight.shape)) for _, mod in named) + 3) // 4,
                         dtype=torch.float32, device=named[0][1].weight.device)
        q4: Dict[str, tuple] = {}
        with torch.no_grad():
            for name, mod in named:
                q, sc, _ = ops.quantize_nf4(mod.weight.data.contiguous(), ws=ws)
                mod.q4 = q4[name] = (q, sc, tuple(mod.weight.shape))
                del mod.weight                          # quant.py:163
        self._q4 = q4
        self._packed, self._packed_version = {}, None
        self._lora_ver = None

    def _quantize_base_fp8(self) -> None:
        if self.head_dim not in (64, 128):
            raise ValueError(f"fp8 base weights need head_dim 64 or 128 (the fused qkv GEMM); got {self.head_dim}")
        for i, lyr in enumerate(self.layers):
            for kind, names in GROUPS.items():
                for nm, mod in zip(names, group_modules(lyr, kind)):
                    w = mod.weight
                    if w.dtype != torch.bfloat16 or w.device.type != "cuda":
                        raise ValueError(f"fp8 base weights need a bf16 model on the GPU (quantise after .to(device)); layers.{i}.{nm}.weight "
                                         f"is {w.dtype} on {w.device}")
                    if w.shape[1] % 128:
                        raise ValueError(f"fp8 base weights need K % 128 == 0 for every decoder linear; layers.{i}.{nm}.weight is {tuple(w.shape)}")
        q8: Dict[str, tuple] = {}
        with torch.no_grad():
            for i, lyr in enumerate(self.layers):
                for kind in GROUPS:
                    mods = group_modules(lyr, kind)
                    w = torch.cat([mod.weight.data for mod in mods], dim=0) if len(mods) > 1 else mods[0].weight.data.contiguous()
                    N, K = w.shape
                    wq = torch.empty(N, K, dtype=torch.uint8, device=w.device)
                    sw = torch.empty(N, dtype=torch.float32, device=w.device)
                    ops.quantize_rows_fp8(w, wq, sw)
                    wqt = torch.zeros(K, (N + 127) // 128 * 128, dtype=torch.uint8, device=w.device)
                    wqt[:, :N] = wq.t()                      # the byte transpose (runs once per model: data movement only)
                    q8[f"{kind}.{i}"] = (wq, sw, wqt)
                    for mod in mods:
                        mod.q8_shape = tuple(mod.weight.shape)
                        del mod.weight
                    del w
        self._q8base = q8
        self._packed, self._packed_version = {}, None
        self._lora_ver = None

    def _q8_dequantize(self, key: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Wd = bf16(float(Wq) * sw) of fused group ``key`` [N, K] (a torch cast and multiply: correctness paths only)."""
        wq, sw, _ = self._q8base[key]
        wd = (wq.view(torch.float8_e4m3fn).float() * sw[:, None]).to(torch.bfloat16)
        return wd if out is None else out.copy_(wd)

    def _q8_layer_weights(self, i: int):
        """Wd of layer i in the reused scratch, in the row orders of ``_pack``: (wqkv, wo, w13 in 16-row blocks, w2)."""
        a = self.args
        H, Hkv, hd, F, dim = self.n_heads, self.n_kv_heads, self.head_dim, self.ffn, a.dim
        shapes = (((H + 2 * Hkv) * hd, dim), (dim, H * hd), (2 * F, dim), (dim, F))
        buf = self._buf("q4_scratch", (sum(n * k for n, k in shapes),), torch.bfloat16)
        views, o = [], 0
        for n, k in shapes:
            views.append(buf[o:o + n * k].view(n, k))
            o += n * k
        wqkv, wo, w13, w2 = views
        self._q8_dequantize(f"qkv.{i}", wqkv)
        self._q8_dequantize(f"wo.{i}", wo)
        self._q8_dequantize(f"w2.{i}", w2)
        tmp = self._q8_dequantize(f"w13.{i}")
        w13.view(F // 16, 2, 16, dim).copy_(tmp.view(2, F // 16, 16, dim).transpose(0, 1))     # data movement only (the SwiGLU row order)
        return wqkv, wo, w13, w2

    def merge_adapters(self) -> None:
        """Fold every adapter into its base matrix, ``weight <- weight + lora_b . lora_a`` (a3v_lora_merge: fp32 accumulation, the base
        added in fp32, ONE rounding), and drop the adapters.  In place and irreversible.  Afterwards the object behaves as a
        ``llama_ens5.Transformer``: no ``lora_a`` / ``lora_b`` modules, the state-dict keys and ``args`` of the base plugin, ``is_peft``
        false, and forward, prefill, decode (the single-call step) and ``quantize_decode_weights("fp8" | "nf4")`` are the base
        class's; ``quantize_base_weights`` and a second ``merge_adapters`` raise ``RuntimeError``.

        The adapters are cast to the dtype of the base matrices first, as ``lora_images`` does for the adapter GEMMs (a trainer
        keeps them in fp32).  The merge works on the original modules in module row order.  Over ``quantize_base_weights("nf4")``
        the base of a module is its Wd = bf16(NF4[q] * s_b) -- what the QLoRA run trained against -- read straight from the NF4
        image: each freed ``weight`` comes back as a bf16 parameter, bit-equal to merging a bf16 model that holds Wd, and the
        image of a module is dropped as soon as it is merged, so the bf16 decoder is never alive twice.  ``output`` has no adapter
        and is dequantised.  Re-quantising such a model (``quantize_decode_weights("nf4")``) quantises W' afresh: a second
        quantisation error on top of the one inside Wd.

        Needs the model on the GPU and bf16 or fp32 base matrices of one dtype."""
        if self._merged:
            raise RuntimeError("the adapters are already merged")
        if self._q8base is not None:
            # fp8 base: every freed ``weight`` comes back as its bf16 Wd (one fused group alive at a time), then the bf16 route below
            with torch.no_grad():
                for i, lyr in enumerate(self.layers):
                    for kind in GROUPS:
                        wd, row = self._q8_dequantize(f"{kind}.{i}"), 0
                        del self._q8base[f"{kind}.{i}"]
                        for mod in group_modules(lyr, kind):
                            n = mod.q8_shape[0]
                            mod.weight = nn.Parameter(wd[row:row + n].clone(), requires_grad=False)
                            del mod.q8_shape
                            row += n
                        del wd
            self._q8base = None
        named = []
        for i, lyr in enumerate(self.layers):
            at, f = lyr.attention, lyr.feed_forward
            named += [(f"layers.{i}.attention.{n}", getattr(at, n)) for n in ("wq", "wk", "wv", "wo")]
            named += [(f"layers.{i}.feed_forward.{n}", getattr(f, n)) for n in ("w1", "w3", "w2")]
        q4 = self._q4
        dtypes = set()
        for name, mod in named:
            for t in (mod.lora_a.weight, mod.lora_b.weight) + (() if q4 is not None else (mod.weight,)):
                if t.device.type != "cuda":
                    raise ValueError(f"merge_adapters needs the model on the GPU (merge after .to(device)); {name} is on {t.device}")
            dtypes.add(torch.bfloat16 if q4 is not None else mod.weight.dtype)
        if len(dtypes) != 1 or not dtypes <= {torch.bfloat16, torch.float32}:
            raise ValueError(f"merge_adapters needs bf16 or fp32 base matrices of one dtype, got {sorted(map(str, dtypes))}")
        dtype = dtypes.pop()
        with torch.no_grad():
            for name, mod in named:
                lb = mod.lora_b.weight.detach().to(dtype).contiguous()
                la = mod.lora_a.weight.detach().to(dtype).contiguous()
                if q4 is None:
                    ops.lora_merge(mod.weight.data, lb, la)
                else:
                    q, sc, _ = q4.pop(name)
                    mod.weight = nn.Parameter(ops.lora_merge((q, sc), lb, la), requires_grad=False)
                    del mod.q4, q, sc
                del mod.lora_a, mod.lora_b
            if q4 is not None:
                q, sc, (n, k) = q4.pop("output")
                w = torch.empty(n, k, dtype=torch.bfloat16, device=q.device)
                ops.dequantize_nf4_images(q, sc, wd=w)
                self.output.weight = nn.Parameter(w, requires_grad=False)
                del self.output.q4
        self._q4 = None
        self._merged = True
        self.is_peft = False
        del self._per_kernel_decode
        self.args = merged_args(self.args)
        self._packed, self._packed_version = {}, None
        self._lora_img, self._lora_ver = {}, None
        for key in [k for k in self._ws if k[0] in ("q4_scratch", "q4_head", "lora_t", "lora_o")]:
            del self._ws[key]

    def _pack(self, check: bool = False) -> Dict[str, torch.Tensor]:
        if self._q4 is None and self._q8base is None:
            return super()._pack(check)
        if self._packed_version is not None and not check:
            return self._packed
        ver = self._weights_version()
        if self._packed_version != ver:              # NF4 / fp8 base: the decoder matrices live only as quantised images
            with torch.no_grad():
                self._packed = self._pack_vision() if self.with_visual else {}
            self._packed_version = ver
        return self._packed

    def _q4_layer_weights(self, i: int):
        """Wd of layer i in the reused scratch, in the row orders of ``_pack``: (wqkv, wo, w13 in 16-row blocks, w2)."""
        a = self.args
        H, Hkv, hd, F, dim = self.n_heads, self.n_kv_heads, self.head_dim, self.ffn, a.dim
        shapes = (((H + 2 * Hkv) * hd, dim), (dim, H * hd), (2 * F, dim), (dim, F), (2 * F, dim))
        buf = self._buf("q4_scratch", (sum(n * k for n, k in shapes),), torch.bfloat16)
        views, o = [], 0
        for n, k in shapes:
            views.append(buf[o:o + n * k].view(n, k))
            o += n * k
        wqkv, wo, w13, w2, tmp = views
        p = f"layers.{i}."
        row = 0
        for nm in ("wq", "wk", "wv"):
            q, sc, (n, _) = self._q4[p + "attention." + nm]
            ops.dequantize_nf4_images(q, sc, wd=wqkv[row:row + n])
            row += n
        ops.dequantize_nf4_images(*self._q4[p + "attention.wo"][:2], wd=wo)
        ops.dequantize_nf4_images(*self._q4[p + "feed_forward.w2"][:2], wd=w2)
        ops.dequantize_nf4_images(*self._q4[p + "feed_forward.w1"][:2], wd=tmp[:F])
        ops.dequantize_nf4_images(*self._q4[p + "feed_forward.w3"][:2], wd=tmp[F:])
        w13.view(F // 16, 2, 16, dim).copy_(tmp.view(2, F // 16, 16, dim).transpose(0, 1))     # data movement only (the SwiGLU row order)
        return wqkv, wo, w13, w2

    def _head_weight(self) -> torch.Tensor:
        if self._q4 is None:
            return super()._head_weight()
        q, sc, (n, k) = self._q4["output"]
        w = self._buf("q4_head", (n, k), torch.bfloat16)
        ops.dequantize_nf4_images(q, sc, wd=w)
        return w

    def _lm_head_f32(self, xn: torch.Tensor, logits: torch.Tensor) -> None:
        if self._q4 is None:
            return super()._lm_head_f32(xn, logits)
        self._linear(xn, self._head_weight(), logits, epilogue=ops.EPI_OUT_F32)

    def get_trainable_params(self, pretrain_stage: bool = False):
        if self._merged:
            return super().get_trainable_params(pretrain_stage)
        frozen_pre = ("qformer.", "openclip_convnext_xxl.", "clip.", "dinov2_vitg14.", "tok_embeddings.", "output.")
        out = {}
        for n, p in self.named_parameters():
            if n.startswith(frozen_pre):
                continue
            if n.startswith("layers.") and not ("lora_" in n or "norm" in n):
                continue
            out[n] = p
        return out

    # ------------------------------------------------------------------ fused adapter images
    def lora_groups(self, i: int):
        """(key, [modules sharing the input], interleave16) for layer i, in the row order of the fused base GEMMs."""
        return [(f"{kind}.{i}", group_modules(self.layers[i], kind), kind == "w13") for kind in GROUPS]

    def lora_images(self, dtype: Optional[torch.dtype] = None, interleave_w13: bool = True) -> Dict[str, torch.Tensor]:
        """Per group: ``A`` [Rp, in] (stacked lora_a, zero rows up to Rp = pad64(n*r)) and ``B`` [N, Rp] (block-diagonal
        lora_b in the row order of the fused base weight; w1/w3 rows interleaved in 16-row blocks when the base image is)."""
        dtype = dtype or self._dtype
        from ...util import param_state_key
        ver = (tuple(param_state_key(p) for n, p in self.named_parameters() if "lora_" in n), dtype, interleave_w13, str(self._device))
        if self._lora_ver == ver:
            return self._lora_img
        r = self.lora_rank
        im: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            for i in range(self.n_layers):
                for key, mods, inter in self.lora_groups(i):
                    Rp = _pad64(len(mods) * r)
                    in_f = base_shape(mods[0])[1]
                    A = torch.zeros(Rp, in_f, dtype=dtype, device=self._device)
                    blocks = []
                    for j, mod in enumerate(mods):
                        A[j * r:(j + 1) * r] = mod.lora_a.weight.to(dtype)
                        Bj = torch.zeros(base_shape(mod)[0], Rp, dtype=dtype, device=self._device)
                        Bj[:, j * r:(j + 1) * r] = mod.lora_b.weight.to(dtype)
                        blocks.append(Bj)
                    if inter and interleave_w13:
                        nb = blocks[0].shape[0] // 16
                        Bm = torch.stack([blocks[0].view(nb, 16, Rp), blocks[1].view(nb, 16, Rp)], dim=1).reshape(-1, Rp)
                    else:
                        Bm = torch.cat(blocks, dim=0)
                    im[key + ".A"], im[key + ".B"] = A, Bm.contiguous()
        self._lora_img, self._lora_ver = im, ver
        return im

    def _lora_add(self, key: str, x: torch.Tensor, y: torch.Tensor) -> None:
        """y += lora_b(lora_a(x)) for a fused group (peft.py:89-95)."""
        im = self.lora_images()
        A, Bm = im[key + ".A"], im[key + ".B"]
        t = self._buf("lora_t", (x.shape[0], A.shape[0]))
        self._linear(x, A, t)
        self._linear(t, Bm, y, residual=y)

    # ------------------------------------------------------------------ decoder stack with adapters
    def _decoder_layers(self, h: torch.Tensor, B: int, S: int, start_pos: int, rope_pos0: int,
                        k_caches, vt_caches, causal: bool) -> None:
        if self._merged:
            return super()._decoder_layers(h, B, S, start_pos, rope_pos0, k_caches, vt_caches, causal)
        a = self.args
        H, Hkv, hd, dim = self.n_heads, self.n_kv_heads, self.head_dim, a.dim
        rows = B * S
        pk = self._pack()
        cs = self._cos_sin_dev()
        xn = self._buf("xn", (rows, dim))
        qkv = self._buf("qkv", (rows, (H + 2 * Hkv) * hd))
        att = self._buf("att", (rows, H * hd))
        gu = self._buf("gu", (rows, 2 * self.ffn))
        act = self._buf("act", (rows, self.ffn))
        o = self._buf("lora_o", (rows, dim))
        Sk = start_pos + S
        scratch = None
        if S == 1 and h.dtype == torch.bfloat16:
            scratch = self._buf("attn_scratch", (2 * ops.attention_scratch_floats(B, H, hd, a.max_seq_len + 64),), torch.float32)
        ldq = qkv.stride(0)
        for i, lyr in enumerate(self.layers):
            kc, vc = k_caches[i], vt_caches[i]
            smax = kc.shape[2]
            if self._q8base is not None:       # fp8 base: likewise, Wd = bf16(Wq * sw)
                wqkv, wo, w13, w2 = self._q8_layer_weights(i)
            elif self._q4 is None:
                wqkv, wo, w13, w2 = pk[f"wqkv.{i}"], lyr.attention.wo.weight, pk[f"w13.{i}"], lyr.feed_forward.w2.weight
            else:                              # NF4 base: the layer's Wd in a reused scratch, then the bf16 kernels unchanged
                wqkv, wo, w13, w2 = self._q4_layer_weights(i)
            ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
            if rows > 16 and h.dtype == torch.bfloat16 and hd in (64, 128) and self._fuse_qkv_rope:
                # prefill: the adapter term is written into the qkv buffer and enters the fused qkv / RoPE / cache GEMM as an
                # additive term before the rotation (in place: a lane reads its delta before it stores the rotated q)
                im = self.lora_images()
                A, Bm = im[f"qkv.{i}.A"], im[f"qkv.{i}.B"]
                t = self._buf("lora_t", (rows, A.shape[0]))
                self._linear(xn, A, t)
                self._linear(t, Bm, qkv)
                ops.gemm_qkv_rope(xn, wqkv, qkv, kc, vc, cs, B, S, H, Hkv, hd, start_pos, rope_pos0, delta=qkv)
            else:
                self._linear(xn, wqkv, qkv)
                self._lora_add(f"qkv.{i}", xn, qkv)
                ops.rope_kvcache(qkv, qkv, kc, vc, cs, B, S, H, Hkv, hd, start_pos, rope_pos0)
            strides = (S * ldq, ldq, hd, Hkv * smax * hd, smax * hd, hd, Hkv * hd * smax, hd * smax, smax, S * H * hd, H * hd, hd)
            ops.attention(qkv, kc, vc, att, B, S, Sk, H, Hkv, hd, strides, causal and S > 1, scratch)
            # out = wo(att) + lora (rounded), then the residual add -- the reference's order (peft.py:95, llama_ens5.py:238)
            self._linear(att, wo, o)
            self._lora_add(f"wo.{i}", att, o)
            ops.add2d(h, o)
            ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
            self._linear(xn, w13, gu)                 # un-fused SwiGLU: the adapters add before the activation
            self._lora_add(f"w13.{i}", xn, gu)
            ops.swiglu_fwd(gu, act, self.ffn, interleaved=True)
            self._linear(act, w2, o)
            self._lora_add(f"w2.{i}", act, o)
            ops.add2d(h, o)
