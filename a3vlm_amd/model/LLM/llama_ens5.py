"""MI355X-native model plugin with the interface of the reference's
``accessory.model.LLM.llama_ens5`` (reference: model/accessory/model/LLM/llama_ens5.py).

Drop-in contract (what ``MetaModel`` reads): module-level ``ModelArgs``
and ``Transformer``; ``Transformer(args, with_visual)`` is an ``nn.Module`` exposing
``.args .image_words .image_size .layers``, ``forward(examples, image) -> logits[B,T,V]``,
``forward_inference(tokens, start_pos, image) -> fp32 [B,V]`` (stateful KV cache keyed on
``start_pos == 0``) and ``get_trainable_params()``; parameter names are the reference's
checkpoint keys (``tok_embeddings.weight``, ``layers.{i}.attention.wq.weight`` ...,
``clip.visual.*``, ``visual_proj.{0,1}.*``, ``start_img``, ``end_img``).

Nothing here computes with torch ops: every arithmetic step is a kernel of
``liba3vlm_hip.so`` (``a3vlm_amd.ops``).  torch owns memory, streams and the module tree.

Differences from the reference that are deliberate and documented in DESIGN.md:
  * only the CLIP ViT branch of the 4-encoder ensemble is native; the Q-Former / ConvNeXt /
    DINOv2 streams (OUT OF SCOPE frozen third-party nets) enter through ``extra_feats`` /
    ``qformer_feats`` hooks and default to absent (``ModelArgs.extra_feat_dim = 0``,
    ``qformer_tokens = 0``);
  * the KV cache is stored as K [B,Hkv,S,hd] and V^T [B,Hkv,hd,S] (kernel-friendly), not
    [B,S,Hkv,hd]; it is private to the plugin in the reference too (llama_ens5.py:171-179).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch
from torch import nn

from ... import lib as _lib
from ... import ops
from .weight_formats import FORMATS, LAYER_KEYS, DecodeWeights, WeightImage, head_path, layer_path


@dataclass
class ModelArgs:
    # --- identical to the reference (llama_ens5.py:33-50) ---
    dim: int = 5120
    n_layers: int = 40
    n_heads: int = 40
    n_kv_heads: Optional[int] = None
    vocab_size: int = -1
    multiple_of: int = 256
    ffn_dim_multiplier: Optional[float] = None
    norm_eps: float = 1e-5
    rope_theta: float = 10000
    max_batch_size: int = 32
    max_seq_len: int = 2048
    rope_scaling: Optional[float] = None
    load_pretrained_visual_encoder: bool = False
    # --- vision geometry (reference values are hard-coded at llama_ens5.py:297,335-336,383) ---
    vit_width: int = 1024
    vit_layers: int = 24
    vit_heads: int = 16
    vit_patch: int = 14
    vit_crop: int = 224          # side of one ViT input view
    n_views: int = 5             # 5 = global + 4 quadrants of a (2*crop)^2 image; 1 = single crop
    vit_quick_gelu: bool = False
    extra_feat_dim: int = 0      # reference: 3072 (ConvNeXt-XXL) + 1536 (DINOv2-g), via hooks
    qformer_tokens: int = 0      # reference: 32 (BLIP-2 Q-Former), via hook


def _ffn_hidden(dim: int, multiple_of: int, mult: Optional[float]) -> int:
    hidden = int(2 * (4 * dim) / 3)   # llama_ens5.py:196-200,229
    if mult is not None:
        hidden = int(mult * hidden)
    return multiple_of * ((hidden + multiple_of - 1) // multiple_of)


def precompute_cos_sin(head_dim: int, end: int, theta: float, scaling: Optional[float]) -> torch.Tensor:
    """fp32 [end, head_dim/2, 2] = (cos, sin) of the reference's complex table
    (``precompute_freqs_cis`` of the missing llama.py; call site llama_ens5.py:271-274).
    Built on the host with the same torch CPU ops the reference uses so the table is
    bit-identical to ``torch.polar``'s real/imag parts."""
    freqs = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device="cpu")[: head_dim // 2].float() / head_dim))
    t = torch.arange(end, dtype=torch.float32, device="cpu")
    if scaling is not None:
        t = t * scaling
    ang = torch.outer(t, freqs).float()
    fc = torch.polar(torch.ones_like(ang), ang)
    return torch.stack([fc.real, fc.imag], dim=-1).contiguous()


class _W(nn.Module):
    """Holder of a ``weight`` (and optional ``bias``) so state-dict keys match the reference."""

    def __init__(self, *shape, bias: bool = False, init: str = "linear"):
        super().__init__()
        w = torch.empty(*shape)
        if init == "linear":      # default_linear_init, llama_ens5.py:28
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        elif init == "ones":
            nn.init.ones_(w)
        else:
            nn.init.normal_(w, std=0.02)
        self.weight = nn.Parameter(w)
        if bias:
            self.bias = nn.Parameter(torch.zeros(shape[0]))


class Attention(nn.Module):
    def __init__(self, args: ModelArgs):
        super().__init__()
        n_kv = args.n_heads if args.n_kv_heads is None else args.n_kv_heads
        hd = args.dim // args.n_heads
        self.wq = _W(args.n_heads * hd, args.dim)
        self.wk = _W(n_kv * hd, args.dim)
        self.wv = _W(n_kv * hd, args.dim)
        self.wo = _W(args.dim, args.n_heads * hd)


class FeedForward(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.w1 = _W(hidden, dim)
        self.w2 = _W(dim, hidden)
        self.w3 = _W(hidden, dim)


class TransformerBlock(nn.Module):
    def __init__(self, layer_id: int, args: ModelArgs):
        super().__init__()
        self.layer_id = layer_id
        self.attention = Attention(args)
        self.feed_forward = FeedForward(args.dim, _ffn_hidden(args.dim, args.multiple_of, args.ffn_dim_multiplier))
        self.attention_norm = _W(args.dim, init="ones")
        self.ffn_norm = _W(args.dim, init="ones")


class _ResBlock(nn.Module):
    """Parameter tree of one open_clip ResidualAttentionBlock (key names: util/param_group.py:80-88)."""

    def __init__(self, w: int):
        super().__init__()
        self.ln_1 = _LN(w)
        self.attn = _MHA(w)
        self.ln_2 = _LN(w)
        self.mlp = nn.Module()
        self.mlp.c_fc = _W(4 * w, w, bias=True, init="normal")
        self.mlp.c_proj = _W(w, 4 * w, bias=True, init="normal")


class _LN(nn.Module):
    def __init__(self, w: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(w))
        self.bias = nn.Parameter(torch.zeros(w))


class _MHA(nn.Module):
    def __init__(self, w: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.randn(3 * w, w) * 0.02)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * w))
        self.out_proj = _W(w, w, bias=True, init="normal")


class _Visual(nn.Module):
    def __init__(self, args: ModelArgs):
        super().__init__()
        w, p = args.vit_width, args.vit_patch
        g = args.vit_crop // p
        self.conv1 = _W(w, 3, p, p, init="normal")
        self.class_embedding = nn.Parameter(torch.randn(w) * w ** -0.5)
        self.positional_embedding = nn.Parameter(torch.randn(g * g + 1, w) * w ** -0.5)
        self.ln_pre = _LN(w)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList([_ResBlock(w) for _ in range(args.vit_layers)])
        self.ln_post = _LN(w)


class _Clip(nn.Module):
    def __init__(self, args: ModelArgs):
        super().__init__()
        self.visual = _Visual(args)


class _Seq(nn.Module):
    """nn.Sequential(Linear, LayerNorm) parameter tree: keys ``0.weight 0.bias 1.weight 1.bias``."""

    def __init__(self, fin: int, fout: int):
        super().__init__()
        self.add_module("0", _W(fout, fin, bias=True))
        self.add_module("1", _LN(fout))


class Transformer(nn.Module):
    def __init__(self, args: ModelArgs, with_visual: bool = False):
        super().__init__()
        self.args = args
        self._fuse_qkv_rope = True      # prefill: RoPE + KV-cache write in the qkv GEMM epilogue (False: separate kernel; test hook)
        self.vocab_size = args.vocab_size
        self.n_layers = args.n_layers
        self.n_heads = args.n_heads
        self.n_kv_heads = args.n_heads if args.n_kv_heads is None else args.n_kv_heads
        self.head_dim = args.dim // args.n_heads
        self.ffn = _ffn_hidden(args.dim, args.multiple_of, args.ffn_dim_multiplier)
        self.tok_embeddings = _W(args.vocab_size, args.dim)
        self.layers = nn.ModuleList([TransformerBlock(i, args) for i in range(args.n_layers)])
        self.norm = _W(args.dim, init="ones")
        self.output = _W(args.vocab_size, args.dim)
        # llama_ens5.py:271-274
        self._cos_sin_cpu = precompute_cos_sin(self.head_dim, args.max_seq_len * 2, args.rope_theta, args.rope_scaling)
        self._cos_sin = None

        self.with_visual = with_visual
        self.image_words = 0
        self.cache_image_words = 0
        self.image_size = 224
        if with_visual:
            g = args.vit_crop // args.vit_patch
            self.clip = _Clip(args)
            self.visual_proj = _Seq(args.vit_width + args.extra_feat_dim, args.dim)
            if args.qformer_tokens:
                self.qformer_proj = _Seq(768, args.dim)
            self.image_words = (args.qformer_tokens + g * g + 1 + 2) * args.n_views
            self.image_size = args.vit_crop * (2 if args.n_views == 5 else 1)
            self.start_img = nn.Parameter(torch.rand(1, 1, args.dim))   # llama_ens5.py:338-339
            self.end_img = nn.Parameter(torch.rand(1, 1, args.dim))
        # hooks for the OUT-OF-SCOPE frozen encoders: callables views[N,3,c,c] -> features
        self.qformer_fn: Optional[Callable] = None          # -> [N, 32, 768]
        self.extra_feat_fns: List[Callable] = []            # each -> [N, L, C_i]

        self._packed: Dict[str, torch.Tensor] = {}
        self._packed_version = None
        self._weights: Optional[DecodeWeights] = None     # quantize_decode_weights: None = the bf16 parameters alone
        self._layer_tab_key = None
        self._k_cache: List[torch.Tensor] = []
        self._vt_cache: List[torch.Tensor] = []
        self._cache_shape = None
        self._kv_quant: Optional[str] = None        # quantize_kv_cache: None = bf16 caches, "fp8" = e4m3 caches + per-position scales
        self._kv8: Optional[Dict[str, object]] = None
        self._kv_rows = False                       # quantize_kv_cache("fp8", rows=True): the fp8 cache of the ragged decode path
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._row_maps: Dict[tuple, tuple] = {}

    # ------------------------------------------------------------------ plugin API
    def get_trainable_params(self, pretrain_stage: bool = False):
        """llama_ens5.py:342-349: everything except the frozen visual encoders."""
        no_train = ["qformer.", "openclip_convnext_xxl.", "clip.", "dinov2_vitg14."]
        return {n: p for n, p in self.named_parameters() if not any(n.startswith(x) for x in no_train)}

    def get_quant_blocklist(self) -> List[str]:
        pre = ["clip.", "openclip_convnext_xxl.", "dinov2_vitg14.", "qformer.", "visual_proj.", "qformer_proj."]
        return [n for n, _ in self.named_modules() if any(n.startswith(x) for x in pre)]

    # ------------------------------------------------------------------ helpers
    @property
    def _dtype(self) -> torch.dtype:
        return self.norm.weight.dtype

    @property
    def _device(self) -> torch.device:
        return self.norm.weight.device

    @property
    def weight_format(self) -> str:
        """How the decoder weights are held: "bf16", or "fp8" / "nf4" / "mxfp4" after quantize_decode_weights (weight_formats.FORMATS)."""
        return "bf16" if self._weights is None else self._weights.fmt

    def _buf(self, name: str, shape, dtype=None) -> torch.Tensor:
        """Workspace cache: one allocation per (name, shape, dtype); re-used across calls so the
        steady state allocates nothing (graph-capturable, no allocator traffic in the hot loop)."""
        dtype = dtype or self._dtype
        key = (name, tuple(shape), dtype)
        t = self._ws.get(key)
        if t is None:
            t = torch.empty(*shape, dtype=dtype, device=self._device)
            self._ws[key] = t
        return t

    def invalidate_packed_weights(self) -> None:
        """Call after parameters change (optimizer step / load_state_dict)."""
        self._packed_version = None

    def _weights_version(self):
        from ...util import param_state_key
        return tuple(param_state_key(p) for p in self.parameters()) + (self._dtype, str(self._device))

    def _pack(self, check: bool = False) -> Dict[str, torch.Tensor]:
        """Kernel-side weight images (built once per weight version):
        wqkv.{i} = [wq; wk; wv] rows (one fused QKV GEMM); w13.{i} = w1/w3 interleaved in
        16-row blocks (SwiGLU fused in the GEMM epilogue); conv1 as [width, Kpad] zero padded.
        ``check`` re-validates against the parameters' version counters (done once per
        forward / prefill, not per decode step)."""
        if self._packed_version is not None and not check:
            return self._packed
        ver = self._weights_version()
        if self._packed_version == ver:
            return self._packed
        dtp = self._dtype
        pk: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            for i, lyr in enumerate(self.layers):
                if FORMATS[self.weight_format].frees_weights:
                    break                  # NF4 / MXFP4 model: the decoder weights live only as images (self._weights.images)
                a, f = lyr.attention, lyr.feed_forward
                pk[f"wqkv.{i}"] = torch.cat([a.wq.weight, a.wk.weight, a.wv.weight], dim=0).to(dtp).contiguous()
                w1, w3 = f.w1.weight, f.w3.weight
                nb = w1.shape[0] // 16
                pk[f"w13.{i}"] = torch.stack([w1.view(nb, 16, -1), w3.view(nb, 16, -1)], dim=1).reshape(2 * w1.shape[0], -1).to(dtp).contiguous()
            if self.with_visual:
                pk.update(self._pack_vision())
        self._packed = pk
        self._packed_version = ver
        return pk

    def _pack_vision(self) -> Dict[str, torch.Tensor]:
        """conv1 as a [width, Kpad] GEMM weight (zero padded to the GEMM's K granule) in the ViT's own dtype;
        visual_proj.0 padded likewise in the model dtype."""
        pk: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            cw = self.clip.visual.conv1.weight
            vdt = cw.dtype
            K = cw[0].numel()
            Kpad = (K + 63) // 64 * 64
            w2d = torch.zeros(cw.shape[0], Kpad, dtype=vdt, device=cw.device)
            w2d[:, :K] = cw.reshape(cw.shape[0], -1)
            pk["conv1"] = w2d
            pw = getattr(self.visual_proj, "0").weight
            dtp = self._dtype
            Kp = pw.shape[1]
            Kp_pad = (Kp + 63) // 64 * 64
            if Kp_pad != Kp:
                w2 = torch.zeros(pw.shape[0], Kp_pad, dtype=dtp, device=pw.device)
                w2[:, :Kp] = pw.to(dtp)
                pk["visual_proj"] = w2
            else:
                pk["visual_proj"] = pw.to(dtp).contiguous()
        return pk

    def _vision_images(self) -> Dict[str, torch.Tensor]:
        """Vision-only weight images (used by the training engine, which keeps its own decoder images)."""
        key = (self.clip.visual.conv1.weight._version, self.clip.visual.conv1.weight.dtype, str(self._device))
        if getattr(self, "_vis_pack_key", None) != key:
            self._vis_pack = self._pack_vision()
            self._vis_pack_key = key
        return self._vis_pack

    def _cos_sin_dev(self) -> torch.Tensor:
        if self._cos_sin is None or self._cos_sin.device != self._device:
            self._cos_sin = self._cos_sin_cpu.to(self._device)
        return self._cos_sin

    # ------------------------------------------------------------------ KV cache
    def _allocate_kv_cache(self, bsz: int, rows: bool = False) -> None:
        """llama_ens5.py:171-176,533-535 (re-allocated only when the shape changes).  ``rows``: the cache of allocate_rows -- under
        quantize_kv_cache("fp8", rows=True) a kind of its own (below), else the same cache."""
        smax = (self.args.max_seq_len + 63) // 64 * 64
        kind = "fp8-rows" if rows and self._kv_quant == "fp8" and self._kv_rows else self._kv_quant
        shape = (bsz, self.n_kv_heads, smax, self.head_dim, self._dtype, str(self._device), kind)
        if self._cache_shape == shape:
            return
        dev, dtp = self._device, self._dtype
        if kind == "fp8-rows":
            # e4m3 caches and scales of bsz rows per layer; the shared bf16 K / V^T pair holds ONE row (prefill_row is a batch-1
            # forward); no staging pair (a3v_rope_kvquant_rows writes the new position straight into the fp8 cache)
            if dtp != torch.bfloat16:
                raise RuntimeError("the fp8 KV cache needs a bf16 model")
            Hkv, hd, L = self.n_kv_heads, self.head_dim, self.n_layers
            self._destroy_kv_cache()
            pair_k = torch.zeros(1, Hkv, smax, hd, dtype=dtp, device=dev)
            pair_vt = torch.zeros(1, Hkv, hd, smax, dtype=dtp, device=dev)
            self._kv8 = dict(
                k_q=[torch.zeros(bsz, Hkv, smax, hd, dtype=torch.uint8, device=dev) for _ in range(L)],
                vt_q=[torch.zeros(bsz, Hkv, hd, smax, dtype=torch.uint8, device=dev) for _ in range(L)],
                k_scale=[torch.zeros(bsz, Hkv, smax, dtype=torch.float32, device=dev) for _ in range(L)],
                v_scale=[torch.zeros(bsz, Hkv, smax, dtype=torch.float32, device=dev) for _ in range(L)])
            self._k_cache, self._vt_cache = [pair_k] * L, [pair_vt] * L
            self._cache_shape = shape
            return
        if self._kv_quant == "fp8":
            # e4m3 caches and per-(batch, kv-head, position) scales per layer; ONE bf16 K / V^T pair at full Smax shared by all layers
            # (the multi-token forward runs unchanged on it, layer after layer) and one single-position staging pair for decode
            if dtp != torch.bfloat16:
                raise RuntimeError("the fp8 KV cache needs a bf16 model")
            Hkv, hd, L = self.n_kv_heads, self.head_dim, self.n_layers
            self._destroy_kv_cache()
            pair_k = torch.zeros(bsz, Hkv, smax, hd, dtype=dtp, device=dev)
            pair_vt = torch.zeros(bsz, Hkv, hd, smax, dtype=dtp, device=dev)
            self._kv8 = dict(
                k_q=[torch.zeros(bsz, Hkv, smax, hd, dtype=torch.uint8, device=dev) for _ in range(L)],
                vt_q=[torch.zeros(bsz, Hkv, hd, smax, dtype=torch.uint8, device=dev) for _ in range(L)],
                k_scale=[torch.zeros(bsz, Hkv, smax, dtype=torch.float32, device=dev) for _ in range(L)],
                v_scale=[torch.zeros(bsz, Hkv, smax, dtype=torch.float32, device=dev) for _ in range(L)],
                stage_k=torch.zeros(bsz, Hkv, 1, hd, dtype=dtp, device=dev),
                stage_vt=torch.zeros(bsz, Hkv, hd, 1, dtype=dtp, device=dev))
            self._k_cache, self._vt_cache = [pair_k] * L, [pair_vt] * L
            self._cache_shape = shape
            return
        self._kv8 = None
        self._k_cache = [torch.zeros(bsz, self.n_kv_heads, smax, self.head_dim, dtype=dtp, device=dev)
                         for _ in range(self.n_layers)]
        self._vt_cache = [torch.zeros(bsz, self.n_kv_heads, self.head_dim, smax, dtype=dtp, device=dev)
                          for _ in range(self.n_layers)]
        self._cache_shape = shape

    def _destroy_kv_cache(self) -> None:
        self._k_cache, self._vt_cache, self._cache_shape, self._kv8 = [], [], None, None
        self._layer_tab_key = None         # the step's pointer tables follow the allocation: a later cache of the same shape is another one

    def quantize_kv_cache(self, mode: Optional[str] = "fp8", rows: bool = False) -> None:
        """Opt-in fp8 (OCP e4m3fn) KV cache for ``forward_inference`` (format: include/a3vlm_hip.h, "fp8 KV cache"): half the cache
        bytes a decode step reads and half the cache allocation.  ``None`` restores the bf16 cache.  Any allocated cache is dropped
        (the next prefill allocates the new kind).  Independent of ``quantize_decode_weights`` -- either order.

        Prefill is bit-identical to the bf16-cache model: every layer runs the unchanged bf16 kernels on one shared bf16 K / V^T pair
        and a3v_kv_quantize_fp8 then moves the layer's new positions into its fp8 cache.  Decode (one token) quantises the new
        position and runs a3v_attention_decode_fp8kv -- inside a3v_llama_decode_step_kv8 where the fused step form exists.  A
        multi-token continuation dequantises each layer's prefix into the shared pair first.  bf16 models, head_dim 64 or 128.

        ``rows=True`` (with ``"fp8"`` only) also opens the ragged decode path -- ``allocate_rows``, ``prefill_row``,
        ``forward_inference_rows`` (with or without shared prompt keys), ``share_prefix``, ``generate_many`` -- which ``"fp8"`` alone
        refuses.  ``allocate_rows(R)`` then makes a cache of its own kind: fp8 caches and scales for R rows, the shared bf16 pair
        for ONE row (``prefill_row`` is a batch-1 forward; its logits are the bf16-cache model's bit for bit) and no staging pair
        (a3v_rope_kvquant_rows writes the new position, a3v_attention_decode_rows_fp8kv reads the cache -- inside
        a3v_llama_decode_step_rows_kv8 where the fused form exists).  ``forward_inference`` / ``generate`` on the same object
        allocate and behave as under ``"fp8"`` alone.  Lookup decoding and beam search have no fp8 form and are refused."""
        if mode not in (None, "fp8"):
            raise ValueError(f"unknown KV-cache format {mode!r}: only 'fp8' (OCP e4m3fn, per-position scales) or None (bf16) exist")
        if rows and mode != "fp8":
            raise ValueError(f"quantize_kv_cache(rows=True) is the ragged form of the fp8 cache: it needs mode 'fp8', not {mode!r}")
        if mode == "fp8" and self.head_dim not in (64, 128):
            raise ValueError(f"the fp8 KV cache needs head_dim 64 or 128, this model has {self.head_dim}")
        self._kv_quant = mode
        self._kv_rows = bool(rows)
        self._destroy_kv_cache()
        self._layer_tab_key = None

    # ------------------------------------------------------------------ linear dispatch
    def _skinny_ws(self, M: int, N: int, K: int, ws_bytes=ops.gemm_skinny_ws_bytes) -> torch.Tensor:
        """The one zero-initialised GEMV workspace, grown on demand to ``ws_bytes(M, N, K)`` (every GEMV family has the same layout;
        the kernels leave its counters zero)."""
        need = ws_bytes(M, N, K)
        ws = self._ws.get("skinny_ws")
        if ws is None or ws.numel() * 4 < need:
            ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device=self._device)
            self._ws["skinny_ws"] = ws
        return ws

    def _mx4_gemm(self, x, img, out, norm_w=None, **kw):
        """W4A8 product on an MXFP4 image for any row count (quantize_decode_weights("mxfp4", prefill=True)): the rows of x -- of its
        bf16 RMSNorm when ``norm_w`` is given, which is then never written -- quantised once to MXFP8, then a3v_gemm_nt_mxfp4."""
        rows, K = x.shape
        xq = self._buf("mx8_q", (rows, max(self.args.dim, self.n_heads * self.head_dim, self.ffn)), torch.uint8)[:, :K]
        xe = self._buf(f"mx8_e{K}", (rows, K // 32), torch.uint8)
        ops.quantize_rows_mxfp8(x, xq, xe, norm_w, self.args.norm_eps if norm_w is not None else 0.0)
        return ops.gemm_nt_mxfp4(xq, xe, img.q, img.s, out, residual=kw.get("residual"), epilogue=kw.get("epilogue", 0))

    def _linear(self, x, w, out, **kw):
        if isinstance(w, WeightImage):     # an image of this model's 4-bit format: its GEMV, gemv_rows rows per call
            f = FORMATS[self._weights.fmt]
            rows, res = x.shape[0], kw.get("residual")
            if rows > f.gemv_max_rows:
                raise RuntimeError(f"an {f.name} image takes at most {f.gemv_max_rows} rows: larger products run on the dequantised layer")
            for r0 in range(0, rows, f.gemv_rows):
                r1 = r0 + f.gemv_rows
                f.gemv(x[r0:r1], w.q, w.s, out[r0:r1], self._skinny_ws(min(f.gemv_rows, rows - r0), w.q.shape[0], x.shape[1], f.gemv_ws_bytes),
                       residual=None if res is None else res[r0:r1], epilogue=kw.get("epilogue", 0))
            return out
        if x.shape[0] <= 16 and x.dtype == torch.bfloat16 and "bias" not in kw and w.shape[1] % 32 == 0:
            ep = kw.get("epilogue", 0)
            return ops.gemm_skinny(x, w, out, self._skinny_ws(x.shape[0], w.shape[0], w.shape[1]), residual=kw.get("residual"), epilogue=ep)
        return ops.gemm_nt(x, w, out, **kw)

    # ------------------------------------------------------------------ decoder stack
    def _row_buffers(self, rows: int, scratch: bool):
        """xn, qkv, att, act of a pass over ``rows`` rows and, if ``scratch``, the split-KV scratch of a decode attention of as many
        rows (else None)."""
        a = self.args
        H, Hkv, hd = self.n_heads, self.n_kv_heads, self.head_dim
        xn = self._buf("xn", (rows, a.dim))
        qkv = self._buf("qkv", (rows, (H + 2 * Hkv) * hd))
        att = self._buf("att", (rows, H * hd))
        act = self._buf("act", (rows, self.ffn))
        sc = self._buf("attn_scratch", (2 * ops.attention_scratch_floats(rows, H, hd, a.max_seq_len + 64),), torch.float32) if scratch else None
        return xn, qkv, att, act, sc

    def _layer_path(self, h: torch.Tensor, rows: int, decode: bool, ragged: bool = False) -> str:
        """weight_formats.layer_path of this model for a pass over ``rows`` rows of the stream h."""
        w = self._weights
        return layer_path(self.weight_format, w is not None and w.prefill, rows, decode, self.args.dim, self.head_dim,
                          h.dtype == torch.bfloat16, ragged)

    def _layer_operands(self, i: int, path: str):
        """(wqkv, wo, w13, w2) of layer i for ``path``: the bf16 weights, the layer's Wd in the scratch, or the images."""
        if path == "bf16":
            pk, lyr = self._pack(), self.layers[i]
            return pk[f"wqkv.{i}"], lyr.attention.wo.weight, pk[f"w13.{i}"], lyr.feed_forward.w2.weight
        if path == "dequant":              # the layer's Wd in a reused bf16 scratch, then the bf16 GEMMs unchanged (weight-only)
            return self._dequant_layer(i)
        return [self._weights.images[f"{k}.{i}"] for k in LAYER_KEYS]

    def _layer(self, i: int, path: str, h, bufs, rope, attend, qkv_rope=None) -> None:
        """Decoder block i on h in place.  The callers' own steps: ``rope()`` rotates q and k in the qkv buffer and writes the cache,
        ``attend()`` fills att, and ``qkv_rope(wqkv)``, if given, stands for the qkv product and rope() together."""
        a, lyr = self.args, self.layers[i]
        xn, qkv, att, act = bufs
        wqkv, wo, w13, w2 = self._layer_operands(i, path)
        if path == "w4a8":
            # W4A8 (opt-in): every product on the image -- rows quantised to MXFP8 once per product (the two RMSNorm outputs never
            # exist in bf16), both block scales in the scaled MFMA; qkv stored plainly, then the rope kernel as the GEMV path
            self._mx4_gemm(h, wqkv, qkv, lyr.attention_norm.weight)
            rope()
            attend()
            self._mx4_gemm(att, wo, h, residual=h)
            self._mx4_gemm(h, w13, act, lyr.ffn_norm.weight, epilogue=ops.EPI_SWIGLU)
            self._mx4_gemm(act, w2, h, residual=h)
            return
        ops.rmsnorm(h, lyr.attention_norm.weight, xn, a.norm_eps)
        if qkv_rope is not None:
            qkv_rope(wqkv)
        else:
            self._linear(xn, wqkv, qkv)
            rope()
        attend()
        self._linear(att, wo, h, residual=h)
        ops.rmsnorm(h, lyr.ffn_norm.weight, xn, a.norm_eps)
        self._linear(xn, w13, act, epilogue=ops.EPI_SWIGLU)
        self._linear(act, w2, h, residual=h)

    def _decoder_layers(self, h: torch.Tensor, B: int, S: int, start_pos: int, rope_pos0: int,
                        k_caches, vt_caches, causal: bool, kv8=None) -> None:
        """h [B*S, dim] updated in place through all blocks (llama_ens5.py:237-249).  ``kv8``: the fp8 arrays that take the new
        positions when they are not the model's whole cache (prefill_row: its views of one cache row)."""
        a = self.args
        H, Hkv, hd, dim = self.n_heads, self.n_kv_heads, self.head_dim, a.dim
        rows = B * S
        self._pack()
        cs = self._cos_sin_dev()
        xn, qkv, att, act, scratch = self._row_buffers(rows, S == 1 and h.dtype == torch.bfloat16)
        Sk = start_pos + S
        ldq = qkv.stride(0)
        path = self._layer_path(h, rows, S == 1)
        # rotary embedding + cache write in the qkv GEMM epilogue (qkv never makes a second trip through HBM): not on the GEMV images
        fuse = path != "gemv" and rows > 16 and h.dtype == torch.bfloat16 and hd in (64, 128) and self._fuse_qkv_rope
        # fp8 KV cache (quantize_kv_cache): k_caches / vt_caches then hold the ONE shared bf16 pair.  S > 1: the layer runs unchanged on
        # the pair (a continuation dequantises the layer's prefix into it first) and its new positions are quantised afterwards;
        # S == 1: the new position goes through the staging pair into the fp8 cache and the attention reads the fp8 cache.
        if kv8 is None and k_caches is self._k_cache:
            kv8 = self._kv8
        stage = kv8 is not None and S == 1 and "stage_k" in kv8      # (a rows cache has no staging pair: S == 1 runs as S > 1)
        cpos = 0 if stage else start_pos             # where the qkv epilogue / rope kernel writes in the cache it is handed

        def attend(i, kc, vc, strides):
            if kv8 is None:
                return ops.attention(qkv, kc, vc, att, B, S, Sk, H, Hkv, hd, strides, causal and S > 1, scratch)
            fp8c = (kv8["k_q"][i], kv8["vt_q"][i], kv8["k_scale"][i], kv8["v_scale"][i])
            if stage:
                ops.kv_quantize_fp8(kc, vc, 0, *fp8c, 1, start_pos)
                return ops.attention_decode_fp8kv(qkv, *fp8c, att, B, Sk, H, Hkv, hd, scratch)
            ops.attention(qkv, kc, vc, att, B, S, Sk, H, Hkv, hd, strides, causal and S > 1, scratch)
            ops.kv_quantize_fp8(kc, vc, start_pos, *fp8c, S, start_pos)
        if path == "w8a8":
            if self._weights.version != self._packed_version:
                raise RuntimeError("parameters changed after quantize_decode_weights(): call it again (or with mode=None)")
            xq = self._buf("fp8_x", (rows, max(dim, H * hd)), torch.uint8)
            aq = self._buf("fp8_act", (rows, self.ffn), torch.uint8)
            sx = self._buf("fp8_sx", (rows,), torch.float32)
        for i, lyr in enumerate(self.layers):
            kc, vc = k_caches[i], vt_caches[i]
            if stage:
                kc, vc = kv8["stage_k"], kv8["stage_vt"]
            elif kv8 is not None and start_pos > 0:
                ops.kv_dequantize_fp8(kv8["k_q"][i], kv8["vt_q"][i], kv8["k_scale"][i], kv8["v_scale"][i], kc, vc, start_pos)
            smax = kc.shape[2]
            strides = (S * ldq, ldq, hd,                       # q: view into the qkv buffer
                       Hkv * smax * hd, smax * hd, hd,         # k cache
                       Hkv * hd * smax, hd * smax, smax,       # v^T cache
                       S * H * hd, H * hd, hd)                 # out
            if path == "w8a8":
                # W8A8 prefill (opt-in, BASELINE config 5): every decoder GEMM on fp8 operands -- activations quantised per
                # token on the fly (the RMSNorm output never exists in bf16), weights per output row, MX-scaled MFMA
                (wqkv_q, wqkv_s), (wo_q, wo_s), (w13_q, w13_s), (w2_q, w2_s) = self._layer_operands(i, path)
                ops.quantize_rows_fp8(h, xq[:, :dim], sx, lyr.attention_norm.weight, a.norm_eps)
                ops.gemm_qkv_rope_fp8(xq[:, :dim], sx, wqkv_q, wqkv_s, qkv, kc, vc, cs, B, S, H, Hkv, hd, cpos, rope_pos0)
                attend(i, kc, vc, strides)
                ops.quantize_rows_fp8(att, xq[:, :H * hd], sx)
                ops.gemm_nt_fp8(xq[:, :H * hd], sx, wo_q, wo_s, h, residual=h)
                ops.quantize_rows_fp8(h, xq[:, :dim], sx, lyr.ffn_norm.weight, a.norm_eps)
                ops.gemm_nt_fp8(xq[:, :dim], sx, w13_q, w13_s, act, epilogue=ops.EPI_SWIGLU)
                ops.quantize_rows_fp8(act, aq, sx)
                ops.gemm_nt_fp8(aq, sx, w2_q, w2_s, h, residual=h)
                continue
            self._layer(i, path, h, (xn, qkv, att, act),
                        lambda: ops.rope_kvcache(qkv, qkv, kc, vc, cs, B, S, H, Hkv, hd, cpos, rope_pos0),
                        lambda: attend(i, kc, vc, strides),
                        (lambda wqkv: ops.gemm_qkv_rope(xn, wqkv, qkv, kc, vc, cs, B, S, H, Hkv, hd, cpos, rope_pos0)) if fuse else None)

    def quantize_decode_weights(self, mode: str = "fp8", prefill: bool = False) -> None:
        """Opt-in weight images for inference: ``"fp8"`` (per-row e4m3 images beside the bf16 weights; ``mode=None`` drops them; re-run
        after the weights change), ``"nf4"`` (the reference's bitsandbytes Linear4bit mode, util/quant.py:95-163) or ``"mxfp4"`` (OCP
        MXFP4).  The 4-bit formats also take the LM head and FREE every bf16 weight they quantise (as the reference's ``del
        module.weight``): irreversible, and gone from ``state_dict()``.  What a format needs, frees and runs on is its row of
        weight_formats.FORMATS; the path a product of a given shape takes is weight_formats.layer_path / head_path.  Quantise after
        ``.to(device)``: the images are not module buffers and do not move with the model.

        ``prefill=True``, fp8: the multi-token forward W8A8 (a3v_gemm_nt_fp8) instead of on the bf16 weights.  MXFP4 (DESIGN.md 7e
        "W4A8 GEMM"): every product that is not a GEMV of at most 32 decode rows W4A8 on the images, instead of dequantising every
        layer for it (~400 MB written per layer at 7B, for every token of a decode batch above 32 rows); logits are then no longer
        those of the bf16 model on Wd.  Measured at 7B: the 64-row decode step 1.4x faster, products of 128 rows and more slower (a
        1100-token prefill 3.8x): hence opt-in."""
        held = FORMATS[self.weight_format]
        if held.frees_weights:
            raise RuntimeError(f"this model holds {held.name} weights: quantize_decode_weights('{self.weight_format}') freed its bf16 decoder "
                               "weights and cannot be undone or combined with another mode; reload the checkpoint instead")
        if mode in ("nf4", "mxfp4"):
            self._quantize_4bit(mode, bool(prefill) and mode == "mxfp4")     # (NF4 has no prefill form)
            return
        self._weights, self._layer_tab_key = None, None
        if mode is None:
            return
        if mode != "fp8":
            raise ValueError("only weight-only 'fp8' (OCP e4m3fn) is implemented")
        f = FORMATS["fp8"]
        f.check(self)
        self._pack(check=True)
        images: Dict[str, WeightImage] = {}
        with torch.no_grad():
            for i in range(self.n_layers):
                for key, w in zip(LAYER_KEYS, self._layer_operands(i, "bf16")):
                    images[f"{key}.{i}"] = WeightImage(*f.quantize(w, None))
        self._weights = DecodeWeights("fp8", bool(prefill), images, self._packed_version)

    def _quantize_4bit(self, fmt: str, prefill: bool) -> None:
        """Every decoder linear and the LM head as ``fmt`` images, one original module at a time, its bf16 weight dropped at once."""
        a, f = self.args, FORMATS[fmt]
        f.check(self)
        self._weights, self._layer_tab_key = None, None
        ws = None if f.quantize_ws_bytes is None else torch.empty(
            (f.quantize_ws_bytes(max(a.vocab_size, self.ffn * 2), max(a.dim, self.ffn)) + 3) // 4, dtype=torch.float32, device=self._device)

        def quant(mod):
            img = WeightImage(*f.quantize(mod.weight.data.contiguous(), ws))
            del mod.weight
            return img

        def rows16(x, y):                  # w1 / w3 interleaved in 16-row blocks (the SwiGLU GEMV row order, as _pack)
            nb = x.shape[0] // 16
            return torch.stack([x.view(nb, 16, -1), y.view(nb, 16, -1)], dim=1).reshape(2 * x.shape[0], -1).contiguous()
        images: Dict[str, WeightImage] = {}
        with torch.no_grad():
            for i, lyr in enumerate(self.layers):
                at, ff = lyr.attention, lyr.feed_forward
                wq, wk, wv = quant(at.wq), quant(at.wk), quant(at.wv)
                images[f"wqkv.{i}"] = WeightImage(torch.cat([wq.q, wk.q, wv.q]), torch.cat([wq.s, wk.s, wv.s]))
                images[f"wo.{i}"] = quant(at.wo)
                w1, w3 = quant(ff.w1), quant(ff.w3)
                images[f"w13.{i}"] = WeightImage(rows16(w1.q, w3.q), rows16(w1.s, w3.s))
                images[f"w2.{i}"] = quant(ff.w2)
                del wq, wk, wv, w1, w3
                self._packed.pop(f"wqkv.{i}", None)
                self._packed.pop(f"w13.{i}", None)
            images["output"] = quant(self.output)
        self._weights = DecodeWeights(fmt, prefill, images)
        self._packed_version = None
        self._ws.pop("nf4_scratch", None)

    def _dequant_scratch(self, n: int) -> torch.Tensor:
        """The one bf16 scratch a 4-bit model dequantises into: a whole layer or the LM head, whichever is larger."""
        buf = self._ws.get("nf4_scratch")
        if buf is None or buf.numel() < n:
            self._ws.pop("nf4_scratch", None)
            a = self.args
            need = max(((self.n_heads + 2 * self.n_kv_heads) * self.head_dim + 2 * self.ffn) * a.dim + a.dim * (self.n_heads * self.head_dim + self.ffn),
                       a.vocab_size * a.dim, n)
            buf = torch.empty(need, dtype=torch.bfloat16, device=self._device)
            self._ws["nf4_scratch"] = buf
        return buf

    def _dequant_layer(self, i: int):
        """Wd of layer i's four (packed) matrices in the reused scratch: views (wqkv, wo, w13, w2)."""
        a, w = self.args, self._weights
        shapes = (((self.n_heads + 2 * self.n_kv_heads) * self.head_dim, a.dim), (a.dim, self.n_heads * self.head_dim),
                  (2 * self.ffn, a.dim), (a.dim, self.ffn))
        buf = self._dequant_scratch(sum(n * k for n, k in shapes))
        out, o = [], 0
        for key, (n, k) in zip(LAYER_KEYS, shapes):
            wd = buf[o:o + n * k].view(n, k)
            FORMATS[w.fmt].dequantize(*w.images[f"{key}.{i}"], wd)
            out.append(wd)
            o += n * k
        return out

    def _head_weight(self) -> torch.Tensor:
        """The LM head as a bf16 GEMM operand (a 4-bit model: dequantised into the reused scratch)."""
        w, a = self._weights, self.args
        if not FORMATS[self.weight_format].frees_weights:
            return self.output.weight
        wd = self._dequant_scratch(a.vocab_size * a.dim)[:a.vocab_size * a.dim].view(a.vocab_size, a.dim)
        return FORMATS[w.fmt].dequantize(*w.images["output"], wd)

    def _lm_head_last(self, xn: torch.Tensor, logits: torch.Tensor, decode: bool) -> None:
        """fp32 logits of the last rows of a forward, on weight_formats.head_path (``decode``: a decode step of at most 32 rows)."""
        w = self._weights
        path = head_path(self.weight_format, w is not None and w.prefill, decode, self._dtype == torch.float32)
        if path == "gemm_nt":
            ops.gemm_nt(xn, self.output.weight, logits)
        elif path == "w4a8":               # the head on its image too, no dequantisation scratch
            self._mx4_gemm(xn, w.images["output"], logits, epilogue=ops.EPI_OUT_F32)
        elif path == "dequant":
            self._linear(xn, self._head_weight(), logits, epilogue=ops.EPI_OUT_F32)
        else:
            self._lm_head_f32(xn, logits)

    def _lm_head_f32(self, xn: torch.Tensor, logits: torch.Tensor) -> None:
        """fp32 logits of bf16 rows xn: the NF4 / MXFP4 GEMV in chunks of 16 rows on such a model, the bf16 path otherwise."""
        f = FORMATS[self.weight_format]
        if not f.frees_weights:
            self._linear(xn, self.output.weight, logits, epilogue=ops.EPI_OUT_F32)
            return
        for r0 in range(0, xn.shape[0], f.gemv_rows):
            self._linear(xn[r0:r0 + f.gemv_rows], self._weights.images["output"], logits[r0:r0 + f.gemv_rows], epilogue=ops.EPI_OUT_F32)


    def _step_format_code(self) -> Optional[int]:
        """The weight-format argument of the C step entries (a3v_llama_decode_step_form); None: this format has no C step."""
        return FORMATS[self.weight_format].step_code

    def _llama_layer_table(self):
        """The a3v_llama_layer table of the C step entries (and the a3v_kv8_layer table of an fp8 KV cache), rebuilt when weights,
        caches or weight images change."""
        self._pack()
        w, fmt = self._weights, FORMATS[self.weight_format]
        if w is not None and w.version is not None and w.version != self._packed_version:
            raise RuntimeError("parameters changed after quantize_decode_weights(): call it again (or with mode=None)")
        kv8 = self._kv8
        key = (self._packed_version, self._cache_shape, self.weight_format)
        if self._layer_tab_key != key:
            tab = (_lib.LlamaLayer * self.n_layers)()
            self._kv8_tab = None
            if kv8 is not None:            # fp8 KV cache: the k_cache / vt_cache fields below (the shared bf16 pair) are not read by the step
                self._kv8_tab = (_lib.Kv8Layer * self.n_layers)()
                for i in range(self.n_layers):
                    for f in ("k_q", "vt_q", "k_scale", "v_scale"):
                        setattr(self._kv8_tab[i], f, kv8[f][i].data_ptr())
            for i, lyr in enumerate(self.layers):
                if fmt.step_fields is not None:        # the images: <key>_q / <key>_s (fp8) or <key>_n4 / <key>_n4s
                    for k in LAYER_KEYS:
                        img = w.images[f"{k}.{i}"]
                        setattr(tab[i], k + fmt.step_fields[0], img.q.data_ptr())
                        setattr(tab[i], k + fmt.step_fields[1], img.s.data_ptr())
                if not fmt.frees_weights:              # (NF4 images only: the bf16 fields stay NULL)
                    tab[i].wqkv, tab[i].wo, tab[i].w13, tab[i].w2 = (t.data_ptr() for t in self._layer_operands(i, "bf16"))
                tab[i].attn_norm_w = lyr.attention_norm.weight.data_ptr()
                tab[i].ffn_norm_w = lyr.ffn_norm.weight.data_ptr()
                tab[i].k_cache = self._k_cache[i].data_ptr()
                tab[i].vt_cache = self._vt_cache[i].data_ptr()
            self._layer_tab, self._layer_tab_key = tab, key
        return self._layer_tab

    def _decode_step_buffers(self, B: int):
        """xn, qkv, att, act, attention scratch and GEMV workspace of a C step call at B rows."""
        a = self.args
        H, Hkv, hd = self.n_heads, self.n_kv_heads, self.head_dim
        xn, qkv, att, act, scratch = self._row_buffers(B, True)
        Bc = B if B <= 16 else (B + 1) // 2          # 17..32 rows run as two row chunks inside the C call
        sws = self._skinny_ws(Bc, max((H + 2 * Hkv) * hd, 2 * self.ffn, a.dim), max(a.dim, self.ffn))
        for (n_, k_) in (((H + 2 * Hkv) * hd, a.dim), (a.dim, H * hd), (2 * self.ffn, a.dim), (a.dim, self.ffn)):
            sws = self._skinny_ws(Bc, n_, k_)
        return xn, qkv, att, act, scratch, sws


    def _call_step(self, entry: str, h: torch.Tensor, bufs, rows, after=(), tables=()) -> None:
        """One C step entry: (layer table, *tables, n_layers, h, xn, qkv, att, act, scratch, sws, cos_sin, *rows, dim, H, Hkv, hd, ffn,
        Smax, *after, eps, stream) -- ``rows`` are the entry's position / row-count arguments, ``bufs`` its _decode_step_buffers()."""
        a = self.args
        tab = self._llama_layer_table()
        rc = getattr(_lib.load(), entry)(tab, *tables, self.n_layers, h.data_ptr(), *(t.data_ptr() for t in bufs),
                                         self._cos_sin_dev().data_ptr(), *rows, a.dim, self.n_heads, self.n_kv_heads, self.head_dim,
                                         self.ffn, self._k_cache[0].shape[2], *after, a.norm_eps, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, entry)

    def _decode_step(self, h: torch.Tensor, B: int, pos: int) -> None:
        """seqlen == 1, bf16: the whole layer stack from one C call (a3v_llama_decode_step; with an fp8 KV cache a3v_llama_decode_step_kv8)."""
        self._llama_layer_table()      # (builds the kv8 table too)
        bufs, kv8 = self._decode_step_buffers(B), self._kv8
        if kv8 is not None:
            self._call_step("a3v_llama_decode_step_kv8", h, bufs, (kv8["stage_k"].data_ptr(), kv8["stage_vt"].data_ptr(), B), (pos,),
                            tables=(self._kv8_tab,))
        else:
            self._call_step("a3v_llama_decode_step", h, bufs, (B,), (pos,))

    # ------------------------------------------------------------------ vision
    def _vit_geometry(self):
        a = self.args
        g = a.vit_crop // a.vit_patch
        return g, g * g, g * g + 1     # grid, patch tokens, tokens incl. cls

    def clip_encode_image(self, views: torch.Tensor) -> torch.Tensor:
        """llama_ens5.py:351-375 on [N,3,c,c] views -> [N*L, width] (row = n*L + token)."""
        a = self.args
        pk = self._vision_images()
        vis = self.clip.visual
        vdt = vis.conv1.weight.dtype
        _mbuf = self._buf

        def _vbuf(name, shape):
            return _mbuf(name, shape, vdt)
        N = views.shape[0]
        g, T, L = self._vit_geometry()
        W, Hh = a.vit_width, a.vit_heads
        hd = W // Hh
        Kpad = pk["conv1"].shape[1]
        cols = _vbuf("vit_cols", (N * T, Kpad))
        ops.patch_im2col(views.contiguous(), cols, a.vit_patch)
        patch = _vbuf("vit_patch", (N * T, W))
        ops.gemm_nt(cols, pk["conv1"], patch)
        x = _vbuf("vit_x", (N * L, W))
        ops.vit_embed(patch, vis.class_embedding, vis.positional_embedding, x, N, T, W)
        ops.layernorm(x, vis.ln_pre.weight, vis.ln_pre.bias, x)
        y = _vbuf("vit_y", (N * L, W))
        qkv = _vbuf("vit_qkv", (N * L, 3 * W))
        Lpad = (L + 63) // 64 * 64
        vt = _vbuf("vit_vt", (N, Hh, hd, Lpad))
        att = _vbuf("vit_att", (N * L, W))
        mlp = _vbuf("vit_mlp", (N * L, 4 * W))
        act = ops.EPI_QUICKGELU if a.vit_quick_gelu else ops.EPI_GELU
        ld = 3 * W
        strides = (L * ld, ld, hd, L * ld, hd, ld, Hh * hd * Lpad, hd * Lpad, Lpad, L * W, W, hd)
        for blk in vis.transformer.resblocks:
            ops.layernorm(x, blk.ln_1.weight, blk.ln_1.bias, y)
            ops.gemm_nt(y, blk.attn.in_proj_weight, qkv, bias=blk.attn.in_proj_bias)
            ops.vt_pack(qkv[:, 2 * W:], ld, vt, N, L, Hh, hd, Lpad)
            ops.attention(qkv, qkv[:, W:], vt, att, N, L, L, Hh, Hh, hd, strides, False, None)
            ops.gemm_nt(att, blk.attn.out_proj.weight, x, bias=blk.attn.out_proj.bias, residual=x)
            ops.layernorm(x, blk.ln_2.weight, blk.ln_2.bias, y)
            ops.gemm_nt(y, blk.mlp.c_fc.weight, mlp, bias=blk.mlp.c_fc.bias, epilogue=act)
            ops.gemm_nt(mlp, blk.mlp.c_proj.weight, x, bias=blk.mlp.c_proj.bias, residual=x)
        feats = _vbuf("vit_feats", (N * L, W))
        ops.layernorm(x, vis.ln_post.weight, vis.ln_post.bias, feats)
        return feats

    def _image_slots(self):
        """(start tag, end tag) parameters per image slot; slot 0 = RGB (llama_ens5.py:338-339)."""
        return [(self.start_img, self.end_img)]

    @property
    def words_per_image(self) -> int:
        _, _, L = self._vit_geometry()
        return (self.args.qformer_tokens + L + 2) * self.args.n_views

    def _image_row_maps(self, B: int, S: int, slots=(0,)):
        """int32 device maps from projector rows to rows of the [B*S, dim] sequence buffer
        for the layout of llama_ens5.py:471-479: h = [BOS | per image: per view (start, [qformer], clip, end) | text].
        Image j of the call occupies words [j*Wv, (j+1)*Wv); projector rows are ordered (image, view, batch)."""
        key = (B, S, tuple(slots), str(self._device))
        m = self._row_maps.get(key)
        if m is not None:
            return m
        a = self.args
        _, _, L = self._vit_geometry()
        Q, V, J = a.qformer_tokens, a.n_views, len(slots)
        per_view = Q + L + 2
        clip_map = torch.empty(J * V * B * L, dtype=torch.int32)
        qf_map = torch.empty(J * V * B * max(Q, 1), dtype=torch.int32)
        start_rows, end_rows = [[] for _ in slots], [[] for _ in slots]
        for j in range(J):
            for v in range(V):
                for b in range(B):
                    base = b * S + 1 + (j * V + v) * per_view
                    start_rows[j].append(base)
                    end_rows[j].append(base + 1 + Q + L)
                    n = (j * V + v) * B + b
                    clip_map[n * L:(n + 1) * L] = torch.arange(base + 1 + Q, base + 1 + Q + L, dtype=torch.int32)
                    if Q:
                        qf_map[n * Q:(n + 1) * Q] = torch.arange(base + 1, base + 1 + Q, dtype=torch.int32)
        dev = self._device
        m = (clip_map.to(dev), qf_map.to(dev) if Q else None,
             [torch.tensor(r, dtype=torch.int32, device=dev) for r in start_rows],
             [torch.tensor(r, dtype=torch.int32, device=dev) for r in end_rows])
        self._row_maps[key] = m
        return m

    def _gather_views(self, images, B: int, dtype=None) -> torch.Tensor:
        """[J*V*B, 3, c, c] crops of the J images of a call (llama_ens5.py:381-392: fp16 bicubic 2x down + quadrants)."""
        a = self.args
        c, J = a.vit_crop, len(images)
        if a.n_views == 5:
            views = self._buf("views", (J * 5 * B, 3, c, c), dtype)
            for j, img in enumerate(images):
                assert img.shape[-1] == 2 * c and img.shape[-2] == 2 * c, img.shape
                ops.split_views(img.contiguous(), views[j * 5 * B:(j + 1) * 5 * B])
            return views
        assert a.n_views == 1
        if J == 1:
            return images[0]
        views = self._buf("views", (J * B, 3, c, c), images[0].dtype)
        for j, img in enumerate(images):
            views[j * B:(j + 1) * B].copy_(img)        # data movement only
        return views

    def encode_image_into(self, h: torch.Tensor, image, B: int, S: int,
                          qformer_feats: Optional[torch.Tensor] = None,
                          extra_feats: Optional[List[torch.Tensor]] = None, slots=(0,)) -> None:
        """llama_ens5.py:377-458 + 471-478, writing the image words straight into rows 1..W of
        every sequence of ``h`` [B*S, dim].  ``image`` is one tensor or a list of len(slots) tensors (the
        two-image plugin encodes RGB and depth in one ViT/projector pass)."""
        a = self.args
        dtp = self._dtype
        _, _, L = self._vit_geometry()
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        assert len(images) == len(slots)
        views = self._gather_views(images, B)
        N = len(images) * a.n_views * B
        feats = self.clip_encode_image(views)
        if extra_feats is None and self.extra_feat_fns:
            extra_feats = [fn(views) for fn in self.extra_feat_fns]
        if qformer_feats is None and self.qformer_fn is not None:
            qformer_feats = self.qformer_fn(views)
        pk = self._pack()
        pw = pk["visual_proj"]
        if a.extra_feat_dim or pw.shape[1] != feats.shape[1]:
            assert (extra_feats is not None) == bool(a.extra_feat_dim), "extra_feat_dim set but no extra features given"
            cat = self._buf("proj_in", (N * L, pw.shape[1]))
            cat.zero_()
            cat[:, :a.vit_width] = feats              # data movement only (concat, llama_ens5.py:436-440)
            o = a.vit_width
            for e in (extra_feats or []):
                e2 = e.reshape(N * L, -1).to(dtp)
                cat[:, o:o + e2.shape[1]] = e2
                o += e2.shape[1]
            feats = cat
        proj = self._buf("proj_out", (N * L, a.dim))
        vp0, vp1 = getattr(self.visual_proj, "0"), getattr(self.visual_proj, "1")
        ops.gemm_nt(feats, pw, proj, bias=vp0.bias)
        clip_map, qf_map, start_rows, end_rows = self._image_row_maps(B, S, slots)
        ops.layernorm(proj, vp1.weight, vp1.bias, h, row_map=clip_map)
        if a.qformer_tokens:
            assert qformer_feats is not None, "qformer_tokens set but no Q-Former features given"
            Q = a.qformer_tokens
            qin = qformer_feats.reshape(N * Q, 768).to(dtp).contiguous()
            qp0, qp1 = getattr(self.qformer_proj, "0"), getattr(self.qformer_proj, "1")
            qout = self._buf("qf_out", (N * Q, a.dim))
            ops.gemm_nt(qin, qp0.weight, qout, bias=qp0.bias)
            ops.layernorm(qout, qp1.weight, qp1.bias, h, row_map=qf_map)
        tags = self._image_slots()
        for j, sl in enumerate(slots):
            ops.fill_rows(tags[sl][0].view(-1), h, start_rows[j])
            ops.fill_rows(tags[sl][1].view(-1), h, end_rows[j])

    # ------------------------------------------------------------------ forward (teacher forced)
    def forward(self, examples: torch.Tensor, image: Optional[torch.Tensor] = None, *,
                qformer_feats=None, extra_feats=None) -> torch.Tensor:
        """llama_ens5.py:461-487: logits [B, T, V] in the model dtype for all text positions."""
        return self._forward_images(examples, [] if image is None else [image], (0,) if image is not None else (),
                                    qformer_feats, extra_feats)

    def _forward_images(self, examples, images, slots, qformer_feats=None, extra_feats=None, out_from=None) -> torch.Tensor:
        self._destroy_kv_cache()
        self._pack(check=True)
        a = self.args
        B, T = examples.shape
        W = self.words_per_image * len(images) if images else 0
        S = T + W
        h = self._buf("h", (B * S, a.dim))
        ops.embed_assemble(examples.contiguous(), self.tok_embeddings.weight, h, B, T, W, a.dim)
        if images:
            self.encode_image_into(h, images, B, S, qformer_feats, extra_feats, slots)
        spad = (S + 63) // 64 * 64
        kc = self._buf("fw_k", (B, self.n_kv_heads, spad, self.head_dim))
        vc = self._buf("fw_vt", (B, self.n_kv_heads, self.head_dim, spad))
        L = self.n_layers
        self._decoder_layers(h, B, S, 0, 0, [kc] * L, [vc] * L, True)
        xn = self._buf("xn_final", (B * S, a.dim))
        ops.rmsnorm(h, self.norm.weight, xn, a.norm_eps)
        o0 = W if out_from is None else out_from       # h[:, image_words:] (llama_ens5.py:486)
        out = torch.empty(B, S - o0, a.vocab_size, dtype=self._dtype, device=self._device)
        xv = xn.view(B, S, a.dim)
        w4a8 = self.weight_format == "mxfp4" and self._weights.prefill     # the head on its image (bf16 logits: the NONE epilogue)
        wout = self._weights.images["output"] if w4a8 else self._head_weight()
        for b in range(B):
            (self._mx4_gemm if w4a8 else ops.gemm_nt)(xv[b, o0:], wout, out[b])
        return out

    # ------------------------------------------------------------------ forward_inference (KV cached)
    @torch.no_grad()
    def forward_inference(self, tokens: torch.Tensor, start_pos: int, image: Optional[torch.Tensor] = None, *,
                          qformer_feats=None, extra_feats=None) -> torch.Tensor:
        """llama_ens5.py:490-531: fp32 logits [B, V] of the last position."""
        return self._forward_inference_images(tokens, start_pos, [] if image is None else [image],
                                              (0,) if image is not None else (), qformer_feats, extra_feats)

    def _forward_inference_images(self, tokens, start_pos, images, slots, qformer_feats=None, extra_feats=None) -> torch.Tensor:
        a = self.args
        B, T = tokens.shape
        if start_pos == 0:
            self._allocate_kv_cache(B)
            self._pack(check=True)
        W = 0
        image = images if images else None
        if image is not None:
            assert start_pos == 0
            W = self.words_per_image * len(images)
            self.cache_image_words = W
            assert self.cache_image_words == self.image_words
            rope0 = 0
        else:
            if start_pos == 0:
                self.cache_image_words = 0
                rope0 = 0
            else:
                start_pos = start_pos + self.cache_image_words
                rope0 = start_pos
        S = T + W
        h = self._buf("h", (B * S, a.dim))
        ops.embed_assemble(tokens.contiguous(), self.tok_embeddings.weight, h, B, T, W, a.dim)
        if image is not None:
            self.encode_image_into(h, image, B, S, qformer_feats, extra_feats, slots)
        w8 = self._step_format_code()
        if (S == 1 and (B <= 16 or (B <= 32 and a.dim % 128 == 0 and self.ffn % 128 == 0)) and self._dtype == torch.bfloat16
                and self.head_dim in (64, 128) and a.dim % 32 == 0 and self.ffn % 32 == 0
                and w8 is not None                                       # MXFP4 images: the kernel-by-kernel form only
                and not getattr(self, "_per_kernel_decode", False)):     # test hook: run the step kernel by kernel
            # the C entry says up front which form it takes (a3v_llama_decode_step_form): 17..32 rows need the fused GEMV forms (two row
            # chunks); a geometry they do not take goes through the general kernels -- decided BEFORE h or the KV cache are touched, an
            # error from inside the step is never papered over
            form = _lib.load().a3v_llama_decode_step_form(B, a.dim, a.n_heads, self.n_kv_heads, self.head_dim, self.ffn, w8)
            # (an fp8 KV cache has the fused form only: elsewhere the per-kernel sequence of _decoder_layers)
            if form == 2 or (self._kv8 is None and (form or (B <= 16 and w8 != 2))):
                self._decode_step(h, B, start_pos)
            else:
                self._decoder_layers(h, B, S, start_pos, rope0, self._k_cache, self._vt_cache, True)
        else:
            self._decoder_layers(h, B, S, start_pos, rope0, self._k_cache, self._vt_cache, True)
        last = h.view(B, S, a.dim)[:, -1, :]            # strided rows, no copy
        xn = self._buf("xn_last", (B, a.dim))
        ops.rmsnorm(last, self.norm.weight, xn, a.norm_eps)
        logits = self._buf("logits", (B, a.vocab_size), torch.float32)
        self._lm_head_last(xn, logits, S == 1 and B <= 32)     # (an MXFP4 model: the head as the layers, GEMV up to 32 rows)
        # the reference returns a fresh tensor (output(h[:, -1, :]).float(), llama_ens5.py:530-531); `logits` is a cached workspace
        # that the next call overwrites, so hand out a copy (B x V fp32 = 1 MB at bs 8: microseconds next to a 4 ms step)
        return logits.clone()

    # ------------------------------------------------------------------ ragged decode (every cache row at its own position)
    def _ragged_check(self, what: Optional[str] = None) -> None:
        """Refusals of the ragged path, raised before anything is allocated or launched.  ``what``: an entry that exists for the bf16
        cache alone ("lookup decoding", "forward_verify_rows", "beam_search")."""
        if self._kv_quant == "fp8" and not self._kv_rows:
            raise RuntimeError("ragged decode (prefill_row / forward_inference_rows / generate_many) is not open on this fp8 KV cache: "
                               "call quantize_kv_cache(None) for the bf16 cache, or quantize_kv_cache('fp8', rows=True) for the fp8 "
                               "cache of the ragged path, or use generate()")
        if self._kv_quant == "fp8" and what == "extend_rows":
            raise RuntimeError("extend_rows (generate_many(prefix_sharing=True)) is not implemented on the fp8 KV cache (no prefill "
                               "attention reads fp8 keys): call quantize_kv_cache(None) for the bf16 cache, or use prefix_sharing=False")
        if self._kv_quant == "fp8" and what is not None:
            missing = "a3v_kv_permute_tails has no fp8 form" if what == "beam_search" else "there is no fp8 verify attention"
            raise RuntimeError(f"{what} is not implemented on the fp8 KV cache ({missing}): call quantize_kv_cache(None) for the bf16 "
                               "cache" + ("" if what == "beam_search" else ", or use lookup=0"))

    def _cache_rows(self) -> int:
        """Rows of the allocated cache (0: none).  Under an fp8 rows cache the shared bf16 pair holds one row, the fp8 arrays all."""
        if self._kv8 is not None:
            return self._kv8["k_q"][0].shape[0]
        return self._k_cache[0].shape[0] if self._k_cache else 0

    def _kv8_rows(self) -> Optional[Dict[str, object]]:
        """The fp8 arrays of a cache made by allocate_rows under quantize_kv_cache("fp8", rows=True); None on a bf16 cache."""
        if self._kv8 is None:
            return None
        assert "stage_k" not in self._kv8, "allocate_rows(batch_rows) first: this fp8 cache is forward_inference's"
        return self._kv8

    def allocate_rows(self, batch_rows: int) -> None:
        """The KV cache of ``batch_rows`` independent rows for prefill_row / forward_inference_rows."""
        self._ragged_check()
        assert 0 < batch_rows <= self.args.max_batch_size, (batch_rows, self.args.max_batch_size)
        self._allocate_kv_cache(batch_rows, rows=True)
        self._pack(check=True)

    @torch.no_grad()
    def prefill_row(self, row: int, tokens: torch.Tensor, image: Optional[torch.Tensor] = None, *,
                    qformer_feats=None, extra_feats=None) -> torch.Tensor:
        """The multi-token forward of ONE prompt (tokens [1, T], with its image words if ``image`` is given) on cache row ``row``
        of a cache made by ``allocate_rows``: the other rows are not touched.  Returns that row's last-position logits [1, V] fp32."""
        self._ragged_check()
        a = self.args
        assert tokens.dim() == 2 and tokens.shape[0] == 1, tuple(tokens.shape)
        assert 0 <= row < self._cache_rows(), "allocate_rows(batch_rows) first"
        T = tokens.shape[1]
        W = 0
        if image is not None:
            W = self.words_per_image
            assert W == self.image_words
        self.cache_image_words = W
        S = T + W
        assert S <= self._k_cache[0].shape[2], (S, self._k_cache[0].shape[2])
        h = self._buf("h", (S, a.dim))
        ops.embed_assemble(tokens.contiguous(), self.tok_embeddings.weight, h, 1, T, W, a.dim)
        if image is not None:
            self.encode_image_into(h, [image], 1, S, qformer_feats, extra_feats, (0,))
        # the batch is the outermost dimension of both caches: one row of them is a contiguous cache of batch 1
        kv8 = self._kv8_rows()
        if kv8 is not None:
            # fp8 rows cache: the unchanged bf16 forward on the one-row pair; after each layer a3v_kv_quantize_fp8 moves its positions
            # into that layer's views of the row
            views = {f: [t[row:row + 1] for t in kv8[f]] for f in ("k_q", "vt_q", "k_scale", "v_scale")}
            self._decoder_layers(h, 1, S, 0, 0, list(self._k_cache), list(self._vt_cache), True, kv8=views)
        else:
            kc = [k[row:row + 1] for k in self._k_cache]
            vc = [v[row:row + 1] for v in self._vt_cache]
            self._decoder_layers(h, 1, S, 0, 0, kc, vc, True)
        xn = self._buf("xn_last", (1, a.dim))
        ops.rmsnorm(h[S - 1:S], self.norm.weight, xn, a.norm_eps)
        logits = torch.empty(1, a.vocab_size, dtype=torch.float32, device=self._device)
        self._lm_head_last(xn, logits, False)
        return logits

    def _decode_step_rows(self, h: torch.Tensor, B: int, pos: torch.Tensor, pos_max: int, src_row=None, shared=None) -> None:
        """One bf16 decode step with row b at cache position pos[b] from one C call (a3v_llama_decode_step_rows; with shared prompt
        keys a3v_llama_decode_step_rows_shared)."""
        bufs = self._decode_step_buffers(B)
        if self._kv8 is not None:          # fp8 rows cache: one entry, the two arrays NULL without shared prompt keys
            self._llama_layer_table()      # (builds the kv8 table too)
            sp = (src_row.data_ptr(), shared.data_ptr()) if src_row is not None else (None, None)
            self._call_step("a3v_llama_decode_step_rows_kv8", h, bufs, (pos.data_ptr(), *sp, pos_max, B), tables=(self._kv8_tab,))
        elif src_row is not None:
            self._call_step("a3v_llama_decode_step_rows_shared", h, bufs, (pos.data_ptr(), src_row.data_ptr(), shared.data_ptr(), pos_max, B))
        else:
            self._call_step("a3v_llama_decode_step_rows", h, bufs, (pos.data_ptr(), pos_max, B))

    def _decoder_layers_rows(self, h: torch.Tensor, B: int, pos: torch.Tensor, pos_max: int, src_row=None, shared=None) -> None:
        """The ragged step kernel by kernel: _decoder_layers at S = 1 with a3v_rope_kvcache_rows / a3v_attention_decode_rows (with
        shared prompt keys: a3v_attention_decode_rows_shared)."""
        a = self.args
        H, Hkv, hd = self.n_heads, self.n_kv_heads, self.head_dim
        self._pack()
        cs = self._cos_sin_dev()
        xn, qkv, att, act, scratch = self._row_buffers(B, h.dtype == torch.bfloat16 and hd in (64, 128))
        counters = None
        if scratch is not None:
            counters = self._ws.get("rows_counters")
            if counters is None or counters.numel() < B * H:
                counters = self._ws["rows_counters"] = torch.zeros(B * H, dtype=torch.int32, device=self._device)
        sk = self._buf("rows_sk", (B,), torch.int32)
        torch.add(pos, 1, out=sk)                      # keys of row b (idle rows: <= 0)
        ldq = qkv.stride(0)
        path = self._layer_path(h, B, True, ragged=True)
        kv8 = self._kv8_rows()
        for i in range(self.n_layers):
            if kv8 is not None:            # fp8 rows cache: a3v_rope_kvquant_rows, then the fp8 rows attention (plain or shared)
                fp8c = (kv8["k_q"][i], kv8["vt_q"][i], kv8["k_scale"][i], kv8["v_scale"][i])
                self._layer(i, path, h, (xn, qkv, att, act),
                            lambda: ops.rope_kvquant_rows(qkv, qkv, *fp8c, cs, pos, B, H, Hkv, hd),
                            lambda: ops.attention_decode_rows_fp8kv(qkv, *fp8c, att, sk, pos_max + 1, B, H, Hkv, hd, scratch, counters,
                                                                    src_row, shared))
                continue
            kc, vc = self._k_cache[i], self._vt_cache[i]
            smax = kc.shape[2]
            strides = (ldq, ldq, hd, Hkv * smax * hd, smax * hd, hd, Hkv * hd * smax, hd * smax, smax, H * hd, H * hd, hd)
            if src_row is None:
                attend = lambda: ops.attention_decode_rows(qkv, kc, vc, att, sk, pos_max + 1, B, H, Hkv, hd, strides, scratch, counters)
            else:
                attend = lambda: ops.attention_decode_rows_shared(qkv, kc, vc, att, sk, src_row, shared, pos_max + 1, B, H, Hkv, hd, strides,
                                                                  scratch, counters)
            self._layer(i, path, h, (xn, qkv, att, act), lambda: ops.rope_kvcache_rows(qkv, qkv, kc, vc, cs, pos, B, H, Hkv, hd), attend)

    @torch.no_grad()
    def forward_inference_rows(self, next_tok: torch.Tensor, pos: torch.Tensor, pos_max: int,
                               out: Optional[torch.Tensor] = None, *, src_row: Optional[torch.Tensor] = None,
                               shared: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One decode step with every cache row at its own position: next_tok [B] (int64, device) is embedded, row b is written at
        cache position pos[b] (int32, device, image words included; negative = idle row: nothing written, its logits are not
        meaningful) and attends to pos[b] + 1 keys.  ``pos_max`` = the largest position (host value).  fp32 logits [B, V] (into
        ``out`` if given).  bf16 and fp32 streams.
        ``src_row`` / ``shared`` (both or neither; int32 [B], device): shared prompt keys -- row b reads its keys below shared[b]
        (a multiple of 64, see ``share_prefix``) from cache row src_row[b] (include/a3vlm_hip.h, "Shared prompt keys").  Without
        them the call is the one it was."""
        self._ragged_check()
        a = self.args
        B = next_tok.shape[0]
        if (src_row is None) != (shared is None):
            raise ValueError("forward_inference_rows: src_row and shared are given together, or neither")
        if src_row is not None:
            assert all(t.dtype == torch.int32 and t.numel() == B and t.is_contiguous() and t.is_cuda for t in (src_row, shared))
        assert self._cache_rows() == B, "allocate_rows(batch_rows) first; one token per cache row"
        assert next_tok.dtype == torch.int64 and pos.dtype == torch.int32 and pos.numel() == B and pos.is_contiguous()
        assert 0 <= pos_max < min(self._k_cache[0].shape[2], self._cos_sin_cpu.shape[0]), pos_max
        h = self._buf("h", (B, a.dim))
        ops.embed_assemble(next_tok.view(B, 1).contiguous(), self.tok_embeddings.weight, h, B, 1, 0, a.dim)
        w8 = self._step_format_code()
        form = "a3v_llama_decode_step_rows_form" if self._kv8_rows() is None else "a3v_llama_decode_step_rows_kv8_form"
        fused = (self._dtype == torch.bfloat16 and not getattr(self, "_per_kernel_decode", False) and w8 is not None
                 and getattr(_lib.load(), form)(B, a.dim, a.n_heads, self.n_kv_heads, self.head_dim, self.ffn, w8) == 2)
        if fused:
            self._decode_step_rows(h, B, pos, pos_max, src_row, shared)
        else:
            self._decoder_layers_rows(h, B, pos, pos_max, src_row, shared)
        xn = self._buf("xn_last", (B, a.dim))
        ops.rmsnorm(h, self.norm.weight, xn, a.norm_eps)
        logits = out if out is not None else torch.empty(B, a.vocab_size, dtype=torch.float32, device=self._device)
        self._lm_head_last(xn, logits, B <= 32)
        return logits

    def _verify_buffers(self, B: int, Q: int):
        """The split-KV scratch and the arrival counters of a3v_attention_verify_rows at B cache rows of Q queries (any sk_max)."""
        H, hd = self.n_heads, self.head_dim
        want = -(-768 // (B * H))                      # the decode plan never takes more key ranges than this
        scratch = self._buf("verify_scratch", (B * Q * H * want * (hd + 2),), torch.float32)
        counters = self._ws.get("verify_counters")
        if counters is None or counters.numel() < 2 * B * H:
            counters = self._ws["verify_counters"] = torch.zeros(2 * B * H, dtype=torch.int32, device=self._device)
        return scratch, counters

    @torch.no_grad()
    def forward_verify_rows(self, x: torch.Tensor, pos: torch.Tensor, nq: torch.Tensor, pos_max: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One lookup-decoding step: x [B, Q] (int64, device) holds per cache row its last emitted token and up to Q - 1 drafted
        ones; query j of row b is embedded, written at cache position pos[b] + j (pos: int32 [B], device; negative = idle row)
        and attends to pos[b] + j + 1 keys; only the first nq[b] (int32 [B], 1 <= nq[b] <= Q) queries of a row are live.
        ``pos_max`` >= the largest pos[b] (host value).  fp32 logits [B * Q, V], row b * Q + j for query j of row b (into ``out``
        if given); the rows of idle queries are not meaningful.  bf16 and fp32 streams.
        INVARIANT: the step leaves keys at pos[b] .. pos[b] + nq[b] - 1.  Those of rejected drafts lie behind the position the row
        continues from: no later query reads them (each masks at its own key count) and the next step overwrites them."""
        self._ragged_check("forward_verify_rows")
        a = self.args
        B, Q = x.shape
        M = B * Q
        assert 1 <= Q <= 8 and M <= 32, (B, Q)
        assert self._k_cache and self._k_cache[0].shape[0] == B, "allocate_rows(batch_rows) first; Q tokens per cache row"
        assert x.dtype == torch.int64 and x.is_contiguous()
        assert all(t.dtype == torch.int32 and t.numel() == B and t.is_contiguous() for t in (pos, nq))
        smax = self._k_cache[0].shape[2]
        assert 0 <= pos_max < min(smax, self._cos_sin_cpu.shape[0]), pos_max
        H, Hkv, hd = self.n_heads, self.n_kv_heads, self.head_dim
        h = self._buf("h", (M, a.dim))
        ops.embed_assemble(x.view(M, 1), self.tok_embeddings.weight, h, M, 1, 0, a.dim)
        w8 = self._step_format_code()
        fused = (self._dtype == torch.bfloat16 and not getattr(self, "_per_kernel_decode", False) and w8 is not None
                 and _lib.load().a3v_llama_decode_step_verify_form(B, Q, a.dim, H, Hkv, hd, self.ffn, w8) == 2)
        sk_max = min(pos_max + Q, smax)
        if fused:
            sws = self._decode_step_buffers(min(M, 16))[5]
            scratch, _ = self._verify_buffers(B, Q)
            self._call_step("a3v_llama_decode_step_verify", h, (*self._row_buffers(M, False)[:4], scratch, sws),
                            (pos.data_ptr(), nq.data_ptr(), pos_max, B, Q))
        else:
            self._pack()
            cs = self._cos_sin_dev()
            xn, qkv, att, act, _ = self._row_buffers(M, False)
            scratch = counters = None
            if h.dtype == torch.bfloat16 and hd in (64, 128):
                scratch, counters = self._verify_buffers(B, Q)
            ldq = qkv.stride(0)
            path = self._layer_path(h, M, True, ragged=True)
            for i in range(self.n_layers):
                kc, vc = self._k_cache[i], self._vt_cache[i]
                strides = (ldq, ldq, hd, Hkv * smax * hd, smax * hd, hd, Hkv * hd * smax, hd * smax, smax, H * hd, H * hd, hd)
                self._layer(i, path, h, (xn, qkv, att, act),
                            lambda: ops.rope_kvcache_spans(qkv, qkv, kc, vc, cs, pos, nq, B, Q, H, Hkv, hd),
                            lambda: ops.attention_verify_rows(qkv, kc, vc, att, pos, nq, sk_max, B, Q, H, Hkv, hd, strides, scratch, counters))
        xn = self._buf("xn_last", (M, a.dim))
        ops.rmsnorm(h, self.norm.weight, xn, a.norm_eps)
        logits = out if out is not None else torch.empty(M, a.vocab_size, dtype=torch.float32, device=self._device)
        self._lm_head_last(xn, logits, True)
        return logits

    @torch.no_grad()
    def extend_rows(self, rows, tokens, start, src_row=None, shared=None) -> torch.Tensor:
        """The forward of SUFFIX tokens over keys that are already cached (include/a3vlm_hip.h, "Extend prefill"): cache row
        ``rows[i]`` takes the ids ``tokens[i]`` (1-D, non-empty) at positions ``start[i]`` .. (image words included) and attends to
        the keys [0, start[i]) below them -- its own, or with ``src_row[i]`` / ``shared[i]`` (both or neither; host ints) those
        below shared[i] rounded down to 64 from cache row src_row[i] (``share_prefix``'s rule).  One packed pass over
        M = sum of the suffix lengths rows: embed, every decoder block with a3v_rope_kvcache_extend + a3v_attention_extend_rows as
        its attention stage, the final RMSNorm and the LM head on each suffix's last row only.  Returns fp32 logits
        [len(rows), V] in the order of ``rows``.  The other cache rows are not touched.  bf16 and fp32 streams, the bf16 / fp32
        KV cache; the weights run as in ``prefill_row``."""
        if (src_row is None) != (shared is None):
            raise ValueError("extend_rows: src_row and shared are given together, or neither")
        self._ragged_check("extend_rows")
        a = self.args
        R = self._cache_rows()
        if R == 0:
            raise ValueError("extend_rows: allocate_rows(batch_rows) first")
        smax = min(self._k_cache[0].shape[2], self._cos_sin_cpu.shape[0])
        rows, start = [int(r) for r in rows], [int(x) for x in start]
        n = len(rows)
        if not (n == len(tokens) == len(start)) or n == 0 or len(set(rows)) != n or min(rows) < 0 or max(rows) >= R:
            raise ValueError(f"extend_rows: rows {rows} must be distinct rows of the {R}-row cache, one suffix and one start each")
        lens = [int(t.numel()) for t in tokens]
        for r, ln, st, t in zip(rows, lens, start, tokens):
            if t.dim() != 1 or ln == 0:
                raise ValueError(f"extend_rows: row {r} has an empty suffix: every row takes at least one token (a prompt that is all "
                                 "prefix is cut one token earlier: share P = min(C, len - 1) & ~63)")
            if st < 0 or st + ln > smax:
                raise ValueError(f"extend_rows: row {r}: start {st} + {ln} tokens > the cache length {smax}: use a larger max_seq_len "
                                 "or a shorter prompt")
        H, Hkv, hd = self.n_heads, self.n_kv_heads, self.head_dim
        dev = self._device
        order = sorted(range(n), key=lambda j: rows[j])        # the packing follows the cache rows: q_off is indexed by row
        q_off, sk, src, shr, last = [0] * (R + 1), [0] * R, list(range(R)), [0] * R, [0] * n
        o = 0
        for j in order:
            r = rows[j]
            q_off[r], o = o, o + lens[j]
            sk[r], last[j] = start[j] + lens[j], o - 1
            if src_row is not None:
                src[r], shr[r] = int(src_row[j]), int(shared[j])
        M = o
        for r in range(R - 1, -1, -1):                         # rows without a suffix: an empty span in front of the next row's
            if sk[r] == 0:
                q_off[r] = q_off[r + 1] if r + 1 < R else M
        q_off[R] = M
        for r in range(R):                                     # (a row's span ends where the next one starts)
            assert q_off[r] <= q_off[r + 1]
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
        q_off_d, sk_d = i32(q_off), i32(sk)
        src_d, shr_d = (i32(src), i32(shr)) if src_row is not None else (None, None)
        nq_max, sk_max = max(lens), max(sk)
        x = torch.cat([tokens[j].to(device=dev, dtype=torch.long) for j in order]).view(M, 1).contiguous()
        h = self._buf("h", (M, a.dim))
        ops.embed_assemble(x, self.tok_embeddings.weight, h, M, 1, 0, a.dim)
        self._pack()
        cs = self._cos_sin_dev()
        xn, qkv, att, act, _ = self._row_buffers(M, False)
        scratch = None
        if h.dtype == torch.bfloat16 and hd in (64, 128):
            scratch = self._buf("extend_scratch", (ops.attention_extend_rows_scratch_floats(R, H, hd, self._k_cache[0].shape[2]),), torch.float32)
        ldq = qkv.stride(0)
        path = self._layer_path(h, M, False)
        if path == "w8a8":
            if self._weights.version != self._packed_version:
                raise RuntimeError("parameters changed after quantize_decode_weights(): call it again (or with mode=None)")
            xq = self._buf("fp8_x", (M, max(a.dim, H * hd)), torch.uint8)
            aq = self._buf("fp8_act", (M, self.ffn), torch.uint8)
            sx = self._buf("fp8_sx", (M,), torch.float32)
        for i, lyr in enumerate(self.layers):
            kc, vc = self._k_cache[i], self._vt_cache[i]
            cap = kc.shape[2]
            strides = (ldq, ldq, hd, Hkv * cap * hd, cap * hd, hd, Hkv * hd * cap, hd * cap, cap, H * hd, H * hd, hd)
            rope = lambda: ops.rope_kvcache_extend(qkv, qkv, kc, vc, cs, q_off_d, sk_d, nq_max, R, H, Hkv, hd)
            attend = lambda: ops.attention_extend_rows(qkv, kc, vc, att, q_off_d, sk_d, nq_max, sk_max, R, H, Hkv, hd, strides, scratch,
                                                       src_d, shr_d)
            if path == "w8a8":             # W8A8 as _decoder_layers runs it, the qkv product stored plainly (its RoPE epilogue has one
                # position for all rows) and rotated by the span kernel
                (wqkv_q, wqkv_s), (wo_q, wo_s), (w13_q, w13_s), (w2_q, w2_s) = self._layer_operands(i, path)
                ops.quantize_rows_fp8(h, xq[:, :a.dim], sx, lyr.attention_norm.weight, a.norm_eps)
                ops.gemm_nt_fp8(xq[:, :a.dim], sx, wqkv_q, wqkv_s, qkv)
                rope()
                attend()
                ops.quantize_rows_fp8(att, xq[:, :H * hd], sx)
                ops.gemm_nt_fp8(xq[:, :H * hd], sx, wo_q, wo_s, h, residual=h)
                ops.quantize_rows_fp8(h, xq[:, :a.dim], sx, lyr.ffn_norm.weight, a.norm_eps)
                ops.gemm_nt_fp8(xq[:, :a.dim], sx, w13_q, w13_s, act, epilogue=ops.EPI_SWIGLU)
                ops.quantize_rows_fp8(act, aq, sx)
                ops.gemm_nt_fp8(aq, sx, w2_q, w2_s, h, residual=h)
                continue
            self._layer(i, path, h, (xn, qkv, att, act), rope, attend)
        xl = self._buf("xn_last", (n, a.dim))
        ops.rmsnorm(h, self.norm.weight, xl, a.norm_eps, row_idx=i32(last))
        logits = torch.empty(n, a.vocab_size, dtype=torch.float32, device=dev)
        self._lm_head_last(xl, logits, False)
        return logits

    def share_prefix(self, src_row: int, dst_rows, P: int) -> int:
        """Makes the rows ``dst_rows`` siblings of cache row ``src_row``, whose prompt fills positions [0, P) (image words
        included): the keys below the last 64 boundary, P & ~63, stay in the source row alone and are read from there
        (``forward_inference_rows(..., src_row=, shared=)``); the rest of the prompt, [P & ~63, P), is copied into every sibling's
        own row by one launch over all layers (a3v_kv_copy_span; an fp8 rows cache: a3v_kv8_copy_span, bytes and scales).  Returns
        P & ~63, the value to put in ``shared[]``."""
        self._ragged_check()
        assert 0 <= src_row < self._cache_rows(), "allocate_rows(batch_rows) first"
        assert 0 <= P <= self._k_cache[0].shape[2], (P, self._k_cache[0].shape[2])
        lo = P & ~63
        dst = dst_rows if isinstance(dst_rows, torch.Tensor) else torch.tensor(list(dst_rows), dtype=torch.int32, device=self._device)
        kv8 = self._kv8_rows()
        if dst.numel() and P > lo and kv8 is not None:
            arrays = [kv8[f] for f in ("k_q", "vt_q", "k_scale", "v_scale")]
            key = tuple(t.data_ptr() for ts in arrays for t in ts)
            ptrs = self._ws.get("kv8_ptrs")
            if ptrs is None or ptrs[0] != key:             # the device table of base pointers follows the cache allocation
                ptrs = (key, None)
            self._ws["kv8_ptrs"] = (key, ops.kv8_copy_span(*arrays, src_row, dst, lo, P, ptrs[1]))
        elif dst.numel() and P > lo:
            key = tuple(t.data_ptr() for t in self._k_cache) + tuple(t.data_ptr() for t in self._vt_cache)
            ptrs = self._ws.get("kv_ptrs")
            if ptrs is None or ptrs[0] != key:             # the device table of base pointers follows the cache allocation
                ptrs = self._ws["kv_ptrs"] = (key, None)
            tab = ops.kv_copy_span(self._k_cache, self._vt_cache, src_row, dst, lo, P, ptrs[1])
            self._ws["kv_ptrs"] = (key, tab)
        return lo
