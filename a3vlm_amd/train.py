"""Training step of the plugin: forward + backward of the multimodal path through HIP kernels.

Reference semantics (model/accessory/engine_finetune.py:44-68, main_finetune.py:212-217,268-276):
autocast(bf16) over fp32 master weights of the trainables, bf16 frozen visual encoder, fp32
residual stream, activation checkpointing per TransformerBlock, loss = CE(ignore_index=0).
Here that is: one custom autograd node per step whose forward runs the kernels and keeps only each
block's input (fp32) and whose backward recomputes a block, then back-propagates through it with
GEMMs on transposed operand images (dgrad / wgrad), RMSNorm / SwiGLU / RoPE / attention backward
kernels, and accumulates fp32 gradients straight into one flat buffer that ``param.grad`` views
alias (wq|wk|wv and w1|w3 share fused buffers).  ``on_layer_grads_ready`` lets the DP reducer start
an all-reduce of a layer's gradient range while earlier layers are still back-propagating.
"""
from __future__ import annotations

import os

from contextlib import contextmanager
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import grad_finish, ops
from .train_images import GROUPS, _AdapterImages, _Fp8Images, _Images, _Nf4Images, _pad64, group_modules
from .util import install_param_epoch_hook


def skinny_slices(M: int, N: int, K: int, cus: int) -> int:
    """Split-K slices for an adapter-sized product out[M, N] = a[M, K] @ w[N, K]^T (``TrainEngine._skinny``).  ``cus`` = compute units of
    the device (0: not a GPU tensor).  N <= 64 and M >= 2048: 256-row blocks, ONE resident block per CU -- a3v_gemm_nt_splitk takes that form
    when S x ceil(M / 256) fills between half and all of the CUs: 8728 rows -> 35 row tiles x 7 slices = 245 blocks; one slice more and the
    blocks that wait for a CU double the time (profiles/r04k_skinny_stages_sweep.txt)."""
    blocks = ((M + 127) // 128) * ((N + 127) // 128)
    nk = K // 64
    S = 1
    while blocks * S < 512 and S * 2 <= nk and S < 32:
        S *= 2
    if N <= 64 and M >= 2048 and cus > 0:
        S = max(1, min(cus // ((M + 255) // 256), nk // 2, 32))
    elif N <= 64 and M >= 512 and S > 4:
        S = 4            # 64-row tiles (a3v_gemm_nt_splitk): M / 64 blocks per slice already fill the chip; more slices only add reduce work
    return S


def label_rows_ref(labels: torch.Tensor, W: int, S: int):
    """What ``ops.label_rows`` (a3v_label_rows) computes, in torch: for the shifted labels [B, T], the positions whose label is not 0 in
    ascending order -- as rows b S + W + t of the decoder stream, as rows b T + t of the head, and the labels there."""
    T = labels.shape[1]
    flat = labels.reshape(-1)
    pos = torch.nonzero(flat != 0).reshape(-1)
    b = torch.div(pos, T, rounding_mode="floor")
    return (b * S + W + (pos - b * T)).to(torch.int32), pos.to(torch.int32), flat[pos]


class TrainEngine:
    # A/B and test hooks (environment A3V_FUSE_QKV_ROPE=0 / A3V_TN_WGRAD=0 / A3V_NN_DGRAD=0 flips the default for a whole process)
    fuse_qkv_rope = os.environ.get("A3V_FUSE_QKV_ROPE", "1") != "0"   # qkv GEMM with the RoPE / cache-write epilogue
    tn_wgrad = os.environ.get("A3V_TN_WGRAD", "1") != "0"              # weight gradients by a3v_gemm_tn (else transposes + NT)
    nn_dgrad = os.environ.get("A3V_NN_DGRAD", "1") != "0"              # input gradients by a3v_gemm_nn (else NT on W^T images); unset: see __init__
    packed_attn_bwd = os.environ.get("A3V_PACKED_ATTN_BWD", "1") != "0"  # attention backward writes the rotated-back qkv gradient itself
    lora_kext = os.environ.get("A3V_LORA_KEXT", "1") != "0"            # adapters inside the main GEMMs: [x | t] . [W | B]^T (K extended by Rp)
    # LoRA input gradients dx = [dy | dt] . [W ; A]: the base matrices are FROZEN, so a transposed image [W^T | A^T] can be kept for
    # free and the product runs on the NT ring kernel (1.38-1.42 PF) instead of the NN kernel (1.28-1.30) for the groups named here
    # ("0": none, "all", or a comma list of qkv / wo / w13 / w2).  Same-box LoRA step: 253.0 ms without, 248.9 with wo,w13,w2, 247.9 all
    lora_nt_dgrad = os.environ.get("A3V_LORA_NT_DGRAD", "all")
    strip_wgrad = os.environ.get("A3V_STRIP_WGRAD", "1") != "0"        # adapter weight gradients by a3v_gemm_tn_strip (0: the 256 x 256 TN split-K kernel)
    fuse_swiglu_bwd = os.environ.get("A3V_FUSE_SWIGLU_BWD", "1") != "0"   # LoRA: SwiGLU backward in the epilogue of w2's input-gradient GEMM (0: separate pass, A/B)
    # the last block's wo / FFN branch, the final norm, the head and the loss on the rows with a label only (0: on every row); DESIGN.md 11
    label_rows = os.environ.get("A3V_LABEL_ROWS", "1") != "0"
    # LoRA: the adapter strips' split-K planes and the RMSNorm partial rows stay in a step-long arena and ONE a3v_grad_finish_multi launch
    # after the last block's backward turns them into gradients (0: every product finishes its own sums, A/B); DESIGN.md 5, 11
    finish_defer = os.environ.get("A3V_FINISH_DEFER", "1") != "0"
    finish_budget = int(float(os.environ.get("A3V_FINISH_BUDGET_MB", grad_finish.DEFAULT_BUDGET // 2 ** 20)) * 2 ** 20)   # bytes of arena at most

    def __init__(self, model, compute_dtype: torch.dtype = torch.bfloat16, recompute: Optional[bool] = None,
                 stream_dtype: Optional[torch.dtype] = None, zero1_world: int = 0):
        """``stream_dtype``: dtype of the residual stream h, of its per-layer checkpoints and of its gradient dh.  Default = the compute
        dtype: under ``--precision bf16`` the reference wraps the model in FSDP with MixedPrecision(param_dtype=bf16)
        (main_finetune.py:241-263) and runs it under autocast (engine_finetune.py:44-50), so the embeddings come out in bf16 and every
        ``h = h + block(h)`` -- and autograd's gradient of it -- is a bf16 tensor; the fp32 masters only exist for the optimizer.  fp32
        (``A3V_STREAM_FP32=1`` or ``stream_dtype=torch.float32``) keeps the more precise stream of rounds 1-2 (+5 ms per step at 7B:
        twice the bytes in every norm / norm-backward / residual epilogue pass).
        ``recompute``: True = keep only each block's input and re-run the block in backward (the reference's
        activation checkpointing, main_finetune.py:268-276); False = keep every block's intermediates (about
        1.15 GB per 7B layer at 8 x 1091 tokens -- affordable in 288 GB of HBM and ~1/4 fewer GEMM FLOPs per step).
        None = decide from free HBM at the first step.
        ``zero1_world`` = N > 0 (``a3vlm_amd.zero1``, the reference's FSDP(SHARD_GRAD_OP) sizing for configs[3]): trainable parameters left in
        the compute dtype (the big matrices: not promoted to fp32) have NO fp32 replica here -- they become views of one flat buffer in the
        compute dtype laid out like the flat gradient buffer (every bucket's sharded span padded to a multiple of 64 N elements, so that
        reduce-scatter / all-gather work on it in place), the GEMM images are views of the same storage, and ``Zero1Optimizer`` owns the
        fp32 master / AdamW state of 1/N of it.  fp32 parameters (norms, projector) stay replicated as before."""
        install_param_epoch_hook()     # weight-image caches must notice optimizers that do not bump Tensor._version
        self.m = model
        self.lora = int(getattr(model, "lora_rank", 0) or 0) > 0
        self.act = compute_dtype
        if stream_dtype is None:
            stream_dtype = torch.float32 if os.environ.get("A3V_STREAM_FP32", "0") == "1" else compute_dtype
        self.stream = stream_dtype
        self.recompute = recompute
        self._img = None
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._flat: Optional[torch.Tensor] = None
        self._views: Dict[str, torch.Tensor] = {}
        self._ranges: List[Tuple[str, int, int]] = []       # (bucket name, start, end) in the flat grad buffer
        self._fresh: set = set()                            # grads attached this step whose storage is still undefined
        self._gemm_written: set = set()                     # names whose gradient comes from exactly one wgrad GEMM per micro-step
        self.on_layer_grads_ready: Optional[Callable[[str, int, int], None]] = None
        self.sumsq_sink = None               # see _wgrad
        self.static_grad_scale: Optional[float] = None      # set by a trainer that knows d(total)/d(loss) (1 / accum_iter)
        self._saved = None
        self._weights_ready: Dict[str, torch.cuda.Event] = {}   # bucket -> event of FusedAdamW.step(overlap=True), see await_weights
        self.zero1_world = int(zero1_world or 0)
        if "A3V_NN_DGRAD" not in os.environ:
            # full fine-tune (round 5): input gradients on the NT ring kernel over transposed images W^T that a3v_adamw_scaled_t keeps
            # current in the optimizer pass (+2 B of writes per parameter; same-box 336.0 -> 328 ms per 7B step).  ZeRO-1 updates flat
            # slices (no per-matrix pass to write W^T from): the NN kernel on the forward images stays there.
            self.nn_dgrad = bool(self.zero1_world)
        if self._q4base() and self.zero1_world:
            raise ValueError("ZeRO-1 shards compute-dtype base matrices; an NF4 base (quantize_base_weights) has none")
        if self._q8base():
            if self.zero1_world:
                raise ValueError("ZeRO-1 shards compute-dtype base matrices; an fp8 base (quantize_base_weights) has none")
            if compute_dtype != torch.bfloat16:
                raise ValueError(f"an fp8 base trains under the bf16 compute dtype (the products of its GEMMs are bf16); got {compute_dtype}")
        self._flat_params: Optional[torch.Tensor] = None    # zero1: the sharded parameters' storage (compute dtype, flat-gradient layout)
        self._z1: List[tuple] = []                          # zero1: (bucket, start, end, shard_start, shard_end, [(seg_start, seg_end, name)])
        self._z1_fresh = True                               # zero1: the sharded gradients restart (store / zero) at the next backward
        self._params: Dict[str, torch.nn.Parameter] = {}    # name -> parameter with gradient storage (ensure_grads)
        self._offs: Dict[str, Tuple[int, int]] = {}         # name -> (offset, padded length) in the flat gradient buffer
        self._adapters = _AdapterImages(self)               # LoRA: the adapter images and their validation state
        self._cu_count: Optional[int] = None                # compute units of the device (_skinny)
        self._nt_mem_checked = False                        # the transposed images' HBM headroom was checked (first backward)
        self._opt_stepped = False                           # an optimizer step has happened (its moments are allocated)
        self._dha_ready = False                             # fp32 stream: the last norm backward left the bf16 copy of dh in place
        self._dh_full: Optional[torch.Tensor] = None        # bf16 stream + K-ext: [dh | room for dt], see backward
        self._sel_rows: Optional[Tuple[int, int]] = None    # inside a labelled-row section: (n rows now, at most this many), see _sel_buf
        self.bucket_overlap = False                         # a DP reducer sends gradient buckets while the backward runs (dp.GradReducer)
        self._fin: Optional[grad_finish.GradFinisher] = None    # deferred gradient finish: plan, arena, tables (_fin_begin)
        self._fin_mode: Optional[str] = None                # this backward: "plan" (record the producer calls), "defer", None (off)
        self._fin_hold: Optional[List[str]] = None          # buckets announced while their gradients wait for the finish launch

    # ------------------------------------------------------------------ buffers
    def _buf(self, name, shape, dtype=None, zero=False):
        dtype = dtype or self.act
        if self._sel_rows is not None:
            return self._sel_buf(name, tuple(shape), dtype, zero)
        key = (name, tuple(shape), dtype)
        t = self._ws.get(key)
        if t is None:
            t = torch.empty(*shape, dtype=dtype, device=self.m._device)
            self._ws[key] = t
        if zero:
            t.zero_()
        return t

    def _sel_buf(self, name, shape, dtype, zero):
        """``_buf`` inside a labelled-row section (n rows this step, never more than cap): a buffer of n rows is the first n rows of
        ONE buffer of cap rows, and any other (split-K planes, pads: sized by their caller's rows) a view of one flat scratch per name
        that only grows.  So the section keeps one set of buffers however n moves from step to step, and none of them shares a name
        -- hence storage or size -- with the buffers of the every-row blocks."""
        n, cap = self._sel_rows
        name += ".sel"
        if shape[0] == n:
            key = (name, (cap,) + shape[1:], dtype)
            t = self._ws.get(key)
            if t is None:
                t = self._ws[key] = torch.empty(*key[1], dtype=dtype, device=self.m._device)
            t = t[:n]
        else:
            numel = 1
            for d in shape:
                numel *= d
            key = (name, "flat", dtype)
            t = self._ws.get(key)
            if t is None or t.numel() < numel:
                t = self._ws[key] = torch.empty(numel, dtype=dtype, device=self.m._device)
            t = t[:numel].view(shape)
        if zero:
            t.zero_()
        return t

    @contextmanager
    def _sel_section(self, sel: dict):
        """One step on the labelled rows ``sel`` (``_label_rows``' answer): buffers asked for inside are labelled-row buffers (``_sel_buf``)."""
        old = self._sel_rows
        self._sel_rows = (sel["n"], sel["cap"])
        try:
            yield
        finally:
            self._sel_rows = old

    # ------------------------------------------------------------------ optimizer hand-off (a3vlm_amd.optim.FusedAdamW(engine=...))
    def image_sink(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        """Where the optimizer may store the bf16 value of the updated parameter p (its rows of the fused forward image)."""
        return self._images().sink(p)

    def image_sink_t(self, p: torch.Tensor):
        """(bf16 view of p's columns inside the TRANSPOSED image of its fused matrix, row stride) when that image is in use (full
        fine-tune input gradients on the NT kernel) -- ``a3v_adamw_scaled_t`` then keeps it current; else None."""
        if self.nn_dgrad or self.lora:
            return None
        return self._images().sink_t(p)

    def images_adopted(self, written_ids, written_t_ids=()) -> None:
        self._opt_stepped = True
        self._images().adopted(written_ids, written_t_ids)

    def forward_order(self):
        """Gradient buckets in the order the forward first touches their parameters: ``FusedAdamW.step(overlap=True)`` updates
        them in this order on its own stream, and the next forward waits per bucket (``await_weights``) -- the HBM-bound update
        of layer i+1.. runs under the MFMA-bound GEMMs of layers ..i of the next step."""
        lay = self._layout()
        rank = {"embed": 0, "vision_proj": 1, "head": 3}
        return sorted(lay, key=lambda it: rank.get(it[0], 2))          # stable: the layers keep their order

    def await_weights(self, bucket: str) -> None:
        """The current stream waits until the optimizer has written this bucket's parameters (no-op without an overlapped step)."""
        ev = self._weights_ready.pop(bucket, None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def sync_optimizer(self) -> None:
        """The current stream waits for every update still in flight: before anything but ``forward_loss`` reads parameters or
        writes gradients (backward, checkpoints, evaluation through the model)."""
        if self._weights_ready:
            for ev in self._weights_ready.values():
                torch.cuda.current_stream().wait_event(ev)
            self._weights_ready.clear()

    def _q4base(self) -> bool:
        """The base matrices are NF4 (``llama_ens5_peft.Transformer.quantize_base_weights``): no bf16 ``weight`` exists; the GEMM images
        of one layer at a time are dequantised into a reused scratch (``_Nf4Images``)."""
        return getattr(self.m, "_q4", None) is not None

    def _q8base(self) -> bool:
        """The base matrices are fp8 (``quantize_base_weights("fp8")``): no bf16 ``weight`` exists; the base products of
        the decoder GEMM groups run on a3v_gemm_nt_fp8 over the persistent e4m3 images (``_Fp8Images``), adapters beside them."""
        return getattr(self.m, "_q8base", None) is not None

    def weight_image_bytes(self, head: bool = True) -> int:
        """Bytes of weight images the engine holds right now (decoder GEMM images and their transposes; ``head``: also the LM
        head's).  bf16 base: grows with the layers served so far.  NF4 base: one layer's worth whatever the depth.  fp8 base: the
        e4m3 image, its byte transpose and the row scales of every layer (2 B per decoder parameter), from the start."""
        return self._images().nbytes(head)

    def _kext_cols(self, key: str) -> int:
        """Width of the adapter block appended to the image / input of decoder GEMM ``key`` (0: adapters not folded in)."""
        kind = key.split(".")[0]
        return _pad64(len(GROUPS[kind]) * int(self.m.lora_rank)) if self._kext() and kind in GROUPS else 0

    def _nt_dgrad(self, key: str) -> bool:
        sel = self.lora_nt_dgrad
        if not self._kext() or sel in ("", "0"):
            return False
        g, i = key.split(".")[:2]
        frozen = self._q4base() or not any(mod.weight.requires_grad for mod in group_modules(self.m.layers[int(i)], g))
        return frozen and (sel == "all" or g in sel.split(","))

    def _kext(self) -> int:
        """Columns appended to the inputs / weight images of the four decoder GEMMs when the adapters ride inside them
        (LoRA, bf16): y = [x | t] . [W | B]^T with t = x . A^T -- no separate read-modify-write pass over y."""
        if not (self.lora and self.lora_kext and self.act == torch.bfloat16) or self._q8base():
            return 0                                       # (fp8 base: the adapters stay bf16 and separate, beside the fp8 product)
        return _pad64(3 * int(self.m.lora_rank))          # the widest group (wq|wk|wv) sets one width for all four

    def _kx(self, rows: int) -> bool:
        """This step runs the adapters inside the decoder GEMMs (K-ext): only together with the fused qkv + RoPE GEMM."""
        return self._kext() > 0 and rows > 16 and self.m.head_dim in (64, 128) and self.fuse_qkv_rope

    def _res_epi(self, out: torch.Tensor) -> int:
        """Epilogue flag of a residual add into ``out``: fp32 residual / output beside bf16 operands, else the plain one."""
        return ops.EPI_RES_F32 if out.dtype == torch.float32 and self.act == torch.bfloat16 else 0

    def _check_dtypes(self):
        if self._q8base() and (self.act != torch.bfloat16 or self.zero1_world):
            raise TypeError("an fp8 base (quantize_base_weights) trains under the bf16 compute dtype and without ZeRO-1")
        for n, p in self.m.get_trainable_params().items():
            if p.requires_grad and p.dtype != torch.float32 and not (self.zero1_world and p.dtype == self.act):
                raise TypeError(f"trainable parameter {n} must be fp32 (promote_trainable_params_to_fp32, "
                                f"util/tensor_type.py:60-66); got {p.dtype}")

    # ------------------------------------------------------------------ flat gradient buffer
    def _layout(self):
        """Order = backward completion order reversed (layer-major), so one layer's grads are contiguous."""
        m = self.m
        items: List[Tuple[str, List[Tuple[str, torch.nn.Parameter]]]] = []
        items.append(("embed", [("tok_embeddings.weight", m.tok_embeddings.weight)]))
        w = lambda mod: getattr(mod, "weight", None)       # None: an NF4 base matrix (frozen, no bf16 parameter)
        for i, l in enumerate(m.layers):
            p = f"layers.{i}."
            groups = [list(zip(GROUPS[kind], group_modules(l, kind))) for kind in GROUPS]
            items.append((f"layer{i}", [(p + sub + ".weight", w(mod)) for group in groups for sub, mod in group]
                          + [(p + "attention_norm.weight", l.attention_norm.weight), (p + "ffn_norm.weight", l.ffn_norm.weight)]))
            if self.lora:
                # group-major: the lora_a of the modules that share an input are adjacent ([n r, in] as one matrix: the group's dA
                # GEMM writes the gradients in place), then their lora_b
                for group in groups:
                    items[-1][1].extend((f"{p}{sub}.{ab}.weight", getattr(mod, ab).weight) for ab in ("lora_a", "lora_b") for sub, mod in group)
        items.append(("head", [("norm.weight", m.norm.weight), ("output.weight", w(m.output))]))
        if m.with_visual:
            vp0, vp1 = getattr(m.visual_proj, "0"), getattr(m.visual_proj, "1")
            vis = [("visual_proj.0.weight", vp0.weight), ("visual_proj.0.bias", vp0.bias),
                   ("visual_proj.1.weight", vp1.weight), ("visual_proj.1.bias", vp1.bias),
                   ("start_img", m.start_img), ("end_img", m.end_img)]
            if hasattr(m, "start_depth_img"):                  # two-image plugin (llama_ens5_2images.py:343-344)
                vis += [("start_depth_img", m.start_depth_img), ("end_depth_img", m.end_depth_img)]
            if m.args.qformer_tokens:
                q0, q1 = getattr(m.qformer_proj, "0"), getattr(m.qformer_proj, "1")
                vis += [("qformer_proj.0.weight", q0.weight), ("qformer_proj.0.bias", q0.bias),
                        ("qformer_proj.1.weight", q1.weight), ("qformer_proj.1.bias", q1.bias)]
            items.append(("vision_proj", vis))
        # frozen parameters get no gradient storage (LoRA / partial fine-tuning)
        lay = [(b, [(n, q) for n, q in plist if q is not None and q.requires_grad]) for b, plist in items]
        if self.zero1_world:           # sharded (compute-dtype) parameters first in every bucket: one contiguous span per bucket (stable order)
            lay = [(b, [it for it in pl if it[1].dtype != torch.float32] + [it for it in pl if it[1].dtype == torch.float32]) for b, pl in lay]
        return lay

    def ensure_grads(self):
        """Allocate the flat fp32 gradient buffer once; (re)attach zeroed views where .grad is None."""
        m = self.m
        if self._flat is None:
            total = 0
            offs = {}
            self._ranges = []
            zw = self.zero1_world
            granule = lambda n: (n + 64 * zw - 1) // (64 * zw) * (64 * zw)              # noqa: E731  (ZeRO-1: up to whole 64 N granules)
            for bucket, plist in self._layout():
                if zw:
                    total = granule(total)                                              # a bucket's sharded span starts on a 64 N granule
                start = total
                segs = []
                for name, p in plist:
                    if zw and p.dtype == torch.float32 and segs and segs[-1] is not None:
                        total = granule(total)                                          # end of the bucket's sharded span: whole 64 N granules
                        self._z1.append((bucket, segs))
                        segs = [None]                                                   # (closed)
                    offs[name] = (total, p)
                    if zw and p.dtype != torch.float32:
                        segs.append((total, total + p.numel(), name))
                    total += (p.numel() + 63) // 64 * 64
                if zw and segs and segs[-1] is not None:
                    total = granule(total)
                    self._z1.append((bucket, segs))
                self._ranges.append((bucket, start, total))
            self._flat = torch.zeros(total, dtype=torch.float32, device=m._device)
            for name, (o, p) in offs.items():
                self._views[name] = self._flat[o:o + p.numel()].view(p.shape)
            self._params = {name: p for name, (o, p) in offs.items()}
            self._offs = {name: (o, (p.numel() + 63) // 64 * 64) for name, (o, p) in offs.items()}
            base = {sub + ".weight" for subs in GROUPS.values() for sub in subs}
            self._gemm_written = {n for n in self._params if n == "output.weight" or (n.startswith("layers.") and n.split(".", 2)[2] in base)}
            if zw:
                # the sharded parameters move into ONE flat buffer in the compute dtype with the gradient buffer's layout (their old
                # storage is released): reduce-scatter / all-gather address it by the same flat ranges as the gradients
                rng = {b: (st, en) for b, st, en in self._ranges}
                z1 = []
                for bucket, segs in self._z1:
                    segs = [x for x in segs if x is not None]
                    ss = segs[0][0]
                    se = granule(segs[-1][1])
                    assert (se - ss) % (64 * zw) == 0 and se <= rng[bucket][1], (bucket, ss, se, rng[bucket])
                    z1.append((bucket, rng[bucket][0], rng[bucket][1], ss, se, segs))
                self._z1 = z1
                self._flat_params = torch.zeros(total, dtype=self.act, device=m._device)
                with torch.no_grad():
                    for _, _, _, _, _, segs in z1:
                        for a, z, name in segs:
                            q = self._params[name]
                            dst = self._flat_params[a:z].view(q.shape)
                            dst.copy_(q.data)
                            q.data = dst
                if hasattr(m, "invalidate_packed_weights"):
                    m.invalidate_packed_weights()
        runs = []                     # [start, end) float ranges of the flat buffer to zero, adjacent ones merged (one fill per run)

        def add_run(name):            # this gradient restarts: stored by its first wgrad GEMM of the step, else zeroed here
            if name in self._gemm_written:
                return self._fresh.add(name)
            o, n = self._offs[name]
            if runs and runs[-1][1] == o:
                runs[-1][1] = o + n
            else:
                runs.append([o, o + n])
        for name, p in self._params.items():
            if not p.requires_grad:
                if p.grad is not None and p.grad.data_ptr() == self._views[name].data_ptr():
                    p.grad = None
                continue
            v = self._views[name]
            if self.zero1_world and p.dtype != torch.float32:
                # a sharded parameter: its gradient lives in the flat buffer only (torch refuses an fp32 .grad on a bf16 tensor); it
                # restarts after every Zero1Optimizer.step (zero1_mark_fresh)
                if self._z1_fresh:
                    add_run(name)
                continue
            if p.grad is None:
                # big decoder / head matrices are written (not accumulated) by their first weight-gradient GEMM of the
                # step: no 27 GB zero-fill and no read of the old value.  Everything else is zeroed here.
                add_run(name)
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():
                raise RuntimeError(f"{name}.grad was replaced by a foreign tensor; use zero_grad(set_to_none=True) or keep the views")
        for o, e in runs:
            self._flat[o:e].zero_()
        self._z1_fresh = False

    # ------------------------------------------------------------------ ZeRO-1 (a3vlm_amd.zero1.Zero1Optimizer)
    def flat_params(self) -> torch.Tensor:
        if self._flat is None:
            self.ensure_grads()
        if self._flat_params is None:
            raise RuntimeError("flat_params(): the engine was not built with zero1_world")
        return self._flat_params

    def zero1_buckets(self, weight_decay: float = 0.0):
        """[(bucket, start, end, shard_start, shard_end, [(seg_start, seg_end, weight_decay)])]: per-parameter pieces of each bucket's sharded
        span with the reference's decay rule (no decay for *.bias / *norm.weight, util/misc.py:586-599: none of the sharded matrices)."""
        self.flat_params()
        return [(b, s, e, ss, se, [(a, z, 0.0 if (n.endswith(".bias") or n.endswith("norm.weight")) else weight_decay) for a, z, n in segs])
                for b, s, e, ss, se, segs in self._z1]

    def zero1_mark_fresh(self) -> None:
        """The sharded parameters were updated in place (all-gather into flat_params): their gradients restart at the next backward and
        every cache keyed on parameter state (packed inference weights) is stale; the training images are views and need nothing."""
        self._z1_fresh = True
        for _, _, _, _, _, segs in self._z1:
            for _, _, name in segs:
                torch.autograd.graph.increment_version(self._params[name])

    def _pview(self, ps) -> Optional[torch.Tensor]:
        """[rows, cols] view of consecutive sharded parameters (wq|wk|wv, w1|w3, or one matrix) in the flat parameter buffer, or None."""
        fp = self._flat_params
        if fp is None or any(q.dtype != fp.dtype or q.untyped_storage().data_ptr() != fp.untyped_storage().data_ptr() for q in ps):
            return None
        es = fp.element_size()
        o = (ps[0].data_ptr() - fp.data_ptr()) // es
        n, cols = sum(q.numel() for q in ps), ps[0].shape[1]
        for a, b2 in zip(ps, ps[1:]):
            if b2.data_ptr() != a.data_ptr() + a.numel() * es or b2.shape[1] != cols:
                return None
        return fp[o:o + n].view(n // cols, cols)

    def grad_ranges(self):
        return list(self._ranges)

    def flat_grads(self) -> torch.Tensor:
        return self._flat

    def _has(self, *names: str) -> bool:
        return all(n in self._views for n in names)

    def _gview(self, first: str, last: str) -> torch.Tensor:
        """Fused [rows, cols] view over consecutive parameters (wq|wk|wv, w1|w3)."""
        a, b = self._views[first], self._views[last]
        cols = a.shape[1]
        n = (b.data_ptr() - a.data_ptr()) // 4 + b.numel()
        assert n % cols == 0
        base = self._flat[(a.data_ptr() - self._flat.data_ptr()) // 4:]
        return base[:n].view(n // cols, cols)

    # ------------------------------------------------------------------ weight images in the compute dtype
    def _images(self):
        """Lazy bf16 weight images: group ``L{i}`` (qkv / wo / w13 / w2 and their transposes of layer i), ``out``, ``vp``; a group
        is (re)built on first use after its parameters changed.  (Issuing the AdamW update per layer on a side stream under the
        next forward was tried on top of this and measured no gain: the 256x256 GEMM leaves no VGPRs for a co-resident kernel.)"""
        if self._img is None or not isinstance(self._img, _Images):
            self._img = _Nf4Images(self) if self._q4base() else _Fp8Images(self) if self._q8base() else _Images(self)
        if self._q8base() and not isinstance(self._img, _Fp8Images):
            self._img = _Fp8Images(self)                  # (the model was quantised after this engine first ran)
        return self._img

    # ------------------------------------------------------------------ GEMM helpers
    def _wgrad(self, dy: torch.Tensor, x: torch.Tensor, grad: torch.Tensor, tag: str, names=(), store: bool = False):
        """grad[N,K] (fp32) += dy[M,N]^T @ x[M,K]; plain store when every parameter in ``names`` is fresh this step (or ``store``)."""
        M, N = dy.shape
        K = x.shape[1]
        fresh = store or (bool(names) and all(n in self._fresh for n in names))
        assert fresh or not any(n in self._fresh for n in names), "partially fresh fused gradient view"
        self._fresh.difference_update(names if fresh else ())
        tn_ok = (self.tn_wgrad and self.act == torch.bfloat16 and N % 8 == 0 and K % 4 == 0 and dy.stride(0) % 8 == 0
                 and x.stride(0) % 8 == 0 and 2 * M * max(dy.stride(0), x.stride(0)) < 2 ** 31)
        if tn_ok and min(N, K) >= 256:
            # both operands as they are (token-major): the TN kernel transposes fragments on the LDS read
            sink = self.sumsq_sink            # dp.GradSquareSums (one rank): the clip's sum of squares comes out of this GEMM's epilogue
            sq = sink.wgrad_slots(grad, N, K) if sink is not None and grad.is_contiguous() else None
            ops.gemm_tn(dy, x, grad, residual=None if fresh else grad, epilogue=ops.EPI_OUT_F32 if fresh else ops.EPI_RES_F32, sumsq=sq)
            return
        if tn_ok and self._strip_ok(dy, x):
            # adapter gradients [N <= 64, K]: the small-block streaming kernel (three blocks per CU; token slices chosen so that the
            # grid holds ~2 blocks per CU: fewer slices = less reduce work, tools/lora_skinny_bench.py)
            S = self._strip_slices(M, K)
            ops.gemm_tn_strip(dy, x, grad, self._buf("splitk", (S * N * K,), torch.float32), S, accumulate=not fresh)
            return
        if tn_ok and min(N, K) <= 64 and max(N, K) >= 256:
            # adapter gradients: a strip of 256 x 256 tiles, split over the tokens so the whole chip streams dy / x once
            blocks = ((N + 255) // 256) * ((K + 255) // 256)
            S = 1
            while blocks * S < 256 and S < 16 and 2 * S <= (M + 63) // 64:
                S *= 2
            ops.gemm_tn_splitk(dy, x, grad, self._buf("splitk", (S * N * K,), torch.float32), S, accumulate=not fresh)
            return
        Mp = _pad64(M)
        dyt = self._buf("wg_dyt" + tag, (N, Mp))
        xt = self._buf("wg_xt" + tag, (K, Mp))
        ops.transpose(dy, dyt, M, N, Mp)
        ops.transpose(x, xt, M, K, Mp)
        if min(N, K) <= 64:
            self._skinny(dyt, xt, grad, accumulate=not fresh)
        else:
            ops.gemm_nt(dyt, xt, grad, residual=None if fresh else grad,
                        epilogue=(ops.EPI_OUT_F32 if fresh else ops.EPI_RES_F32) if self.act == torch.bfloat16 else 0)

    def _strip_ok(self, dy: torch.Tensor, x: torch.Tensor) -> bool:
        """``_wgrad`` of dy [M, N], x [M, K] (both taken by the TN kernels) runs on a3v_gemm_tn_strip."""
        N, K = dy.shape[1], x.shape[1]
        return bool(self.strip_wgrad and N <= 64 and N % 4 == 0 and K >= 256 and dy.stride(0) >= 64
                    and (dy.data_ptr() | x.data_ptr()) % 16 == 0)

    @staticmethod
    def _strip_slices(M: int, K: int) -> int:
        """Token slices of a strip product over M tokens with K output columns (at most ``_strip_slices(1 << 30, K)``)."""
        return max(1, min(64, (M + 63) // 64, -(-512 // ((K + 127) // 128))))

    # ------------------------------------------------------------------ deferred gradient finish (a3v_grad_finish_multi)
    def _fin_begin(self) -> None:
        """Start of a backward: does this one leave its adapter / norm gradient partials to one finish launch?  Not under the engines
        whose gradients leave before the backward ends or restart differently (recompute, ZeRO-1, DP bucket overlap), and only on the
        bf16 stream the headline runs.  The engine's FIRST such backward only records what its producer calls need (``plan``); the
        arena is allocated behind it if it fits ``finish_budget``, and later backwards defer."""
        self._fin_mode, self._fin_hold = None, None
        flat = self._flat
        if not (self.finish_defer and self.lora and not self.recompute and not self.zero1_world and not self.bucket_overlap
                and self.stream == torch.bfloat16 and self.act == torch.bfloat16 and flat is not None and flat.is_cuda):
            return
        if self._fin is None or self._fin.flat_ptr != flat.data_ptr() or self._fin.plan.budget_bytes != self.finish_budget:
            self._fin = grad_finish.GradFinisher(self.finish_budget, flat.data_ptr())
            self._fin_mode = "plan"
        elif self._fin.arena is not None:
            self._fin.pending = {}
            self._fin_mode, self._fin_hold = "defer", []

    def _fin_end(self) -> None:
        """After the last block's backward: the finish launch, then the bucket announcements that waited for it (whoever takes sums of
        squares of a bucket, or sends it, must see finished gradients)."""
        if self._fin_mode == "plan":
            self._fin.commit(self._flat.device)
        elif self._fin_mode == "defer":
            self._fin.launch()
        self._fin_mode = None
        held, self._fin_hold = self._fin_hold, None
        for bucket in held or ():
            self._notify(bucket)

    def _fin_slot(self, key, add, signature: tuple, count: int):
        """The arena slot of producer call ``key`` for ``count`` planes / partial rows, or None: the call finishes its own sums (not
        deferring, the recording backward -- ``add(plan)`` registers the call there --, or a call the plan does not cover)."""
        if self._fin_mode == "plan":
            try:
                add(self._fin.plan)
            except ValueError:
                pass                                      # a shape the finish kernel does not take: stays on its own reduce
            return None
        if self._fin_mode != "defer":
            return None
        slot = self._fin.plan.slots.get(key)
        if slot is None or slot.signature() != signature or count > slot.count_cap or key in self._fin.pending:
            return None
        return slot

    def _wgrad_deferred(self, key, dy: torch.Tensor, x: torch.Tensor, dst=None, scatter=None) -> bool:
        """``_wgrad`` of an adapter strip with its sum left to the finish launch: the planes of dy^T x go into the call's arena slice.
        ``dst``: the [N, K] gradient view they are added into; ``scatter`` = (r, views, row0s): the blocks are added, transposed, into
        the modules' [n_j, r] views.  False: nothing was launched (the caller runs ``_wgrad``)."""
        if self._fin_mode is None or self.act != torch.bfloat16 or not self.tn_wgrad or not self._strip_ok(dy, x):
            return False
        (M, N), K = dy.shape, x.shape[1]
        if dy.stride(0) % 8 or x.stride(0) % 8 or 2 * M * max(dy.stride(0), x.stride(0)) >= 2 ** 31:
            return False
        S, S_cap = self._strip_slices(M, K), self._strip_slices(1 << 30, K)
        if scatter is None:
            sig = (grad_finish.PLANES, N, K, (dst.data_ptr(),), dst.stride(0), True, 0, (), ())
            add = lambda plan: plan.add_planes(key, N, K, S_cap, dst.data_ptr(), dst.stride(0), True)      # noqa: E731
        else:
            r, views, row0s = scatter
            ptrs, njs = tuple(v.data_ptr() for v in views), tuple(int(v.shape[0]) for v in views)
            if not all(v.is_contiguous() and v.shape[1] == r for v in views):
                return False
            sig = (grad_finish.SCATTER, N, K, ptrs, 0, True, r, tuple(row0s), njs)
            add = lambda plan: plan.add_scatter(key, N, K, S_cap, r, ptrs, row0s, njs)                     # noqa: E731
        slot = self._fin_slot(key, add, sig, S)
        if slot is None:
            return False
        ops.gemm_tn_strip_planes(dy, x, self._fin.slice_of(slot, S * N * K), S)
        self._fin.pending[key] = S
        return True

    def _norm_bwd(self, key, x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, dh: torch.Tensor, dw: Optional[torch.Tensor], eps: float,
                  dh_lowp: Optional[torch.Tensor] = None):
        """``ops.rmsnorm_bwd``; when this backward defers, the weight gradient's partial rows stay in the call's arena slice."""
        rows, dim = x.shape
        if (self._fin_mode is not None and dw is not None and dh_lowp is None and x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
                and dim % 4 == 0 and dim <= 8192 and x.stride(0) % 4 == 0 and dy.stride(0) % 4 == 0 and dh.stride(0) % 4 == 0
                and (x.data_ptr() | dh.data_ptr() | dy.data_ptr()) % 8 == 0 and w.data_ptr() % 16 == 0):
            nb = (rows + 7) // 8                             # partial rows now; the slice holds those of a section's row cap
            cap = max(nb, (self._sel_rows[1] + 7) // 8 if self._sel_rows is not None else 0)
            sig = (grad_finish.COLSUM, 0, dim, (dw.data_ptr(),), 0, True, 0, (), ())
            slot = self._fin_slot(key, lambda plan: plan.add_colsum(key, cap, dim, dw.data_ptr()), sig, nb)
            if slot is not None:
                ops.rmsnorm_bwd_parts(x, w, dy, dh, self._fin.slice_of(slot, nb * dim), eps)
                self._fin.pending[key] = nb
                return
        ops.rmsnorm_bwd(x, w, dy, dh, dw, eps, dh_lowp=dh_lowp)

    def _skinny(self, a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, accumulate: bool = False):
        """out (+)= a @ w.T for adapter-sized problems (M or N <= 64, long K): split-K planes of the 128x128 kernel + one
        reduce pass; a plain launch would be a handful of blocks with a serial K loop (122 us instead of ~25 at 8728 x 64 x 4096)."""
        M, K = a.shape
        N = w.shape[0]
        S = skinny_slices(M, N, K, self._cus(a.device) if a.is_cuda else 0)
        if S == 1 or self.act != torch.bfloat16 or K % 64:
            ops.gemm_nt(a, w, out, residual=out if accumulate else None,
                        epilogue=(ops.EPI_RES_F32 if accumulate else ops.EPI_OUT_F32) if self._res_epi(out) else 0)
            return
        ops.gemm_nt_splitk(a, w, out, self._buf("splitk", (S * M * N,), torch.float32), S, accumulate)

    def _cus(self, dev) -> int:
        if self._cu_count is None:
            self._cu_count = int(torch.cuda.get_device_properties(dev).multi_processor_count)
        return self._cu_count

    def _dgrad_w(self, dy: torch.Tensor, key: str, out: torch.Tensor):
        """out[M,K] = dy[M,N] @ W[N,K] for the weight image ``key``: the NN kernel on the forward image itself (the transposed
        image ``key.t`` is then never built: no per-step transpose of the updated weights, no second copy in HBM); falls back
        to the NT kernel on the transposed image for shapes / dtypes the NN kernel does not take."""
        im = self._images()
        M, N = dy.shape
        if self._q8base() and key.split(".")[0] in GROUPS:
            # fp8 base: dx = (dy * sw) . Wq -- the row scales of W folded into dy, quantised per row into the zero-padded width of the
            # byte transpose, then the fp8 NT GEMM over it (weight-side scale 1)
            wqt = im[key + ".qT"]
            gq = self._buf("q8_g", (M, wqt.shape[1]), torch.uint8)
            sg = self._buf("q8_sg", (M,), torch.float32)
            ops.quantize_rows_fp8_cs(dy, im[key + ".s"], gq, sg)
            ops.gemm_nt_fp8(gq, sg, wqt, im[key + ".one"], out)
            return
        if self.nn_dgrad and self.act == torch.bfloat16 and N % 64 == 0 and dy.stride(0) % 8 == 0:
            w = im[key]
            if w.shape[0] == N and w.shape[1] % 8 == 0 and w.shape[1] >= 256 and 2 * M * dy.stride(0) < 2 ** 31 and 2 * w.numel() < 2 ** 31:
                ops.gemm_nn(dy, w, out)
                return
        self._dgrad(dy, im[key + ".t"], out)

    def _dgrad(self, dy: torch.Tensor, wt: torch.Tensor, out: torch.Tensor):
        """out[M,K] = dy[M,N] @ W[N,K] with wt = W^T [K, Np]; dy may have N < Np columns -> padded copy."""
        M, N = dy.shape
        Np = wt.shape[1]
        if Np != N:
            dyp = self._buf("dg_pad", (M, Np), zero=True)
            dyp[:, :N].copy_(dy)
            dy = dyp
        if wt.shape[0] <= 64:
            self._skinny(dy, wt, out)
        else:
            ops.gemm_nt(dy, wt, out)

    # ------------------------------------------------------------------ LoRA adapters (model/peft.py semantics)
    def _lora_step_images(self):
        return self._adapters.images()

    def adapter_sink(self, p: torch.Tensor):
        return self._adapters.sink(p)

    def adapters_adopted(self, written_ids) -> None:
        self._adapters.adopted(written_ids)

    @property
    def _li_ver(self):
        return self._adapters.ver

    def _lora_t(self, key: str, x: torch.Tensor, tag: str, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """t = lora_a(x) = x . A^T of a fused adapter group (kept for the backward), into ``t`` (K-ext: the tail columns of the GEMM's
        input) or a buffer of its own."""
        A = self._lora_step_images()[key + ".A"]
        if t is None:
            t = self._buf("lora_t." + key.split(".")[0] + tag, (x.shape[0], A.shape[0]))
        self._skinny(x, A, t)
        return t

    def _lora_add(self, key: str, t: torch.Tensor, y: torch.Tensor):
        """y += lora_b(t) for a fused adapter group."""
        ops.gemm_nt(t, self._lora_step_images()[key + ".B"], y, residual=y, epilogue=self._res_epi(y))

    # ------------------------------------------------------------------ one decoder GEMM group (GROUPS): forward and backward
    def _x_buf(self, name: str, cols: int, key: str, rows: int, kx: bool):
        """Input buffer of decoder GEMM ``key``: (x, full, t).  K-ext: ``full`` = [x | t] with room for the adapter projection
        t = x . A^T behind x; else ``full`` is x itself and t is None."""
        full = self._buf(name, (rows, cols + (self._lora_step_images()[key + ".A"].shape[0] if kx else 0)))
        return (full[:, :cols], full, full[:, cols:]) if kx else (full, full, None)

    def _dy_buf(self, name: str, cols: int, key: str, rows: int, kx: bool):
        """Output-gradient buffer of decoder GEMM ``key``: (dy, full).  K-ext: ``full`` = [dy | dt] (buffer ``name``.x) with room for
        dt = dy . B behind dy; else full is None."""
        dy, full, _ = self._x_buf(name + ".x" if kx else name, cols, key, rows, kx)
        return dy, (full if kx else None)

    def _base_fwd_fp8(self, key: str, x: torch.Tensor, out: torch.Tensor, residual: Optional[torch.Tensor] = None, epilogue: int = 0):
        """out = epilogue((quant_rows(x) . Wq^T) * sx[m] * sw[n]): the base product of decoder GEMM ``key`` over an fp8 base."""
        im = self._images()
        xq = self._buf("q8_x", tuple(x.shape), torch.uint8)
        sx = self._buf("q8_sx", (x.shape[0],), torch.float32)
        ops.quantize_rows_fp8(x, xq, sx)
        ops.gemm_nt_fp8(xq, sx, im[key + ".q"], im[key + ".s"], out, residual=residual, epilogue=epilogue)
        return xq, sx

    def _group_fwd(self, i: int, kind: str, x: torch.Tensor, x_full: torch.Tensor, t: Optional[torch.Tensor], out: torch.Tensor,
                   residual: Optional[torch.Tensor] = None, epilogue: int = 0, tag: str = "") -> Optional[torch.Tensor]:
        """out = x . W^T (+ residual) of GEMM group ``kind`` of layer i with its adapters; (x, x_full, t) from ``_x_buf``.  Returns
        t = lora_a(x) for the backward (None without adapters)."""
        im, key = self._images(), f"{kind}.{i}"
        if t is not None:
            # K-ext, adapters inside the GEMM: t goes into the tail columns of the input, B sits in the tail columns of the image
            self._lora_t(key, x, tag, t)
            ops.gemm_nt(x_full, im[key + ".x"], out, residual=residual, epilogue=epilogue)
            return t
        if self._q8base():
            self._base_fwd_fp8(key, x, out, residual, epilogue)
        else:
            ops.gemm_nt(x, im[key], out, residual=residual, epilogue=epilogue)
        if not self.lora:
            return None
        t = self._lora_t(key, x, tag)                     # separate adapters: a read-modify-write pass over the output
        self._lora_add(key, t, out)
        return t

    def _group_bwd(self, i: int, kind: str, dy: torch.Tensor, dy_full: Optional[torch.Tensor], x: torch.Tensor, t: Optional[torch.Tensor],
                   dx: torch.Tensor, swiglu_gu: Optional[torch.Tensor] = None):
        """dx = dy . W (+ the adapter term) of GEMM group ``kind`` of layer i and its adapter weight gradients; (dy, dy_full) from
        ``_dy_buf``.  K-ext: dy_full = [dy | dt] (dt = dy . B in the tail columns) times [W ; A] in ONE GEMM (dx = dy W + dt A).
        ``swiglu_gu`` (K-ext w2 only): the product is d(act) of the SwiGLU and ``dx`` the [rows, 2 F] gradient of the gate | up
        rows -- the SwiGLU backward runs in the GEMM epilogue."""
        key = f"{kind}.{i}"
        if dy_full is None:
            self._dgrad_w(dy, key, dx)
            if self.lora:
                self._lora_bwd(i, key, dy, x, t, dx)
            return
        dt = dy_full[:, dy.shape[1]:]
        self._dgrad(dy, self._lora_step_images()[key + ".Bt"], dt)
        im = self._images()
        if swiglu_gu is not None:
            ops.gemm_nt(dy_full, im[key + ".yT"], dx, residual=swiglu_gu, epilogue=ops.EPI_SWIGLU_BWD)
        elif self._nt_dgrad(key):
            ops.gemm_nt(dy_full, im[key + ".yT"], dx)          # frozen base: the transposed image is free (built once)
        else:
            ops.gemm_nn(dy_full, im[key + ".y"], dx)
        self._lora_bwd(i, key, dy, x, t, None, dt=dt)

    def _group_wgrad(self, i: int, kind: str, dy: torch.Tensor, x: torch.Tensor):
        """Base weight gradient of GEMM group ``kind`` of layer i, into the fused view of its modules' gradients (none when frozen)."""
        names = tuple(f"layers.{i}.{sub}.weight" for sub in GROUPS[kind])
        if self._has(*names):
            self._wgrad(dy, x, self._gview(names[0], names[-1]), kind, names)

    def _lora_bwd(self, i: int, key: str, dy: torch.Tensor, x: torch.Tensor, t: torch.Tensor, dx: Optional[torch.Tensor], dt=None):
        """Adapter gradients of a fused group and the adapter term of the input gradient (dx += (dy B) A)."""
        m = self.m
        li = self._lora_step_images()
        r = m.lora_rank
        Bt, At = li[key + ".Bt"], li[key + ".At"]          # [Rp, Npad], [in, Rp]
        M, N = dy.shape
        Rp = t.shape[1]
        if dt is None:
            dt = self._buf("lora_dt", (M, Rp))
            self._dgrad(dy, Bt, dt)                          # dt = dy @ B
        g = key.split(".")[0]
        # dB is produced transposed ([Rp, N] = t^T dy): the strip with the adapter rank as its ROW index streams dy 1.2-1.5x
        # faster through the TN kernel than the [N, Rp] strip (tools/lora_skinny_bench.py); the r x N_j blocks are added
        # into the [N_j, r] gradient views below
        names = GROUPS[g]
        vas = [self._views[f"layers.{i}.{nm}.lora_a.weight"] for nm in names]
        vbs = [self._views[f"layers.{i}.{nm}.lora_b.weight"] for nm in names]
        nr = len(names) * r
        row0s, row = [], 0
        for vb in vbs:
            row0s.append(row)
            row += vb.shape[0]
        # (deferred finish: only the nr rows that hold adapter blocks are produced, and the finish launch adds the blocks)
        gBt = None
        if not (t.is_cuda and nr % 4 == 0 and self._wgrad_deferred((i, g, "gB"), t[:, :nr], dy, scatter=(r, vbs, row0s))):
            gBt = self._buf("lora_gBt." + g, (Rp, N), torch.float32)
            self._wgrad(t, dy, gBt, "lb", store=True)
        # dA of the whole group straight into the flat gradient buffer: the group's lora_a gradients are adjacent = ONE [n r, in] matrix
        adjacent = all(vas[j + 1].data_ptr() == vas[j].data_ptr() + 4 * vas[j].numel() for j in range(len(vas) - 1))
        if adjacent and dt.stride(0) % 8 == 0:
            off = (vas[0].data_ptr() - self._flat.data_ptr()) // 4
            gA = self._flat[off:off + nr * x.shape[1]].view(nr, x.shape[1])
            if not self._wgrad_deferred((i, g, "gA"), dt[:, :nr], x, dst=gA):
                self._wgrad(dt[:, :nr], x, gA, "la", store=False)
        else:
            gA = self._buf("lora_gA." + g, (Rp, x.shape[1]), torch.float32)
            self._wgrad(dt, x, gA, "la", store=True)
            for j, va in enumerate(vas):
                ops.add2d(va, gA[j * r:(j + 1) * r])
        if gBt is None:
            pass
        elif gBt.is_cuda:
            ops.lora_gb_scatter(gBt, r, vbs, row0s)          # one launch: each module's [n_j, r] += its diagonal block transposed
        else:
            for j, vb in enumerate(vbs):
                vb.add_(gBt[j * r:(j + 1) * r, row0s[j]:row0s[j] + vb.shape[0]].t())
        if dx is not None:
            ops.gemm_nt(dt, At, dx, residual=dx)             # dx += dt @ A

    # ------------------------------------------------------------------ one decoder block: the attention half, then the row-wise tail
    def _block_forward(self, i: int, h: torch.Tensor, B: int, S: int, keep: bool, tag: str = "", h_out: Optional[torch.Tensor] = None):
        """One decoder block on the stream h [B*S, dim], every row.
        keep=False: h is updated in place (checkpointing forward).
        keep=True : h is only read; h_mid goes to its own buffer and the intermediates the backward needs are
        returned; the block output is written to ``h_out`` if given (stored-activation forward, per-layer buffers
        selected by ``tag``) or not computed at all (recompute inside backward)."""
        kept, att = self._attn_forward(i, h, B, S, tag)
        return self._tail_forward(i, h, att, keep, tag, h_out, kept)

    def _attn_forward(self, i: int, h: torch.Tensor, B: int, S: int, tag: str):
        """The attention half of block i, on every row: att = attn(rope(qkv(norm(h)))).  Returns what the backward keeps of it and
        ``att`` as wo's input (x, full, t) from ``_x_buf``."""
        m, a = self.m, self.m.args
        H, Hkv, hd, dim = m.n_heads, m.n_kv_heads, m.head_dim, a.dim
        rows = B * S
        spad = _pad64(S)
        kx = self._kx(rows)
        xn, xn_full, t_qkv = self._x_buf("xn" + tag, dim, f"qkv.{i}", rows, kx)
        att3 = self._x_buf("att" + tag, H * hd, f"wo.{i}", rows, kx)
        att = att3[0]
        qkv = self._buf("qkv" + tag, (rows, (H + 2 * Hkv) * hd))
        qrot = self._buf("qrot" + tag, (rows, H * hd))
        kc = self._buf("kc" + tag, (B, Hkv, spad, hd))
        vc = self._buf("vc", (B, Hkv, hd, spad))
        lse = self._buf("lse" + tag, (B, H, S), torch.float32)
        ops.rmsnorm(h, m.layers[i].attention_norm.weight, xn, a.norm_eps)
        t = self._qkv_fwd(i, xn, xn_full, t_qkv, qkv, qrot, kc, vc, B, S, tag)
        ldo = att.stride(0)
        strides = (S * H * hd, H * hd, hd, Hkv * spad * hd, spad * hd, hd, Hkv * hd * spad, hd * spad, spad, S * ldo, ldo, hd)
        ops.attention_lse(qrot, kc, vc, att, lse, B, S, S, H, Hkv, hd, strides, True)
        return dict(xn=xn, qkv=qkv, qrot=qrot, kc=kc, att=att, lse=lse, spad=spad, lt={"qkv": t}), att3

    def _tail_forward(self, i: int, h: torch.Tensor, att3, keep: bool, tag: str, h_out: Optional[torch.Tensor], kept: dict):
        """The row-wise tail of block i: h_mid = h + wo(att), out = h_mid + w2(silu(g) * u) with g | u = w1|w3(norm(h_mid)), on the rows
        of its operands -- h [rows, dim] and ``att3`` = (att, full, t) from ``_x_buf``: every row of the stream, or any rows of it side by
        side.  keep / tag / h_out as in ``_block_forward``; returns ``kept`` with what the tail's backward needs added."""
        m, a, im = self.m, self.m.args, self._images()
        dim, F = a.dim, m.ffn
        rows = h.shape[0]
        l = m.layers[i]
        att, att_full, t_wo = att3
        kx = t_wo is not None
        lt = kept["lt"]
        res_flag = self._res_epi(h)                       # bf16 stream: plain bf16 residual
        h_mid = self._buf("h_mid" + tag, (rows, dim), self.stream) if keep else h
        lt["wo"] = self._group_fwd(i, "wo", att, att_full, t_wo, h_mid, h, res_flag, tag)
        gu = self._buf("gu" + tag, (rows, 2 * F))
        xn2, xn2_full, t_w13 = self._x_buf("xn2" + tag, dim, f"w13.{i}", rows, kx)
        actb, act_full, t_w2 = self._x_buf("act" + tag, F, f"w2.{i}", rows, kx)
        ops.rmsnorm(h_mid, l.ffn_norm.weight, xn2, a.norm_eps)
        lt["w13"] = self._group_fwd(i, "w13", xn2, xn2_full, t_w13, gu, tag=tag)
        ops.swiglu_fwd(gu, actb, F, interleaved=False)
        # w2 is not a _group_fwd: t = lora_a(act) is needed by the backward even when the block output is not computed, so it comes
        # first and the output GEMM(s) only when there is an output
        lt["w2"] = self._lora_t(f"w2.{i}", actb, tag, t_w2) if self.lora else None
        # (att_wo: wo's input here; kept["att"]: every row of it, for the attention backward -- the same buffer in an every-row block)
        kept.update(att_wo=att, h_mid=h_mid, xn2=xn2, gu=gu, act=actb)
        if keep and h_out is None:
            return kept                                   # recompute inside backward: the block output is not needed
        out = h_out if keep else h
        if self._q8base():
            self._base_fwd_fp8(f"w2.{i}", actb, out, h_mid, res_flag)
        else:
            ops.gemm_nt(act_full, im[f"w2.{i}.x" if kx else f"w2.{i}"], out, residual=h_mid, epilogue=res_flag)
        if self.lora and not kx:
            self._lora_add(f"w2.{i}", lt["w2"], out)
        return kept

    def _last_block_forward_rows(self, i: int, h: torch.Tensor, B: int, S: int, tag: str, sel: dict):
        """The last block when the loss reads the rows ``sel`` only (stored activations): the attention half on every row, then the
        rows sel["rows"][j] of att and of the block input side by side and the tail on those n rows, in labelled-row buffers.  Returns
        (kept, the block output at those rows [n, dim])."""
        m, n = self.m, sel["n"]
        kept, (att_all, _, t_wo) = self._attn_forward(i, h, B, S, tag)
        with self._sel_section(sel):
            att3 = self._x_buf("att", m.n_heads * m.head_dim, f"wo.{i}", n, t_wo is not None)     # (K-ext: the block's answer at B S rows)
            ops.gather_rows(att_all, sel["rows"], att3[0])
            h_in = ops.gather_rows(h, sel["rows"], self._buf("h_in", (n, m.args.dim), self.stream))
            h_out = self._buf("h_out", (n, m.args.dim), self.stream)
            return self._tail_forward(i, h_in, att3, True, "", h_out, kept), h_out

    def _qkv_fwd(self, i: int, xn, xn_full, t, qkv, qrot, kc, vc, B: int, S: int, tag: str) -> Optional[torch.Tensor]:
        """The qkv step of a block: q (rotated) into ``qrot``, K / V^T into the caches, v token-major in its columns of ``qkv``
        (attention backward); returns t = lora_a(xn) or None.  Three forms of the GEMM with the RoPE / cache-write epilogue -- plain,
        K-ext, and adapters as an additive term -- and the un-fused fallback."""
        m, im, key = self.m, self._images(), f"qkv.{i}"
        H, Hkv, hd = m.n_heads, m.n_kv_heads, m.head_dim
        fused = self.act == torch.bfloat16 and hd in (64, 128) and xn.shape[0] > 16 and self.fuse_qkv_rope
        v_rows = qkv[:, (H + Hkv) * hd:]
        if fused and not self.lora:
            ops.gemm_qkv_rope(xn, im[key], qrot, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, 0, 0, v_rows=v_rows)
            return None
        if t is not None:
            # K-ext (implies ``fused``): t = x . A^T in the tail columns of the input, B in the tail columns of the image
            self._lora_t(key, xn, tag, t)
            ops.gemm_qkv_rope(xn_full, im[key + ".x"], qrot, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, 0, 0, v_rows=v_rows)
            return t
        if fused and self._q8base():
            # fp8 base: the same additive form on the fp8 product (a3v_gemm_qkv_rope_fp8_train: v_rows and delta as the bf16 entry)
            t = self._lora_t(key, xn, tag)
            ops.gemm_nt(t, self._lora_step_images()[key + ".B"], qkv)
            xq = self._buf("q8_x", tuple(xn.shape), torch.uint8)
            sx = self._buf("q8_sx", (xn.shape[0],), torch.float32)
            ops.quantize_rows_fp8(xn, xq, sx)
            ops.gemm_qkv_rope_fp8_train(xq, sx, im[key + ".q"], im[key + ".s"], qrot, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, 0, 0,
                                        v_rows=v_rows, delta=qkv)
            return t
        if fused:
            # adapters: the LoRA term t . B^T is written into the qkv buffer first and enters the fused GEMM as an additive term
            # before the rotation (the reference's order: linear output + modification, rounded, then RoPE)
            t = self._lora_t(key, xn, tag)
            ops.gemm_nt(t, self._lora_step_images()[key + ".B"], qkv)
            ops.gemm_qkv_rope(xn, im[key], qrot, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, 0, 0, v_rows=v_rows, delta=qkv)
            return t
        t = self._group_fwd(i, "qkv", xn, xn_full, None, qkv, tag=tag)
        ops.rope_kvcache(qkv, qrot, kc, vc, m._cos_sin_dev(), B, S, H, Hkv, hd, 0, 0)
        return t

    def _block_backward(self, i: int, h_in: torch.Tensor, dh: torch.Tensor, B: int, S: int):
        """Backward of block i on every row: the tail, then the attention half; dh [rows, dim] is the stream gradient, updated in place."""
        rows, dim = B * S, self.m.args.dim
        if not self._saved.get("kept"):
            self._images().recompute_backward(i)     # (NF4 base: the block's forward and input-gradient images from one read of its codes)
        k = self._saved["kept"][i] if self._saved.get("kept") else self._block_forward(i, h_in, B, S, keep=True)
        kx = self._kx(rows)
        if self.stream == torch.bfloat16 and self.act == torch.bfloat16:
            dha, dha_full = dh, (self._dh_full if kx else None)         # dh itself is the bf16 operand of the GEMMs
        else:
            dha, dha_full = self._dy_buf("dh_act", dim, f"w2.{i}", rows, kx)
        datt = self._tail_backward(i, k, dh, dha, dha_full)
        self._attn_backward(i, k, h_in, dh, dha, datt, B, S)

    def _last_block_backward_rows(self, i: int, h_in: torch.Tensor, dh: torch.Tensor, dh_sel: torch.Tensor, B: int, S: int, sel: dict):
        """Backward of the block ``_last_block_forward_rows`` ran: the tail back-propagates the compact stream gradient ``dh_sel``
        [n, dim (+ room for dt)] of the rows sel["rows"][j]; then dh_sel and wo's input gradient are scattered into the every-row dh /
        datt (zero at every other row, written by the same launches) and the attention half runs on every row."""
        m, k = self.m, self._saved["kept"][i]
        rows, dim = B * S, m.args.dim
        kx = self._kx(rows)
        assert k["h_mid"].shape[0] == sel["n"]
        with self._sel_section(sel):
            datt_sel = self._tail_backward(i, k, dh_sel[:, :dim], dh_sel[:, :dim], dh_sel if kx else None)
        datt = ops.scatter_rows(datt_sel, sel["rows"], self._buf("datt", (rows, m.n_heads * m.head_dim)))
        ops.scatter_rows(dh_sel[:, :dim], sel["rows"], dh)
        self._attn_backward(i, k, h_in, dh, dh, datt, B, S)

    def _tail_backward(self, i: int, k: dict, dh: torch.Tensor, dha: torch.Tensor, dha_full: Optional[torch.Tensor]) -> torch.Tensor:
        """Backward of ``_tail_forward`` on the rows of its operands: dh [rows, dim] is the stream gradient of those rows, updated in
        place to that of h_mid; dha its operand form for the GEMMs -- dh itself (bf16 stream) or a bf16 buffer this pass fills -- and
        dha_full = [dha | room for dt] under K-ext (``_dy_buf``), else None.  Returns wo's input gradient datt [rows, H hd]."""
        m, a, im = self.m, self.m.args, self._images()
        H, hd, dim, F = m.n_heads, m.head_dim, a.dim, m.ffn
        rows = dha.shape[0]
        l = m.layers[i]
        lt = k["lt"]
        kx = dha_full is not None
        stream_lp = self.stream == torch.bfloat16 and self.act == torch.bfloat16
        fuse_cast = self.act == torch.bfloat16 and not stream_lp   # fp32 stream: the norm backward that produced dh also wrote its bf16 copy
        if not stream_lp and not (fuse_cast and self._dha_ready):
            ops.cast(dh, dha)
        self._dha_ready = False
        # ---- FFN: out = h_mid + w2(silu(g) * u)
        self._group_wgrad(i, "w2", dha, k["act"])
        dgu, dgu_full = self._dy_buf("dgu", 2 * F, f"w13.{i}", rows, kx)
        # w2's input gradient is d(act); three forms keep it out of HBM by applying the SwiGLU backward in the GEMM epilogue
        # (a3v_swiglu_bwd on the bf16-rounded product, bit for bit), writing d(gate) | d(up) straight into the w1|w3 gradient buffer
        ft_epi = (not self.lora and self.fuse_swiglu_bwd and self.act == torch.bfloat16 and dim % 64 == 0 and F % 8 == 0
                  and dha.stride(0) % 8 == 0)
        if kx and self.fuse_swiglu_bwd and self._nt_dgrad(f"w2.{i}") and F % 8 == 0:
            self._group_bwd(i, "w2", dha, dha_full, k["act"], lt["w2"], dgu, swiglu_gu=k["gu"])       # LoRA K-ext on the NT ring kernel
        elif (ft_epi and self.nn_dgrad and F >= 256 and 2 * rows * dha.stride(0) < 2 ** 31 and 2 * F * dim < 2 ** 31
              and tuple(im[f"w2.{i}"].shape) == (dim, F)):
            # full fine-tune: the same epilogue on the NN kernel (dX = dY . W on the forward image)
            ops.gemm_nn(dha, im[f"w2.{i}"], dgu, residual=k["gu"], epilogue=ops.EPI_SWIGLU_BWD)
        elif ft_epi and not self.nn_dgrad and tuple(im[f"w2.{i}.t"].shape) == (F, dim):
            # full fine-tune with input gradients on the NT ring kernel (W^T images): the same epilogue there
            ops.gemm_nt(dha, im[f"w2.{i}.t"], dgu, residual=k["gu"], epilogue=ops.EPI_SWIGLU_BWD)
        else:
            dact = self._buf("dact", (rows, F))
            self._group_bwd(i, "w2", dha, dha_full, k["act"], lt["w2"], dact)
            ops.swiglu_bwd(k["gu"], dact, dgu, F, interleaved=False)
        self._group_wgrad(i, "w13", dgu, k["xn2"])
        dxn = self._buf("dxn", (rows, dim))
        self._group_bwd(i, "w13", dgu, dgu_full, k["xn2"], lt["w13"], dxn)
        self._norm_bwd((i, "ffn_norm"), k["h_mid"], l.ffn_norm.weight, dxn, dh, self._views.get(f"layers.{i}.ffn_norm.weight"), a.norm_eps,
                       dh_lowp=dha if fuse_cast else None)
        # ---- wo: h_mid = h_in + wo(att)
        if not fuse_cast and not stream_lp:
            ops.cast(dh, dha)
        self._group_wgrad(i, "wo", dha, k["att_wo"])
        datt = self._buf("datt", (rows, H * hd))
        self._group_bwd(i, "wo", dha, dha_full, k["att_wo"], lt["wo"], datt)
        return datt

    def _attn_backward(self, i: int, k: dict, h_in: torch.Tensor, dh: torch.Tensor, dha: torch.Tensor, datt: torch.Tensor, B: int, S: int):
        """Backward of ``_attn_forward``, on every row: att = attn(rope(qkv(norm(h_in)))) from its output gradient datt; adds the
        result into dh (fp32 stream: and leaves its bf16 copy in dha for the next block, ``_dha_ready``)."""
        m, a = self.m, self.m.args
        H, Hkv, hd, dim = m.n_heads, m.n_kv_heads, m.head_dim, a.dim
        rows = B * S
        kx = self._kx(rows)
        fuse_cast = self.act == torch.bfloat16 and self.stream != torch.bfloat16
        D = self._buf("attn_D", (B, S, H), torch.float32)
        qkv = k["qkv"]
        ld = qkv.stride(0)
        vrows = qkv[:, (H + Hkv) * hd:]
        spad = k["spad"]
        dqkv, dqkv_full = self._dy_buf("dqkv", (H + 2 * Hkv) * hd, f"qkv.{i}", rows, kx)
        if self.act == torch.bfloat16 and hd in (64, 128) and self.packed_attn_bwd:
            # the MFMA kernels rotate dq / dk back and store [dq | dk | dv] straight into the fused-qkv gradient
            ops.attention_bwd_packed(k["qrot"], k["kc"], Hkv * spad * hd, spad * hd, vrows, S * ld, ld, hd, k["att"], datt, k["lse"], D,
                                     dqkv, m._cos_sin_dev(), B, S, H, Hkv, hd, True, 0)
        else:
            dq = self._buf("dq", (rows, H * hd))
            dk = self._buf("dk", (B, Hkv, S, hd))
            dv = self._buf("dv", (B, Hkv, S, hd))
            wsp = None
            if self.act == torch.bfloat16 and hd in (64, 128):
                wsp = self._buf("attn_bwd_ws", (ops.attention_bwd_workspace_bytes(B, S, H, Hkv, hd),), torch.uint8)
            att_c = k["att"] if k["att"].is_contiguous() else k["att"].contiguous()      # (K_ext keeps att inside a wider buffer)
            ops.attention_bwd(k["qrot"], k["kc"], Hkv * spad * hd, spad * hd, vrows, S * ld, ld, hd, att_c, datt, k["lse"], D,
                              dq, dk, dv, B, S, H, Hkv, hd, True, workspace=wsp)
            ops.rope_bwd_pack(dq, dk, dv, dqkv, m._cos_sin_dev(), B, S, H, Hkv, hd, 0)
        self._group_wgrad(i, "qkv", dqkv, k["xn"])
        dxn = self._buf("dxn", (rows, dim))
        self._group_bwd(i, "qkv", dqkv, dqkv_full, k["xn"], k["lt"]["qkv"], dxn)
        self._norm_bwd((i, "attention_norm"), h_in, m.layers[i].attention_norm.weight, dxn, dh,
                       self._views.get(f"layers.{i}.attention_norm.weight"), a.norm_eps, dh_lowp=dha if fuse_cast else None)
        self._dha_ready = fuse_cast                        # the next block's backward finds its bf16 operand in place

    # ------------------------------------------------------------------ the rows the loss reads
    def _label_rows_engine(self) -> bool:
        """This engine may run the row-wise tail of the step -- the last block's wo and FFN branch, the final norm, the head, the loss and
        their backwards -- on the labelled rows only: stored activations, bf16 stream and operands, replicated parameters."""
        return bool(self.label_rows and not self.recompute and not self.zero1_world
                    and self.stream == torch.bfloat16 and self.act == torch.bfloat16)

    @staticmethod
    def _label_rows_take(n: int, rows: int) -> bool:
        """... and does so for n labelled rows of ``rows``: not when there is none (nothing of zero size is launched; the full path
        gives loss 0 and zero gradients) and not when nothing would be left out."""
        return 0 < n < rows

    def _label_rows(self, lab: torch.Tensor, W: int, S: int) -> Optional[dict]:
        """The labelled rows of the shifted labels ``lab`` [B, T] (one launch and the step's one host wait, before any decoder launch),
        or None when the step runs every row."""
        B, T = lab.shape
        srows = self._buf("sel_stream_rows", (B * T,), torch.int32)
        hrows = self._buf("sel_head_rows", (B * T,), torch.int32)
        labs = self._buf("sel_labels", (B * T,), torch.int64)
        n_valid = self._buf("n_valid", (1,), torch.int32)
        n = int(ops.label_rows(lab, W, S, srows, hrows, labs, n_valid))
        if not self._label_rows_take(n, B * S):
            return None
        return dict(n=n, cap=B * T, rows=srows[:n], head=hrows[:n], lab=labs[:n], n_valid=n_valid)

    # ------------------------------------------------------------------ forward (loss) and backward
    @torch.no_grad()
    def forward_loss(self, examples: torch.Tensor, labels: torch.Tensor, image: Optional[torch.Tensor] = None,
                     qformer_feats=None, extra_feats=None) -> torch.Tensor:
        self._check_dtypes()
        self._adapters.checked = False
        self._sel_rows = None
        m, a = self.m, self.m.args
        B, T = examples.shape
        n_img = 0 if image is None else (len(image) if isinstance(image, (list, tuple)) else 1)
        W = m.words_per_image * n_img if n_img else 0
        S = T + W
        rows, dim = B * S, a.dim
        h = self._buf("h", (rows, dim), self.stream)
        if self.lora or self.act != torch.bfloat16:
            self.sync_optimizer()          # adapter / fp32 images are rebuilt from all parameters at once
        self.await_weights("embed")
        ops.embed_assemble(examples.contiguous(), m.tok_embeddings.weight, h, B, T, W, dim)
        vis = None
        if image is not None:
            self.await_weights("vision_proj")
            vis = self._encode_image_train(h, image, B, S, qformer_feats, extra_feats)
        hs = self._buf("h_saved", (m.n_layers + 1, rows, dim), self.stream)
        if self.recompute is None:
            F_, Hq = m.ffn, (m.n_heads + 2 * m.n_kv_heads) * m.head_dim
            esz = 2 if self.act == torch.bfloat16 else 4
            need = m.n_layers * rows * ((2 * dim + Hq + 2 * m.n_heads * m.head_dim + 3 * F_) * esz + dim * (4 if self.stream == torch.float32 else 2)) * 1.1
            free, _ = torch.cuda.mem_get_info(m._device)
            self.recompute = need > 0.5 * free
        kept = []
        lab = self._buf("lab", (B, T), torch.int64, zero=True)
        lab[:, :T - 1].copy_(labels[:, 1:])      # shift (meta.py:256-257); last position predicts nothing
        sel = self._label_rows(lab, W, S) if self._label_rows_engine() else None
        if self.recompute:
            for i in range(m.n_layers):
                hs[i].copy_(h)                   # the block input (checkpoint, main_finetune.py:268-276)
                self.await_weights(f"layer{i}")
                self._block_forward(i, h, B, S, keep=False)
        else:
            # stored activations: block i reads hs[i] and writes hs[i + 1] (its w2 GEMM's residual epilogue stores there), so the
            # checkpoints cost no copy (was one 143-MB read + write per layer)
            hs[0].copy_(h)
            last = m.n_layers - 1
            for i in range(m.n_layers):
                self.await_weights(f"layer{i}")
                if sel is not None and i == last:
                    # the last block's output is read by the final norm at the labelled rows only: it comes out compact ([n, dim])
                    k, h = self._last_block_forward_rows(i, hs[i], B, S, f".L{i}", sel)
                else:
                    k, h = self._block_forward(i, hs[i], B, S, keep=True, tag=f".L{i}", h_out=hs[i + 1]), hs[i + 1]
                kept.append(k)
        self.sync_optimizer()                    # "head" is last in forward_order: everything has landed from here on
        step = dict(B=B, T=T, W=W, S=S, hs=hs, tokens=examples.contiguous(), vis=vis, kept=kept)
        if sel is None:
            return self._head_forward(h, lab, None, step)
        with self._sel_section(sel):
            return self._head_forward(h, lab, sel, step)

    def _head_forward(self, h: torch.Tensor, lab: torch.Tensor, sel: Optional[dict], step: dict) -> torch.Tensor:
        """Final norm, LM head and loss of the step ``step`` (what ``backward`` needs of the forward so far; completed here into
        ``_saved``).  ``sel`` None: h is the stream [B S, dim] and the head runs on its B T text rows against the shifted labels
        ``lab`` [B, T]; else h is [n, dim], the labelled rows only, and so are the head's buffers (the caller's section)."""
        m, a, im = self.m, self.m.args, self._images()
        B, T, W, S = step["B"], step["T"], step["W"], step["S"]
        dim, V = a.dim, a.vocab_size
        n = B * T if sel is None else sel["n"]
        xt = self._buf("xn_text", (n, dim))
        if sel is None:
            hv = h.view(B, S, dim)
            for b in range(B):
                ops.rmsnorm(hv[b, W:], m.norm.weight, xt[b * T:(b + 1) * T], a.norm_eps)
            lab, n_valid = lab.view(-1), self._buf("n_valid", (1,), torch.int32)
        else:
            ops.rmsnorm(h, m.norm.weight, xt, a.norm_eps)
            lab, n_valid = sel["lab"], sel["n_valid"]
        logits = self._buf("logits", (n, V))
        ops.gemm_nt(xt, im["out"], logits)
        row_loss = self._buf("row_loss", (n,), torch.float32)
        if sel is None:
            ops.count_valid(lab, n_valid)
        ops.cross_entropy(logits, lab, row_loss)
        if sel is None:                                                                                   # meta.py:259-262
            nv = n_valid.to(torch.float32)[0]
            loss = torch.where(nv > 0, row_loss.sum() / torch.clamp(nv, min=1.0), torch.zeros_like(nv))
        else:
            loss = row_loss.sum() / float(n)
        self._saved = dict(step, h=h, xt=xt, logits=logits, lab=lab, n_valid=n_valid, sel=sel)
        return loss

    @torch.no_grad()
    def backward(self, grad_scale: float = 1.0) -> None:
        s = self._saved
        self._dha_ready = False
        self._sel_rows = None
        self._adapters.checked = False
        assert s is not None, "backward() without forward_loss()"
        m, a = self.m, self.m.args
        self.sync_optimizer()                    # the update reads the gradients this backward overwrites
        self.ensure_grads()
        if not self.nn_dgrad and not self.lora and not self._nt_mem_checked:
            # the transposed images cost 2 B per matrix parameter (12.3 GiB at 7B, 23.9 at 13B): on a replica that would not leave
            # 8 GiB free after them (13B at DP 8 with persistent wire buckets is at 270 of 288 GiB), stay on the NN kernel
            self._nt_mem_checked = True
            # the AdamW moments (8 B per trainable parameter) are allocated by the first optimizer step
            moments = 0 if self._opt_stepped else 8 * sum(q.numel() for q in m.parameters() if q.requires_grad)
            # (a replica that recomputes its blocks is one sized against the HBM limit -- 13B at micro-batch 4: measured 452.5 / 453.7 ms
            # with the transposed images against 455.5 / 452.4 without, for 24 GiB: not taken there unless A3V_NN_DGRAD=0 asks for it)
            if not self._nt_images_fit(moments) or (self.recompute and "A3V_NN_DGRAD" not in os.environ):
                self.nn_dgrad = True
        if self.lora and not self._q4base() and not self._q8base() and not self._nt_mem_checked:
            # LoRA engines: the input gradients of the frozen matrices run on the NT kernel over transposed images that
            # are built once (2 B per base parameter: 12.3 GiB at 7B) and, with nn_dgrad off, the head's W^T too -- the same headroom
            # rule as the full fine-tune above: without 8 GiB left after them the NN kernel on the forward images is used instead
            self._nt_mem_checked = True
            if (not self.nn_dgrad or self.lora_nt_dgrad not in ("", "0")) and not self._nt_images_fit():
                self.nn_dgrad = True
                self.lora_nt_dgrad = "0"
        if self.sumsq_sink is not None:
            self.sumsq_sink.begin_backward()
        self._fin_begin()
        B, T, W, S, dim = s["B"], s["T"], s["W"], s["S"], a.dim
        dh, dh_sel = self._head_backward(s, grad_scale)
        self._notify("head")
        # ---- decoder blocks, last to first (recompute from the saved block input)
        for i in range(m.n_layers - 1, -1, -1):
            if dh_sel is not None and i == m.n_layers - 1:
                self._last_block_backward_rows(i, s["hs"][i], dh, dh_sel, B, S, s["sel"])
            else:
                self._block_backward(i, s["hs"][i], dh, B, S)
            self._notify(f"layer{i}")
        self._fin_end()
        # ---- embeddings and projector
        if self._has("tok_embeddings.weight"):
            ops.embed_bwd(s["tokens"], dh, self._views["tok_embeddings.weight"], B, T, W, dim)
        self._notify("embed")
        if s["vis"] is not None:
            self._encode_image_backward(dh, s["vis"], B, S)
        # announced on EVERY backward, image or not: under accumulation an earlier micro-step of the cycle may have put projector
        # gradients there, and every rank must hand the same buckets to the collective on the boundary micro-step
        self._notify("vision_proj")
        self._saved = None

    def _head_grads(self, s: dict, n: int, grad_scale: float) -> torch.Tensor:
        """CE and LM head backward on the head's n rows: the head's weight gradient; returns the final norm's output gradient [n, dim]."""
        dlog = self._buf("dlogits", (n, self.m.args.vocab_size))
        ops.cross_entropy(s["logits"], s["lab"], self._buf("row_loss", (n,), torch.float32), dlog, s["n_valid"], grad_scale)
        if self._has("output.weight"):
            self._wgrad(dlog, s["xt"], self._views["output.weight"], "out", ("output.weight",))
        dxt = self._buf("dxn_text", (n, self.m.args.dim))
        self._dgrad_w(dlog, "out", dxt)
        return dxt

    def _head_backward(self, s: dict, grad_scale: float):
        """Backward of ``_head_forward``.  Returns (dh, dh_sel): the stream gradient dh [B S, dim] the blocks update in place, and --
        when the head ran on the labelled rows -- the gradient of those rows, compact and laid out like dh, for the last block's tail
        (``_last_block_backward_rows``, whose scatter writes every row of dh: it is not zeroed here); else None."""
        m, a = self.m, self.m.args
        B, T, W, S, sel = s["B"], s["T"], s["W"], s["S"], s["sel"]
        rows, dim = B * S, a.dim
        # bf16 stream + adapters inside the GEMMs: dh IS the dy operand of the wo / w2 groups, so it lives in the first `dim` columns
        # of a buffer with room for dt = dy . B behind it (no copy of dh per layer)
        # (width of the wo / w2 groups' adapter block, pad64(r) -- NOT _kext(), the qkv group's pad64(3 r): the two differ from r = 22 on)
        wide = self.stream == torch.bfloat16 and self.act == torch.bfloat16 and self._kx(rows)
        name, cols = ("dh.x", dim + self._kext_cols("w2.0")) if wide else ("dh", dim)
        norm_dw = self._views.get("norm.weight")
        if sel is None:
            dxt = self._head_grads(s, B * T, grad_scale)
            dh_full, dh_sel = self._buf(name, (rows, cols), self.stream, zero=True), None
            hv, dhv = s["h"].view(B, S, dim), dh_full[:, :dim].view(B, S, dim)
            for b in range(B):
                ops.rmsnorm_bwd(hv[b, W:], m.norm.weight, dxt[b * T:(b + 1) * T], dhv[b, W:], norm_dw, a.norm_eps)
        else:
            with self._sel_section(sel):
                dxt = self._head_grads(s, sel["n"], grad_scale)
                dh_sel = self._buf(name, (sel["n"], cols), self.stream, zero=True)
            dh_full = self._buf(name, (rows, cols), self.stream)
            with self._sel_section(sel):                    # (its partial-row slice is sized for every labelled-row count)
                self._norm_bwd("norm", s["h"], m.norm.weight, dxt, dh_sel[:, :dim], norm_dw, a.norm_eps)
        self._dh_full = dh_full if wide else None
        return dh_full[:, :dim], dh_sel

    def _nt_images_fit(self, extra: int = 0) -> bool:
        """Would 8 GiB of HBM stay free after the transposed images of the decoder / head matrices (2 B per parameter) and ``extra``
        more bytes?  (Memory the caching allocator holds but has not handed out counts as free.)"""
        im = self._images()
        need = extra + 2 * sum(q.numel() for g_ in im.groups() if g_ != "vp" for q in im._params(g_)[0])
        free, _ = torch.cuda.mem_get_info(self.m._device)
        free += torch.cuda.memory_reserved(self.m._device) - torch.cuda.memory_allocated(self.m._device)
        return free - need >= 8 * 2 ** 30

    def _notify(self, bucket: str):
        if self.on_layer_grads_ready is None:
            return
        if self._fin_hold is not None:
            return self._fin_hold.append(bucket)           # its adapter / norm gradients are final after the finish launch (_fin_end)
        for name, st, en in self._ranges:
            if name == bucket:
                self.on_layer_grads_ready(name, st, en)

    # ------------------------------------------------------------------ vision (frozen ViT, trainable projector)
    def _encode_image_train(self, h, image, B, S, qformer_feats, extra_feats):
        """Image words of the training forward (LLM/llama_ens5.py:377-458, 471-478): frozen CLIP ViT on the HIP path, then the two
        TRAINABLE projectors -- visual_proj over the concat [CLIP | ConvNeXt-XXL | DINOv2] (5632 wide in the reference configuration)
        and qformer_proj over the 32 Q-Former tokens.  The three out-of-scope encoders are frozen and run under no_grad in the
        reference (:399): their outputs are INPUTS here (``extra_feats`` / ``qformer_feats`` or the plugin's provider hooks), and
        only the projectors are differentiated (_encode_image_backward)."""
        m, a = self.m, self.m.args
        im = self._images()
        _, _, L = m._vit_geometry()
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        slots = tuple(range(len(images)))
        views = m._gather_views(images, B, m.clip.visual.conv1.weight.dtype)
        N = len(images) * a.n_views * B
        feats = m.clip_encode_image(views)                      # frozen, compute dtype of the clip params
        if extra_feats is None and getattr(m, "extra_feat_fns", None):
            extra_feats = [fn(views) for fn in m.extra_feat_fns]
        if qformer_feats is None and getattr(m, "qformer_fn", None) is not None:
            qformer_feats = m.qformer_fn(views)
        if a.extra_feat_dim:
            if extra_feats is None:
                raise ValueError("extra_feat_dim is set but no ConvNeXt / DINOv2 features were given (extra_feats= or provider hooks)")
            cat = self._buf("feats_cat", (N * L, a.vit_width + a.extra_feat_dim))
            cat[:, :a.vit_width] = feats                        # data movement only (concat, llama_ens5.py:436-440)
            o = a.vit_width
            for e in extra_feats:
                e2 = e.reshape(N * L, -1)
                cat[:, o:o + e2.shape[1]] = e2
                o += e2.shape[1]
            assert o == cat.shape[1], "extra feature widths do not add up to extra_feat_dim"
            feats = cat
        elif feats.dtype != self.act:
            f2 = self._buf("feats_act", tuple(feats.shape))
            ops.cast(feats, f2)
            feats = f2
        proj = self._buf("proj", (N * L, a.dim))
        ops.gemm_nt(feats, im["vp"], proj, bias=im["vp.b"])
        vp1 = getattr(m.visual_proj, "1")
        clip_map, qf_map, start_rows, end_rows = m._image_row_maps(B, S, slots)
        ops.layernorm(proj, vp1.weight, vp1.bias, h, row_map=clip_map)
        out = dict(feats=feats, proj=proj, clip_map=clip_map, start_rows=start_rows, end_rows=end_rows, N=N, L=L, slots=slots)
        if a.qformer_tokens:
            if qformer_feats is None:
                raise ValueError("qformer_tokens is set but no Q-Former features were given (qformer_feats= or provider hook)")
            Q = a.qformer_tokens
            qin = self._buf("qf_in", (N * Q, 768))
            qin.copy_(qformer_feats.reshape(N * Q, 768))
            qout = self._buf("qf_out", (N * Q, a.dim))
            ops.gemm_nt(qin, im["vq"], qout, bias=im["vq.b"])
            qp1 = getattr(m.qformer_proj, "1")
            ops.layernorm(qout, qp1.weight, qp1.bias, h, row_map=qf_map)
            out.update(qin=qin, qout=qout, qf_map=qf_map, Q=Q)
        tags = m._image_slots()
        for j, sl in enumerate(slots):
            ops.fill_rows(tags[sl][0].view(-1), h, start_rows[j])
            ops.fill_rows(tags[sl][1].view(-1), h, end_rows[j])
        return out

    def _encode_image_backward(self, dh, vis, B, S):
        m, a = self.m, self.m.args
        vp1 = getattr(m.visual_proj, "1")
        rowsv = vis["N"] * vis["L"]
        dproj = self._buf("dproj", (rowsv, a.dim))
        ops.layernorm_bwd(vis["proj"], vp1.weight, dh, vis["clip_map"], dproj, self._views["visual_proj.1.weight"],
                          self._views["visual_proj.1.bias"])
        self._wgrad(dproj, vis["feats"], self._views["visual_proj.0.weight"], "vp")
        ops.rows_sum(dproj, None, rowsv, self._views["visual_proj.0.bias"])
        if "qin" in vis:
            qp1 = getattr(m.qformer_proj, "1")
            rowsq = vis["N"] * vis["Q"]
            dq = self._buf("dqf", (rowsq, a.dim))
            ops.layernorm_bwd(vis["qout"], qp1.weight, dh, vis["qf_map"], dq, self._views["qformer_proj.1.weight"],
                              self._views["qformer_proj.1.bias"])
            self._wgrad(dq, vis["qin"], self._views["qformer_proj.0.weight"], "vq")
            ops.rows_sum(dq, None, rowsq, self._views["qformer_proj.0.bias"])
        names = [("start_img", "end_img"), ("start_depth_img", "end_depth_img")]
        for j, sl in enumerate(vis["slots"]):
            ops.rows_sum(dh, vis["start_rows"][j], vis["start_rows"][j].numel(), self._views[names[sl][0]].view(-1))
            ops.rows_sum(dh, vis["end_rows"][j], vis["end_rows"][j].numel(), self._views[names[sl][1]].view(-1))


class _StepLoss(torch.autograd.Function):
    """loss = engine.forward_loss(...); backward runs the HIP backward and fills param.grad itself."""

    @staticmethod
    def forward(ctx, anchor, engine, examples, labels, image):
        ctx.engine = engine
        return engine.forward_loss(examples, labels, image)

    @staticmethod
    def backward(ctx, grad_out):
        # the incoming gradient of the loss is the caller's 1 / accum_iter: a trainer that knows it sets
        # engine.static_grad_scale and spares the host read of a device scalar on every micro-step
        hint = getattr(ctx.engine, "static_grad_scale", None)
        ctx.engine.backward(float(grad_out) if hint is None else float(hint))
        return torch.zeros((), device=grad_out.device), None, None, None, None


def step_loss(engine: TrainEngine, anchor: torch.Tensor, examples, labels, image=None) -> torch.Tensor:
    return _StepLoss.apply(anchor, engine, examples, labels, image)


def hbm_budget(dim: int, n_layers: int, n_heads: int, ffn: int, vocab: int, batch: int, seq: int, text: int, n_kv_heads: Optional[int] = None,
               vit_params: int = 304_000_000, proj_in: int = 1024, world: int = 1, wire_bytes: int = 2, recompute: bool = False,
               stream_bytes: int = 2, zero1: bool = False, transposed_images: bool = False, base_bytes: Optional[int] = None) -> Dict[str, int]:
    """Bytes of one pure-DP replica of the FULL fine-tune (every rank of a DP job holds exactly this; SURVEY 7 "13B full fine-tune
    memory", main_finetune.py:241-276): what ``TrainEngine`` + ``FusedAdamW`` + ``dp.GradReducer`` allocate, from their own layouts.
    fp32 masters / flat gradient buffer / two AdamW moments of every trainable parameter, the bf16 GEMM images of the decoder and
    head matrices, the frozen bf16 ViT, the reducer's persistent wire buckets (``wire_bytes`` per gradient element when world > 1
    and the wire dtype is not fp32), the residual-stream checkpoints [L+1, rows, dim] (``stream_bytes`` per element: 2 = the bf16 stream
    of round 3 on, 4 = the fp32 stream of rounds 1-2), the block intermediates (per layer when activations are stored, once when
    blocks are recomputed), and the CE buffers; ``transposed_images``: + the W^T images of the round-5 default; ``base_bytes``: the
    decoder matrices' images, both orientations together, cost this many bytes per parameter instead (a frozen fp8 base,
    ``quantize_base_weights("fp8")``: 2 = e4m3 image + byte transpose, plus 4 B per output row of scales; the head's stay bf16).  Checked against the measured peaks of the bench
    (tests/test_dp_cpu.py::test_dp_replica_fits_288_gib)."""
    hkv = n_kv_heads or n_heads
    hd = dim // n_heads
    qkv = (n_heads + 2 * hkv) * hd
    p_layer = dim * qkv + dim * dim + 3 * dim * ffn
    p_mat = n_layers * p_layer + dim * vocab                      # matrices that get a bf16 GEMM image
    p_train = p_mat + dim * vocab + (2 * n_layers + 1) * dim + proj_in * dim + 4 * dim     # + embeddings, norms, projector, tags
    rows = batch * seq
    spad = (seq + 63) // 64 * 64
    sb = stream_bytes
    block = rows * (2 * dim * 2 + qkv * 2 + 2 * n_heads * hd * 2 + 3 * ffn * 2 + dim * sb) + batch * hkv * spad * hd * 2 + batch * n_heads * seq * 4
    bwd_ws = rows * ((dim * 2 if sb == 4 else 0) + ffn * 2 + 2 * ffn * 2 + dim * 2 + n_heads * hd * 2 + qkv * 2 + dim * sb) + batch * hkv * hd * spad * 2
    if zero1:
        # ZeRO-1 (zero1.Zero1Optimizer, TrainEngine(zero1_world=world)): the big matrices (decoder linears, embeddings, head) exist once in
        # bf16 (parameters = GEMM images = all-gather destination), their fp32 masters, both moments, the fp32 gradient slice and the bf16
        # output slice only for 1 / world of them; ONE wire bucket of the largest layer instead of persistent buckets for all
        p_big = p_mat + dim * vocab
        p_small = p_train - p_big
        layer_big = p_layer if n_layers else 0
        out = {"masters_fp32": 4 * p_small + 4 * p_big // world, "grads_fp32": 4 * p_train + 4 * p_big // world,
               "adamw_moments_fp32": 8 * p_small + 8 * p_big // world, "images_bf16": 2 * p_big + 2 * p_big // world,
               "vit_bf16": 2 * vit_params,
               "wire_buckets": (wire_bytes * max(layer_big, dim * vocab) + wire_bytes * max(layer_big, dim * vocab) // world) if wire_bytes != 4 else 0}
    else:
        out = {
            "masters_fp32": 4 * p_train, "grads_fp32": 4 * p_train, "adamw_moments_fp32": 8 * p_train, "images_bf16": 2 * p_mat,
            "vit_bf16": 2 * vit_params,
            "wire_buckets": wire_bytes * p_train if world > 1 and wire_bytes != 4 else 0}
    if transposed_images and not zero1:
        out["images_t_bf16"] = 2 * p_mat          # W^T of every decoder / head matrix (round 5: input gradients on the NT kernel, a3v_adamw_scaled_t)
    out.update({
        "stream_checkpoints": (n_layers + 1) * rows * dim * sb + rows * dim * sb,
        "block_activations": block * (1 if recompute else n_layers),
        "backward_workspace": bwd_ws,
        "ce_buffers": batch * text * vocab * 2 * 2 + batch * text * dim * 2 * 2,
    })
    if base_bytes is not None and not zero1:
        p_dec = n_layers * p_layer
        out["images_bf16"] = 2 * (p_mat - p_dec)
        if "images_t_bf16" in out:
            out["images_t_bf16"] = 2 * (p_mat - p_dec)
        out["images_base"] = base_bytes * p_dec + 4 * n_layers * (qkv + 2 * dim + 2 * ffn)
    out["total"] = sum(out.values())
    return out
