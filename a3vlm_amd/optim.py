"""AdamW on the HIP kernel ``a3v_adamw`` with the state layout of ``torch.optim.AdamW`` (``step`` / ``exp_avg`` /
``exp_avg_sq`` per parameter), so optimizer checkpoints written by either (util/misc.py:324-569 layout, ``checkpoint.py``)
load into the other.  Reference: the trainer builds ``torch.optim.AdamW(param_groups, lr, betas=(0.9, 0.95))``
(main_finetune.py:138 of this package mirrors accessory/main_finetune.py) and calls ``optimizer.step()`` once per
accumulation cycle (engine_finetune.py:63).

One launch per parameter tensor streams p, g, m, v once (28 B per parameter).  ``image_of`` (optional) maps a parameter to a
bf16 tensor of the same shape that receives the rounded updated values in the same pass (the compute-dtype operand of the next
step's GEMMs).

``step(overlap=True)`` (with ``engine``): the launches go to the optimizer's own stream in the order the forward first touches the
parameters (``TrainEngine.forward_order``), one event per gradient bucket; ``TrainEngine.forward_loss`` of the next step waits
bucket by bucket, so the 28-B/parameter HBM stream of the update runs under the MFMA-bound GEMMs of the next forward instead of
in front of it.  Same arithmetic, same order per parameter.  The caller's contract: between ``step(overlap=True)`` and the next
``forward_loss`` / ``backward`` only the host and ``zero_grad(set_to_none=True)`` touch parameters or gradients; anything else
(checkpoints, evaluation through the model, a stock ``zero_grad(set_to_none=False)``) calls ``engine.sync_optimizer()`` first
(``MetaModel.zero_grad(set_to_none=False)``, ``MetaModel.state_dict`` and this optimizer's ``state_dict`` do so themselves).

Skipped steps: a negative or NaN ``grad_scale`` makes ``a3v_adamw_scaled`` a no-op on masters, moments and bf16 images (the trainer's
device-side non-finite guard).  The host cannot know that without reading the flag, so ``state[p]["step"]`` counts LAUNCHES, not
applied updates, and the weight images are marked current either way (they are: nothing changed).  The trainer reads the flag at
its logging / checkpoint / epoch boundaries and exits there, before anything is saved, so a skipped step is never followed by a
step whose bias correction would be off by one.

``moments="e4m3"`` (opt-in): the moments of the big tensors -- ``numel() > multi_threshold`` and ``numel() % 256 == 0`` -- are kept as
blockwise e4m3 codes (include/a3vlm_hip.h, "8-bit AdamW moments": one byte per element and one fp32 scale per 256, 2.03 B per parameter
for both moments instead of 8) and updated by ``a3v_adamw8_scaled``; their state is ``step`` / ``exp_avg_q`` / ``exp_avg_scale`` /
``exp_avg_sq_q`` / ``exp_avg_sq_scale``.  Every other tensor (adapters, norms, odd sizes) keeps fp32 moments and the paths above, the
multi-tensor launch included.  ``state_dict()`` writes that native state and marks every group with ``"moments": "e4m3x256"``;
``load_state_dict`` of either mode takes either layout and converts tensor by tensor (a stock fp32 state is quantised on load, a
native one dequantised by an fp32 optimizer), so no whole-model fp32 copy of the moments exists at any time.
``a3v_adamw8_scaled`` has no scalar form for misaligned data: a parameter that does not start on 16 bytes keeps fp32 moments, and a
GRADIENT that does not (a view at an odd offset of a flat buffer) is an explicit ``A3V_ERR_SHAPE`` at the step.  There is no 8-bit form of
``a3v_adamw_scaled_t``: an engine that keeps transposed weight images is refused (build it in the NN input-gradient form)."""
from __future__ import annotations

import os
from typing import Callable, Optional

import torch

from . import lib as _l


MOMENTS_TAG = "e4m3x256"                    # param-group marker of a state_dict with 8-bit moments
BLOCK = 256                                 # elements per scale of the 8-bit moments
_F32_KEYS = ("exp_avg", "exp_avg_sq")
_Q_KEYS = ("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale")
_ZERO_SCALE = 1e-30 / 448.0                 # the scale of an all-zero block


def _quantize_state(m: torch.Tensor, v: torch.Tensor):
    """fp32 device moments of one tensor -> (exp_avg_q, exp_avg_scale, exp_avg_sq_q, exp_avg_sq_scale) by ``a3v_adam8_quantize``."""
    if not m.is_cuda:
        raise RuntimeError("8-bit AdamW moments are quantised by a HIP kernel: the parameter must be on the GPU (no CPU fallback)")
    m, v = m.contiguous(), v.contiguous()
    n = m.numel()
    mq, rq = torch.empty(m.shape, dtype=torch.uint8, device=m.device), torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    ms, rs = torch.empty(n // BLOCK, dtype=torch.float32, device=m.device), torch.empty(n // BLOCK, dtype=torch.float32, device=m.device)
    rc = _l.load().a3v_adam8_quantize(m.data_ptr(), v.data_ptr(), mq.data_ptr(), ms.data_ptr(), rq.data_ptr(), rs.data_ptr(), n,
                                      torch.cuda.current_stream().cuda_stream)
    _l.check(rc, "a3v_adam8_quantize")
    return mq, ms, rq, rs


def _dequantize_state(mq: torch.Tensor, ms: torch.Tensor, rq: torch.Tensor, rs: torch.Tensor):
    """The inverse: the codes and scales of one tensor -> fp32 (exp_avg, exp_avg_sq) by ``a3v_adam8_dequantize``."""
    if not mq.is_cuda:
        raise RuntimeError("8-bit AdamW moments are dequantised by a HIP kernel: the parameter must be on the GPU (no CPU fallback)")
    m, v = torch.empty(mq.shape, dtype=torch.float32, device=mq.device), torch.empty(mq.shape, dtype=torch.float32, device=mq.device)
    rc = _l.load().a3v_adam8_dequantize(mq.data_ptr(), ms.data_ptr(), rq.data_ptr(), rs.data_ptr(), m.data_ptr(), v.data_ptr(), mq.numel(),
                                        torch.cuda.current_stream().cuda_stream)
    _l.check(rc, "a3v_adam8_dequantize")
    return m, v


class FusedAdamW(torch.optim.Optimizer):
    bumps_version = True        # parameters' Tensor._version is incremented by step(): version-keyed caches need no extra hook

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 image_of: Optional[Callable[[torch.Tensor], Optional[torch.Tensor]]] = None, engine=None, moments: str = "fp32"):
        if moments not in ("fp32", "e4m3"):
            raise ValueError(f"unknown AdamW moment format {moments!r}: 'fp32' or 'e4m3'")
        self.moments = moments
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        # ``engine`` (a TrainEngine): the bf16 values go straight into the engine's fused weight images, which are then marked
        # current -- the next step does not re-cast 6.7 G fp32 parameters (cat + cast = 14 B per parameter) to rebuild them
        self.engine = engine
        self.image_of = image_of if engine is None else engine.image_sink
        self._stream: Optional[torch.cuda.Stream] = None
        # small tensors (adapters, norm weights, ...) of a param group go through ONE a3v_adamw_multi launch per step instead of one
        # launch each; A3V_ADAMW_MULTI=0 (A/B runs, equality tests) keeps the per-tensor launches
        self.multi_threshold = int(os.environ.get("A3V_ADAMW_MULTI", str(1 << 20)))
        self._tables = {}                      # param-group index -> (key, device table, max_n, [params])

    def state_dict(self):
        if self.engine is not None:
            self.engine.sync_optimizer()
        sd = super().state_dict()
        if self.moments == "e4m3":
            sd["param_groups"] = [{**g, "moments": MOMENTS_TAG} for g in sd["param_groups"]]
        return sd

    def _is8(self, p: torch.Tensor) -> bool:
        """Whether p's moments are kept as e4m3 codes: the big tensors only (bitsandbytes' ``min_8bit_size`` idea)."""
        return self.moments == "e4m3" and p.numel() > self.multi_threshold and p.numel() % BLOCK == 0 and p.data_ptr() % 16 == 0

    def _convert_moments(self, p: torch.Tensor, saved: dict) -> dict:
        """The moments of one saved entry in the layout this optimizer keeps for p, on p's device; copies, never views of ``saved``."""
        want8, dev, n = self._is8(p), p.device, p.numel()
        if all(k in saved for k in _Q_KEYS):
            q = {k: saved[k].to(dev, copy=True) for k in _Q_KEYS}
            if q["exp_avg_q"].dtype != torch.uint8 or q["exp_avg_sq_q"].dtype != torch.uint8 or q["exp_avg_q"].numel() != n \
                    or q["exp_avg_sq_q"].numel() != n or n % BLOCK or q["exp_avg_scale"].numel() != n // BLOCK or q["exp_avg_sq_scale"].numel() != n // BLOCK:
                raise ValueError(f"8-bit AdamW state of a {tuple(p.shape)} parameter has the wrong sizes or dtypes")
            if want8:
                return {"exp_avg_q": q["exp_avg_q"].view(p.shape), "exp_avg_scale": q["exp_avg_scale"].float().reshape(-1),
                        "exp_avg_sq_q": q["exp_avg_sq_q"].view(p.shape), "exp_avg_sq_scale": q["exp_avg_sq_scale"].float().reshape(-1)}
            m, v = _dequantize_state(q["exp_avg_q"].view(p.shape), q["exp_avg_scale"], q["exp_avg_sq_q"].view(p.shape), q["exp_avg_sq_scale"])
            return {"exp_avg": m, "exp_avg_sq": v}
        if all(k in saved for k in _F32_KEYS):
            m, v = (saved[k].to(dev, dtype=torch.float32, copy=True).view(p.shape) for k in _F32_KEYS)
            if not want8:
                return {"exp_avg": m, "exp_avg_sq": v}
            return dict(zip(_Q_KEYS, _quantize_state(m, v)))           # m and v die here: one tensor's fp32 moments at a time
        if any(k in saved for k in _Q_KEYS + _F32_KEYS):
            raise ValueError(f"incomplete AdamW state: {sorted(saved)}")
        return {}

    def load_state_dict(self, state_dict):
        """The device tables of the multi-tensor launch hold raw pointers of the moment tensors, which a load replaces.
        Takes the stock layout (``exp_avg`` / ``exp_avg_sq``, ``torch.optim.AdamW``'s and the fp32 mode's) and the native 8-bit one
        (groups marked ``"moments": "e4m3x256"``), whichever mode this optimizer is in; see the module docstring."""
        if self.engine is not None:
            self.engine.sync_optimizer()
        groups = state_dict["param_groups"]
        tags = {g.get("moments") for g in groups} - {None}
        if tags - {MOMENTS_TAG}:
            raise ValueError(f"optimizer state with unknown moment format {sorted(tags - {MOMENTS_TAG})}: this build reads fp32 and {MOMENTS_TAG!r}")
        if self.moments == "fp32" and not tags:
            super().load_state_dict(state_dict)
            self._tables.clear()
            return
        # torch's loader casts every state tensor of a floating-point parameter to the parameter's dtype -- codes included -- and
        # copies all of them at once: it gets the groups and the step counts, the moments are placed here, one tensor at a time
        saved = state_dict["state"]
        moment_keys = _Q_KEYS + _F32_KEYS
        super().load_state_dict({"state": {i: {k: x for k, x in st.items() if k not in moment_keys} for i, st in saved.items()},
                                 "param_groups": [{k: x for k, x in g.items() if k != "moments"} for g in groups]})
        ids = [i for g in groups for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            if i in saved:
                st = self.state[p]
                if torch.is_tensor(st.get("step")):
                    st["step"] = st["step"].clone()          # torch hands a host ``step`` through as it is: never share it with the source
                st.update(self._convert_moments(p, saved[i]))
        self._tables.clear()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):
            self._tables.clear()

    def _ordered(self):
        """[(bucket or None, group, parameter)] in forward order (parameters the engine does not know first)."""
        rank, name = {}, {}
        for r, (bucket, plist) in enumerate(self.engine.forward_order()):
            for _, q in plist:
                rank[id(q)], name[id(q)] = r, bucket
        items = [(rank.get(id(p), -1), name.get(id(p)), g, p) for g in self.param_groups for p in g["params"]]
        items.sort(key=lambda it: it[0])
        return [(b, g, p) for _, b, g, p in items]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None, overlap: bool = False):
        """``grad_scale``: optional fp32 device scalar every gradient is multiplied by as it is read (the clip coefficient of
        ``dp.clip_grad_norm(..., defer=True)``): same update as ``grad.mul_(coef)`` + ``step()``; ``p.grad`` is left unscaled.
        ``overlap``: see the module docstring."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _l.load()
        overlap = bool(overlap) and self.engine is not None
        if grad_scale is not None and (not grad_scale.is_cuda or grad_scale.dtype != torch.float32 or grad_scale.numel() != 1):
            raise RuntimeError("grad_scale must be a one-element fp32 device tensor")
        gs_ptr = grad_scale.data_ptr() if grad_scale is not None else None
        order = self._ordered() if overlap else [(None, g, p) for g in self.param_groups for p in g["params"]]
        for _, _, p in order:                  # states first: their zero fills are ordered before the hand-over to the other stream
            if p.grad is None:
                continue
            if not p.is_cuda or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous() \
                    or not p.grad.is_contiguous():
                raise RuntimeError("FusedAdamW takes contiguous fp32 device parameters and gradients (no CPU fallback)")
            st = self.state[p]
            if len(st) == 0 and self._is8(p):
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                for k in ("exp_avg", "exp_avg_sq"):                          # the all-zero state of the format: codes 0, scale 1e-30 / 448
                    st[k + "_q"] = torch.zeros_like(p, dtype=torch.uint8, memory_format=torch.preserve_format)
                    st[k + "_scale"] = torch.full((p.numel() // BLOCK,), _ZERO_SCALE, dtype=torch.float32, device=p.device)
            elif len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)          # torch.optim.AdamW's (non-capturable) layout
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        cur = torch.cuda.current_stream()
        if overlap:
            if self._stream is None:
                self._stream = torch.cuda.Stream(priority=int(os.environ.get("A3V_ADAMW_STREAM_PRIO", "-1")))
            self.engine.sync_optimizer()                       # a previous overlapped step nobody consumed
            self._stream.wait_stream(cur)                      # gradients, states and the clip coefficient are ready
            if grad_scale is not None:
                grad_scale.record_stream(self._stream)
            stream = self._stream.cuda_stream
        else:
            stream = cur.cuda_stream
        written = set()
        written_t = set()
        adapters = set()
        last = None
        small = {}                             # id(group) -> [(p, sink)] handled by the multi-tensor launch (not with overlap: per-bucket events)
        if not overlap and self.multi_threshold > 0:
            for gi, group in enumerate(self.param_groups):
                lst = []
                for p in group["params"]:
                    if p.grad is None or p.numel() > self.multi_threshold:
                        continue
                    img = self.image_of(p) if self.image_of is not None else None
                    sink = None
                    if img is not None and self.engine is not None and hasattr(self.engine, "image_sink_t") and self.engine.image_sink_t(p) is not None:
                        continue                     # a matrix whose transposed image is in use: the per-tensor a3v_adamw_scaled_t launch below
                    if img is not None:
                        if img.dtype != torch.bfloat16 or img.shape != p.shape or not img.is_contiguous():
                            raise RuntimeError("image_of must return a contiguous bf16 tensor of the parameter's shape")
                        sink = (img.data_ptr(), p.shape[-1] if p.dim() > 1 else p.numel(), 1, 0, 0, 0)
                    elif self.engine is not None and hasattr(self.engine, "adapter_sink"):
                        sink = self.engine.adapter_sink(p)          # (d1, s1r, s1c, d2, s2r, s2c) inside the fused LoRA group images
                    st = self.state[p]
                    # a3v_adamw_multi does 16-byte vector accesses on p / g / m / v (and 8-byte ones on a contiguous image) through a table
                    # the C entry cannot check: anything misaligned or non-contiguous takes the per-tensor launch, which checks for itself
                    ok = all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (p, p.grad, st["exp_avg"], st["exp_avg_sq"]))
                    if img is not None and img.data_ptr() % 8:
                        ok = False
                    if not ok:
                        continue
                    lst.append((p, sink, img is not None))
                if len(lst) >= 2:
                    small[gi] = lst
        in_multi = {id(p) for lst in small.values() for p, _, _ in lst}
        # only adapters whose bf16 values the multi launch really writes into the fused images count as adopted by the engine
        adapters = {id(p) for lst in small.values() for p, sink, same in lst if sink is not None and not same}
        for bucket, group, p in order:
            if overlap and bucket != last:
                if last is not None:
                    self.engine._weights_ready[last] = self._stream.record_event()
                last = bucket
            if p.grad is None or id(p) in in_multi:
                continue
            b1, b2 = group["betas"]
            st = self.state[p]
            st["step"] += 1
            img = self.image_of(p) if self.image_of is not None else None
            if img is not None and (img.dtype != torch.bfloat16 or img.shape != p.shape or not img.is_contiguous()):
                raise RuntimeError("image_of must return a contiguous bf16 tensor of the parameter's shape")
            imgt = self.engine.image_sink_t(p) if (img is not None and self.engine is not None and hasattr(self.engine, "image_sink_t")) else None
            if "exp_avg_q" in st:
                if imgt is not None:
                    raise RuntimeError("FusedAdamW(moments='e4m3'): the engine keeps a transposed bf16 image of this matrix current in the "
                                       "optimizer pass (a3v_adamw_scaled_t), and that pass has no 8-bit form: build the engine in the NN "
                                       "input-gradient form (engine.nn_dgrad = True before the first step, or A3V_NN_DGRAD=1; "
                                       "main_finetune --adam8bit does)")
                rc = lib.a3v_adamw8_scaled(p.data_ptr(), p.grad.data_ptr(), st["exp_avg_q"].data_ptr(), st["exp_avg_scale"].data_ptr(),
                                           st["exp_avg_sq_q"].data_ptr(), st["exp_avg_sq_scale"].data_ptr(), p.numel(), float(group["lr"]),
                                           float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), int(st["step"].item()),
                                           img.data_ptr() if img is not None else None, gs_ptr, stream)
                _l.check(rc, "a3v_adamw8_scaled")
            elif imgt is not None and p.is_contiguous():
                # full fine-tune with input gradients on the NT kernel: the same pass also writes p's columns of the transposed image
                rc = lib.a3v_adamw_scaled_t(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                            p.shape[0], p.shape[1], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                            float(group["weight_decay"]), int(st["step"].item()), img.data_ptr(), imgt[0].data_ptr(),
                                            imgt[1], gs_ptr, stream)
                _l.check(rc, "a3v_adamw_scaled_t")
                written_t.add(id(p))
            else:
                rc = lib.a3v_adamw_scaled(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                                          float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                          int(st["step"].item()), img.data_ptr() if img is not None else None, gs_ptr, stream)
                _l.check(rc, "a3v_adamw_scaled")
            # the kernel wrote through raw pointers: tell autograd / version-keyed caches (the engine's bf16 weight images)
            torch.autograd.graph.increment_version(p)
            if img is not None:
                written.add(id(p))
        for gi, lst in small.items():
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            steps = set()
            for p, _, _ in lst:
                st = self.state[p]
                st["step"] += 1
                steps.add(int(st["step"].item()))
            if len(steps) != 1:
                raise RuntimeError("FusedAdamW multi-tensor launch: the small tensors of a param group must share their step count")
            # the table holds raw pointers of the moments too: load_state_dict() replaces those tensors
            key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(), sink)
                        for p, sink, _ in lst)
            ent = self._tables.get(gi)
            if ent is None or ent[0] != key:
                rows = []
                for p, sink, _ in lst:
                    st = self.state[p]
                    cols = p.shape[-1] if p.dim() > 1 else p.numel()
                    d = sink if sink is not None else (0, 0, 0, 0, 0, 0)
                    rows.append([p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), cols,
                                 d[0], d[1], d[2], d[3], d[4], d[5]])
                tab = torch.tensor(rows, dtype=torch.int64).to(lst[0][0].device)
                ent = self._tables[gi] = (key, tab, max(p.numel() for p, _, _ in lst))
            rc = lib.a3v_adamw_multi(ent[1].data_ptr(), len(lst), ent[2], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                     float(group["weight_decay"]), steps.pop(), gs_ptr, stream)
            _l.check(rc, "a3v_adamw_multi")
            for p, sink, same_shape in lst:
                torch.autograd.graph.increment_version(p)
                if same_shape:
                    written.add(id(p))
        if overlap:
            self.engine._weights_ready[last if last is not None else "head"] = self._stream.record_event()
        if self.engine is not None:
            if written_t:
                self.engine.images_adopted(written, written_t)
            else:
                self.engine.images_adopted(written)
            if adapters and hasattr(self.engine, "adapters_adopted"):
                self.engine.adapters_adopted(adapters)
        return loss
