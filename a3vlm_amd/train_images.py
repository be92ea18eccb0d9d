"""Compute-dtype operand images of the training step (``a3vlm_amd.train.TrainEngine``): the weight images of the decoder / head /
projector GEMMs (``_Images``; over an NF4 base ``_Nf4Images``, over an fp8 base ``_Fp8Images``) and the adapter images of a LoRA step (``_AdapterImages``), and the one
table of the decoder's four GEMM groups that they, the engine and the LoRA plugin share."""
from __future__ import annotations

from functools import reduce
from typing import Dict, Optional

import torch

from . import ops
from .util import optimizer_steps, param_state_key

# The four decoder GEMM kinds -> the modules that share the kind's input, in the row order of the fused image.  Module objects, base
# weights, adapter counts, parameter names and the first rows inside the fused image are all derived from this.
GROUPS = {"qkv": ("attention.wq", "attention.wk", "attention.wv"), "wo": ("attention.wo",),
          "w13": ("feed_forward.w1", "feed_forward.w3"), "w2": ("feed_forward.w2",)}


def group_modules(layer, kind: str) -> list:
    """The linear modules of decoder layer ``layer`` that make up GEMM group ``kind``."""
    return [reduce(getattr, name.split("."), layer) for name in GROUPS[kind]]


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


class _Images:
    """dict-like view of the engine's compute-dtype weight images, built per group on demand."""

    def __init__(self, eng: "TrainEngine"):
        self.eng = eng
        self.store: Dict[str, torch.Tensor] = {}
        self.ver: Dict[str, tuple] = {}
        self.tver: Dict[str, tuple] = {}      # version of each transposed image (built lazily, per key)
        self._sinks = None                    # id(param) -> (image key, first row), built on first use

    def _group(self, key: str):
        if key.split(".")[0] in GROUPS:
            return "L" + key.split(".")[1]
        return "vp" if key.startswith(("vp", "vq")) else "out"

    def _fused(self, ps):
        """The fused matrix of consecutive parameters: a VIEW of the flat parameter buffer under ZeRO-1 (always current, no copy: the
        image IS the parameter storage), else their concatenation."""
        v = self.eng._pview(list(ps)) if self.eng.zero1_world and not self.eng.lora else None
        if v is not None:
            return v
        return torch.cat(list(ps), dim=0) if len(ps) > 1 else ps[0]

    def _both(self, key, w):      # forward image W [N,K] now; W^T [K, N padded to 64] only when somebody asks for key + ".t"
        ext = self.eng._kext_cols(key)
        if ext:                   # LoRA inside the GEMMs: one [N + Rp, K + Rp] image = [[W, B], [A, 0]]; forward reads [W | B] (rows 0..N),
            N, K = w.shape        # the input gradient reads [W ; A] (columns 0..K); A / B blocks written by _lora_step_images / a3v_lora_refresh
            full = torch.zeros(N + ext, K + ext, dtype=self.eng.act, device=w.device)
            full[:N, :K] = w.to(self.eng.act)
            self.store[key] = full[:N, :K]
            self.store[key + ".x"] = full[:N]
            self.store[key + ".y"] = full[:, :K]
            if self.eng._nt_dgrad(key):
                # [W^T | A^T]  [K, N + Rp]: dx = [dy | dt] . (this)^T on the NT ring kernel; W is frozen, the A^T block is re-written
                # with the adapters (a3v_adamw_multi / a3v_lora_refresh)
                ft = torch.zeros(K, N + ext, dtype=self.eng.act, device=w.device)
                ft[:, :N] = full[:N, :K].t()
                self.store[key + ".yT"] = ft
        else:
            self.store[key] = w.to(self.eng.act).contiguous()

    def _transposed(self, key: str, ver) -> torch.Tensor:
        if self.tver.get(key) != ver:
            act = self.eng.act
            wa = self.store[key[:-2]]
            N, K = wa.shape
            Np = _pad64(N)
            if Np != N:
                wp = torch.zeros(Np, K, dtype=act, device=wa.device)
                wp[:N] = wa
            else:
                wp = wa
            wt = self.store.get(key)
            if wt is None or wt.shape != (K, Np) or wt.dtype != act:
                # row pitch off the powers of two: a3v_adamw_scaled_t writes 64 rows of this image per tile, and at an 8-KiB pitch they
                # all fall on the same HBM channels (w2 / wo at 7B: 281 vs 255 us per update)
                ld = Np + 64 if (Np * wa.element_size()) % 4096 == 0 else Np
                wt = torch.empty(K, ld, dtype=act, device=wa.device)[:, :Np]
            ops.transpose(wp, wt, Np, K, Np)
            self.store[key] = wt
            self.tver[key] = ver
        return self.store[key]

    def _params(self, g: str):
        """(parameters, [(image key, first row)] in the same order) of image group g."""
        m = self.eng.m
        if g.startswith("L"):
            i = int(g[1:])
            ws = {kind: [mod.weight for mod in group_modules(m.layers[i], kind)] for kind in GROUPS}
            return (tuple(w for g_ in ws.values() for w in g_),
                    tuple((f"{kind}.{i}", sum(w.shape[0] for w in g_[:j])) for kind, g_ in ws.items() for j in range(len(g_))))
        if g == "out":
            return (m.output.weight,), (("out", 0),)
        vp0 = getattr(m.visual_proj, "0")
        if getattr(m.args, "qformer_tokens", 0):
            qp0 = getattr(m.qformer_proj, "0")
            return (vp0.weight, vp0.bias, qp0.weight, qp0.bias), (("vp", 0), ("vp.b", 0), ("vq", 0), ("vq.b", 0))
        return (vp0.weight, vp0.bias), (("vp", 0), ("vp.b", 0))

    def _key(self, ps) -> tuple:
        return tuple(param_state_key(q) for q in ps) + (self.eng.act, str(self.eng.m._device))

    def groups(self):
        m = self.eng.m
        return [f"L{i}" for i in range(m.n_layers)] + ["out"] + (["vp"] if getattr(m, "visual_proj", None) is not None else [])

    def sink(self, p) -> Optional[torch.Tensor]:
        """bf16 destination of parameter p inside its (already built) forward image, or None."""
        if self.eng.act != torch.bfloat16:
            return None
        if self._sinks is None:
            self._sinks = {}
            for g in self.groups():
                ps, where = self._params(g)
                for q, (key, row) in zip(ps, where):
                    self._sinks[id(q)] = (key, row)
        ent = self._sinks.get(id(p))
        if ent is None:
            return None
        img = self.store.get(ent[0])
        if img is None or img.dtype != torch.bfloat16:
            return None
        return img[ent[1]:ent[1] + p.shape[0]] if img.dim() == 2 else img

    def sink_t(self, p):
        """(columns of parameter p inside the transposed image of its fused matrix [K, Np], Np) -- only once that image exists (the
        first backward built it) and p is a 64-aligned block of it."""
        if self.eng.act != torch.bfloat16 or p.dim() != 2 or (p.shape[0] & 63) or (p.shape[1] & 63):
            return None
        self.sink(p)                                   # (builds the parameter -> (key, row) map)
        ent = self._sinks.get(id(p))
        if ent is None or ent[0].endswith(".b"):
            return None
        wt = self.store.get(ent[0] + ".t")
        if wt is None or wt.dtype != torch.bfloat16 or wt.dim() != 2 or wt.shape[0] != p.shape[1] or ent[1] + p.shape[0] > wt.shape[1] \
                or (ent[1] & 3) or self.tver.get(ent[0] + ".t") is None:
            return None
        return wt[:, ent[1]:ent[1] + p.shape[0]], int(wt.stride(0))

    def adopted(self, written_ids, written_t_ids=()) -> None:
        """The optimizer wrote the bf16 values of these parameters into their images: groups written completely are current (and
        the transposed image of a fused matrix whose every parameter also went through ``a3v_adamw_scaled_t``)."""
        for g in self.groups():
            ps, where = self._params(g)
            if g in self.ver and all(id(q) in written_ids for q in ps):
                old = self.ver[g]
                self.ver[g] = self._key(ps)
                for key in {k for k, _ in where}:
                    if self.tver.get(key + ".t") == old and all(id(q) in written_t_ids for q, (k, _) in zip(ps, where) if k == key):
                        self.tver[key + ".t"] = self.ver[g]

    def recompute_backward(self, i: int) -> None:
        """Layer i is about to be recomputed and back-propagated (persistent images: nothing to prepare)."""

    def nbytes(self, head: bool = True) -> int:
        seen = {}
        for k, t in self.store.items():
            g = self._group(k)
            if g.startswith("L") or (head and g == "out"):
                st = t.untyped_storage()
                seen[st.data_ptr()] = st.nbytes()
        return sum(seen.values())

    def __getitem__(self, key: str) -> torch.Tensor:
        eng, g = self.eng, self._group(key)
        ps, _ = self._params(g)
        if g.startswith("L"):
            i = int(g[1:])
        ver = self._key(ps)
        if self.ver.get(g) != ver:
            with torch.no_grad():
                if g.startswith("L"):
                    n0 = 0
                    for kind, names in GROUPS.items():
                        self._both(f"{kind}.{i}", self._fused(ps[n0:n0 + len(names)]))
                        n0 += len(names)
                elif g == "out":
                    self._both("out", self._fused(ps[0:1]))
                else:
                    self._both("vp", ps[0])
                    self.store["vp.b"] = ps[1].to(eng.act)
                    if len(ps) == 4:
                        self._both("vq", ps[2])
                        self.store["vq.b"] = ps[3].to(eng.act)
            self.ver[g] = ver
        if key.endswith(".t"):
            return self._transposed(key, ver)
        return self.store[key]


class _Nf4Images(_Images):
    """The same keys over an NF4 base (QLoRA): ``qkv.i`` / ``wo.i`` / ``w13.i`` / ``w2.i`` (+ ``.x`` ``.y`` ``.yT`` ``.t``) are views of ONE
    scratch per group kind, shared by all layers and shaped exactly like the persistent images of the bf16 engine (so the GEMMs run
    the same plans on the same bits); ``out`` / ``out.t`` have a scratch of their own, filled once.  A request for another layer than the
    resident one drops the kind's contents; an orientation is filled on first request by a3v_dequantize_nf4_images (one call per original
    module, into its row / column window).  In the backward of a recomputed block the forward image and the transposed one are both
    needed: ``recompute_backward`` fills them by ONE call.  The dequantiser writes only the N x K window, so the adapter blocks in the tails survive a
    fill; they are copied there from the engine's persistent per-layer A / B / A^T images when the layer or the adapter version changed.
    The projector images (group ``vp``) are the parent's."""

    _TARGET = {"": "d", "x": "d", "y": "d", "yT": "yT", "t": "t"}

    def __init__(self, eng: "TrainEngine"):
        super().__init__(eng)
        assert eng.act == torch.bfloat16, "an NF4 base trains under --precision bf16 (the dequantised images are bf16)"
        self.kinds: Dict[str, dict] = {}

    def groups(self):                         # the parameter-backed groups (optimizer sinks, adoption): the projector only
        return ["vp"] if getattr(self.eng.m, "visual_proj", None) is not None else []

    def nbytes(self, head: bool = True) -> int:
        return sum(t.untyped_storage().nbytes() for kind, st in self.kinds.items() if head or kind != "out" for t in st["buf"].values())

    def _entries(self, kind: str, i: int):
        q4 = self.eng.m._q4
        return [q4["output"]] if kind == "out" else [q4[f"layers.{i}.{nm}"] for nm in GROUPS[kind]]

    def _state(self, kind: str, i: int) -> dict:
        """The scratch of a group kind, serving layer i from now on: another layer's contents are dropped."""
        st = self.kinds.get(kind)
        if st is None:
            ent = self._entries(kind, 0)
            st = self.kinds[kind] = dict(N=sum(e[2][0] for e in ent), K=ent[0][2][1], ext=self.eng._kext_cols(kind + ".0"), layer=None,
                                         valid=set(), tails={}, buf={})
        if st["layer"] != i:
            st["layer"], st["valid"], st["tails"] = i, set(), {}
        return st

    def _buffer(self, st: dict, target: str) -> torch.Tensor:
        b = st["buf"].get(target)
        if b is None:
            N, K, ext = st["N"], st["K"], st["ext"]
            dev = self.eng.m._device
            if target == "d":                 # [[W, B], [A, 0]] (or plain W): zero once, the corner and the pads are never written again
                b = torch.zeros(N + ext, K + ext, dtype=torch.bfloat16, device=dev)
            elif target == "yT":              # [W^T | A^T]
                b = torch.zeros(K, N + ext, dtype=torch.bfloat16, device=dev)
            else:                             # W^T [K, N padded to 64], row pitch as _Images._transposed
                Np = _pad64(N)
                ld = Np + 64 if (Np * 2) % 4096 == 0 else Np
                b = torch.zeros(K, ld, dtype=torch.bfloat16, device=dev)[:, :Np]
            st["buf"][target] = b
        return b

    def _fill(self, kind: str, i: int, st: dict, targets) -> None:
        wd = self._buffer(st, "d") if "d" in targets else None
        for tt in [t for t in ("yT", "t") if t in targets] or [None]:
            wt = self._buffer(st, tt) if tt is not None else None
            row = 0
            for q, sc, (n, k) in self._entries(kind, i):
                assert row % 8 == 0, "module rows must keep the 16-B alignment of the transposed window"
                ops.dequantize_nf4_images(q, sc, wd=None if wd is None else wd[row:row + n, :k],
                                          wt=None if wt is None else wt[:, row:row + n])
                row += n
            wd = None                          # (a second transposed target re-reads the codes; the forward image is written once)
        st["valid"] |= set(targets)

    def recompute_backward(self, i: int) -> None:
        """The backward of a recomputed block reads the forward image of each of its GEMMs, then the image of its input gradient:
        both orientations from one read of the codes.  (Only a saving: an orientation this misses is filled on its first request.)"""
        eng = self.eng
        with torch.no_grad():
            for kind in GROUPS:
                st = self._state(kind, i)
                if st["ext"]:
                    bwd = "yT" if eng._nt_dgrad(f"{kind}.{i}") else "d"
                else:
                    bwd = "d" if eng.nn_dgrad else "t"
                need = {"d", bwd} - st["valid"]
                if need:
                    self._fill(kind, i, st, need)

    def _place_tails(self, kind: str, i: int, st: dict, target: str) -> None:
        eng = self.eng
        li = eng._lora_step_images()
        ver = eng._li_ver
        # identity on purpose: _AdapterImages.images / .adopted bind a NEW tuple to the version whenever the adapters changed and keep
        # the same object otherwise; a miss only copies the blocks again
        if st["tails"].get(target) is ver:
            return
        N, K, ext = st["N"], st["K"], st["ext"]
        key = f"{kind}.{i}"
        if target == "d":
            full = st["buf"]["d"]
            full[:N, K:].copy_(li[key + ".B"])
            full[N:, :K].copy_(li[key + ".A"])
        else:
            st["buf"]["yT"][:, N:].copy_(li[key + ".At"][:K])
        st["tails"][target] = ver

    def __getitem__(self, key: str) -> torch.Tensor:
        if self._group(key) == "vp":
            return super().__getitem__(key)
        parts = key.split(".")
        if parts[0] == "out":
            kind, i, suffix = "out", 0, ".".join(parts[1:])
        else:
            kind, i, suffix = parts[0], int(parts[1]), ".".join(parts[2:])
        target = self._TARGET[suffix]
        eng = self.eng
        st = self._state(kind, i)
        with torch.no_grad():
            if target not in st["valid"]:
                self._fill(kind, i, st, {target})
            if st["ext"] and target in ("d", "yT"):
                self._place_tails(kind, i, st, target)
        b = st["buf"][target]
        N, K = st["N"], st["K"]
        if target != "d":
            return b
        return {"": b[:N, :K], "x": b[:N], "y": b[:, :K]}[suffix]


class _Fp8Images(_Images):
    """The same keys over an fp8 base (``quantize_base_weights("fp8")``): for each decoder group ``qkv.i`` / ``wo.i`` /
    ``w13.i`` / ``w2.i`` the model's persistent images -- ``.q`` Wq [N, K] e4m3 bytes, ``.s`` sw [N] fp32, ``.qT`` the byte transpose
    [K, N padded to 128] -- with no scratch and nothing to rebuild (the base is frozen and has no bf16 form); ``.one`` is a vector
    of K ones, the weight-side scale of the input-gradient GEMM (sw is folded into the gradient rows instead).  The head and the
    projector images (``out``, ``vp``) are the parent's."""

    _SLOT = {"q": 0, "s": 1, "qT": 2}

    def __init__(self, eng: "TrainEngine"):
        super().__init__(eng)
        assert eng.act == torch.bfloat16, "an fp8 base trains under --precision bf16"
        self.ones: Dict[int, torch.Tensor] = {}

    def groups(self):                         # the parameter-backed groups (optimizer sinks, adoption): the head and the projector
        return ["out"] + (["vp"] if getattr(self.eng.m, "visual_proj", None) is not None else [])

    def nbytes(self, head: bool = True) -> int:
        q8 = self.eng.m._q8base
        n = sum(t.untyped_storage().nbytes() for ent in q8.values() for t in ent)
        return n + (super().nbytes(True) if head else 0)

    def __getitem__(self, key: str) -> torch.Tensor:
        parts = key.split(".")
        if parts[0] not in GROUPS:
            return super().__getitem__(key)
        ent = self.eng.m._q8base[f"{parts[0]}.{parts[1]}"]
        if parts[2] == "one":
            K = ent[0].shape[1]
            one = self.ones.get(K)
            if one is None:
                one = self.ones[K] = torch.ones(K, dtype=torch.float32, device=ent[0].device)
            return one
        return ent[self._SLOT[parts[2]]]


class _AdapterImages:
    """The LoRA step's adapter images: per group A [Rp, in], B [N, Rp] and their transposes in the compute dtype, and everything the
    engine keeps about them -- when they were last validated, for which adapter values, and where the optimizer may write into them."""

    def __init__(self, eng):
        self.eng = eng
        self.li: Optional[Dict[str, torch.Tensor]] = None     # the images (key + ".A" / ".B" / ".At" / ".Bt")
        self.ver: Optional[tuple] = None      # adapter values they hold; a NEW tuple is bound only when the adapters changed (_Nf4Images._place_tails)
        self.act = None                       # compute dtype they were built for
        self.checked = False                  # validated for this forward / backward (the engine resets it at their entry)
        self.steps = -1                       # optimizer_steps() at that validation
        self.plist = None                     # the adapter parameters
        self.sinks = None                     # id(param) -> destination strides for FusedAdamW, built on first use

    def images(self):
        """A [Rp,in], B [N,Rp] (+ transposes for the backward GEMMs) of every adapter group in the compute dtype.  Built once;
        after an optimizer step only the r rows / columns each adapter owns are re-written in place (one a3v_lora_refresh
        launch per adapter) -- rebuilding the padded / block-diagonal images from scratch was ~2500 small launches per step."""
        eng, m = self.eng, self.eng.m
        if self.checked and self.steps == optimizer_steps():
            return self.li                                 # validated for this forward / backward, no step since
        self.steps = optimizer_steps()
        if self.plist is None:
            self.plist = [q for n, q in m.named_parameters() if "lora_" in n]
        ver = tuple(param_state_key(q) for q in self.plist)
        if self.ver == ver:
            self.checked = True
            return self.li
        li = self.li
        if li is not None and self.act == eng.act:
            r = m.lora_rank
            with torch.no_grad():
                for i in range(m.n_layers):
                    for key, mods, _ in m.lora_groups(i):
                        A, Bm, At, Bt = li[key + ".A"], li[key + ".B"], li[key + ".At"], li[key + ".Bt"]
                        row = 0
                        for j, mod in enumerate(mods):
                            wa, wb = mod.lora_a.weight, mod.lora_b.weight          # [r, in], [N_j, r]
                            nj = wb.shape[0]
                            if eng.act == torch.bfloat16 and wa.dtype == torch.float32 and wa.is_contiguous() and wb.is_contiguous():
                                ops.lora_refresh(wa, wb, A, At, Bm, Bt, j * r, row)
                            else:
                                A[j * r:(j + 1) * r].copy_(wa)
                                At[:wa.shape[1], j * r:(j + 1) * r].copy_(wa.t())
                                Bm[row:row + nj, j * r:(j + 1) * r].copy_(wb)
                                Bt[j * r:(j + 1) * r, row:row + nj].copy_(wb.t())
                            row += nj
            self.ver = ver
            self.checked = True
            return li
        src = m.lora_images(dtype=eng.act, interleave_w13=False)
        li = {}
        for k, v in src.items():
            li[k] = v.clone()              # the engine's own copies (updated in place from now on)
            R, C = v.shape
            vt = torch.empty(C, _pad64(R), dtype=v.dtype, device=v.device)
            if _pad64(R) != R:
                vp = torch.zeros(_pad64(R), C, dtype=v.dtype, device=v.device)
                vp[:R] = v
            else:
                vp = v
            ops.transpose(vp, vt, _pad64(R), C, _pad64(R))
            li[k + "t"] = vt
        if eng._kext() and not eng._q4base():
            # (NF4 base: every layer's images share one scratch, so the adapter blocks stay these persistent tensors -- the optimizer
            # sinks and a3v_lora_refresh write them -- and _Nf4Images copies them into the scratch tails of the layer it serves)
            im = eng._images()
            for i in range(m.n_layers):
                for key, _, _ in m.lora_groups(i):
                    fx, fy = im[key + ".x"], im[key + ".y"]   # [N, K + Rp] = [W | B],  [N + Rp, K] = [W ; A]
                    Rp = li[key + ".A"].shape[0]
                    blk = fx[:, fx.shape[1] - Rp:]
                    blk.copy_(li[key + ".B"])
                    li[key + ".B"] = blk                        # refreshed in place from now on (row stride K + Rp)
                    rows_a = fy[fy.shape[0] - Rp:]
                    rows_a.copy_(li[key + ".A"])
                    li[key + ".A"] = rows_a
                    if eng._nt_dgrad(key):
                        ft = im[key + ".yT"]                      # [K, N + Rp]: the A^T block lives in its tail columns
                        cols_at = ft[:, ft.shape[1] - Rp:]
                        cols_at.copy_(li[key + ".At"][:cols_at.shape[0]])
                        li[key + ".At"] = cols_at
        self.li, self.ver, self.act = li, ver, eng.act
        self.checked = True
        self.sinks = None
        return li

    def sink(self, p: torch.Tensor):
        """For ``FusedAdamW``'s multi-tensor launch: where the bf16 value of element (i, j) of adapter parameter ``p`` lives inside
        the fused group images, as (d1, s1r, s1c, d2, s2r, s2c) in element strides -- lora_a [r, in]: its rows of A and its columns
        of A^T; lora_b [n_j, r]: its columns of B and its rows of B^T.  None when ``p`` is not an adapter or the images are not
        built yet (first step: a3v_lora_refresh does it)."""
        li, m = self.li, self.eng.m
        if li is None or self.eng.act != torch.bfloat16 or self.act != self.eng.act:
            return None
        if self.sinks is None:
            self.sinks = {}
            r = m.lora_rank
            for i in range(m.n_layers):
                for key, mods, _ in m.lora_groups(i):
                    A, Bm, At, Bt = li[key + ".A"], li[key + ".B"], li[key + ".At"], li[key + ".Bt"]
                    row = 0
                    for j, mod in enumerate(mods):
                        wa, wb = mod.lora_a.weight, mod.lora_b.weight
                        self.sinks[id(wa)] = (A.data_ptr() + 2 * (j * r) * A.stride(0), A.stride(0), 1,
                                              At.data_ptr() + 2 * (j * r), 1, At.stride(0))
                        self.sinks[id(wb)] = (Bm.data_ptr() + 2 * (row * Bm.stride(0) + j * r), Bm.stride(0), 1,
                                              Bt.data_ptr() + 2 * ((j * r) * Bt.stride(0) + row), 1, Bt.stride(0))
                        row += wb.shape[0]
        return self.sinks.get(id(p))

    def adopted(self, written_ids) -> None:
        """The optimizer wrote every adapter's bf16 values into the group images itself: they are current for the new parameters."""
        if self.plist is None or self.li is None:
            return
        if all(id(q) in written_ids for q in self.plist if q.requires_grad):
            self.ver = tuple(param_state_key(q) for q in self.plist)
