"""The call trace of the training step: every ``a3vlm_amd.ops`` call ``TrainEngine`` makes, in order, with its operands' identities.

    python tools/train_step_trace.py --tsv ROWS.tsv                              (no GPU: every ops function is a recorder)
    python tools/train_step_trace.py --digests profiles/train_trace_NEW.tsv      (the committed form: six hex digits per row)
    python tools/train_step_trace.py --check profiles/train_trace_<sha>.tsv      (exit 1 and the first differing row per case)

Each case of cases() builds a tiny model on the CPU, replaces every public function of ``a3vlm_amd.ops`` with a recorder and drives
``forward_loss`` + ``backward(1.0)``, touches every trainable parameter in place (as an optimizer step would), then ``forward_loss`` +
``backward(0.5)`` -- the second step shows the "accumulate" side of the weight-gradient GEMMs and the refresh of the adapter images.
With the kernels stubbed the step's control flow depends on no value, so the table is the host side of the step and nothing else.

One line per call: the op name, then its arguments in the order of the op's signature (one at its default is left out, and those
after it and the keyword-only ones are written ``name=value``).  A tensor is ``dtype[shape;strides]@s+o`` (strides
only when not contiguous): ``s`` is the ordinal of its storage by first appearance inside the case, ``o`` the storage offset in
elements -- machine-independent, and still different for a wrong view, a wrong buffer tag or a lost alias.  ``img[] key`` and
``recompute_backward i`` lines are the requests to the engine's weight images (over an NF4 base: the scratch's fill / evict order).

tests/test_train_trace_cpu.py holds the engine to the committed table, row for row.  The table is made from the commit in its name
and keeps a digest per row; a row that differs afterwards is a change of the launch sequence -- to see it whole, write --tsv from
both commits and diff the two files.
"""
from __future__ import annotations

import argparse
import hashlib
import inspect
import os
import sys
from contextlib import contextmanager

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DIM, LAYERS, HEADS, KV, VOCAB, MULT, B, T = 256, 2, 4, 2, 320, 256, 3, 47          # 141 rows: ragged against 64 and 128; head_dim 64
SWITCHES = ("fuse_qkv_rope", "tn_wgrad", "nn_dgrad", "packed_attn_bwd", "lora_kext", "lora_nt_dgrad", "strip_wgrad", "fuse_swiglu_bwd")
_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.int64: "i64", torch.int32: "i32", torch.uint8: "u8", torch.float16: "f16",
       torch.bool: "b8", torch.int8: "i8", torch.int16: "i16", torch.float64: "f64"}


def cases():
    """(name, spec): spec keys -- model: full | lora | visual | two_image | qformer | nf4; dtype; rank; heads (head_dim = DIM / heads);
    recompute; stream; zero1; free_gib (what the stubbed mem_get_info reports); every other key is a TrainEngine switch."""
    out = []

    def add(name, model, dtype="bf16", recompute=False, **kw):
        out.append((name, dict(model=model, dtype=dtype, recompute=recompute, **kw)))

    add("full", "full")
    add("full.nn_dgrad", "full", nn_dgrad=True)
    add("full.nt_dgrad", "full", nn_dgrad=False)
    add("full.no_swiglu_bwd", "full", fuse_swiglu_bwd=False)
    add("full.nn_dgrad.no_swiglu_bwd", "full", nn_dgrad=True, fuse_swiglu_bwd=False)
    add("full.no_tn_wgrad", "full", tn_wgrad=False)
    add("full.no_packed_attn_bwd", "full", packed_attn_bwd=False)
    add("full.no_fuse_qkv_rope", "full", fuse_qkv_rope=False)
    add("full.recompute", "full", recompute=True)
    add("full.stream_f32", "full", stream="f32")
    add("full.hd32", "full", heads=8)
    add("full.low_hbm", "full", free_gib=1)
    add("full.f32", "full", dtype="f32")
    add("lora.r8", "lora", rank=8)
    add("lora.r24", "lora", rank=24)
    add("lora.no_kext", "lora", rank=8, lora_kext=False)
    add("lora.no_kext.no_fuse_qkv_rope", "lora", rank=8, lora_kext=False, fuse_qkv_rope=False)
    add("lora.nt_dgrad_0", "lora", rank=8, lora_nt_dgrad="0")
    add("lora.nt_dgrad_wo_w2", "lora", rank=8, lora_nt_dgrad="wo,w2")
    add("lora.no_strip_wgrad", "lora", rank=8, strip_wgrad=False)
    add("lora.no_swiglu_bwd", "lora", rank=8, fuse_swiglu_bwd=False)
    add("lora.no_packed_attn_bwd", "lora", rank=8, packed_attn_bwd=False)
    add("lora.recompute", "lora", rank=8, recompute=True)
    add("lora.stream_f32", "lora", rank=8, stream="f32")
    add("lora.hd32", "lora", rank=8, heads=8)
    add("lora.low_hbm", "lora", rank=8, free_gib=1)
    add("lora.f32", "lora", rank=8, dtype="f32")
    add("visual.lora", "visual", rank=8)
    add("visual.full", "visual", rank=0)
    add("two_image.full", "two_image", rank=0)
    add("qformer.full", "qformer", rank=0)
    add("zero1", "full", zero1=2)
    add("nf4", "nf4", rank=8)
    add("nf4.recompute", "nf4", rank=8, recompute=True)
    add("nf4.nt_dgrad_0", "nf4", rank=8, lora_nt_dgrad="0")
    add("nf4.nt_dgrad_0.recompute", "nf4", rank=8, lora_nt_dgrad="0", recompute=True)
    add("nf4.no_kext.recompute", "nf4", rank=8, lora_kext=False, recompute=True)
    return out


def label_rows_cases():
    """The cases of the second table (profiles/label_rows_trace_<sha>.tsv, tests/test_label_rows_trace_cpu.py): engines with
    ``label_rows`` on -- the last block's wo / FFN branch, the final norm, the head and the loss on the labelled rows -- and the
    engines that fall back to every row (recompute, fp32 stream, ZeRO-1: their rows are those of the first table)."""
    out = []

    def add(name, model, dtype="bf16", recompute=False, **kw):
        out.append((name, dict(model=model, dtype=dtype, recompute=recompute, label_rows=True, **kw)))

    add("lora.r8", "lora", rank=8)
    add("lora.r24", "lora", rank=24)
    add("lora.no_kext", "lora", rank=8, lora_kext=False)
    add("lora.nt_dgrad_0", "lora", rank=8, lora_nt_dgrad="0")
    add("lora.no_swiglu_bwd", "lora", rank=8, fuse_swiglu_bwd=False)
    add("lora.no_strip_wgrad", "lora", rank=8, strip_wgrad=False)
    add("visual.lora", "visual", rank=8)
    add("nf4", "nf4", rank=8)
    add("full", "full")
    add("full.nn_dgrad", "full", nn_dgrad=True)
    add("lora.recompute", "lora", rank=8, recompute=True)
    add("lora.stream_f32", "lora", rank=8, stream="f32")
    add("zero1", "full", zero1=2)
    add("lora.no_packed_attn_bwd", "lora", rank=8, packed_attn_bwd=False)
    add("lora.no_kext.no_fuse_qkv_rope", "lora", rank=8, lora_kext=False, fuse_qkv_rope=False)
    add("lora.hd32", "lora", rank=8, heads=8)
    add("lora.nt_dgrad_wo_w2", "lora", rank=8, lora_nt_dgrad="wo,w2")
    add("lora.low_hbm", "lora", rank=8, free_gib=1)
    add("nf4.nt_dgrad_0", "nf4", rank=8, lora_nt_dgrad="0")
    return out


CASE_SETS = {"step": cases, "label_rows": label_rows_cases}


# ---------------------------------------------------------------------------------------------------------------- the recorder
class Recorder:
    def __init__(self):
        self.lines = []
        self.ids = {}
        self.keep = []           # storages stay alive: an address is never handed out twice inside a case

    def tensor(self, t):
        st = t.untyped_storage()
        s = self.ids.get(st.data_ptr())
        if s is None:
            s = self.ids[st.data_ptr()] = len(self.ids)
            self.keep.append(st)
        dims = ",".join(map(str, t.shape))
        if not t.is_contiguous():
            dims += ";" + ",".join(map(str, t.stride()))
        return f"{_DT.get(t.dtype, str(t.dtype))}[{dims}]@{s}+{t.storage_offset()}"

    def value(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, (list, tuple)):
            return "(" + " ".join(self.value(x) for x in v) + ")"
        if isinstance(v, torch.dtype):
            return _DT.get(v, str(v))
        if isinstance(v, float):
            return repr(v)
        return str(v)

    def call(self, name, sig, args, kwargs):
        ba = sig.bind(*args, **kwargs)
        ba.apply_defaults()
        cols, named = [name], False
        for k, v in ba.arguments.items():
            par = sig.parameters[k]
            if not isinstance(v, torch.Tensor) and par.default is not par.empty and v == par.default:
                named = True                           # left out: an argument at its default; the ones after it carry their names
                continue
            named = named or par.kind is par.KEYWORD_ONLY
            cols.append(f"{k}={self.value(v)}" if named else self.value(v))
        self.lines.append("\t".join(cols))
        return ba.arguments


def _n_labelled(a):
    from a3vlm_amd.train import label_rows_ref
    return int(label_rows_ref(a["labels"], a["W"], a["S"])[0].numel())


_RETURNS = {"label_rows": _n_labelled, "attention_bwd_workspace_bytes": lambda a: 64 * a["B"] * a["H"] * a["S"], "gemm_tn_sumsq_slots": lambda a: 4,
            "attention_scratch_floats": lambda a: 64, "gemm_skinny_split": lambda a: 1, "gemm_skinny_ws_bytes": lambda a: 64}


@contextmanager
def stubbed(rec: Recorder, free_gib: int):
    """Every public function of a3vlm_amd.ops records instead of launching; the torch.cuda queries the step makes answer fixed values."""
    from a3vlm_amd import ops
    saved = {}
    for name, fn in list(vars(ops).items()):
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__ or name == "dt":
            continue
        saved[name] = fn

        def stub(*args, _name=name, _sig=inspect.signature(fn), **kwargs):
            a = rec.call(_name, _sig, args, kwargs)
            if _name in _RETURNS:
                return _RETURNS[_name](a)
            return a.get("out")
        setattr(ops, name, stub)
    cuda = {k: getattr(torch.cuda, k) for k in ("mem_get_info", "memory_reserved", "memory_allocated")}
    torch.cuda.mem_get_info = lambda *a, **k: (free_gib << 30, 288 << 30)
    torch.cuda.memory_reserved = torch.cuda.memory_allocated = lambda *a, **k: 0
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        for k, v in cuda.items():
            setattr(torch.cuda, k, v)


def watch_images(rec: Recorder, eng):
    """Record the requests to the engine's weight images (every class of the object's MRO that defines the method: super() calls too)."""
    img = eng._images()
    undo = []
    for cls in type(img).__mro__[:-1]:
        for meth, label in (("__getitem__", "img[]"), ("recompute_backward", "recompute_backward")):
            fn = cls.__dict__.get(meth)
            if fn is None:
                continue

            def wrapped(self, arg, _fn=fn, _label=label):
                rec.lines.append(f"{_label}\t{arg}")
                return _fn(self, arg)
            setattr(cls, meth, wrapped)
            undo.append((cls, meth, fn))
    return undo


# ---------------------------------------------------------------------------------------------------------------- the models
def _fake_nf4(m):
    """What ``quantize_base_weights("nf4")`` leaves behind, with empty codes: that method insists on bf16 weights on a GPU and sizes its
    workspace through the library; the step only looks at the shapes of the codes and scales."""
    q4 = {}
    named = [(f"layers.{i}.{grp}.{n}", getattr(getattr(lyr, grp), n)) for i, lyr in enumerate(m.layers)
             for grp, ns in (("attention", ("wq", "wk", "wv", "wo")), ("feed_forward", ("w1", "w3", "w2"))) for n in ns]
    for name, mod in named + [("output", m.output)]:
        N, K = mod.weight.shape
        mod.q4 = q4[name] = (torch.empty(N, K // 2, dtype=torch.uint8), torch.empty(N, K // 64, dtype=torch.float32), (N, K))
        del mod.weight
    m._q4 = q4
    m._packed, m._packed_version, m._lora_ver = {}, None, None


def build(spec):
    from a3vlm_amd.util import promote_trainable_params_to_fp32
    kind, rank = spec["model"], int(spec.get("rank", 0))
    dtype = torch.bfloat16 if spec["dtype"] == "bf16" else torch.float32
    base = dict(dim=DIM, n_layers=LAYERS, n_heads=spec.get("heads", HEADS), n_kv_heads=KV, vocab_size=VOCAB, multiple_of=MULT, max_seq_len=512)
    vit = dict(vit_width=64, vit_layers=2, vit_heads=4, vit_crop=112, n_views=1)
    torch.manual_seed(0)
    if kind == "two_image":
        from a3vlm_amd.model.LLM import llama_ens5_2images as plugin
        m = plugin.Transformer(plugin.ModelArgs(**base, **vit, **({"lora_rank": rank} if rank else {})), with_visual=True)
    elif kind in ("visual", "qformer"):
        from a3vlm_amd.model.LLM import llama_ens5 as full, llama_ens5_peft as peft
        plugin = peft if rank else full
        extra = dict(qformer_tokens=4) if kind == "qformer" else {}
        m = plugin.Transformer(plugin.ModelArgs(**base, **vit, **extra, **({"lora_rank": rank} if rank else {})), with_visual=True)
    elif kind in ("lora", "nf4"):
        from a3vlm_amd.model.LLM import llama_ens5_peft as peft
        m = peft.Transformer(peft.ModelArgs(**base, lora_rank=rank))
    else:
        from a3vlm_amd.model.LLM import llama_ens5 as full
        m = full.Transformer(full.ModelArgs(**base))
    train = m.get_trainable_params()
    for n, p in m.named_parameters():
        p.requires_grad = n in train
    m.to(dtype)
    promote_trainable_params_to_fp32(m, keep_matrices_sharded=bool(spec.get("zero1")))
    if kind == "nf4":
        _fake_nf4(m)
    return m, dtype


def trace(spec):
    """The row list of one case."""
    from a3vlm_amd.train import TrainEngine
    rec = Recorder()
    m, dtype = build(spec)
    with stubbed(rec, int(spec.get("free_gib", 200))):
        stream = {"f32": torch.float32, "bf16": torch.bfloat16, None: None}[spec.get("stream")]
        eng = TrainEngine(m, dtype, recompute=bool(spec["recompute"]), stream_dtype=stream, zero1_world=int(spec.get("zero1", 0)))
        for k in SWITCHES:
            if k in spec:
                setattr(eng, k, spec[k])
        eng.label_rows = bool(spec.get("label_rows", False))     # the first table's engines run every row, as when it was recorded
        undo = watch_images(rec, eng)
        try:
            g = torch.Generator().manual_seed(1)
            ex = torch.randint(3, VOCAB, (B, T), generator=g)
            lab = ex.clone()
            lab[:, :5] = 0
            image, kw = None, {}
            if spec["model"] in ("visual", "two_image", "qformer"):
                image = torch.zeros(B, 3, 112, 112, dtype=dtype)
                if spec["model"] == "two_image":
                    image = [image, image.clone()]
                if spec["model"] == "qformer":
                    kw["qformer_feats"] = torch.zeros(B, 4, 768, dtype=dtype)
            for step, scale in enumerate((1.0, 0.5)):
                rec.lines.append(f"# step {step}")
                eng.forward_loss(ex, lab, image, **kw)
                eng.backward(scale)
                with torch.no_grad():
                    for p in m.parameters():
                        if p.requires_grad:
                            p.add_(0)                  # an optimizer step's version bump: the images are rebuilt / refreshed
        finally:
            for cls, meth, fn in undo:
                setattr(cls, meth, fn)
    return rec.lines


def digest(row: str) -> str:
    """Six hex digits of a row: what the committed table keeps of it (the rows themselves are some 800 kB)."""
    return hashlib.sha1(row.encode()).hexdigest()[:6]


def table(digests: bool = False, case_set: str = "step"):
    lines = ["# digests"] if digests else []
    for name, spec in CASE_SETS[case_set]():
        lines.append(f"## {name}\t" + " ".join(f"{k}={v}" for k, v in spec.items()))
        rows = trace(spec)
        lines += [" ".join(map(digest, rows[j:j + 32])) for j in range(0, len(rows), 32)] if digests else rows
    return lines


def read_table(path):
    """{case: [digest of each row]} of a table in either form (--tsv or --digests), in file order."""
    out, cur = {}, None
    lines = open(path).read().splitlines()
    digests = lines[:1] == ["# digests"]
    for ln in lines[1:] if digests else lines:
        if ln.startswith("## "):
            cur = out.setdefault(ln[3:].split("\t")[0], [])
        else:
            cur += ln.split() if digests else [digest(ln)]
    return out


def first_difference(rows, want):
    """Index of the first row whose digest is not the table's (None: identical)."""
    got = list(map(digest, rows))
    if got == want:
        return None
    return next((j for j, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tsv", help="write every row of every case (to read, and to diff against the same from another commit)")
    ap.add_argument("--digests", help="write the committed form: per case, six hex digits per row")
    ap.add_argument("--check", metavar="TABLE", help="compare this tree with a table of either form")
    ap.add_argument("--cases", choices=sorted(CASE_SETS), default="step", help="which table: the step's (default) or the label-rows engines'")
    a = ap.parse_args()
    cases = CASE_SETS[a.cases]
    if a.tsv or a.digests:
        with open(a.tsv or a.digests, "w") as f:
            f.write("\n".join(table(digests=bool(a.digests), case_set=a.cases)) + "\n")
        return 0
    want = read_table(a.check)
    bad = 0
    for name, spec in cases():
        rows = trace(spec)
        j = first_difference(rows, want.get(name) or [])
        if j is not None:
            bad += 1
            print(f"{name}: row {j} of {len(rows)} (table: {len(want.get(name) or [])})\n  got  {rows[j] if j < len(rows) else '-'}")
    print(f"{len(cases()) - bad} of {len(cases())} cases identical")
    return 1 if bad or list(want) != [n for n, _ in cases()] else 0


if __name__ == "__main__":
    sys.exit(main())
