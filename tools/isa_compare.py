#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of liba3vlm_hip.so (runs without a GPU).

usage: tools/isa_compare.py OLD.so NEW.so [--map FILE] [--counts PATTERN]

Every code object of the .hip_fatbin section is taken apart; per kernel the instruction bytes (from the kernel's own start, so
placement does not matter: branches are pc-relative) and the 64-byte kernel descriptor (without its entry-offset field) are
compared.  Kernels are matched by demangled name; --map names a file of `old demangled name<TAB>new demangled name` lines for
kernels whose template arguments were renamed.  Kernels that differ are listed with their register / LDS / scratch / kernarg
figures and, with --counts, the number of MFMA, LDS-DMA, ds_read_b128 and s_barrier instructions of the kernels whose name
contains PATTERN.  Exit status 0 only if every kernel has an identical partner."""
import os, re, shutil, struct, subprocess, sys, tempfile
from collections import Counter

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
COUNTED = (("mfma", r"^v_mfma"), ("lds_dma", r"^(global_load_lds|buffer_load_\S+ .*\blds\b)"), ("ds_read_b128", r"^ds_read_b128"), ("s_barrier", r"^s_barrier"))


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    fb = os.path.join(tmp, "fb.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", lib, os.devnull], check=True)
    d = open(fb, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    for n, at in enumerate(m.start() for m in re.finditer(magic, d)):
        cnt, = struct.unpack_from("<Q", d, at + 24)
        pos = at + 32
        for _ in range(cnt):
            off, size, tl = struct.unpack_from("<QQQ", d, pos)
            triple = d[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if "gfx" in triple and size:
                path = os.path.join(tmp, f"co{n}.elf")
                open(path, "wb").write(d[at + off:at + off + size])
                yield path


def kernels(lib):
    """demangled name -> dict(text=bytes, kd=bytes, dis=[instructions])"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            raw = open(co, "rb").read()
            secs = {}   # index -> (addr, file offset)
            for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", "-W", co), re.M):
                secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
            syms = {}
            for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+(\d+)\s+(\S+)$", run(f"{LLVM}/llvm-readelf", "-s", "-W", co), re.M):
                addr, size, typ, shndx, name = int(m.group(1), 16), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5)
                sa, so = secs[shndx]
                syms[name] = raw[so + addr - sa:so + addr - sa + size]
            dis = {}
            for m in re.finditer(r"^(?:[0-9a-f]+ )?<(\S+)>:\n(.*?)(?=^\S|\Z)", run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co), re.S | re.M):
                dis[m.group(1)] = [re.sub(r"\s*//.*", "", l).strip() for l in m.group(2).split("\n") if l.strip()]
            names = [n[:-3] for n in syms if n.endswith(".kd")]
            filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
            dem = subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
            for n, dn in zip(names, dem):
                kd = syms[n + ".kd"]
                assert len(kd) == 64 and dn not in out, dn
                out[dn] = dict(text=syms[n], kd=kd[:16] + kd[24:], dis=dis[n])
    return out


def figures(k):
    kd = k["kd"]   # entry offset (bytes 16..23) already cut out: rsrc3 / rsrc1 / rsrc2 sit at 36 / 40 / 44 of what is left
    lds, scratch, kernarg = struct.unpack_from("<III", kd, 0)
    rsrc3, rsrc1 = struct.unpack_from("<II", kd, 36)
    regs = ((rsrc1 & 0x3f) + 1) * 8            # unified VGPR + AGPR allocation (granule 8)
    accum = ((rsrc3 & 0x3f) + 1) * 4           # first AGPR = number of arch VGPRs allocated
    return dict(vgpr=accum, agpr=regs - accum, sgpr_blocks=(rsrc1 >> 6) & 0xf, lds=lds, scratch=scratch, kernarg=kernarg)


def counts(k):
    c = Counter()
    for ins in k["dis"]:
        for key, pat in COUNTED:
            if re.match(pat, ins): c[key] += 1
    return {key: c[key] for key, _ in COUNTED}


def main():
    args = sys.argv[1:]
    opt = {}
    for o in ("--map", "--counts"):
        if o in args:
            i = args.index(o); opt[o] = args[i + 1]; del args[i:i + 2]
    old, new = kernels(args[0]), kernels(args[1])
    ren = dict(l.rstrip("\n").split("\t") for l in open(opt["--map"]) if "\t" in l) if "--map" in opt else {}
    same = 0
    for dn, k in sorted(old.items()):
        nn = ren.get(dn, dn)
        if nn not in new:
            print("NO PARTNER (old)", dn); continue
        n = new.pop(nn)
        ident = n["text"] == k["text"] and n["kd"] == k["kd"]
        same += ident
        if not ident or (opt.get("--counts") and opt["--counts"] in dn):
            print("identical" if ident else "DIFFERENT", nn)
            print("   old", len(k["dis"]), "instr", figures(k), counts(k))
            print("   new", len(n["dis"]), "instr", figures(n), counts(n))
    for nn in new: print("NO PARTNER (new)", nn)
    print(f"{same} of {len(old)} kernels identical; {len(new)} new kernels without a partner")
    return 0 if same == len(old) and not new else 1


if __name__ == "__main__":
    sys.exit(main())
