"""CPU: the NF4 weight format (tests/nf4_ref.py, include/a3vlm_hip.h a3v_quantize_nf4) and the pieces of the NF4 decode GEMV that
can be checked without a GPU: the code-book byte tables and selector arithmetic of its v_perm_b32 lookup (emulated), and the scratch
budget of its instantiations."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import nf4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_tables():
    t = R.NF4
    assert t.numel() == 16 and bool((t[1:] > t[:-1]).all()) and t[7] == 0 and t[0] == -1 and t[15] == 1
    m = R.dynamic_map()
    assert m.numel() == 256 and bool((m[1:] > m[:-1]).all())
    assert bool((m == 0).any()) and bool((m == 1).any())
    assert float(m.min()) > -1 and float(m.abs()[m != 0].min()) < 1e-6


def test_nibble_order_and_roundtrip_of_the_packing():
    q = torch.tensor([[1, 2, 15, 0, 7, 8, 3, 12]])
    b = R.pack_nibbles(q)
    assert b.tolist() == [[0x12, 0xF0, 0x78, 0x3C]]          # earlier element in the high nibble
    assert torch.equal(R.unpack_nibbles(b), q)


def test_zero_block_rule():
    w = torch.randn(2, 128).to(torch.bfloat16)
    w[1, 64:] = 0
    nib, s, _ = R.quantize(w)
    assert float(s[1, 1]) == 0.0
    assert bool((R.unpack_nibbles(nib)[1, 64:] == 7).all())
    assert bool((R.dequantize(nib, s)[1, 64:] == 0).all())
    assert float(s[0, 0]) > 0


def test_nearest_code_at_the_midpoint_thresholds():
    t = R.NF4
    xs, want = [], []
    for i in range(15):
        mid = float((t[i] + t[i + 1]) / 2)
        for d, j in ((-2e-3, i), (2e-3, i + 1)):
            xs.append(mid + d)
            want.append(j)
    xs += [-1.0, 1.0, 0.0]
    want += [0, 15, 7]
    n = len(xs)
    w = torch.zeros(1, 64)
    w[0, :n] = torch.tensor(xs)
    w[0, 63] = 1.0                                            # absmax 1: the scaled value is the weight itself
    q = R.quantize_codes(w.to(torch.float32))
    assert q[0, :n].tolist() == want


def test_quantise_dequantise_error_bound():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 1024, generator=g) * 0.05).to(torch.bfloat16)
    w[3, 128:192] *= 40                                       # an outlier block
    nib, s, off = R.quantize(w)
    q = R.unpack_nibbles(nib)
    wd = R.dequantize(nib, s).float()
    t = R.NF4
    gap = torch.maximum(t[1:] - t[:-1], torch.zeros(15))
    half_gap = torch.zeros(16)
    half_gap[:15] = gap / 2
    half_gap[1:] = torch.maximum(half_gap[1:], gap / 2)
    sb = s.repeat_interleave(64, dim=1)
    am = R.absmax_blocks(w).reshape(64, -1).repeat_interleave(64, dim=1)
    # first level exact: |w - NF4[q] absmax| <= half the code gap x absmax; second level: s_b replaces absmax
    err1 = (w.float() - t[q] * am).abs()
    assert bool((err1 <= half_gap[q] * am * (1 + 1e-6) + 1e-12).all())
    err = (w.float() - wd).abs()
    bound = half_gap[q] * torch.maximum(sb, am) + (sb - am).abs() + wd.abs() * 2 ** -8
    assert bool((err <= bound * (1 + 1e-6)).all())
    assert float((sb - am).abs().max() / am.max()) < 1e-2     # the 8-bit double quantisation of the block scales
    assert abs(off - float(R.absmax_blocks(w).mean())) <= 1e-6 * off


def test_per_module_quantisation_then_row_packing_equals_packed_wd():
    g = torch.Generator().manual_seed(1)
    wq, wk, wv = [(torch.randn(n, 512, generator=g) * 0.02).to(torch.bfloat16) for n in (512, 256, 256)]
    w1, w3 = [(torch.randn(768, 512, generator=g) * 0.02).to(torch.bfloat16) for _ in range(2)]
    imgs = {k: R.quantize(w)[:2] for k, w in dict(wq=wq, wk=wk, wv=wv, w1=w1, w3=w3).items()}
    qkv_n = torch.cat([imgs[k][0] for k in ("wq", "wk", "wv")])
    qkv_s = torch.cat([imgs[k][1] for k in ("wq", "wk", "wv")])
    want = torch.cat([R.dequantize(*imgs[k]) for k in ("wq", "wk", "wv")])
    assert torch.equal(R.dequantize(qkv_n, qkv_s), want)
    n13 = R.pack_w13_rows(imgs["w1"][0], imgs["w3"][0])
    s13 = R.pack_w13_rows(imgs["w1"][1], imgs["w3"][1])
    assert torch.equal(R.dequantize(n13, s13), R.pack_w13_rows(R.dequantize(*imgs["w1"]), R.dequantize(*imgs["w3"])))
    # the double-quant groups are those of the original modules: quantising the packed matrix is NOT the same image
    assert not torch.equal(R.quantize(torch.cat([wq, wk, wv]))[1], qkv_s)


def _perm(s0: int, s1: int, sel: int) -> int:
    """v_perm_b32 for selectors 0..7: byte i of the result = byte sel_i of {s0, s1} (s1 = bytes 0..3)."""
    data = (s0 << 32) | s1
    out = 0
    for i in range(4):
        k = (sel >> (8 * i)) & 0xFF
        assert k < 8
        out |= ((data >> (8 * k)) & 0xFF) << (8 * i)
    return out


def _gemv_tables():
    src = open(os.path.join(ROOT, "a3vlm_amd", "csrc", "a3v_gemv.hip")).read()
    body = src[src.index("bf16x8 nf4_bf16x8(uint32_t x)"):]
    body = body[:body.index("return __builtin_bit_cast(bf16x8, r)")]
    he = re.search(r"he = look\(ie, me, (0x\w+)u, (0x\w+)u, (0x\w+)u, (0x\w+)u\)", body).groups()
    le = re.search(r"le = look\(ie, me, (0x\w+)u, (0x\w+)u, (0x\w+)u, (0x\w+)u\)", body).groups()
    return [int(v, 16) for v in he], [int(v, 16) for v in le]


def test_gemv_code_book_lookup_emulated():
    """nf4_bf16x8 (a3v_gemv.hip) restated with its own constants: every code in every position gives bf16(NF4[code])."""
    (h0a, h0b, h1a, h1b), (l0a, l0b, l1a, l1b) = _gemv_tables()
    M = 0xFFFFFFFF

    def look(i, m, t0a, t0b, t1a, t1b):
        return (_perm(t1b, t1a, i) & m) | (_perm(t0b, t0a, i) & ~m & M)

    def deq(x):
        io, ie = x & 0x07070707, (x >> 4) & 0x07070707
        mo, me = ((x >> 3) & 0x01010101) * 0xFF, ((x >> 7) & 0x01010101) * 0xFF
        he, le = look(ie, me, h0a, h0b, h1a, h1b), look(ie, me, l0a, l0b, l1a, l1b)
        ho, lo = look(io, mo, h0a, h0b, h1a, h1b), look(io, mo, l0a, l0b, l1a, l1b)
        e01, e23 = _perm(he, le, 0x05010400), _perm(he, le, 0x07030602)
        o01, o23 = _perm(ho, lo, 0x05010400), _perm(ho, lo, 0x07030602)
        r = [_perm(o01, e01, 0x05040100), _perm(o01, e01, 0x07060302), _perm(o23, e23, 0x05040100), _perm(o23, e23, 0x07060302)]
        return [(d >> (16 * h)) & 0xFFFF for d in r for h in range(2)]
    bits = [int(v) & 0xFFFF for v in R.NF4.to(torch.bfloat16).view(torch.int16).tolist()]
    g = torch.Generator().manual_seed(5)
    words = [int(v) for v in torch.randint(0, 2 ** 32, (200,), generator=g, dtype=torch.int64)]
    words += [sum(c << (4 * j) for j in range(8)) for c in range(16)]          # every code in every nibble
    for x in words:
        codes = [(x >> (8 * (e // 2) + (4 if e % 2 == 0 else 0))) & 15 for e in range(8)]   # element e: byte e/2, even = high nibble
        assert deq(x) == [bits[c] for c in codes], hex(x)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_nf4_gemv_instantiations_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "a3vlm_amd", "csrc", "a3v_gemv.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "g.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    n4 = {n: v for n, v in scratch.items() if "gemv_dma_bf16_kernel" in n and n.endswith("ELb1EEEvNS_8GemvArgsE")}
    assert len(n4) == 4, sorted(scratch)            # {8, 16} rows x {RMSNorm prologue, none}; the weight stream is always non-temporal
    assert all(v == 0 for v in n4.values()), n4
