"""Thin tensor wrappers over the C-ABI (include/a3vlm_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every op below is one
call into liba3vlm_hip.so with raw device pointers on torch's CURRENT stream.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import lib as _l
from .lib import BF16, F32, EPI_BIAS, EPI_GELU, EPI_QUICKGELU, EPI_RESIDUAL, EPI_SWIGLU, EPI_OUT_F32, EPI_RES_F32, EPI_SWIGLU_BWD  # noqa: F401

_DT = {torch.bfloat16: BF16, torch.float32: F32}


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"a3vlm_amd supports bf16/fp32 tensors, got {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("a3vlm_amd ops need device tensors (no CPU fallback exists)")


_gemm_ws = {}                 # (device, stream) -> scratch tensor, in order of last use (dicts keep insertion order)
GEMM_WS_MAX_STREAMS = 8       # per process: a stream that has not run a GEMM while eight others did loses its 96-MiB scratch (it gets a new one
                              # on its next GEMM); before round 5 every stream that ever ran a GEMM kept one for the life of the process


def _ensure_gemm_workspace(device) -> None:
    """Register (once per device and stream) the scratch the GEMM entry points may use for the split-K planes of their hybrid dispatch
    (a3v_gemm_set_workspace_for: keyed by stream, so concurrent streams never share planes).  The scratch is allocated while its stream is
    current and only ever used by launches on that stream, so dropping it (least recently used first, beyond GEMM_WS_MAX_STREAMS) is
    ordered like any other free on that stream by the caching allocator; the registration is removed first."""
    st = _stream()
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), st)
    ws = _gemm_ws.pop(key, None)
    if ws is not None:
        _gemm_ws[key] = ws            # most recently used last
        return
    while len(_gemm_ws) >= GEMM_WS_MAX_STREAMS:
        (odev, ost), old = next(iter(_gemm_ws.items()))
        with torch.cuda.device(odev):
            _l.check(_l.load().a3v_gemm_set_workspace_for(ost, None, 0), "a3v_gemm_set_workspace_for(unregister)")
        del _gemm_ws[(odev, ost)], old
    ws = torch.empty(96 << 20, dtype=torch.uint8, device=device)
    _gemm_ws[key] = ws
    with torch.cuda.device(key[0]):
        _l.check(_l.load().a3v_gemm_set_workspace_for(st, ws.data_ptr(), ws.numel()), "a3v_gemm_set_workspace_for")


def gemm_nt(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, residual=None,
            epilogue: int = 0) -> torch.Tensor:
    """out[M, N or N/2] = epilogue(a[M,K] @ w[N,K]^T); a/w/out 2-D with unit inner stride."""
    _dev(a, w, out, bias, residual)
    _ensure_gemm_workspace(a.device)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    ep = epilogue
    if bias is not None:
        ep |= EPI_BIAS
    if residual is not None and not (ep & (EPI_RES_F32 | EPI_SWIGLU_BWD)):      # (EPI_SWIGLU_BWD: `residual` carries the forward's gate | up rows)
        ep |= EPI_RESIDUAL
    rc = _l.load().a3v_gemm_nt(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K,
                               _p(bias), _p(residual), residual.stride(0) if residual is not None else 0,
                               ep, dt(a), _stream())
    _l.check(rc, f"a3v_gemm_nt(M={M},N={N},K={K},epi={ep})")
    return out


def gemm_tn_sumsq_slots(M: int, N: int) -> int:
    return int(_l.load().a3v_gemm_tn_sumsq_slots(M, N))


def gemm_tn(at, wt, out, *, residual=None, epilogue: int = 0, sumsq=None):
    """out[M, N] = epilogue(at[K, M]^T @ wt[K, N]) -- both operands with the contracted index as rows (no transposes).
    ``sumsq`` (fp32 outputs only): a zeroed float32 buffer of >= gemm_tn_sumsq_slots(M, N) elements that receives partial sums of
    squares of the stored values (the clip's norm without a pass over the gradient)."""
    _dev(at, wt, out, residual, sumsq)
    K, M = at.shape
    N = wt.shape[1]
    assert wt.shape[0] == K and at.stride(1) == 1 and wt.stride(1) == 1 and out.stride(1) == 1
    _ensure_gemm_workspace(at.device)
    ep = epilogue
    if residual is not None and not (ep & EPI_RES_F32):
        ep |= EPI_RESIDUAL
    if sumsq is not None:
        assert sumsq.dtype == torch.float32 and sumsq.is_contiguous()
        rc = _l.load().a3v_gemm_tn_sumsq(_p(at), at.stride(0), _p(wt), wt.stride(0), _p(out), out.stride(0), M, N, K,
                                         _p(residual), residual.stride(0) if residual is not None else 0, ep, _p(sumsq), sumsq.numel(), _stream())
        _l.check(rc, f"a3v_gemm_tn_sumsq(M={M},N={N},K={K},epi={ep})")
        return out
    rc = _l.load().a3v_gemm_tn(_p(at), at.stride(0), _p(wt), wt.stride(0), _p(out), out.stride(0), M, N, K,
                               _p(residual), residual.stride(0) if residual is not None else 0, ep, _stream())
    _l.check(rc, f"a3v_gemm_tn(M={M},N={N},K={K},epi={ep})")
    return out


def gemm_nt_splitk(a, w, out, scratch, S: int, accumulate: bool = False):
    """out (+)= a @ w.T through S split-K planes (fp32 scratch of >= S*M*N floats); rounds once to out.dtype."""
    _dev(a, w, out, scratch)
    M, K = a.shape
    N = w.shape[0]
    assert scratch.dtype == torch.float32 and scratch.numel() >= S * M * N
    lib = _l.load()
    _l.check(lib.a3v_gemm_nt_splitk(_p(a), a.stride(0), _p(w), w.stride(0), _p(scratch), M, N, K, S, _stream()), f"a3v_gemm_nt_splitk(M={M},N={N},K={K},S={S})")
    _l.check(lib.a3v_splitk_reduce(_p(scratch), S, M, N, _p(out), out.stride(0), dt(out), 1 if accumulate else 0, _stream()), "a3v_splitk_reduce")
    return out


def gemm_nn(a, wt, out, *, residual=None, epilogue: int = 0):
    """out[M, N] = epilogue(a[M, K] @ wt[K, N]) -- wt row-indexed by the contracted index (dX = dY @ W on the forward image)."""
    _dev(a, wt, out, residual)
    M, K = a.shape
    N = wt.shape[1]
    assert wt.shape[0] == K and a.stride(1) == 1 and wt.stride(1) == 1 and out.stride(1) == 1
    _ensure_gemm_workspace(a.device)
    ep = epilogue
    if residual is not None and not (ep & (EPI_RES_F32 | EPI_SWIGLU_BWD)):
        ep |= EPI_RESIDUAL
    rc = _l.load().a3v_gemm_nn(_p(a), a.stride(0), _p(wt), wt.stride(0), _p(out), out.stride(0), M, N, K,
                               _p(residual), residual.stride(0) if residual is not None else 0, ep, _stream())
    _l.check(rc, f"a3v_gemm_nn(M={M},N={N},K={K},epi={ep})")
    return out


def gemm_tn_strip(t, x, out, scratch, S: int, accumulate: bool = False):
    """out[R, N] (+)= t[Kt, R]^T @ x[Kt, N] for R <= 64 (adapter weight gradients) through the small-block streaming kernel
    a3v_gemm_tn_strip + the split-K reduce; t's rows must hold 64 readable elements (the kernel loads 64 columns)."""
    _dev(t, x, out, scratch)
    Kt, R = t.shape
    N = x.shape[1]
    assert x.shape[0] == Kt and t.stride(1) == 1 and x.stride(1) == 1 and t.stride(0) >= 64
    assert scratch.dtype == torch.float32 and scratch.numel() >= S * R * N
    lib = _l.load()
    _l.check(lib.a3v_gemm_tn_strip(_p(t), t.stride(0), _p(x), x.stride(0), _p(scratch), R, N, Kt, S, _stream()), f"a3v_gemm_tn_strip(R={R},N={N},Kt={Kt},S={S})")
    _l.check(lib.a3v_splitk_reduce(_p(scratch), S, R, N, _p(out), out.stride(0), dt(out), 1 if accumulate else 0, _stream()), "a3v_splitk_reduce")
    return out


def gemm_tn_splitk(at, wt, out, scratch, S: int, accumulate: bool = False):
    """out[M, N] (+)= at[K, M]^T @ wt[K, N] through S split-K planes of the TN kernel (adapter-sized M or N, long K)."""
    _dev(at, wt, out, scratch)
    K, M = at.shape
    N = wt.shape[1]
    assert wt.shape[0] == K and at.stride(1) == 1 and wt.stride(1) == 1
    assert scratch.dtype == torch.float32 and scratch.numel() >= S * M * N
    lib = _l.load()
    _l.check(lib.a3v_gemm_tn_splitk(_p(at), at.stride(0), _p(wt), wt.stride(0), _p(scratch), M, N, K, S, _stream()), f"a3v_gemm_tn_splitk(M={M},N={N},K={K},S={S})")
    _l.check(lib.a3v_splitk_reduce(_p(scratch), S, M, N, _p(out), out.stride(0), dt(out), 1 if accumulate else 0, _stream()), "a3v_splitk_reduce")
    return out


def gemm_skinny_split(M: int, N: int, K: int) -> int:
    return _l.load().a3v_gemm_skinny_split(M, N, K)


def gemm_skinny_ws_bytes(M: int, N: int, K: int) -> int:
    return int(_l.load().a3v_gemm_skinny_ws_bytes(M, N, K))


def gemm_skinny_workspace(M: int, N: int, K: int, device) -> "torch.Tensor":
    """Zero-filled workspace for gemm_skinny (arrival counters first; every call leaves them zero)."""
    import torch
    return torch.zeros((gemm_skinny_ws_bytes(M, N, K) + 3) // 4, dtype=torch.float32, device=device)


def _gemm_skinny(name, a, w, scales, out, workspace, residual, epilogue):
    """The shared body of gemm_skinny / _fp8 / _nf4: one call of the C-ABI entry `name` (scales: None for bf16 weights)."""
    _dev(a, w, scales, out, workspace, residual)
    M, K = a.shape
    N = w.shape[0]
    if workspace.numel() * workspace.element_size() < gemm_skinny_ws_bytes(M, N, K):
        raise ValueError("gemm_skinny workspace too small (a3v_gemm_skinny_ws_bytes)")
    ep = epilogue | (EPI_RESIDUAL if residual is not None else 0)
    rc = getattr(_l.load(), name)(_p(a), a.stride(0), _p(w), w.stride(0), *([] if scales is None else [_p(scales)]), _p(out), out.stride(0),
                                  M, N, K, _p(residual), residual.stride(0) if residual is not None else 0, ep, _p(workspace), _stream())
    _l.check(rc, f"{name}(M={M},N={N},K={K},epi={ep})")
    return out


def gemm_skinny(a, w, out, partial, *, residual=None, epilogue: int = 0):
    return _gemm_skinny("a3v_gemm_skinny", a, w, None, out, partial, residual, epilogue)


def gemv_fused(a, w, out, workspace, *, wscale=None, n4: bool = False, residual=None, epilogue: int = 0, norm_w=None, ssq_in=None,
               eps: float = 0.0, ssq_out=None, rope=None, check: bool = True) -> int:
    """One call of a3v_gemv_fused, the decode step's GEMV building block (include/a3vlm_hip.h): gemm_skinny / _fp8 (``wscale`` [N]) / _nf4
    (``wscale`` = block scales, ``n4``) with the RMSNorm prologue (``norm_w``, ``ssq_in`` [K/16, 16], ``eps``), the sum-of-squares side
    output (``ssq_out`` [N/16, 16]) and / or the RoPE + KV-cache epilogue, ``rope`` = (cos_sin, k_cache [M, Hkv, Smax, hd],
    vt_cache [M, Hkv, hd, Smax], H, Hkv, hd, pos).  N is the row count of ``w``.  Returns the entry point's return code; ``check``
    raises on a non-zero one.  The entry point checks neither strides nor epilogue bits (see the header)."""
    cos_sin, k_cache, vt_cache, H, Hkv, hd, pos = rope if rope is not None else (None, None, None, 0, 0, 0, 0)
    _dev(a, w, wscale, out, workspace, residual, norm_w, ssq_in, ssq_out, cos_sin, k_cache, vt_cache)
    M, K = a.shape
    N = w.shape[0]
    if workspace.numel() * workspace.element_size() < gemm_skinny_ws_bytes(M, N, K):
        raise ValueError("gemv_fused workspace too small (a3v_gemm_skinny_ws_bytes)")
    Smax = k_cache.shape[2] if k_cache is not None else 0
    rc = _l.load().a3v_gemv_fused(_p(a), a.stride(0), _p(w), w.stride(0), _p(wscale), int(n4), _p(out), out.stride(0), M, N, K,
                                  _p(residual), residual.stride(0) if residual is not None else 0, epilogue, _p(norm_w), _p(ssq_in), eps,
                                  _p(ssq_out), int(rope is not None), _p(cos_sin), _p(k_cache), _p(vt_cache), H, Hkv, hd, Smax, pos,
                                  _p(workspace), _stream())
    if check:
        _l.check(rc, f"a3v_gemv_fused(M={M},N={N},K={K},epi={epilogue})")
    return rc


def quantize_rows_fp8(x, q, scales, norm_w=None, eps: float = 0.0):
    """q[r] = fp8(y[r] / scales[r]), scales[r] = max|y[r]| / 448; y = x, or the bf16 RMSNorm of x when norm_w is given."""
    _dev(x, q, scales, norm_w)
    rows, dim = x.shape
    assert q.dtype == torch.uint8 and scales.dtype == torch.float32 and scales.numel() >= rows
    rc = _l.load().a3v_quantize_rows_fp8(_p(x), x.stride(0), _p(norm_w), eps, _p(q), q.stride(0), _p(scales), rows, dim, dt(x), _stream())
    _l.check(rc, "a3v_quantize_rows_fp8")
    return q, scales


def gemm_nt_fp8(aq, sa, wq, sw, out, *, bias=None, residual=None, epilogue: int = 0):
    """out = epilogue((aq @ wq.T) * sa[:, None] * sw[None, :]) with fp8 operands (uint8 views of e4m3fn) on the MX-scaled MFMA."""
    _dev(aq, sa, wq, sw, out, bias, residual)
    M, K = aq.shape
    N = wq.shape[0]
    assert aq.dtype == torch.uint8 and wq.dtype == torch.uint8 and wq.shape[1] == K
    _ensure_gemm_workspace(aq.device)
    ep = epilogue
    if bias is not None:
        ep |= EPI_BIAS
    if residual is not None and not (ep & EPI_RES_F32):
        ep |= EPI_RESIDUAL
    rc = _l.load().a3v_gemm_nt_fp8(_p(aq), aq.stride(0), _p(sa), _p(wq), wq.stride(0), _p(sw), _p(out), out.stride(0), M, N, K,
                                   _p(bias), _p(residual), residual.stride(0) if residual is not None else 0, ep, _stream())
    _l.check(rc, f"a3v_gemm_nt_fp8(M={M},N={N},K={K},epi={ep})")
    return out


def gemm_qkv_rope_fp8(xq, sx, wq, sw, qkv, k_cache, vt_cache, cos_sin, B, S, H, Hkv, hd, start_pos, rope_pos0):
    _dev(xq, sx, wq, sw, qkv, k_cache, vt_cache, cos_sin)
    assert xq.shape[0] == B * S and wq.shape[0] == (H + 2 * Hkv) * hd
    rc = _l.load().a3v_gemm_qkv_rope_fp8(_p(xq), xq.stride(0), _p(sx), _p(wq), wq.stride(0), _p(sw), xq.shape[1], _p(qkv),
                                         qkv.stride(0), _p(k_cache), _p(vt_cache), _p(cos_sin), B, S, H, Hkv, hd,
                                         k_cache.shape[2], start_pos, rope_pos0, _stream())
    _l.check(rc, "a3v_gemm_qkv_rope_fp8")


def quantize_rows_fp8_cs(x, cs, q, scales, cols_pad: Optional[int] = None):
    """q[r, :cols] = fp8(y[r] / scales[r]) with y = x * cs[None, :] (fp32) and scales[r] = max|y[r]| / 448; q[r, cols:cols_pad] = 0."""
    _dev(x, cs, q, scales)
    rows, cols = x.shape
    cols_pad = q.shape[1] if cols_pad is None else cols_pad
    assert q.dtype == torch.uint8 and q.shape[0] >= rows and q.shape[1] >= cols_pad and q.stride(1) == 1 and x.stride(1) == 1
    assert scales.dtype == torch.float32 and scales.numel() >= rows and scales.is_contiguous()
    assert cs.dtype == torch.float32 and cs.numel() >= cols and cs.is_contiguous()
    rc = _l.load().a3v_quantize_rows_fp8_cs(_p(x), x.stride(0), _p(cs), _p(q), q.stride(0), _p(scales), rows, cols, cols_pad, dt(x), _stream())
    _l.check(rc, f"a3v_quantize_rows_fp8_cs(rows={rows},cols={cols},cols_pad={cols_pad})")
    return q, scales


def gemm_qkv_rope_fp8_train(xq, sx, wq, sw, q_out, k_cache, vt_cache, cos_sin, B, S, H, Hkv, hd, start_pos, rope_pos0, v_rows=None, delta=None):
    """gemm_qkv_rope_fp8 with the training operands of gemm_qkv_rope: ``v_rows`` (v token-major) and ``delta`` (bf16 additive term)."""
    _dev(xq, sx, wq, sw, q_out, k_cache, vt_cache, cos_sin, v_rows, delta)
    assert xq.shape[0] == B * S and wq.shape[0] == (H + 2 * Hkv) * hd and xq.dtype == torch.uint8 and wq.dtype == torch.uint8
    assert wq.shape[1] == xq.shape[1]
    _ensure_gemm_workspace(xq.device)
    rc = _l.load().a3v_gemm_qkv_rope_fp8_train(_p(xq), xq.stride(0), _p(sx), _p(wq), wq.stride(0), _p(sw), xq.shape[1], _p(q_out),
                                               q_out.stride(0), _p(k_cache), _p(vt_cache), _p(v_rows), v_rows.stride(0) if v_rows is not None else 0,
                                               _p(delta), delta.stride(0) if delta is not None else 0, _p(cos_sin), B, S, H, Hkv, hd,
                                               k_cache.shape[2], start_pos, rope_pos0, _stream())
    _l.check(rc, "a3v_gemm_qkv_rope_fp8_train")


def gemm_skinny_fp8(a, wq, wscale, out, workspace, *, residual=None, epilogue: int = 0):
    """out = epilogue((a . float(wq)^T) * wscale): weight-only fp8 (torch.float8_e4m3fn / uint8 bytes) decode GEMV."""
    assert wq.element_size() == 1 and wscale.dtype == torch.float32 and wscale.numel() == wq.shape[0]
    return _gemm_skinny("a3v_gemm_skinny_fp8", a, wq, wscale, out, workspace, residual, epilogue)


def quantize_nf4(w, q=None, scales=None, ws=None):
    """NF4 image of one bf16 module weight w [N, K] (a3v_quantize_nf4, the format of include/a3vlm_hip.h): returns
    (nibbles [N, K/2] uint8, block scales [N, K/64] fp32, module offset as a 0-d fp32 device tensor)."""
    N, K = w.shape
    if w.dtype != torch.bfloat16 or not w.is_contiguous():
        raise ValueError("quantize_nf4 needs a contiguous bf16 weight")
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device) if q is None else q
    scales = torch.empty(N, K // 64, dtype=torch.float32, device=w.device) if scales is None else scales
    need = int(_l.load().a3v_quantize_nf4_ws_bytes(N, K))
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=w.device) if ws is None else ws
    _dev(w, q, scales, ws)
    assert q.is_contiguous() and scales.is_contiguous() and ws.numel() * 4 >= need
    rc = _l.load().a3v_quantize_nf4(_p(w), N, K, _p(q), _p(scales), _p(ws), _stream())
    _l.check(rc, f"a3v_quantize_nf4(N={N},K={K})")
    return q, scales, ws[0]


def dequantize_nf4(q, scales, out):
    """out [N, K] bf16 = bf16(NF4[q] * s_b) (a3v_dequantize_nf4)."""
    _dev(q, scales, out)
    N, K = out.shape
    assert q.dtype == torch.uint8 and q.is_contiguous() and q.shape == (N, K // 2) and scales.is_contiguous() and scales.numel() == N * K // 64
    rc = _l.load().a3v_dequantize_nf4(_p(q), _p(scales), _p(out), out.stride(0), N, K, _stream())
    _l.check(rc, f"a3v_dequantize_nf4(N={N},K={K})")
    return out


def dequantize_nf4_images(q, scales, wd=None, wt=None):
    """wd [N, K] and / or wt [K, N] = wd^T (bf16 views, unit column stride, any row stride) from one read of the NF4 image
    (a3v_dequantize_nf4_images).  Only those windows are written: they may sit inside wider images."""
    _dev(q, scales, wd, wt)
    N, K = q.shape[0], q.shape[1] * 2
    assert q.dtype == torch.uint8 and q.is_contiguous() and scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == N * K // 64
    for w, shape in ((wd, (N, K)), (wt, (K, N))):
        assert w is None or (w.dtype == torch.bfloat16 and tuple(w.shape) == shape and w.stride(1) == 1)
    rc = _l.load().a3v_dequantize_nf4_images(_p(q), _p(scales), N, K, _p(wd), wd.stride(0) if wd is not None else 0,
                                             _p(wt), wt.stride(0) if wt is not None else 0, _stream())
    _l.check(rc, f"a3v_dequantize_nf4_images(N={N},K={K})")


def lora_merge(base, lora_b, lora_a, out=None):
    """out = round(base + lora_b . lora_a), fp32 accumulation and ONE rounding (a3v_lora_merge).  ``base``: a bf16 / fp32 matrix [N, K]
    (unit column stride, any row stride) or an NF4 image ``(q [N, K/2] uint8, scales [N, K/64] fp32)`` of ``quantize_nf4``; ``lora_b``
    [N, R] and ``lora_a`` [R, K] in the dtype of ``out``.  ``out=None``: in place into ``base`` (a new bf16 matrix for an NF4 base).
    Only the N x K window of ``out`` is written."""
    R, K = lora_a.shape
    N = lora_b.shape[0]
    if isinstance(base, (tuple, list)):
        w, (q, scales) = None, base[:2]
        _dev(q, scales)
        assert q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (N, K // 2)
        assert scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == N * (K // 64)
        if out is None:
            out = torch.empty(N, K, dtype=torch.bfloat16, device=q.device)
    else:
        w, q, scales = base, None, None
        out = w if out is None else out
        assert tuple(w.shape) == (N, K) and w.stride(1) == 1 and w.dtype == out.dtype
    _dev(w, lora_b, lora_a, out)
    assert lora_b.shape[1] == R and tuple(out.shape) == (N, K) and out.stride(1) == 1 and lora_a.stride(1) == 1 and lora_b.stride(1) == 1
    assert lora_a.dtype == out.dtype and lora_b.dtype == out.dtype
    rc = _l.load().a3v_lora_merge(_p(w), w.stride(0) if w is not None else 0, _p(q), _p(scales), _p(lora_b), lora_b.stride(0),
                                  _p(lora_a), lora_a.stride(0), _p(out), out.stride(0), N, K, R, dt(out), _stream())
    _l.check(rc, f"a3v_lora_merge(N={N},K={K},R={R})")
    return out


def gemm_skinny_nf4(a, q, scales, out, workspace, *, residual=None, epilogue: int = 0):
    """out = epilogue(sum_b s_b * (a . NF4[q])^T): weight-only NF4 decode GEMV (M <= 16, K % 256 == 0)."""
    N, K = q.shape[0], a.shape[1]
    assert q.dtype == torch.uint8 and q.shape[1] * 2 == K and scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == N * K // 64
    return _gemm_skinny("a3v_gemm_skinny_nf4", a, q, scales, out, workspace, residual, epilogue)


def quantize_mxfp4(w, q=None, scales=None):
    """MXFP4 image of a bf16 weight w [N, K] (unit column stride, K % 128 == 0; a3v_quantize_mxfp4, the format of
    include/a3vlm_hip.h "MXFP4 weights"): returns (codes [N, K/2] uint8, e8m0 block scales [N, K/32] uint8)."""
    N, K = w.shape
    if w.dtype != torch.bfloat16 or w.stride(1) != 1:
        raise ValueError("quantize_mxfp4 needs a bf16 weight with unit column stride")
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device) if q is None else q
    scales = torch.empty(N, K // 32, dtype=torch.uint8, device=w.device) if scales is None else scales
    _dev(w, q, scales)
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and q.stride(1) == 1
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.numel() == N * (K // 32)
    rc = _l.load().a3v_quantize_mxfp4(_p(w), w.stride(0), _p(q), q.stride(0), _p(scales), N, K, _stream())
    _l.check(rc, f"a3v_quantize_mxfp4(N={N},K={K})")
    return q, scales


def dequantize_mxfp4(q, scales, out):
    """out [N, K] bf16 = e2m1(q) * 2^(scales - 127), exact (a3v_dequantize_mxfp4)."""
    _dev(q, scales, out)
    N, K = out.shape
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and q.stride(1) == 1 and out.dtype == torch.bfloat16 and out.stride(1) == 1
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.numel() == N * (K // 32)
    rc = _l.load().a3v_dequantize_mxfp4(_p(q), q.stride(0), _p(scales), _p(out), out.stride(0), N, K, _stream())
    _l.check(rc, f"a3v_dequantize_mxfp4(N={N},K={K})")
    return out


def gemm_skinny_mxfp4_ws_bytes(M: int, N: int, K: int) -> int:
    return int(_l.load().a3v_gemm_skinny_mxfp4_ws_bytes(M, N, K))


def mx4_gemv_plan(M: int, N: int, K: int, epilogue: int = 0, cus: int = 256):
    """(rc, plan ints) of a3v_mx4_gemv_plan: grid, block, K slices, rows per block, LDS bytes, 512-k units, row groups, units per slice."""
    import ctypes
    plan = (ctypes.c_int32 * 8)()
    rc = _l.load().a3v_mx4_gemv_plan(M, N, K, epilogue, cus, plan)
    return rc, list(plan)


def gemm_skinny_mxfp4(a, q, scales, out, workspace, *, residual=None, epilogue: int = 0):
    """out = epilogue(sum_blocks 2^(ea + ew) * sum_32 a_q * w_q): MXFP4 weights x MXFP8 activations decode GEMV on the scaled MFMA
    (M <= 16, N % 16 == 0, K % 128 == 0); workspace: zero-filled once, gemm_skinny_mxfp4_ws_bytes (may be gemm_skinny's)."""
    _dev(a, q, scales, out, workspace, residual)
    M, K = a.shape
    N = q.shape[0]
    assert a.dtype == torch.bfloat16 and a.stride(1) == 1, "activations are bf16 rows"
    assert q.dtype == torch.uint8 and q.shape[1] * 2 == K and q.stride(1) == 1
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.numel() == N * (K // 32)
    ncol = N // 2 if epilogue & EPI_SWIGLU else N
    assert out.dtype == (torch.float32 if epilogue & EPI_OUT_F32 else torch.bfloat16) and out.stride(1) == 1 and tuple(out.shape) == (M, ncol)
    assert residual is None or (residual.dtype == torch.bfloat16 and residual.stride(1) == 1 and tuple(residual.shape) == (M, N))
    need = gemm_skinny_mxfp4_ws_bytes(M, N, K)
    if need and workspace.numel() * workspace.element_size() < need:
        raise ValueError("gemm_skinny_mxfp4 workspace too small (a3v_gemm_skinny_mxfp4_ws_bytes)")
    ep = epilogue | (EPI_RESIDUAL if residual is not None else 0)
    rc = _l.load().a3v_gemm_skinny_mxfp4(_p(a), a.stride(0), _p(q), q.stride(0), _p(scales), _p(out), out.stride(0), M, N, K,
                                         _p(residual), residual.stride(0) if residual is not None else 0, ep, _p(workspace), _stream())
    _l.check(rc, f"a3v_gemm_skinny_mxfp4(M={M},N={N},K={K},epi={ep})")
    return out


def quantize_rows_mxfp8(x, q=None, e=None, norm_w=None, eps: float = 0.0):
    """MXFP8 rows of bf16 x [rows, K] (K % 128 == 0; a3v_quantize_rows_mxfp8, the "Activations" rule of include/a3vlm_hip.h): returns
    (e4m3fn codes [rows, K] uint8, e8m0 block exponents [rows, K/32] uint8); with norm_w the rows are the bf16 RMSNorm of x."""
    rows, K = x.shape
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise ValueError("quantize_rows_mxfp8 needs bf16 rows with unit column stride")
    q = torch.empty(rows, K, dtype=torch.uint8, device=x.device) if q is None else q
    e = torch.empty(rows, K // 32, dtype=torch.uint8, device=x.device) if e is None else e
    _dev(x, q, e, norm_w)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (rows, K) and q.stride(1) == 1
    assert e.dtype == torch.uint8 and e.is_contiguous() and e.numel() == rows * (K // 32)
    assert norm_w is None or (norm_w.dtype == torch.bfloat16 and norm_w.is_contiguous() and norm_w.numel() == K)
    rc = _l.load().a3v_quantize_rows_mxfp8(_p(x), x.stride(0), _p(norm_w), eps, _p(q), q.stride(0), _p(e), rows, K, _stream())
    _l.check(rc, f"a3v_quantize_rows_mxfp8(rows={rows},K={K})")
    return q, e


def mx4_gemm_plan(M: int, N: int, K: int, epilogue: int = 0, cus: int = 256):
    """(rc, plan ints) of a3v_mx4_gemm_plan: tile rows, tile columns, K stage in k, grid, block, LDS bytes, K slices, K stages per slice."""
    import ctypes
    plan = (ctypes.c_int32 * 8)()
    rc = _l.load().a3v_mx4_gemm_plan(M, N, K, epilogue, cus, plan)
    return rc, list(plan)


def gemm_nt_mxfp4(aq, ea, q, scales, out, *, residual=None, epilogue: int = 0):
    """out = epilogue(sum_blocks 2^(ea + ew) * sum_32 a_q * w_q): the W4A8 GEMM on an MXFP4 image for any M (a3v_gemm_nt_mxfp4); aq / ea
    from quantize_rows_mxfp8."""
    _dev(aq, ea, q, scales, out, residual)
    M, K = aq.shape
    N = q.shape[0]
    assert aq.dtype == torch.uint8 and aq.stride(1) == 1 and ea.dtype == torch.uint8 and ea.is_contiguous() and ea.numel() == M * (K // 32)
    assert q.dtype == torch.uint8 and q.shape[1] * 2 == K and q.stride(1) == 1
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.numel() == N * (K // 32)
    ncol = N // 2 if epilogue & EPI_SWIGLU else N
    assert out.dtype == (torch.float32 if epilogue & EPI_OUT_F32 else torch.bfloat16) and out.stride(1) == 1 and tuple(out.shape) == (M, ncol)
    assert residual is None or (residual.dtype == torch.bfloat16 and residual.stride(1) == 1 and tuple(residual.shape) == (M, N))
    ep = epilogue | (EPI_RESIDUAL if residual is not None else 0)
    rc = _l.load().a3v_gemm_nt_mxfp4(_p(aq), aq.stride(0), _p(ea), _p(q), q.stride(0), _p(scales), _p(out), out.stride(0), M, N, K,
                                     _p(residual), residual.stride(0) if residual is not None else 0, ep, _stream())
    _l.check(rc, f"a3v_gemm_nt_mxfp4(M={M},N={N},K={K},epi={ep})")
    return out


def rmsnorm(x, w, out, eps: float, row_idx=None):
    """out = rmsnorm(x) * w; ``row_idx`` (int32 [n]): out row i from x row row_idx[i]."""
    _dev(x, w, out, row_idx)
    rows, dim = x.shape
    if row_idx is not None:
        assert row_idx.dtype == torch.int32 and row_idx.is_contiguous() and out.shape[0] == row_idx.numel()
        rc = _l.load().a3v_rmsnorm_rows(_p(x), x.stride(0), _p(row_idx), _p(w), _p(out), out.stride(0), row_idx.numel(), dim, eps,
                                        dt(x), dt(w), dt(out), _stream())
        _l.check(rc, "a3v_rmsnorm_rows")
        return out
    rc = _l.load().a3v_rmsnorm(_p(x), x.stride(0), _p(w), _p(out), out.stride(0), rows, dim, eps,
                               dt(x), dt(w), dt(out), _stream())
    _l.check(rc, "a3v_rmsnorm")
    return out


def layernorm(x, w, b, out, eps: float = 1e-5, row_map=None, rows: Optional[int] = None):
    _dev(x, w, b, out, row_map)
    n, dim = x.shape
    rc = _l.load().a3v_layernorm(_p(x), x.stride(0), _p(w), _p(b), _p(out), out.stride(0), _p(row_map),
                                 n if rows is None else rows, dim, eps, dt(x), dt(w), dt(out), _stream())
    _l.check(rc, "a3v_layernorm")
    return out


def rope_kvcache(qkv, q_out, k_cache, vt_cache, cos_sin, B, S, H, Hkv, hd, start_pos, rope_pos0):
    _dev(qkv, q_out, k_cache, vt_cache, cos_sin)
    Smax = k_cache.shape[2]
    rc = _l.load().a3v_rope_kvcache(_p(qkv), qkv.stride(0), _p(q_out), q_out.stride(0), _p(k_cache), _p(vt_cache),
                                    _p(cos_sin), B, S, H, Hkv, hd, Smax, start_pos, rope_pos0, dt(qkv), _stream())
    _l.check(rc, "a3v_rope_kvcache")


def gemm_qkv_rope(x, wqkv, qkv, k_cache, vt_cache, cos_sin, B, S, H, Hkv, hd, start_pos, rope_pos0, v_rows=None, delta=None):
    """qkv GEMM with RoPE + KV-cache write in the epilogue: rotated q lands in qkv[:, :H*hd] (further columns are not
    written), rotated k in k_cache, v transposed in vt_cache (and token-major in v_rows if given) -- the values of gemm_nt
    followed by rope_kvcache.  ``delta`` [B*S, N] (bf16): added to the projection before the rotation (the LoRA branch)."""
    _dev(x, wqkv, qkv, k_cache, vt_cache, cos_sin, v_rows, delta)
    assert x.shape[0] == B * S and wqkv.shape[0] == (H + 2 * Hkv) * hd and x.dtype == torch.bfloat16
    rc = _l.load().a3v_gemm_qkv_rope(_p(x), x.stride(0), _p(wqkv), wqkv.stride(0), x.shape[1], _p(qkv), qkv.stride(0),
                                     _p(k_cache), _p(vt_cache), _p(v_rows), v_rows.stride(0) if v_rows is not None else 0,
                                     _p(delta), delta.stride(0) if delta is not None else 0,
                                     _p(cos_sin), B, S, H, Hkv, hd, k_cache.shape[2], start_pos, rope_pos0, _stream())
    _l.check(rc, "a3v_gemm_qkv_rope")


def vt_pack(v, ldv, vt, N, L, H, hd, Lpad):
    _dev(v, vt)
    rc = _l.load().a3v_vt_pack(_p(v), ldv, _p(vt), N, L, H, hd, Lpad, dt(v), _stream())
    _l.check(rc, "a3v_vt_pack")


def attention_scratch_floats(B, H, hd, Sk) -> int:
    return _l.load().a3v_attention_scratch_floats(B, H, hd, Sk)


_Strides = ctypes.c_int64 * 12


def attention(q, k, vt, out, B, Sq, Sk, H, Hkv, hd, strides, causal: bool, scratch=None):
    _dev(q, k, vt, out, scratch)
    rc = _l.load().a3v_attention(_p(q), _p(k), _p(vt), _p(out), B, Sq, Sk, H, Hkv, hd, _Strides(*strides),
                                 1 if causal else 0, _p(scratch), dt(q), _stream())
    _l.check(rc, f"a3v_attention(B={B},Sq={Sq},Sk={Sk},H={H},hd={hd})")
    return out


def attention_decode_plan(B: int, H: int, Sk: int, wave: bool = True):
    """(nsplit, chunk) of the library's decode split plan: the wave-streaming entries' (default) or the two-phase kernel's."""
    ns, ch = ctypes.c_int(0), ctypes.c_int(0)
    rc = _l.load().a3v_attention_decode_plan(B, H, Sk, 1 if wave else 0, ctypes.byref(ns), ctypes.byref(ch))
    _l.check(rc, f"a3v_attention_decode_plan(B={B},H={H},Sk={Sk})")
    return ns.value, ch.value


def attention_decode_fused(q, k, vt, out, B, Sk, H, Hkv, hd, strides, scratch, counters):
    """The decode attention of the fused decode step (bf16, hd 64 / 128): strides as ``attention`` at Sq = 1, scratch of
    attention_scratch_floats(B, H, hd, Sk) floats, counters int32 [>= B*H], zero; left zero."""
    _dev(q, k, vt, out, scratch, counters)
    assert q.dtype == k.dtype == vt.dtype == out.dtype == torch.bfloat16
    assert scratch.dtype == torch.float32 and scratch.numel() >= attention_scratch_floats(B, H, hd, Sk)
    assert counters.dtype == torch.int32 and counters.numel() >= B * H
    rc = _l.load().a3v_attention_decode_fused_bf16(_p(q), _p(k), _p(vt), _p(out), B, Sk, H, Hkv, hd, _Strides(*strides), _p(scratch),
                                                   _p(counters), _stream())
    _l.check(rc, f"a3v_attention_decode_fused_bf16(B={B},Sk={Sk},H={H},hd={hd})")
    return out


def kv_quantize_fp8(k_src, vt_src, src_pos: int, k_q, vt_q, k_scale, v_scale, S: int, dst_pos: int):
    """Positions src_pos .. src_pos+S-1 of a bf16 K [B,Hkv,Smax_src,hd] / V^T [B,Hkv,hd,Smax_src] pair -> positions dst_pos .. of the fp8
    caches (uint8, same layouts) and their per-(batch, kv-head, position) fp32 scales."""
    _dev(k_src, vt_src, k_q, vt_q, k_scale, v_scale)
    B, Hkv, Smax, hd = k_q.shape
    assert k_src.dtype == vt_src.dtype == torch.bfloat16 and k_q.dtype == vt_q.dtype == torch.uint8
    assert k_src.is_contiguous() and vt_src.is_contiguous() and k_q.is_contiguous() and vt_q.is_contiguous()
    assert k_src.shape[0] >= B and tuple(vt_q.shape) == (B, Hkv, hd, Smax) and tuple(k_scale.shape) == tuple(v_scale.shape) == (B, Hkv, Smax)
    assert tuple(k_src.shape[1:]) == (Hkv, k_src.shape[2], hd) and tuple(vt_src.shape[1:]) == (Hkv, hd, k_src.shape[2])
    rc = _l.load().a3v_kv_quantize_fp8(_p(k_src), _p(vt_src), k_src.shape[2], src_pos, _p(k_q), _p(vt_q), _p(k_scale), _p(v_scale),
                                       B, Hkv, hd, S, Smax, dst_pos, _stream())
    _l.check(rc, f"a3v_kv_quantize_fp8(B={B},Hkv={Hkv},hd={hd},S={S},dst_pos={dst_pos},Smax={Smax})")


def kv_dequantize_fp8(k_q, vt_q, k_scale, v_scale, k_dst, vt_dst, n: int):
    """Positions 0 .. n-1 of the fp8 caches -> the same positions of a bf16 K / V^T pair: bf16(float(q) * scale)."""
    _dev(k_q, vt_q, k_scale, v_scale, k_dst, vt_dst)
    B, Hkv, Smax, hd = k_q.shape
    assert k_dst.dtype == vt_dst.dtype == torch.bfloat16 and k_q.dtype == vt_q.dtype == torch.uint8
    assert k_dst.is_contiguous() and vt_dst.is_contiguous() and k_q.is_contiguous() and vt_q.is_contiguous()
    assert tuple(k_dst.shape) == (B, Hkv, k_dst.shape[2], hd) and tuple(vt_dst.shape) == (B, Hkv, hd, k_dst.shape[2])
    rc = _l.load().a3v_kv_dequantize_fp8(_p(k_q), _p(vt_q), _p(k_scale), _p(v_scale), Smax, _p(k_dst), _p(vt_dst), k_dst.shape[2],
                                         B, Hkv, hd, n, _stream())
    _l.check(rc, f"a3v_kv_dequantize_fp8(B={B},Hkv={Hkv},hd={hd},n={n})")


def attention_decode_fp8kv_splits(B: int, H: int, Sk: int) -> int:
    return _l.load().a3v_attention_decode_fp8kv_splits(B, H, Sk)


def attention_decode_fp8kv(q, k_q, vt_q, k_scale, v_scale, out, B, Sk, H, Hkv, hd, scratch, counters=None):
    """Decode attention over an fp8 KV cache: q bf16 [B, ldq] (head h at column h*hd; a view into the qkv buffer), out bf16
    [B, >= H*hd].  counters (int32 [>= B*H], zero; left zero): the split partials are merged inside the launch."""
    _dev(q, k_q, vt_q, k_scale, v_scale, out, scratch, counters)
    assert q.dtype == out.dtype == torch.bfloat16 and k_q.dtype == vt_q.dtype == torch.uint8 and scratch.dtype == torch.float32
    assert k_q.is_contiguous() and vt_q.is_contiguous() and k_scale.is_contiguous() and v_scale.is_contiguous()
    assert scratch.numel() >= attention_scratch_floats(B, H, hd, Sk) and (counters is None or counters.numel() >= B * H)
    rc = _l.load().a3v_attention_decode_fp8kv(_p(q), q.stride(0), _p(k_q), _p(vt_q), _p(k_scale), _p(v_scale), _p(out), out.stride(0),
                                              B, Sk, H, Hkv, hd, k_q.shape[2], _p(scratch), _p(counters), _stream())
    _l.check(rc, f"a3v_attention_decode_fp8kv(B={B},Sk={Sk},H={H},hd={hd})")
    return out


def rope_kvcache_rows(qkv, q_out, k_cache, vt_cache, cos_sin, pos, B, H, Hkv, hd):
    """rope_kvcache at S = 1 with row b at cache position pos[b] (device int32 [B]; outside [0, Smax) = idle row: no cache write,
    zero q row)."""
    _dev(qkv, q_out, k_cache, vt_cache, cos_sin, pos)
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.numel() >= B
    assert k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.shape[0] >= B and k_cache.dtype == vt_cache.dtype == qkv.dtype
    rc = _l.load().a3v_rope_kvcache_rows(_p(qkv), qkv.stride(0), _p(q_out), q_out.stride(0), _p(k_cache), _p(vt_cache), _p(cos_sin),
                                         _p(pos), B, H, Hkv, hd, k_cache.shape[2], dt(qkv), _stream())
    _l.check(rc, f"a3v_rope_kvcache_rows(B={B},H={H},Hkv={Hkv},hd={hd})")


def attention_decode_rows_splits(B: int, H: int, sk_max: int) -> int:
    return _l.load().a3v_attention_decode_rows_splits(B, H, sk_max)


def attention_decode_rows(q, k, vt, out, sk, sk_max: int, B, H, Hkv, hd, strides, scratch=None, counters=None):
    """Decode attention with sk[b] keys for row b (device int32 [B]; <= 0 = idle row, zero output); strides as ``attention`` at
    Sq = 1.  bf16 at hd 64 / 128 needs scratch (attention_scratch_floats(B, H, hd, sk_max) floats) and counters (int32 [>= B*H],
    zero; left zero)."""
    _dev(q, k, vt, out, sk, scratch, counters)
    assert sk.dtype == torch.int32 and sk.is_contiguous() and sk.numel() >= B
    assert scratch is None or (scratch.dtype == torch.float32 and scratch.numel() >= attention_scratch_floats(B, H, hd, sk_max))
    assert counters is None or (counters.dtype == torch.int32 and counters.numel() >= B * H)
    rc = _l.load().a3v_attention_decode_rows(_p(q), _p(k), _p(vt), _p(out), _p(sk), int(sk_max), B, H, Hkv, hd, _Strides(*strides),
                                             _p(scratch), _p(counters), dt(q), _stream())
    _l.check(rc, f"a3v_attention_decode_rows(B={B},sk_max={sk_max},H={H},hd={hd})")
    return out


def attention_decode_rows_shared(q, k, vt, out, sk, src_row, shared, sk_max: int, B, H, Hkv, hd, strides, scratch=None, counters=None):
    """``attention_decode_rows`` with shared prompt keys: row b reads its keys below min(shared[b], sk[b]) rounded down to a
    multiple of 64 from cache row src_row[b] (device int32 [B] each; a src_row outside [0, B) or equal to b, or shared <= 0: the
    plain row).  k / vt hold all B rows.  Bit-equal to ``attention_decode_rows`` on caches with that prefix copied."""
    _dev(q, k, vt, out, sk, src_row, shared, scratch, counters)
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (sk, src_row, shared))
    assert k.shape[0] >= B and vt.shape[0] >= B
    assert scratch is None or (scratch.dtype == torch.float32 and scratch.numel() >= attention_scratch_floats(B, H, hd, sk_max))
    assert counters is None or (counters.dtype == torch.int32 and counters.numel() >= B * H)
    rc = _l.load().a3v_attention_decode_rows_shared(_p(q), _p(k), _p(vt), _p(out), _p(sk), _p(src_row), _p(shared), int(sk_max), B, H, Hkv,
                                                    hd, _Strides(*strides), _p(scratch), _p(counters), dt(q), _stream())
    _l.check(rc, f"a3v_attention_decode_rows_shared(B={B},sk_max={sk_max},H={H},hd={hd})")
    return out


def kv_copy_span(k_caches, vt_caches, src_row: int, dst_rows, lo: int, hi: int, ptrs=None):
    """Positions [lo, hi) (0 <= hi - lo < 64) of cache row ``src_row`` into the rows ``dst_rows`` (device int32; entries outside the
    cache are skipped) of every layer, one launch: k_caches / vt_caches are the per-layer [B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] tensors.
    ``ptrs``: the device int64 [2, layers] table of their base pointers if the caller keeps one (returned either way)."""
    k0 = k_caches[0]
    B, Hkv, Smax, hd = k0.shape
    for k, v in zip(k_caches, vt_caches):
        _dev(k, v)
        assert k.is_contiguous() and v.is_contiguous() and k.dtype == v.dtype == k0.dtype
        assert tuple(k.shape) == (B, Hkv, Smax, hd) and tuple(v.shape) == (B, Hkv, hd, Smax)
    _dev(dst_rows)
    assert dst_rows.dtype == torch.int32 and dst_rows.is_contiguous() and len(k_caches) == len(vt_caches)
    if ptrs is None:
        ptrs = torch.tensor([[t.data_ptr() for t in k_caches], [t.data_ptr() for t in vt_caches]], dtype=torch.int64, device=k0.device)
    assert ptrs.dtype == torch.int64 and tuple(ptrs.shape) == (2, len(k_caches)) and ptrs.is_contiguous()
    rc = _l.load().a3v_kv_copy_span(_p(ptrs[0]), _p(ptrs[1]), len(k_caches), int(src_row), _p(dst_rows), dst_rows.numel(), B, int(lo),
                                    int(hi), Hkv, hd, Smax, dt(k0), _stream())
    _l.check(rc, f"a3v_kv_copy_span(src={src_row},lo={lo},hi={hi},hd={hd})")
    return ptrs


def _kv8_arrays(k_q, vt_q, k_scale, v_scale):
    """(B, Hkv, Smax, hd) of the four arrays of one layer's fp8 cache, checked."""
    _dev(k_q, vt_q, k_scale, v_scale)
    B, Hkv, Smax, hd = k_q.shape
    assert k_q.dtype == vt_q.dtype == torch.uint8 and k_scale.dtype == v_scale.dtype == torch.float32
    assert all(t.is_contiguous() for t in (k_q, vt_q, k_scale, v_scale))
    assert tuple(vt_q.shape) == (B, Hkv, hd, Smax) and tuple(k_scale.shape) == tuple(v_scale.shape) == (B, Hkv, Smax)
    return B, Hkv, Smax, hd


def rope_kvquant_rows(qkv, q_out, k_q, vt_q, k_scale, v_scale, cos_sin, pos, B, H, Hkv, hd):
    """``rope_kvcache_rows`` into an fp8 cache, one launch: q rotated into q_out, the rotated bf16 k row and the v row quantised per
    kv-head and written at position pos[b] of row b's own cache (device int32 [B]; outside [0, Smax) = idle row: no cache write,
    zero q row).  Bit-equal to ``rope_kvcache_rows`` into a bf16 cache followed by ``kv_quantize_fp8`` (S = 1) of that position."""
    _dev(qkv, q_out, cos_sin, pos)
    Bc, Hc, Smax, hdc = _kv8_arrays(k_q, vt_q, k_scale, v_scale)
    assert qkv.dtype == q_out.dtype == torch.bfloat16 and pos.dtype == torch.int32 and pos.is_contiguous() and pos.numel() >= B
    assert Bc >= B and (Hc, hdc) == (Hkv, hd)
    rc = _l.load().a3v_rope_kvquant_rows(_p(qkv), qkv.stride(0), _p(q_out), q_out.stride(0), _p(k_q), _p(vt_q), _p(k_scale), _p(v_scale),
                                         _p(cos_sin), _p(pos), B, H, Hkv, hd, Smax, _stream())
    _l.check(rc, f"a3v_rope_kvquant_rows(B={B},H={H},Hkv={Hkv},hd={hd})")


def attention_decode_rows_fp8kv_splits(B: int, H: int, sk_max: int) -> int:
    return _l.load().a3v_attention_decode_rows_fp8kv_splits(B, H, sk_max)


def attention_decode_rows_fp8kv(q, k_q, vt_q, k_scale, v_scale, out, sk, sk_max: int, B, H, Hkv, hd, scratch, counters,
                                src_row=None, shared=None):
    """``attention_decode_fp8kv`` with sk[b] keys for row b (device int32 [B]; <= 0 = idle row, zero output; above sk_max read as
    sk_max).  scratch: attention_scratch_floats(B, H, hd, sk_max) floats; counters int32 [>= B*H], zero; left zero.
    ``src_row`` / ``shared`` (both or neither): shared prompt keys as ``attention_decode_rows_shared`` -- below the shared length
    the K bytes, V^T bytes and both scales of row b are read from cache row src_row[b]; the arrays hold all B rows."""
    _dev(q, out, sk, scratch, counters, src_row, shared)
    Bc, Hc, Smax, hdc = _kv8_arrays(k_q, vt_q, k_scale, v_scale)
    assert q.dtype == out.dtype == torch.bfloat16 and Bc >= B and (Hc, hdc) == (Hkv, hd)
    assert (src_row is None) == (shared is None)
    assert all(t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B) for t in (sk, src_row, shared))
    assert scratch.dtype == torch.float32 and scratch.numel() >= attention_scratch_floats(B, H, hd, sk_max)
    assert counters.dtype == torch.int32 and counters.numel() >= B * H
    head = (_p(q), q.stride(0), _p(k_q), _p(vt_q), _p(k_scale), _p(v_scale), _p(out), out.stride(0), _p(sk))
    tail = (int(sk_max), B, H, Hkv, hd, Smax, _p(scratch), _p(counters), _stream())
    if src_row is None:
        rc = _l.load().a3v_attention_decode_rows_fp8kv(*head, *tail)
    else:
        rc = _l.load().a3v_attention_decode_rows_fp8kv_shared(*head, _p(src_row), _p(shared), *tail)
    _l.check(rc, f"a3v_attention_decode_rows_fp8kv(B={B},sk_max={sk_max},H={H},hd={hd},shared={src_row is not None})")
    return out


def kv8_copy_span(k_q, vt_q, k_scale, v_scale, src_row: int, dst_rows, lo: int, hi: int, ptrs=None):
    """``kv_copy_span`` for an fp8 cache: positions [lo, hi) (0 <= hi - lo < 64) of cache row ``src_row`` -- K bytes, V^T byte runs
    and both scale runs -- into the rows ``dst_rows`` (device int32; entries outside the cache are skipped) of every layer, one
    launch.  The four arguments are the per-layer lists.  ``ptrs``: the device int64 [4, layers] table of their base pointers if the
    caller keeps one (returned either way)."""
    B, Hkv, Smax, hd = k_q[0].shape
    assert len(k_q) == len(vt_q) == len(k_scale) == len(v_scale)
    for arrays in zip(k_q, vt_q, k_scale, v_scale):
        assert _kv8_arrays(*arrays) == (B, Hkv, Smax, hd)
    _dev(dst_rows)
    assert dst_rows.dtype == torch.int32 and dst_rows.is_contiguous()
    if ptrs is None:
        ptrs = torch.tensor([[t.data_ptr() for t in ts] for ts in (k_q, vt_q, k_scale, v_scale)], dtype=torch.int64, device=k_q[0].device)
    assert ptrs.dtype == torch.int64 and tuple(ptrs.shape) == (4, len(k_q)) and ptrs.is_contiguous()
    rc = _l.load().a3v_kv8_copy_span(_p(ptrs[0]), _p(ptrs[1]), _p(ptrs[2]), _p(ptrs[3]), len(k_q), int(src_row), _p(dst_rows),
                                     dst_rows.numel(), B, int(lo), int(hi), Hkv, hd, Smax, _stream())
    _l.check(rc, f"a3v_kv8_copy_span(src={src_row},lo={lo},hi={hi},hd={hd})")
    return ptrs


def generate_step_rows(logits, sampled, tokens, cur, limit, pos_base: int, stop_seq, stop_off, n_stop: int, stopped, stop_pos, live,
                       next_tok, pos):
    """One launch = one step of generate_many's bookkeeping (a3v_generate_step_rows): per row argmax (or the sampled id), the
    tokens[b, cur[b]] write, stop-sequence match, cur[b] += 1, the row's limit, and the (next id, cache position) pair."""
    _dev(tokens, cur, limit, stopped, stop_pos, live, next_tok, pos)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1 and stopped.dtype == torch.bool and stop_pos.dtype == torch.int64
    assert cur.dtype == limit.dtype == pos.dtype == torch.int32 and next_tok.dtype == torch.int64 and (live is None or live.dtype == torch.int32)
    assert all(t.is_contiguous() and t.numel() >= B for t in (cur, limit, pos, next_tok, stopped, stop_pos))
    if sampled is None:
        assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[0] == B
        lp, ld, V = _p(logits), logits.stride(0), logits.shape[1]
    else:
        assert sampled.dtype == torch.int64 and sampled.is_contiguous() and sampled.numel() == B
        lp, ld, V = None, 0, 1
    rc = _l.load().a3v_generate_step_rows(lp, ld, _p(sampled), B, V, _p(tokens), tokens.stride(0), _p(cur), _p(limit), int(pos_base),
                                          _p(stop_seq), _p(stop_off), int(n_stop), _p(stopped), _p(stop_pos), _p(live), _p(next_tok),
                                          _p(pos), _stream())
    _l.check(rc, "a3v_generate_step_rows")


def rope_kvcache_spans(qkv, q_out, k_cache, vt_cache, cos_sin, pos, nq, B, Q, H, Hkv, hd):
    """Lookup decoding: rope_kvcache_rows over Q query positions per cache row -- virtual row b * Q + j of qkv [B*Q, .] is rotated
    at position pos[b] + j and written there into cache row b (pos, nq: device int32 [B]; an idle query -- pos[b] < 0, j >= nq[b] or
    a position outside the cache -- writes nothing and gets a zero q row)."""
    _dev(qkv, q_out, k_cache, vt_cache, cos_sin, pos, nq)
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (pos, nq))
    assert qkv.shape[0] >= B * Q and q_out.shape[0] >= B * Q
    assert k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.shape[0] >= B and k_cache.dtype == vt_cache.dtype == qkv.dtype
    rc = _l.load().a3v_rope_kvcache_spans(_p(qkv), qkv.stride(0), _p(q_out), q_out.stride(0), _p(k_cache), _p(vt_cache), _p(cos_sin),
                                          _p(pos), _p(nq), B, Q, H, Hkv, hd, k_cache.shape[2], dt(qkv), _stream())
    _l.check(rc, f"a3v_rope_kvcache_spans(B={B},Q={Q},H={H},Hkv={Hkv},hd={hd})")


def rope_kvcache_extend(qkv, q_out, k_cache, vt_cache, cos_sin, q_off, sk, nq_max: int, B, H, Hkv, hd):
    """Extend prefill: the packed rows q_off[b] .. q_off[b+1]-1 of qkv are rotated at positions sk[b]-nq[b] .. sk[b]-1 and written
    there into cache row b (q_off: device int32 [B+1]; sk: device int32 [B], the row's key count after the extend).  Per element
    ``rope_kvcache`` at B = 1 on the row's slice.  A row without a span, or whose span does not fit, writes nothing."""
    _dev(qkv, q_out, k_cache, vt_cache, cos_sin, q_off, sk)
    assert q_off.dtype == sk.dtype == torch.int32 and q_off.is_contiguous() and sk.is_contiguous()
    assert q_off.numel() >= B + 1 and sk.numel() >= B
    assert k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.shape[0] >= B and k_cache.dtype == vt_cache.dtype == qkv.dtype
    rc = _l.load().a3v_rope_kvcache_extend(_p(qkv), qkv.stride(0), _p(q_out), q_out.stride(0), _p(k_cache), _p(vt_cache), _p(cos_sin),
                                           _p(q_off), _p(sk), int(nq_max), B, H, Hkv, hd, k_cache.shape[2], dt(qkv), _stream())
    _l.check(rc, f"a3v_rope_kvcache_extend(B={B},nq_max={nq_max},H={H},Hkv={Hkv},hd={hd})")


def attention_extend_rows_scratch_floats(B: int, H: int, hd: int, sk_max: int) -> int:
    return _l.load().a3v_attention_extend_rows_scratch_floats(B, H, hd, sk_max)


def attention_extend_rows(q, k, vt, out, q_off, sk, nq_max: int, sk_max: int, B, H, Hkv, hd, strides, scratch=None, src_row=None,
                          shared=None):
    """Extend prefill: causal attention of packed query spans (rows q_off[b] .. q_off[b+1]-1 of q / out) over per-row caches of
    sk[b] keys; with ``src_row`` / ``shared`` (both or neither, device int32 [B]) row b reads its keys below min(shared[b], sk[b])
    rounded down to 64 from cache row src_row[b].  Row b is bit-equal to ``attention`` at B = 1, Sq = nq[b], Sk = sk[b], causal.
    bf16 at hd 64 / 128 needs scratch (attention_extend_rows_scratch_floats(B, H, hd, sk_max) floats)."""
    _dev(q, k, vt, out, q_off, sk, src_row, shared, scratch)
    assert q_off.dtype == sk.dtype == torch.int32 and q_off.is_contiguous() and sk.is_contiguous()
    assert q_off.numel() >= B + 1 and sk.numel() >= B and k.shape[0] >= B and vt.shape[0] >= B
    assert (src_row is None) == (shared is None)
    if src_row is not None:
        assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (src_row, shared))
    assert scratch is None or (scratch.dtype == torch.float32 and scratch.numel() >= attention_extend_rows_scratch_floats(B, H, hd, sk_max))
    rc = _l.load().a3v_attention_extend_rows(_p(q), _p(k), _p(vt), _p(out), _p(q_off), _p(sk), _p(src_row), _p(shared), int(nq_max),
                                             int(sk_max), B, H, Hkv, hd, _Strides(*strides), _p(scratch), dt(q), _stream())
    _l.check(rc, f"a3v_attention_extend_rows(B={B},nq_max={nq_max},sk_max={sk_max},H={H},hd={hd})")
    return out


def attention_verify_rows_splits(B: int, H: int, sk_max: int) -> int:
    return _l.load().a3v_attention_verify_rows_splits(B, H, sk_max)


def attention_verify_rows_scratch_floats(B: int, Q: int, H: int, hd: int, sk_max: int) -> int:
    return _l.load().a3v_attention_verify_rows_scratch_floats(B, Q, H, hd, sk_max)


def attention_verify_rows(q, k, vt, out, pos, nq, sk_max: int, B, Q, H, Hkv, hd, strides, scratch=None, counters=None):
    """Lookup decoding: query j of cache row b (virtual row b * Q + j of q / out) attends to keys [0, pos[b] + j + 1) of cache row
    b; pos, nq device int32 [B]; strides as ``attention`` at Sq = 1 with the q / out batch strides per virtual row.  bf16 at hd
    64 / 128 needs scratch (attention_verify_rows_scratch_floats) and counters (int32 [>= 2*B*H], zero; left zero)."""
    _dev(q, k, vt, out, pos, nq, scratch, counters)
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (pos, nq))
    assert k.shape[0] >= B and vt.shape[0] >= B and q.shape[0] >= B * Q and out.shape[0] >= B * Q
    assert scratch is None or (scratch.dtype == torch.float32 and scratch.numel() >= attention_verify_rows_scratch_floats(B, Q, H, hd, sk_max))
    assert counters is None or (counters.dtype == torch.int32 and counters.numel() >= 2 * B * H)
    rc = _l.load().a3v_attention_verify_rows(_p(q), _p(k), _p(vt), _p(out), _p(pos), _p(nq), int(sk_max), B, Q, H, Hkv, hd,
                                             _Strides(*strides), _p(scratch), _p(counters), dt(q), _stream())
    _l.check(rc, f"a3v_attention_verify_rows(B={B},Q={Q},sk_max={sk_max},H={H},hd={hd})")
    return out


def lookup_draft_rows(tokens, cur, limit, pos, stopped, next_tok, D: int, max_ngram: int, Smax: int, x, nq):
    """Prompt-lookup drafts (a3v_lookup_draft_rows): x [B, D+1] int64 = the row's next id and up to D drafts copied from behind the
    latest earlier occurrence of its last n-gram (n = max_ngram .. 1), nq [B] int32 = 1 + the number of drafts."""
    _dev(tokens, cur, limit, pos, stopped, next_tok, x, nq)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1 and stopped.dtype == torch.bool and next_tok.dtype == x.dtype == torch.int64
    assert cur.dtype == limit.dtype == pos.dtype == nq.dtype == torch.int32
    assert all(t.is_contiguous() and t.numel() >= B for t in (cur, limit, pos, stopped, next_tok, nq))
    assert x.is_contiguous() and tuple(x.shape) == (B, D + 1)
    rc = _l.load().a3v_lookup_draft_rows(_p(tokens), tokens.stride(0), _p(cur), _p(limit), _p(pos), _p(stopped), _p(next_tok), B, int(D),
                                         int(max_ngram), int(Smax), _p(x), _p(nq), _stream())
    _l.check(rc, f"a3v_lookup_draft_rows(B={B},D={D},max_ngram={max_ngram})")


def accept_rows(logits, x, nq, tokens, cur, limit, pos_base: int, stop_seq, stop_off, n_stop: int, stopped, stop_pos, next_tok, pos,
                stats=None):
    """One launch = the bookkeeping of a lookup-decoding step (a3v_accept_rows): the argmax of every query's logits row, then per
    cache row as many ``generate_step_rows`` token steps as the drafts x[b, 1..] agree with.  stats: int64 [2] (drafted, accepted)."""
    _dev(logits, x, nq, tokens, cur, limit, stopped, stop_pos, next_tok, pos, stats)
    B, Q = x.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[0] == B * Q
    assert tokens.dtype == x.dtype == torch.int64 and tokens.stride(1) == 1 and tokens.shape[0] == B and x.is_contiguous()
    assert stopped.dtype == torch.bool and stop_pos.dtype == torch.int64 and next_tok.dtype == torch.int64
    assert cur.dtype == limit.dtype == pos.dtype == nq.dtype == torch.int32
    assert all(t.is_contiguous() and t.numel() >= B for t in (cur, limit, pos, nq, next_tok, stopped, stop_pos))
    assert stats is None or (stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 2)
    rc = _l.load().a3v_accept_rows(_p(logits), logits.stride(0), B, Q, logits.shape[1], _p(x), _p(nq), _p(tokens), tokens.stride(0),
                                   _p(cur), _p(limit), int(pos_base), _p(stop_seq), _p(stop_off), int(n_stop), _p(stopped), _p(stop_pos),
                                   _p(next_tok), _p(pos), _p(stats), _stream())
    _l.check(rc, f"a3v_accept_rows(B={B},Q={Q})")


def embed_assemble(tokens, table, h, B, T, W, dim):
    _dev(tokens, table, h)
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1
    rc = _l.load().a3v_embed_assemble(_p(tokens), tokens.stride(0), _p(table), _p(h), B, T, W, dim, table.shape[0],
                                      dt(table), dt(h), _stream())
    _l.check(rc, "a3v_embed_assemble")


def fill_rows(src, dst, row_idx):
    _dev(src, dst, row_idx)
    assert row_idx.dtype == torch.int32
    rc = _l.load().a3v_fill_rows(_p(src), _p(dst), dst.stride(0), _p(row_idx), row_idx.numel(), dst.shape[1],
                                 dt(src), dt(dst), _stream())
    _l.check(rc, "a3v_fill_rows")


def patch_im2col(img, cols, P):
    _dev(img, cols)
    N, C, Hi, Wi = img.shape
    assert C == 3 and img.is_contiguous()
    rc = _l.load().a3v_patch_im2col(_p(img), _p(cols), N, Hi, Wi, P, cols.shape[1], dt(img), dt(cols), _stream())
    _l.check(rc, "a3v_patch_im2col")


def split_views(img, out):
    _dev(img, out)
    B, C, S2, _ = img.shape
    assert C == 3 and img.is_contiguous() and out.is_contiguous()
    rc = _l.load().a3v_split_views(_p(img), _p(out), B, S2 // 2, dt(img), dt(out), _stream())
    _l.check(rc, "a3v_split_views")


def vit_embed(patch, cls, pos, x, N, T, width):
    _dev(patch, cls, pos, x)
    rc = _l.load().a3v_vit_embed(_p(patch), _p(cls), _p(pos), _p(x), N, T, width, dt(patch), _stream())
    _l.check(rc, "a3v_vit_embed")


def generate_step(logits, sampled, tokens, text_mask, cur_pos: int, stop_seq, stop_off, n_stop: int, stopped, stop_pos, live):
    """One launch = one step of MetaModel.generate's bookkeeping (a3v_generate_step): argmax (or the sampled ids), teacher
    forcing, tokens[:, cur_pos] write, stop-sequence match, stop_pos / stopped / live update."""
    _dev(tokens, text_mask, stopped, stop_pos, live)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and text_mask.dtype == torch.bool and stopped.dtype == torch.bool and stop_pos.dtype == torch.int64
    assert tokens.stride(1) == 1 and text_mask.stride(1) == 1 and (live is None or live.dtype == torch.int32)      # live is optional in the C ABI
    if sampled is None:
        assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[0] == B
        lp, ld, V = _p(logits), logits.stride(0), logits.shape[1]
    else:
        assert sampled.dtype == torch.int64 and sampled.is_contiguous() and sampled.numel() == B
        lp, ld, V = None, 0, 1
    rc = _l.load().a3v_generate_step(lp, ld, _p(sampled), B, V, _p(tokens), tokens.stride(0), _p(text_mask), text_mask.stride(0), int(cur_pos),
                                     _p(stop_seq), _p(stop_off), int(n_stop), _p(stopped), _p(stop_pos), _p(live), _stream())
    _l.check(rc, "a3v_generate_step")


def sample_top_p(logits, temperature: float, top_p: float, u, out):
    """out[b] = one draw from the top-p nucleus of softmax(logits[b] / temperature) at the uniform number u[b] (a3v_sample_top_p;
    model/meta.py:456-459, 568-583 without the full-vocabulary sort)."""
    _dev(logits, u, out)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and u.dtype == torch.float32 and out.dtype == torch.int64
    B, V = logits.shape
    assert u.numel() >= B and out.numel() >= B and u.is_contiguous() and out.is_contiguous()
    rc = _l.load().a3v_sample_top_p(_p(logits), logits.stride(0), B, V, float(temperature), float(top_p), _p(u), _p(out), _stream())
    _l.check(rc, "a3v_sample_top_p")
    return out


def sample_top_k_p(logits, temperature: float, top_k: int, top_p: float, min_p: float, u, out):
    """sample_top_p with HF's two other filters, in HF's order (a3v_sample_top_k_p): top-k on the logits' own bits (0 or >= V: off,
    ties at the k-th value kept), then top-p over what is left, then min-p (p_i >= min_p * p_max; 0: off), one draw at u[b]."""
    _dev(logits, u, out)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and u.dtype == torch.float32 and out.dtype == torch.int64
    B, V = logits.shape
    assert u.numel() >= B and out.numel() >= B and u.is_contiguous() and out.is_contiguous()
    rc = _l.load().a3v_sample_top_k_p(_p(logits), logits.stride(0), B, V, float(temperature), int(top_k), float(top_p), float(min_p),
                                      _p(u), _p(out), _stream())
    _l.check(rc, "a3v_sample_top_k_p")
    return out


def argmax(logits, out):
    _dev(logits, out)
    assert logits.dtype == torch.float32 and out.dtype == torch.int64
    B, V = logits.shape
    rc = _l.load().a3v_argmax(_p(logits), logits.stride(0), _p(out), B, V, _stream())
    _l.check(rc, "a3v_argmax")
    return out


def _seen_ok(seen, rows: int, V: int):
    assert seen.dtype == torch.int32 and seen.dim() == 2 and seen.stride(1) == 1 and seen.shape[0] >= rows
    assert seen.stride(0) >= (V + 31) // 32, (seen.stride(0), V)


def seen_mark(tokens, lens, seen, V: int):
    """seen[b] |= bits of tokens[b, :lens[b]] (a3v_seen_mark; seen: int32 storage of the uint32 bitmap [B, >= ceil(V / 32)], the row
    stride is its words_per_row).  Ids outside [0, V) are ignored; lens[b] <= 0 leaves the row alone."""
    _dev(tokens, lens, seen)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.stride(1) == 1
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() >= B
    _seen_ok(seen, B, V)
    rc = _l.load().a3v_seen_mark(_p(tokens), tokens.stride(0), _p(lens), _p(seen), seen.stride(0), B, int(V), _stream())
    _l.check(rc, "a3v_seen_mark")
    return seen


def seen_clear_rows(seen, rows):
    """Zero the bitmap rows listed in ``rows`` (device int32; a3v_seen_clear_rows): seen.shape[1] words of each."""
    _dev(seen, rows)
    assert seen.dtype == torch.int32 and seen.dim() == 2 and seen.stride(1) == 1
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() > 0
    rc = _l.load().a3v_seen_clear_rows(_p(seen), _p(rows), rows.numel(), seen.stride(0), seen.shape[1], seen.shape[0], _stream())
    _l.check(rc, "a3v_seen_clear_rows")
    return seen


def logits_prepare(logits, seen, penalty: float, out, lse):
    """One launch, one pass over every row of the raw fp32 logits (a3v_logits_prepare): ``out`` = the rows under the repetition
    penalty of the ``seen`` bitmap (seen None: out is not touched), ``lse[b]`` = logsumexp of the RAW row (lse None: not computed).
    The logits are never written."""
    _dev(logits, seen, out, lse)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    B, V = logits.shape
    assert seen is not None or lse is not None
    if seen is not None:
        _seen_ok(seen, B, V)
        assert out.dtype == torch.float32 and out.shape == logits.shape and out.stride(1) == 1 and out.data_ptr() != logits.data_ptr()
        assert penalty > 0, penalty
    assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B)
    rc = _l.load().a3v_logits_prepare(_p(logits), logits.stride(0), _p(seen), seen.stride(0) if seen is not None else 0, float(penalty),
                                      _p(out), out.stride(0) if out is not None else 0, _p(lse), B, V, _stream())
    _l.check(rc, "a3v_logits_prepare")


def generate_record(logits, lse, tokens, seen, logprob, *, col: int = 0, cur=None, stopped_before=None, idx: int = 0, prompt_len=None):
    """After generate_step / generate_step_rows wrote the chosen ids (a3v_generate_record): per row the id of column ``col`` (uniform
    step) or ``cur[b] - 1`` (ragged), logprob[b, g] = logits[b, id] - lse[b] at the generated index g = column - prompt_len[b] (or
    ``idx``), and the id's bit in ``seen``.  Rows with ``stopped_before[b]`` set, idle rows and teacher-forced positions (g < 0)
    write nothing.  ``seen`` / ``logprob`` may be None (not both)."""
    _dev(logits, lse, tokens, seen, logprob, cur, stopped_before, prompt_len)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.stride(1) == 1
    assert seen is not None or logprob is not None
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == B     # also names V
    V = logits.shape[1]
    if logprob is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B
        assert logprob.dtype == torch.float32 and logprob.dim() == 2 and logprob.stride(1) == 1 and logprob.shape[0] >= B
    if seen is not None:
        _seen_ok(seen, B, V)
    for t, d in ((cur, torch.int32), (stopped_before, torch.bool), (prompt_len, torch.int32)):
        assert t is None or (t.dtype == d and t.is_contiguous() and t.numel() >= B)
    rc = _l.load().a3v_generate_record(_p(logits), logits.stride(0), _p(lse), _p(tokens), tokens.stride(0),
                                       int(col), _p(cur), _p(stopped_before), _p(seen), seen.stride(0) if seen is not None else 0,
                                       _p(logprob), logprob.stride(0) if logprob is not None else 0,
                                       logprob.shape[1] if logprob is not None else 0, int(idx), _p(prompt_len), B, int(V),
                                       _stream())
    _l.check(rc, "a3v_generate_record")


def _trans_ok(trans, V: int):
    assert trans.dtype == torch.int16 and trans.dim() == 2 and trans.is_contiguous() and trans.shape[1] == V, (tuple(trans.shape), V)
    assert 1 <= trans.shape[0] <= 32767, trans.shape[0]


def constrain_logits(logits, trans, state, out):
    """One launch (a3v_constrain_logits): out[b, v] = logits[b, v] where the token automaton ``trans`` (int16 [n_states, V]) allows
    token v in ``state[b]`` (device int32), -inf elsewhere; a row whose state is outside [0, n_states) is copied unchanged.  ``out``
    may be ``logits`` itself (in place).  Kept values keep their bits."""
    _dev(logits, trans, state, out)
    assert logits.dtype == out.dtype == torch.float32 and logits.dim() == out.dim() == 2 and logits.stride(1) == out.stride(1) == 1
    B, V = logits.shape
    assert out.shape == logits.shape, (tuple(out.shape), tuple(logits.shape))
    _trans_ok(trans, V)
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= B
    rc = _l.load().a3v_constrain_logits(_p(logits), logits.stride(0), _p(trans), V, trans.shape[0], _p(state), _p(out), out.stride(0), B,
                                        _stream())
    _l.check(rc, "a3v_constrain_logits")
    return out


def constrain_advance(tokens, trans, state, first, *, col: int = 0, cur=None, stopped_before=None):
    """After generate_step / generate_step_rows wrote the chosen ids (a3v_constrain_advance): state[b] = trans[state[b], id] for the id
    of column ``col`` (uniform step) or ``cur[b] - 1`` (ragged).  Rows with ``stopped_before[b]`` set, idle rows, columns below
    ``first[b]`` (teacher-forced prompt tokens), out-of-range states and ids change nothing."""
    _dev(tokens, trans, state, first, cur, stopped_before)
    B = tokens.shape[0]
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.stride(1) == 1
    _trans_ok(trans, trans.shape[1])
    for t, d in ((state, torch.int32), (first, torch.int32), (cur, torch.int32), (stopped_before, torch.bool)):
        assert t is None or (t.dtype == d and t.is_contiguous() and t.numel() >= B)
    rc = _l.load().a3v_constrain_advance(_p(tokens), tokens.stride(0), int(col), _p(cur), _p(first), _p(stopped_before), _p(trans),
                                         trans.shape[1], trans.shape[0], _p(state), B, _stream())
    _l.check(rc, "a3v_constrain_advance")
    return state


def beam_select(logits, lse, cum, alive, K: int, cand_score, cand_beam, cand_tok, *, trans=None, state=None):
    """One launch (a3v_beam_select): per group of ``K`` consecutive rows of the raw fp32 ``logits`` [R, V] (any row stride) the best
    2K candidates (beam, token) of the rows with ``alive`` set, scored cum[b] + (z[b, v] - lse[b]), ordered by score descending,
    then b * V + v ascending, into cand_* [G, 2K]; unfilled slots (-inf, -1, -1).  ``trans`` / ``state``: only tokens the automaton
    allows in the row's state (a state outside [0, n_states): every token)."""
    _dev(logits, lse, cum, alive, cand_score, cand_beam, cand_tok, trans, state)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R, V = logits.shape
    K = int(K)
    assert 1 <= K <= 8 and R % K == 0, (R, K)
    G = R // K
    for t, d in ((lse, torch.float32), (cum, torch.float32), (alive, torch.uint8)):
        assert t.dtype == d and t.is_contiguous() and t.numel() >= R
    for t, d in ((cand_score, torch.float32), (cand_beam, torch.int32), (cand_tok, torch.int32)):
        assert t.dtype == d and t.is_contiguous() and tuple(t.shape) == (G, 2 * K), (tuple(t.shape), G, K)
    if trans is not None:
        _trans_ok(trans, V)
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= R
    rc = _l.load().a3v_beam_select(_p(logits), logits.stride(0), _p(lse), _p(cum), _p(alive), _p(trans),
                                   trans.shape[0] if trans is not None else 0, _p(state), G, K, V, _p(cand_score), _p(cand_beam),
                                   _p(cand_tok), _stream())
    _l.check(rc, f"a3v_beam_select(G={G},K={K},V={V})")


def beam_advance(cand_score, cand_beam, cand_tok, st, tokens_in, tokens_out, V: int, eos: int, early_stopping: bool, len_div,
                 pos_cap: int, *, trans=None):
    """One launch (a3v_beam_advance): the walk over the 2K candidates of every group that is not done.  ``st`` carries the device
    state (model/beam.py ``BeamState``: cum, alive, state, glen, done, parent, next_tok, pos, base, limit and the pool); the
    token rows are read from ``tokens_in`` and written to ``tokens_out`` (the caller swaps them every step)."""
    G, K2 = cand_score.shape
    K = K2 // 2
    R = G * K
    _dev(cand_score, cand_beam, cand_tok, tokens_in, tokens_out, len_div, trans)
    per_row = ((st.cum, torch.float32), (st.alive, torch.uint8), (st.state, torch.int32), (st.parent, torch.int32),
               (st.next_tok, torch.int64), (st.pos, torch.int32))
    per_group = ((st.glen, torch.int32), (st.done, torch.uint8), (st.base, torch.int32), (st.limit, torch.int32),
                 (st.pool_n, torch.int32), (st.pool_added, torch.int32))
    pool = ((st.pool_score, torch.float32), (st.pool_cum, torch.float32), (st.pool_len, torch.int32), (st.pool_seq, torch.int32))
    for group, n in ((per_row, R), (per_group, G), (pool, R)):
        for t, d in group:
            assert t.is_cuda and t.dtype == d and t.is_contiguous() and t.numel() == n, (t.dtype, d, t.numel(), n)
    for t in (tokens_in, tokens_out):
        assert t.dtype == torch.int64 and tuple(t.shape) == (R, tokens_in.shape[1]) and t.is_contiguous()
    ld = tokens_in.shape[1]
    assert tokens_in.data_ptr() != tokens_out.data_ptr()
    assert st.pool_ids.dtype == torch.int64 and tuple(st.pool_ids.shape) == (G, K, ld) and st.pool_ids.is_contiguous() and st.pool_ids.is_cuda
    assert len_div.dtype == torch.float32 and len_div.is_contiguous() and len_div.numel() >= 2
    assert all(t.dtype == d and t.is_contiguous() for t, d in ((cand_score, torch.float32), (cand_beam, torch.int32), (cand_tok, torch.int32)))
    if trans is not None:
        _trans_ok(trans, V)
    rc = _l.load().a3v_beam_advance(_p(cand_score), _p(cand_beam), _p(cand_tok), G, K, int(V), int(eos), int(bool(early_stopping)),
                                    _p(len_div), len_div.numel(), _p(trans), trans.shape[0] if trans is not None else 0, _p(st.base),
                                    _p(st.limit), int(pos_cap), _p(st.cum), _p(st.alive), _p(st.state), _p(st.glen), _p(st.done),
                                    _p(st.parent), _p(st.next_tok), _p(st.pos), _p(tokens_in), _p(tokens_out), ld, _p(st.pool_n),
                                    _p(st.pool_added), _p(st.pool_score), _p(st.pool_cum), _p(st.pool_len), _p(st.pool_seq),
                                    _p(st.pool_ids), _stream())
    _l.check(rc, f"a3v_beam_advance(G={G},K={K},V={V})")


def kv_permute_tails(k_caches, vt_caches, parent, tail_lo, pos, tail_max: int, K: int, ptrs=None):
    """One launch over every layer (a3v_kv_permute_tails): for every cache row r with parent[r] != r the positions
    [tail_lo[r], pos[r]) of row parent[r] (a row of r's group of ``K`` consecutive rows; the values from before the call) replace
    the same positions of row r in K [B,Hkv,Smax,hd] and V^T [B,Hkv,hd,Smax].  parent / tail_lo / pos: device int32 [B];
    ``tail_max`` (host) >= max(pos) - min(tail_lo) over the moved rows of every group.  ``ptrs`` as in ``kv_copy_span`` (returned either way)."""
    k0 = k_caches[0]
    B, Hkv, Smax, hd = k0.shape
    K = int(K)
    assert 1 <= K <= 8 and B % K == 0, (B, K)
    for k, v in zip(k_caches, vt_caches):
        _dev(k, v)
        assert k.is_contiguous() and v.is_contiguous() and k.dtype == v.dtype == k0.dtype
        assert tuple(k.shape) == (B, Hkv, Smax, hd) and tuple(v.shape) == (B, Hkv, hd, Smax)
    _dev(parent, tail_lo, pos)
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B for t in (parent, tail_lo, pos))
    if ptrs is None:
        ptrs = torch.tensor([[t.data_ptr() for t in k_caches], [t.data_ptr() for t in vt_caches]], dtype=torch.int64, device=k0.device)
    assert ptrs.dtype == torch.int64 and tuple(ptrs.shape) == (2, len(k_caches)) and ptrs.is_contiguous()
    rc = _l.load().a3v_kv_permute_tails(_p(ptrs[0]), _p(ptrs[1]), len(k_caches), _p(parent), _p(tail_lo), _p(pos), int(tail_max), B // K, K,
                                        Hkv, hd, Smax, dt(k0), _stream())
    _l.check(rc, f"a3v_kv_permute_tails(K={K},tail_max={tail_max},hd={hd})")
    return ptrs


def verify_prepare(logits, x, nq, pos, out, *, seen=None, penalty: float = 1.0, trans=None, state=None, lse=None):
    """Lookup decoding, sample and match (a3v_verify_prepare): one pass over the fp32 verify logits [B*Q, V].  ``out`` row b * Q + j =
    the row as the plain loop would prepare it if drafts x[b, 1..j] had been emitted: the repetition penalty over ``seen[b]`` and
    those drafts (seen None: none), then the automaton's mask in the state reached from ``state[b]`` over them (trans None: none; a
    forbidden draft: the row is all -inf); ``lse`` (None: not computed) = logsumexp of the RAW rows.  Idle queries: zeros."""
    _dev(logits, x, nq, pos, out, seen, trans, state, lse)
    B, Q = x.shape
    assert logits.dtype == out.dtype == torch.float32 and logits.dim() == out.dim() == 2 and logits.stride(1) == out.stride(1) == 1
    assert logits.shape[0] == B * Q and out.shape == logits.shape and out.data_ptr() != logits.data_ptr()
    V = logits.shape[1]
    assert x.dtype == torch.int64 and x.is_contiguous()
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (nq, pos))
    if seen is not None:
        _seen_ok(seen, B, V)
        assert penalty > 0, penalty
    if trans is not None:
        _trans_ok(trans, V)
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= B
    assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * Q)
    rc = _l.load().a3v_verify_prepare(_p(logits), logits.stride(0), B, Q, V, _p(x), _p(nq), _p(pos), _p(seen),
                                      seen.stride(0) if seen is not None else 0, float(penalty), _p(trans),
                                      trans.shape[0] if trans is not None else 0, _p(state) if trans is not None else None, _p(lse), _p(out),
                                      out.stride(0), _stream())
    _l.check(rc, f"a3v_verify_prepare(B={B},Q={Q},V={V})")
    return out


def accept_rows_chosen(chosen, x, nq, tokens, cur, limit, pos_base: int, stop_seq, stop_off, n_stop: int, stopped, stop_pos, next_tok, pos,
                       stats=None, *, V: int = 0, logits=None, lse=None, logprob=None, prompt_len=None, seen=None, trans=None, state=None):
    """``accept_rows`` with the per-query choice handed in (a3v_accept_rows_chosen; chosen int64 [B*Q]), plus per emission the plain
    loop's bookkeeping: logprob[b, g] = logits[m, id] - lse[m] on the RAW logits of the producing query, the id's bit in ``seen``,
    ``state[b] = trans[state[b], id]``.  Each of logprob / seen / state may be None; with any of them ``prompt_len`` is needed."""
    _dev(chosen, x, nq, tokens, cur, limit, stopped, stop_pos, next_tok, pos, stats, logits, lse, logprob, prompt_len, seen, trans, state)
    B, Q = x.shape
    assert chosen.dtype == torch.int64 and chosen.is_contiguous() and chosen.numel() >= B * Q
    assert tokens.dtype == x.dtype == torch.int64 and tokens.stride(1) == 1 and tokens.shape[0] == B and x.is_contiguous()
    assert stopped.dtype == torch.bool and stop_pos.dtype == torch.int64 and next_tok.dtype == torch.int64
    assert cur.dtype == limit.dtype == pos.dtype == nq.dtype == torch.int32
    assert all(t.is_contiguous() and t.numel() >= B for t in (cur, limit, pos, nq, next_tok, stopped, stop_pos))
    assert stats is None or (stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 2)
    book = logprob is not None or seen is not None or state is not None
    if book:
        assert V > 0, "the vocabulary size V is needed with logprob / seen / state"
        assert prompt_len is not None and prompt_len.dtype == torch.int32 and prompt_len.is_contiguous() and prompt_len.numel() >= B
    if logprob is not None:
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == B * Q
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * Q
        assert logprob.dtype == torch.float32 and logprob.dim() == 2 and logprob.stride(1) == 1 and logprob.shape[0] >= B
    if seen is not None:
        _seen_ok(seen, B, V)
    if state is not None:
        _trans_ok(trans, V)
        assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= B
    rc = _l.load().a3v_accept_rows_chosen(_p(chosen), B, Q, _p(x), _p(nq), _p(tokens), tokens.stride(0), _p(cur), _p(limit), int(pos_base),
                                          _p(stop_seq), _p(stop_off), int(n_stop), _p(stopped), _p(stop_pos), _p(next_tok), _p(pos), _p(stats),
                                          _p(logits) if logprob is not None else None, logits.stride(0) if logprob is not None else 0, int(V),
                                          _p(lse) if logprob is not None else None, _p(logprob),
                                          logprob.stride(0) if logprob is not None else 0, logprob.shape[1] if logprob is not None else 0,
                                          _p(prompt_len) if book else None, _p(seen), seen.stride(0) if seen is not None else 0,
                                          _p(trans) if state is not None else None, trans.shape[0] if state is not None else 0, _p(state),
                                          _stream())
    _l.check(rc, f"a3v_accept_rows_chosen(B={B},Q={Q})")


def verify_uniforms(uni, row_base, cur, prompt_len, Q: int, u):
    """u[b * Q + j] = uni[row_base[b] + (cur[b] - prompt_len[b]) + j], clamped into ``uni`` (a3v_verify_uniforms): the uniform number
    the plain loop draws the token of that generated index with."""
    _dev(uni, row_base, cur, prompt_len, u)
    B = row_base.numel()
    assert uni.dtype == u.dtype == torch.float32 and uni.is_contiguous() and u.is_contiguous() and u.numel() >= B * Q and uni.numel() > 0
    assert row_base.dtype == torch.int64 and row_base.is_contiguous()
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= B for t in (cur, prompt_len))
    rc = _l.load().a3v_verify_uniforms(_p(uni), uni.numel(), _p(row_base), _p(cur), _p(prompt_len), B, int(Q), _p(u), _stream())
    _l.check(rc, "a3v_verify_uniforms")
    return u


def count_valid(labels, n_valid):
    _dev(labels, n_valid)
    rc = _l.load().a3v_count_valid(_p(labels), labels.numel(), _p(n_valid), _stream())
    _l.check(rc, "a3v_count_valid")


_count_host = {}


def label_rows(labels, W: int, S: int, stream_rows, head_rows, labels_out, count) -> int:
    """The rows the loss reads (a3v_label_rows) into the caller's buffers (room for B T entries each); returns their number, read
    back through ONE pinned 4-byte copy -- the caller's only wait for the device."""
    _dev(labels, stream_rows, head_rows, labels_out, count)
    B, T = labels.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and stream_rows.dtype == torch.int32 and head_rows.dtype == torch.int32
    assert min(stream_rows.numel(), head_rows.numel()) >= B * T and (labels_out is None or (labels_out.dtype == torch.int64 and labels_out.numel() >= B * T))
    assert count.dtype == torch.int32 and stream_rows.is_contiguous() and head_rows.is_contiguous()
    rc = _l.load().a3v_label_rows(_p(labels), B, T, W, S, _p(stream_rows), _p(head_rows), _p(labels_out), _p(count), _stream())
    _l.check(rc, "a3v_label_rows")
    host = _count_host.get(count.device)
    if host is None:
        host = _count_host[count.device] = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(count, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return int(host[0])


def gather_rows(src, row_idx, out):
    """out[i] = src[row_idx[i]] (bf16 / fp32 rows in 16-byte pieces)."""
    _dev(src, row_idx, out)
    n, cols = out.shape
    assert row_idx.dtype == torch.int32 and row_idx.is_contiguous() and row_idx.numel() == n and src.shape[1] == cols and src.dtype == out.dtype
    assert src.stride(1) == 1 and out.stride(1) == 1
    rc = _l.load().a3v_gather_rows(_p(src), src.stride(0), src.shape[0], _p(row_idx), n, _p(out), out.stride(0), cols, dt(src), _stream())
    _l.check(rc, "a3v_gather_rows")
    return out


def scatter_rows(src, row_idx, out):
    """out[row_idx[i]] = src[i] for an ascending list without repeats; every other row of out = 0 (written by the same launch)."""
    _dev(src, row_idx, out)
    n, cols = src.shape
    assert row_idx.dtype == torch.int32 and row_idx.is_contiguous() and row_idx.numel() == n and out.shape[1] == cols and src.dtype == out.dtype
    assert src.stride(1) == 1 and out.stride(1) == 1 and n <= out.shape[0]
    rc = _l.load().a3v_scatter_rows(_p(src), src.stride(0), _p(row_idx), n, _p(out), out.stride(0), out.shape[0], cols, dt(src), _stream())
    _l.check(rc, "a3v_scatter_rows")
    return out


def cross_entropy(logits, labels, row_loss, dlogits=None, n_valid=None, grad_scale: float = 1.0):
    _dev(logits, labels, row_loss, dlogits, n_valid)
    rows, V = logits.shape
    rc = _l.load().a3v_cross_entropy(_p(logits), logits.stride(0), _p(labels), _p(row_loss), _p(dlogits),
                                     dlogits.stride(0) if dlogits is not None else 0, _p(n_valid), grad_scale,
                                     rows, V, dt(logits), _stream())
    _l.check(rc, "a3v_cross_entropy")


# ------------------------------------------------------------------ training (backward) ops
def attention_lse(q, k, vt, out, lse, B, Sq, Sk, H, Hkv, hd, strides, causal: bool):
    _dev(q, k, vt, out, lse)
    rc = _l.load().a3v_attention_lse(_p(q), _p(k), _p(vt), _p(out), _p(lse), B, Sq, Sk, H, Hkv, hd, _Strides(*strides),
                                     1 if causal else 0, dt(q), _stream())
    _l.check(rc, "a3v_attention_lse")


def transpose(src, dst, R, C, Rpad, batch=1, bs_src=0, bs_dst=0):
    """dst[b, c, r] = src[b, r, c]; src/dst 2-D (or batched through element strides)."""
    _dev(src, dst)
    rc = _l.load().a3v_transpose(_p(src), src.stride(-2), bs_src, _p(dst), dst.stride(-2), bs_dst, R, C, Rpad, batch,
                                 dt(src), _stream())
    _l.check(rc, "a3v_transpose")
    return dst


def cast(src, dst):
    _dev(src, dst)
    rows, cols = src.shape
    rc = _l.load().a3v_cast(_p(src), src.stride(0), dt(src), _p(dst), dst.stride(0), dt(dst), rows, cols, _stream())
    _l.check(rc, "a3v_cast")
    return dst


def scale_cast(src, dst, scale: float = 1.0):
    """dst = (dst.dtype)(src * scale) over contiguous 1-D buffers of equal length (DP gradient wire conversions)."""
    _dev(src, dst)
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    rc = _l.load().a3v_scale_cast(_p(src), dt(src), _p(dst), dt(dst), src.numel(), float(scale), _stream())
    _l.check(rc, "a3v_scale_cast")
    return dst


SUMSQ_SLOTS = 1024


def sumsq_partials(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[0 .. SUMSQ_SLOTS) = partial sums of squares of the fp32 vector x (deterministic; the clip's norm = sqrt of their sum)."""
    _dev(x, out)
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and out.numel() >= SUMSQ_SLOTS and x.is_contiguous() and out.is_contiguous()
    rc = _l.load().a3v_sumsq_partials(_p(x), x.numel(), _p(out), _stream())
    _l.check(rc, "a3v_sumsq_partials")
    return out


def add2d(dst, src):
    """dst += src (2-D blocks of one dtype, arbitrary row strides)."""
    _dev(dst, src)
    assert dst.dtype == src.dtype and dst.shape == src.shape
    rows, cols = dst.shape
    rc = _l.load().a3v_add2d(_p(dst), dst.stride(0), _p(src), src.stride(0), rows, cols, dt(dst), _stream())
    _l.check(rc, "a3v_add2d")
    return dst


_rb_scratch = {}


def rmsnorm_bwd(x, w, dy, dh, dw, eps, dh_lowp=None, row_idx=None):
    """dh += d(rmsnorm)/dx . dy (fp32 stream), dw += ...; ``dh_lowp``: the updated dh also as bf16 (the next GEMMs' operand).
    ``row_idx`` (int32 [n], no repeats; bf16 stream): dy [n, dim] is compact, its row i belongs to x row row_idx[i] and dh row row_idx[i]."""
    _dev(x, w, dy, dh, dw, dh_lowp, row_idx)
    assert w.dtype == torch.float32 and x.dtype == dh.dtype and x.dtype in (torch.float32, torch.bfloat16)
    rows, dim = x.shape
    if row_idx is not None:
        assert row_idx.dtype == torch.int32 and row_idx.is_contiguous() and x.dtype == torch.bfloat16 and dh_lowp is None
        rows = row_idx.numel()
        assert dy.shape[0] == rows
    scratch = None
    if dw is not None:                       # per-device scratch for the weight-gradient partial rows (grown on demand)
        need = int(_l.load().a3v_rmsnorm_bwd_scratch_floats(rows, dim))
        scratch = _rb_scratch.get(x.device)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(need, dtype=torch.float32, device=x.device)
            _rb_scratch[x.device] = scratch
    if x.dtype == torch.bfloat16:            # bf16 residual stream: x, dy and the accumulated dh are bf16 (fp32 arithmetic inside)
        assert dh_lowp is None and dy.dtype == torch.bfloat16
        if row_idx is not None:
            rc = _l.load().a3v_rmsnorm_bwd_rows_bf16(_p(x), x.stride(0), _p(row_idx), _p(w), _p(dy), dy.stride(0), _p(dh), dh.stride(0), _p(dw),
                                                     _p(scratch), rows, dim, eps, _stream())
            _l.check(rc, "a3v_rmsnorm_bwd_rows_bf16")
            return
        rc = _l.load().a3v_rmsnorm_bwd_bf16(_p(x), x.stride(0), _p(w), _p(dy), dy.stride(0), _p(dh), dh.stride(0), _p(dw), _p(scratch), rows,
                                            dim, eps, _stream())
        _l.check(rc, "a3v_rmsnorm_bwd_bf16")
        return
    if dh_lowp is not None:
        assert dh_lowp.dtype == torch.bfloat16 and dh_lowp.shape == dh.shape
        rc = _l.load().a3v_rmsnorm_bwd_cast(_p(x), x.stride(0), _p(w), _p(dy), dy.stride(0), _p(dh), dh.stride(0), _p(dw), _p(scratch), rows,
                                            dim, eps, dt(dy), _p(dh_lowp), dh_lowp.stride(0), _stream())
        _l.check(rc, "a3v_rmsnorm_bwd_cast")
        return
    rc = _l.load().a3v_rmsnorm_bwd(_p(x), x.stride(0), _p(w), _p(dy), dy.stride(0), _p(dh), dh.stride(0), _p(dw), _p(scratch), rows, dim,
                                   eps, dt(dy), _stream())
    _l.check(rc, "a3v_rmsnorm_bwd")


def layernorm_bwd(x, w, dy, row_map, dx, dw, db, eps=1e-5):
    _dev(x, w, dy, row_map, dx, dw, db)
    rows, dim = x.shape
    if dy.dtype == torch.bfloat16:           # gradient rows gathered from a bf16 residual stream
        rc = _l.load().a3v_layernorm_bwd_bf16(_p(x), x.stride(0), _p(w), _p(dy), dy.stride(0), _p(row_map), _p(dx), dx.stride(0),
                                              _p(dw), _p(db), rows, dim, eps, _stream())
        _l.check(rc, "a3v_layernorm_bwd_bf16")
        return
    rc = _l.load().a3v_layernorm_bwd(_p(x), x.stride(0), _p(w), _p(dy), dy.stride(0), _p(row_map), _p(dx), dx.stride(0),
                                     _p(dw), _p(db), rows, dim, eps, dt(x), _stream())
    _l.check(rc, "a3v_layernorm_bwd")


def swiglu_fwd(gu, act, F, interleaved: bool):
    _dev(gu, act)
    rc = _l.load().a3v_swiglu_fwd(_p(gu), gu.stride(0), _p(act), act.stride(0), gu.shape[0], F, 1 if interleaved else 0,
                                  dt(gu), _stream())
    _l.check(rc, "a3v_swiglu_fwd")


def swiglu_bwd(gu, dact, dgu, F, interleaved: bool):
    _dev(gu, dact, dgu)
    rc = _l.load().a3v_swiglu_bwd(_p(gu), gu.stride(0), _p(dact), dact.stride(0), _p(dgu), dgu.stride(0), gu.shape[0], F,
                                  1 if interleaved else 0, dt(gu), _stream())
    _l.check(rc, "a3v_swiglu_bwd")


def rope_bwd_pack(dq, dk, dv, dqkv, cos_sin, B, S, H, Hkv, hd, rope_pos0=0):
    _dev(dq, dk, dv, dqkv, cos_sin)
    rc = _l.load().a3v_rope_bwd_pack(_p(dq), _p(dk), _p(dv), _p(dqkv), dqkv.stride(0), _p(cos_sin), B, S, H, Hkv, hd,
                                     rope_pos0, dt(dq), _stream())
    _l.check(rc, "a3v_rope_bwd_pack")


def attention_bwd_workspace_bytes(B, S, H, Hkv, hd) -> int:
    return _l.load().a3v_attention_bwd_workspace_bytes(B, S, H, Hkv, hd)


def attention_bwd(q, k, k_sb, k_sh, v, v_sb, v_ss, v_sh, out, dout, lse, D, dq, dk, dv, B, S, H, Hkv, hd, causal: bool,
                  workspace=None):
    _dev(q, k, v, out, dout, lse, D, dq, dk, dv, workspace)
    rc = _l.load().a3v_attention_bwd(_p(q), _p(k), k_sb, k_sh, _p(v), v_sb, v_ss, v_sh, _p(out), _p(dout), _p(lse), _p(D),
                                     _p(dq), _p(dk), _p(dv), _p(workspace), B, S, H, Hkv, hd, 1 if causal else 0, dt(q), _stream())
    _l.check(rc, "a3v_attention_bwd")


def attention_bwd_packed(q, k, k_sb, k_sh, v, v_sb, v_ss, v_sh, out, dout, lse, D, dqkv, cos_sin, B, S, H, Hkv, hd, causal: bool,
                         rope_pos0: int = 0):
    """attention backward + inverse RoPE + packing into the fused-qkv gradient in one pass (bf16, hd 64 / 128)."""
    _dev(q, k, v, out, dout, lse, D, dqkv, cos_sin)
    ld_out = out.stride(-2) if out.dim() == 2 else out.stride(1)      # token stride of out ([rows, H*hd (+pad)] or [B, S, H, hd])
    rc = _l.load().a3v_attention_bwd_packed(_p(q), _p(k), k_sb, k_sh, _p(v), v_sb, v_ss, v_sh, _p(out), ld_out, _p(dout), _p(lse), _p(D),
                                            _p(dqkv), dqkv.stride(0), _p(cos_sin), rope_pos0, B, S, H, Hkv, hd, 1 if causal else 0,
                                            dt(q), _stream())
    _l.check(rc, "a3v_attention_bwd_packed")


def embed_bwd(tokens, dh, dtable, B, T, W, dim):
    _dev(tokens, dh, dtable)
    assert dh.is_contiguous()
    fn = _l.load().a3v_embed_bwd_bf16 if dh.dtype == torch.bfloat16 else _l.load().a3v_embed_bwd
    rc = fn(_p(tokens), tokens.stride(0), _p(dh), _p(dtable), B, T, W, dim, dtable.shape[0], _stream())
    _l.check(rc, "a3v_embed_bwd")


def rows_sum(src, row_idx, n_rows, out):
    _dev(src, row_idx, out)
    rc = _l.load().a3v_rows_sum(_p(src), src.stride(0), _p(row_idx), n_rows, src.shape[1], _p(out), dt(src), _stream())
    _l.check(rc, "a3v_rows_sum")


def lora_gb_scatter(gbt, r: int, views, row0s):
    """views[j] ([n_j, r] fp32 contiguous) += gbt[j*r:(j+1)*r, row0s[j]:row0s[j]+n_j].T for the modules of a fused adapter group."""
    import ctypes
    _dev(gbt, *views)
    n = len(views)
    assert gbt.dtype == torch.float32 and gbt.stride(1) == 1 and all(v.dtype == torch.float32 and v.is_contiguous() and v.shape[1] == r for v in views)
    dst = (ctypes.c_void_p * n)(*[v.data_ptr() for v in views])
    r0 = (ctypes.c_int * n)(*[int(x) for x in row0s])
    nj = (ctypes.c_int * n)(*[int(v.shape[0]) for v in views])
    rc = _l.load().a3v_lora_gb_scatter(_p(gbt), gbt.stride(0), int(r), n, ctypes.cast(dst, ctypes.c_void_p), ctypes.cast(r0, ctypes.c_void_p),
                                       ctypes.cast(nj, ctypes.c_void_p), _stream())
    _l.check(rc, "a3v_lora_gb_scatter")


def grad_finish_multi(table, n_jobs: int, total_units: int, max_blocks: int = 0):
    """One launch over a device table of a3v_finish_job descriptors (int64 [n_jobs, 22], built by a3vlm_amd.grad_finish): every split-K
    plane set and RMSNorm partial-row block of a backward becomes its gradient.  ``max_blocks``: grid size (0: four blocks per CU)."""
    _dev(table)
    assert table.dtype == torch.int64 and table.is_contiguous() and tuple(table.shape) == (n_jobs, 22)
    rc = _l.load().a3v_grad_finish_multi(_p(table), int(n_jobs), int(total_units), int(max_blocks), _stream())
    _l.check(rc, f"a3v_grad_finish_multi(jobs={n_jobs},units={total_units})")


def rmsnorm_bwd_parts(x, w, dy, dh, parts, eps, row_idx=None):
    """``rmsnorm_bwd`` on the bf16 stream without the column sum of the weight gradient: ``parts`` (fp32, ceil(rows / 8) * dim floats)
    receives the partial rows, which an A3V_FINISH_COLSUM job of ``grad_finish_multi`` adds into dw."""
    _dev(x, w, dy, dh, parts, row_idx)
    assert w.dtype == torch.float32 and x.dtype == dh.dtype == dy.dtype == torch.bfloat16 and parts.dtype == torch.float32
    rows, dim = x.shape
    if row_idx is not None:
        assert row_idx.dtype == torch.int32 and row_idx.is_contiguous()
        rows = row_idx.numel()
        assert dy.shape[0] == rows
    assert parts.is_contiguous() and parts.numel() >= (rows + 7) // 8 * dim
    rc = _l.load().a3v_rmsnorm_bwd_parts_bf16(_p(x), x.stride(0), _p(row_idx), _p(w), _p(dy), dy.stride(0), _p(dh), dh.stride(0), _p(parts),
                                              rows, dim, eps, _stream())
    _l.check(rc, "a3v_rmsnorm_bwd_parts_bf16")


def gemm_tn_strip_planes(t, x, planes, S: int):
    """The launch of ``gemm_tn_strip`` alone: planes[s] ([R, N] fp32, s < S) = the product over token slice s, left un-summed."""
    _dev(t, x, planes)
    Kt, R = t.shape
    N = x.shape[1]
    assert x.shape[0] == Kt and t.stride(1) == 1 and x.stride(1) == 1 and t.stride(0) >= 64
    assert planes.dtype == torch.float32 and planes.is_contiguous() and planes.numel() >= S * R * N
    rc = _l.load().a3v_gemm_tn_strip(_p(t), t.stride(0), _p(x), x.stride(0), _p(planes), R, N, Kt, S, _stream())
    _l.check(rc, f"a3v_gemm_tn_strip(R={R},N={N},Kt={Kt},S={S})")


def lora_refresh(wa, wb, A, At, B, Bt, col0: int, row0: int):
    """One adapter's rows / columns of the fused group images (A, At, B, Bt; bf16) from its fp32 lora_a [r, in], lora_b [nj, r]."""
    _dev(wa, wb, A, At, B, Bt)
    assert wa.dtype == torch.float32 and wb.dtype == torch.float32 and wa.is_contiguous() and wb.is_contiguous()
    assert all(t.dtype == torch.bfloat16 and t.stride(1) == 1 for t in (A, At, B, Bt))
    r, in_f = wa.shape
    nj = wb.shape[0]
    assert wb.shape[1] == r and col0 + r <= A.shape[0] and in_f <= A.shape[1] and row0 + nj <= B.shape[0]
    rc = _l.load().a3v_lora_refresh(_p(wa), _p(wb), r, in_f, nj, _p(A), A.stride(0), _p(At), At.stride(0), _p(B), B.stride(0), _p(Bt),
                                    Bt.stride(0), col0, row0, _stream())
    _l.check(rc, "a3v_lora_refresh")
