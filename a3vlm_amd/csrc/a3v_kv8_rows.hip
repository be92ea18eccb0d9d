// The fp8 KV cache (a3v_kv8.hip, format in include/a3vlm_hip.h "fp8 KV cache") on the ragged decode path (a3v_ragged.hip): every
// batch row at its own cache position.  All position arrays are device int32[B]; an idle row writes nothing into a cache array and
// produces zeros.
//
//  * rope_kvquant_rows_kernel          : rope_kv_rows_kernel's rotation and kv_quant_fp8_kernel's S = 1 quantisation in one launch:
//    one wave per (q head | kv head's k | kv head's v, row).  The hd values of a k / v slot live in one wave (a rotation pair per
//    lane), so amax is one wave reduction and the codes go straight to position pos[b] of the row's own fp8 cache: no bf16 staging
//    pair, no separate quantise launch.  k is rounded to bf16 after the rotation, as the bf16 cache write rounds it, and the
//    quantiser's expressions are a3v_kv8.hip's element for element, so q_out, codes and scales are those of a3v_rope_kvcache_rows
//    followed by a3v_kv_quantize_fp8 (S = 1).
//  * attn_decode_rows_fp8kv_kernel<HD, SH> : the walk of attn_decode_fp8kv_kernel (a3v_kv8.hip) with the row's own key count, as
//    attn_decode_rows_kernel (a3v_ragged.hip) restates the bf16 walk: the split plan comes from sk_max (host), a block's range holds
//    n = min(sk[b], lo + chunk) - lo keys, an empty range contributes (m, l) = (-inf, 0) and still arrives at the combine, an idle
//    row leaves before the combine with its counter untouched and split 0 writes the zeros.  SH = true: shared prompt keys -- the
//    tiles of a row below its shared length are read from another cache row.  All FOUR streams move together: K bytes, V^T bytes,
//    k_scale and v_scale each get the wave-uniform select of one 64-bit offset (the scales' row stride is Hkv * Smax).  Every tile
//    starts at a multiple of 64 in absolute position and the shared length is one too, so a tile, its clamped K / scale re-reads
//    and its 16-byte V^T vectors (16 keys) lie in one row.
//  * kv8_copy_span_kernel              : positions [lo, hi) of one cache row into other rows, bytes and scales, every layer in one launch.
//  * a3v_llama_decode_step_rows_kv8    : the fused layer loop (a3v_decode.hip: a3v_decode_fused_layers) with the first two kernels as
//    its attention stage, six launches per layer.
#include "a3v_common.h"

namespace {

// ---- the e4m3 helpers of a3v_kv8.hip, expression for expression (the codes must be that file's bit for bit)
// two e4m3 bytes of a dword -> two floats (v_cvt_pk_f32_fp8: exact)
__device__ __forceinline__ void fp8x4_to_f32(unsigned w, float* o) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}
// two floats (already divided by the scale) -> two e4m3 bytes (low half of the result), round to nearest even, saturating at +-448
__device__ __forceinline__ unsigned f32x2_to_fp8(float t0, float t1) {
  const float c0 = fminf(fmaxf(t0, -448.f), 448.f), c1 = fminf(fmaxf(t1, -448.f), 448.f);
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, 0, false) & 0xffffu;
}
__device__ __forceinline__ float kv8_scale(float amax) { return fmaxf(amax, 1e-12f) / 448.f; }

struct RopeQuantArgs {
  const bf16_t* qkv; bf16_t* q_out;
  uint8_t* k_q; uint8_t* vt_q; float* k_scale; float* v_scale;
  const float* cos_sin; const int32_t* pos;
  int64_t ldqkv, ldq;
  int H, Hkv, hd, Smax;
};

// grid (H + 2 Hkv, B), one wave: slot < H rotates a q head, the next Hkv slots rotate and quantise k, the last Hkv quantise v.
// Lane pr holds the pair (2 pr, 2 pr + 1) of the slot's hd values (hd <= 128: one pair per lane, lanes >= hd / 2 hold zeros).
__global__ __launch_bounds__(64) void rope_kvquant_rows_kernel(RopeQuantArgs a) {
  const int slot = blockIdx.x, b = blockIdx.y, pr = threadIdx.x;
  const int p = a.pos[b];
  const int half = a.hd / 2, hd = a.hd, H = a.H, Hkv = a.Hkv;
  const bool on = pr < half;
  if (p < 0 || p >= a.Smax) {          // idle row: no cache write; its q row is zeros
    if (slot < H && on) {
      bf16_t* dst = a.q_out + (int64_t)b * a.ldq + (int64_t)slot * hd + 2 * pr;
      dst[0] = f2bf(0.f);
      dst[1] = f2bf(0.f);
    }
    return;
  }
  const bf16_t* src = a.qkv + (int64_t)b * a.ldqkv + (int64_t)slot * hd;
  float x0 = 0.f, x1 = 0.f;
  if (on) {
    const float aa = (float)src[2 * pr], bb = (float)src[2 * pr + 1];
    if (slot < H + Hkv) {
      const float co = a.cos_sin[((int64_t)p * half + pr) * 2], si = a.cos_sin[((int64_t)p * half + pr) * 2 + 1];
      const float o0 = aa * co - bb * si, o1 = aa * si + bb * co;
      if (slot < H) {
        bf16_t* dst = a.q_out + (int64_t)b * a.ldq + (int64_t)slot * hd + 2 * pr;
        dst[0] = f2bf(o0);
        dst[1] = f2bf(o1);
      } else {                         // what the bf16 cache would hold
        x0 = (float)f2bf(o0);
        x1 = (float)f2bf(o1);
      }
    } else {
      x0 = aa;
      x1 = bb;
    }
  }
  if (slot < H) return;                // wave-uniform
  const float scale = kv8_scale(wave_max(fmaxf(fabsf(x0), fabsf(x1))));
  const unsigned w = f32x2_to_fp8(x0 / scale, x1 / scale);
  if (slot < H + Hkv) {
    const int64_t bh = (int64_t)b * Hkv + (slot - H);
    if (on) *reinterpret_cast<uint16_t*>(a.k_q + (bh * a.Smax + p) * hd + 2 * pr) = (uint16_t)w;
    if (pr == 0) a.k_scale[bh * a.Smax + p] = scale;
  } else {
    const int64_t bh = (int64_t)b * Hkv + (slot - H - Hkv);
    if (on) {
      uint8_t* dst = a.vt_q + (bh * hd + 2 * pr) * (int64_t)a.Smax + p;
      dst[0] = (uint8_t)w;
      dst[a.Smax] = (uint8_t)(w >> 8);
    }
    if (pr == 0) a.v_scale[bh * a.Smax + p] = scale;
  }
}

// k / vt / ks / vs are the arrays of ALL Btot cache rows; batch index b of the launch is cache row row0 + b, and src_row[b]
// (SH = true) is a cache row (absolute), read as the own row when outside [0, Btot).
struct Kv8RowsArgs {
  const bf16_t* q; const uint8_t* k; const uint8_t* vt; const float* ks; const float* vs; bf16_t* out;
  const int32_t* sk; const int32_t* src_row; const int32_t* shared;
  int64_t ldq, ldo;
  int sk_add, sk_max, H, Hkv, Smax, row0, Btot;   // keys of row b = min(sk[b] + sk_add, sk_max)
  float scale;
};

template <int HD, bool SH>
__global__ __launch_bounds__(512) void attn_decode_rows_fp8kv_kernel(Kv8RowsArgs p, float* part, int nsplit, int chunk, int* counters) {
  constexpr int LPR = HD / 16;       // lanes per K row (16 B = 16 elements each)
  constexpr int RPW = 64 / LPR;      // K rows per wave-wide load
  constexpr int NKL = 64 / RPW;      // K loads per 64-key tile
  constexpr int NVL = HD / 16;       // V^T loads per tile (16 d rows x 64 B per load)
  __shared__ __attribute__((aligned(16))) float sc_s[8][64];
  __shared__ __attribute__((aligned(16))) float ks_s[8][64];
  __shared__ __attribute__((aligned(16))) float vs_s[8][64];
  __shared__ float comb[8][HD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int sk0 = p.sk[b];
  const int skb = sk0 >= p.sk_max ? p.sk_max : min(sk0 + p.sk_add, p.sk_max);
  if (skb <= 0) {                    // idle row, the same for every block of the row: none of them touches the counter
    if (sp == 0 && tid < HD) p.out[b * p.ldo + h * HD + tid] = f2bf(0.f);
    return;
  }
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int n = min(skb, kv_lo + chunk) - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * nsplit + sp) * (HD + 2);
  const int64_t row = p.row0 + b;
  int64_t dk = 0, ds = 0;            // offsets from the own row to the source row: K / V^T bytes (equal), scales
  int sh_rel = 0;                    // tiles of the range that start below it come from the source row
  if constexpr (SH) {
    int src = p.src_row[b];
    if (src < 0 || src >= p.Btot) src = (int)row;
    sh_rel = (src == (int)row ? 0 : max(min(p.shared[b], skb), 0) & ~63) - kv_lo;
    ds = (src - row) * p.Hkv * p.Smax;
    dk = ds * HD;
  }
  const int64_t bh = row * p.Hkv + hk;
  const bf16_t* Q = p.q + b * p.ldq + h * HD;
  const uint8_t* K = p.k + (bh * p.Smax + kv_lo) * HD;
  const uint8_t* VT = p.vt + bh * HD * p.Smax + kv_lo;
  const float* KS = p.ks + bh * p.Smax + kv_lo;
  const float* VS = p.vs + bh * p.Smax + kv_lo;
  const int lo = wave * 64, hi = max(n, 0);
  float m = -INFINITY, l = 0.f, acc[NVL];
#pragma unroll
  for (int j = 0; j < NVL; ++j) acc[j] = 0.f;
  const int lr = lane / LPR, lc = (lane % LPR) * 16;
  const int dr = lane >> 2, c16 = (lane & 3) * 16;
  if (hi > lo) {
    float qv[16];
    load8(Q + lc, qv);
    load8(Q + lc + 8, qv + 8);
    const int last_vec = (hi - 1) & ~15;
    u32x4 kk[NKL];
    float ksc, vsc;
    auto load_k = [&](int t0) {
      const uint8_t* Kt = K;
      const float* KSt = KS;
      const float* VSt = VS;
      if constexpr (SH) {            // wave-uniform: t0 is a multiple of 64, the clamped rows and scales stay in the tile
        const bool from_src = t0 < sh_rel;
        Kt = K + (from_src ? dk : 0);
        KSt = KS + (from_src ? ds : 0);
        VSt = VS + (from_src ? ds : 0);
      }
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        const int r = min(t0 + u * RPW + lr, hi - 1);
        kk[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Kt + (int64_t)r * HD + lc));   // read once per step by one block
      }
      const int ki = min(t0 + lane, hi - 1);
      ksc = KSt[ki];
      vsc = VSt[ki];
    };
    load_k(lo);
    for (int t0 = lo; t0 < hi; t0 += 512) {
      u32x4 vv[NVL];
      const int kvc = min(t0 + c16, last_vec);             // vectors past the wave's range re-read its last one (masked below)
      const uint8_t* Vt = VT;
      if constexpr (SH) Vt = VT + (t0 < sh_rel ? dk : 0);   // last_vec >= t0: the re-read vector lies in the tile too
#pragma unroll
      for (int j = 0; j < NVL; ++j)
        vv[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Vt + (int64_t)(j * 16 + dr) * p.Smax + kvc));
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          float kf[4];
          fp8x4_to_f32(kk[u][w], kf);
#pragma unroll
          for (int e = 0; e < 4; ++e) a = fmaf(qv[4 * w + e], kf[e], a);
        }
        a += dpp_f<0xB1>(a);
        a += dpp_f<0x4E>(a);
        if (LPR == 8) a += dpp_f<0x141>(a);
        if ((lane % LPR) == 0) sc_s[wave][u * RPW + lr] = a;
      }
      ks_s[wave][lane] = ksc;
      vs_s[wave][lane] = vsc;
      if (t0 + 512 < hi) load_k(t0 + 512);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // wave-private round trip through LDS: no barrier, in-order LDS
      float s16[16], kq[16], vq[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sa = *reinterpret_cast<const f32x4*>(&sc_s[wave][c16 + 4 * g]);
        const f32x4 ka = *reinterpret_cast<const f32x4*>(&ks_s[wave][c16 + 4 * g]);
        const f32x4 va = *reinterpret_cast<const f32x4*>(&vs_s[wave][c16 + 4 * g]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { s16[4 * g + e] = sa[e]; kq[4 * g + e] = ka[e]; vq[4 * g + e] = va[e]; }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int nvalid = hi - (t0 + c16);                    // <= 0 for the vectors past the range
      float mt = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        s16[e] = e < nvalid ? s16[e] * kq[e] * p.scale : -INFINITY;
        mt = fmaxf(mt, s16[e]);
      }
      mt = fmaxf(mt, dpp_f<0xB1>(mt));
      mt = fmaxf(mt, dpp_f<0x4E>(mt));
      const float mn = fmaxf(m, mt);                         // finite: the tile's first key is inside the range
      const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
      float pw[16], ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pe = e < nvalid ? __expf(s16[e] - mn) : 0.f;
        ps += pe;
        pw[e] = e < nvalid ? pe * vq[e] : 0.f;               // the scale tail may hold inf: select, never 0 * x
      }
      l = l * alpha + ps;
#pragma unroll
      for (int j = 0; j < NVL; ++j) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          float vf[4];
          fp8x4_to_f32(vv[j][w], vf);
#pragma unroll
          for (int e = 0; e < 4; ++e) a = fmaf(pw[4 * w + e], 4 * w + e < nvalid ? vf[e] : 0.f, a);   // the cache tail may hold the NaN code
        }
        acc[j] = acc[j] * alpha + a;
      }
      m = mn;
    }
  }
#pragma unroll
  for (int j = 0; j < NVL; ++j) {
    acc[j] += dpp_f<0xB1>(acc[j]);
    acc[j] += dpp_f<0x4E>(acc[j]);
  }
  l += dpp_f<0xB1>(l);
  l += dpp_f<0x4E>(l);
  if ((lane & 3) == 0) {
#pragma unroll
    for (int j = 0; j < NVL; ++j) comb[wave][j * 16 + dr] = acc[j];
  }
  if (lane == 0) { comb[wave][HD] = m; comb[wave][HD + 1] = l; }
  __syncthreads();
  if (tid < HD) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 8; ++w) M = fmaxf(M, comb[w][HD]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const float mw = comb[w][HD];
      const float sw = (mw == -INFINITY) ? 0.f : __expf(mw - M);
      o += sw * comb[w][tid];
      L += sw * comb[w][HD + 1];
    }
    if (nsplit == 1) {
      p.out[b * p.ldo + h * HD + tid] = f2bf(o / L);         // skb >= 1: L > 0
    } else {                                                 // an empty range: o = 0, M = -inf, L = 0
      po[tid] = o;
      if (tid == 0) { po[HD] = M; po[HD + 1] = L; }
    }
  }
  if (nsplit == 1) return;
  decode_combine_tail<HD>(p.out, p.ldo, (int64_t)HD, p.H, part, po, nsplit, counters, b, h, tid);
}

// [lo, hi) of a run that sits at the same offset of 16-byte aligned rows in source and destination: elements up to the first
// 16-byte boundary, vectors, then the elements behind the last whole vector
template <typename T>
__device__ __forceinline__ void copy_run(T* d, const T* s, int lo, int hi) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int a0 = min(hi, (lo + VEC - 1) / VEC * VEC), a1 = a0 + (hi - a0) / VEC * VEC;
  for (int e = lo; e < a0; ++e) d[e] = s[e];
  for (int e = a0; e < a1; e += VEC) *reinterpret_cast<u32x4*>(d + e) = *reinterpret_cast<const u32x4*>(s + e);
  for (int e = a1; e < hi; ++e) d[e] = s[e];
}

// Positions [lo, hi) (0 < hi - lo < 64) of cache row src into the rows dst[0..n_dst): grid (n_dst, Hkv, layers).  K: one contiguous
// run of (hi - lo) * hd bytes per (row, head), 16-byte vectors (hd is a multiple of 16).  V^T: hi - lo bytes per d row, one thread
// per d row; the two scale runs of hi - lo floats, one thread each.  Nothing outside the span is written.
__global__ __launch_bounds__(256) void kv8_copy_span_kernel(const void* const* __restrict__ k_ptrs, const void* const* __restrict__ vt_ptrs,
                                                            const void* const* __restrict__ ks_ptrs, const void* const* __restrict__ vs_ptrs,
                                                            int src, const int32_t* __restrict__ dst, int B, int lo, int hi, int Hkv, int hd,
                                                            int Smax) {
  const int r = dst[blockIdx.x];
  if (r < 0 || r >= B || r == src) return;             // block-uniform
  const int hk = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
  uint8_t* kb = (uint8_t*)k_ptrs[layer];
  uint8_t* vb = (uint8_t*)vt_ptrs[layer];
  const int64_t hs = (int64_t)src * Hkv + hk, hr = (int64_t)r * Hkv + hk;
  const int64_t head = (int64_t)Smax * hd;
  const u32x4* ks = reinterpret_cast<const u32x4*>(kb + hs * head + (int64_t)lo * hd);
  u32x4* kd = reinterpret_cast<u32x4*>(kb + hr * head + (int64_t)lo * hd);
  const int nvec = (hi - lo) * hd / 16;
  for (int i = tid; i < nvec; i += 256) kd[i] = ks[i];
  if (tid < hd) copy_run(vb + (hr * hd + tid) * Smax, (const uint8_t*)vb + (hs * hd + tid) * Smax, lo, hi);
  else if (tid == hd) copy_run((float*)ks_ptrs[layer] + hr * Smax, (const float*)ks_ptrs[layer] + hs * Smax, lo, hi);
  else if (tid == hd + 1) copy_run((float*)vs_ptrs[layer] + hr * Smax, (const float*)vs_ptrs[layer] + hs * Smax, lo, hi);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the write of rows [0, B) of the four arrays handed in (a chunk's caller offsets them to its first row)
int rope_kvquant_rows_impl(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_q, void* vt_q, float* k_scale, float* v_scale,
                           const float* cos_sin, const int32_t* pos, int B, int H, int Hkv, int hd, int Smax, void* stream) {
  if (!qkv || !q_out || !k_q || !vt_q || !k_scale || !v_scale || !cos_sin || !pos || B <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (Smax <= 0 || Smax % 64 || ldqkv % 8 || ldq % 8 || ldqkv < (int64_t)(H + 2 * Hkv) * hd || ldq < (int64_t)H * hd) return A3V_ERR_SHAPE;
  if (!al16(k_q) || !al16(vt_q) || !al16(k_scale) || !al16(v_scale)) return A3V_ERR_SHAPE;
  const RopeQuantArgs a{(const bf16_t*)qkv, (bf16_t*)q_out, (uint8_t*)k_q, (uint8_t*)vt_q, k_scale, v_scale, cos_sin, pos, ldqkv, ldq, H, Hkv, hd, Smax};
  hipLaunchKernelGGL(rope_kvquant_rows_kernel, dim3(H + 2 * Hkv, B), dim3(64), 0, (hipStream_t)stream, a);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

// src_row == NULL: the plain kernel.  The four arrays hold all Btot cache rows; row b of the call is cache row row0 + b.
int attention_rows_fp8kv_impl(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale, const float* v_scale,
                              void* out, int64_t ldo, const int32_t* sk, int sk_add, const int32_t* src_row, const int32_t* shared, int sk_max,
                              int B, int row0, int Btot, int H, int Hkv, int hd, int Smax, float* scratch, int* counters, void* stream) {
  if (!q || !k_q || !vt_q || !k_scale || !v_scale || !out || !sk || !scratch || !counters || B <= 0 || H <= 0 || Hkv <= 0 || sk_max <= 0)
    return A3V_ERR_ARG;
  if (src_row && !shared) return A3V_ERR_ARG;
  if (row0 < 0 || Btot < row0 + B) return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (H % Hkv || Smax <= 0 || Smax % 64 || sk_max > Smax || ldq % 8 || ldq < (int64_t)H * hd || ldo < (int64_t)H * hd) return A3V_ERR_SHAPE;
  if (!al16(q) || !al16(k_q) || !al16(vt_q) || !al16(k_scale) || !al16(v_scale)) return A3V_ERR_SHAPE;
  const Kv8RowsArgs p{(const bf16_t*)q, (const uint8_t*)k_q, (const uint8_t*)vt_q, k_scale, v_scale, (bf16_t*)out, sk, src_row, shared,
                      ldq, ldo, sk_add, sk_max, H, Hkv, Smax, row0, Btot, 1.0f / sqrtf((float)hd)};
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ns, H, B);
  if (src_row) {
    if (hd == 128) hipLaunchKernelGGL((attn_decode_rows_fp8kv_kernel<128, true>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
    else hipLaunchKernelGGL((attn_decode_rows_fp8kv_kernel<64, true>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  } else if (hd == 128) hipLaunchKernelGGL((attn_decode_rows_fp8kv_kernel<128, false>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  else hipLaunchKernelGGL((attn_decode_rows_fp8kv_kernel<64, false>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

}  // namespace

extern "C" int a3v_rope_kvquant_rows(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_q, void* vt_q, float* k_scale,
                                     float* v_scale, const float* cos_sin, const int32_t* pos, int B, int H, int Hkv, int hd, int Smax,
                                     void* stream) {
  return rope_kvquant_rows_impl(qkv, ldqkv, q_out, ldq, k_q, vt_q, k_scale, v_scale, cos_sin, pos, B, H, Hkv, hd, Smax, stream);
}

extern "C" int a3v_attention_decode_rows_fp8kv_splits(int B, int H, int sk_max) {
  if (B <= 0 || H <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  return ns;
}

extern "C" int a3v_attention_decode_rows_fp8kv(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                                               const float* v_scale, void* out, int64_t ldo, const int32_t* sk, int sk_max, int B, int H,
                                               int Hkv, int hd, int Smax, float* scratch, int* counters, void* stream) {
  return attention_rows_fp8kv_impl(q, ldq, k_q, vt_q, k_scale, v_scale, out, ldo, sk, 0, nullptr, nullptr, sk_max, B, 0, B, H, Hkv, hd, Smax,
                                   scratch, counters, stream);
}

extern "C" int a3v_attention_decode_rows_fp8kv_shared(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                                                      const float* v_scale, void* out, int64_t ldo, const int32_t* sk, const int32_t* src_row,
                                                      const int32_t* shared, int sk_max, int B, int H, int Hkv, int hd, int Smax,
                                                      float* scratch, int* counters, void* stream) {
  return attention_rows_fp8kv_impl(q, ldq, k_q, vt_q, k_scale, v_scale, out, ldo, sk, 0, src_row, src_row ? shared : nullptr, sk_max, B, 0, B,
                                   H, Hkv, hd, Smax, scratch, counters, stream);
}

extern "C" int a3v_kv8_copy_span(const void* const* k_ptrs, const void* const* vt_ptrs, const void* const* ks_ptrs,
                                 const void* const* vs_ptrs, int n_layers, int src_row, const int32_t* dst_rows, int n_dst, int B, int lo,
                                 int hi, int Hkv, int hd, int Smax, void* stream) {
  if (!k_ptrs || !vt_ptrs || !ks_ptrs || !vs_ptrs || n_layers <= 0 || n_dst < 0 || (n_dst > 0 && !dst_rows) || B <= 0 || src_row < 0 ||
      src_row >= B)
    return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (Hkv <= 0 || Smax <= 0 || Smax % 64 || lo < 0 || hi < lo || hi - lo >= 64 || hi > Smax) return A3V_ERR_SHAPE;
  if (n_layers > 65535 || Hkv > 65535) return A3V_ERR_SHAPE;
  if (hi == lo || n_dst == 0) return A3V_OK;             // nothing to copy: nothing launched
  hipLaunchKernelGGL(kv8_copy_span_kernel, dim3(n_dst, Hkv, n_layers), dim3(256), 0, (hipStream_t)stream, k_ptrs, vt_ptrs, ks_ptrs, vs_ptrs,
                     src_row, dst_rows, B, lo, hi, Hkv, hd, Smax);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_llama_decode_step_rows_kv8_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8) {
  return a3v_llama_decode_step_rows_form(B, dim, H, Hkv, hd, ffn, w8) == 2 ? 2 : 0;
}

namespace {
// what a3v_decode_fused_layers runs between the plain-store qkv GEMV and the wo GEMV: RoPE + quantising write at the rows' own
// positions, then the per-row fp8 attention -- six launches per layer
struct RowsKv8Stage { const a3v_kv8_layer* kv8; const float* cos_sin; const int32_t* pos; const int32_t* src_row; const int32_t* shared; int pos_max, B; };
int attend_rows_kv8(const void* ctx, const a3v_decode_chunk& c) {
  const RowsKv8Stage& s = *(const RowsKv8Stage*)ctx;
  const a3v_kv8_layer& Q8 = s.kv8[c.layer];
  const int64_t ldq = c.strides[0];
  const int64_t sc_row = (int64_t)c.Hkv * c.Smax;          // scales per cache row; c.kv_row = bytes per row of an fp8 array
  const int32_t* pc = s.pos + c.b0;
  int rc;
  if ((rc = rope_kvquant_rows_impl(c.q, ldq, c.q, ldq, (uint8_t*)Q8.k_q + c.b0 * c.kv_row, (uint8_t*)Q8.vt_q + c.b0 * c.kv_row,
                                   Q8.k_scale + c.b0 * sc_row, Q8.v_scale + c.b0 * sc_row, s.cos_sin, pc, c.nbr, c.H, c.Hkv, c.hd, c.Smax,
                                   c.stream)))
    return rc;
  // src_row[] names rows of the whole cache: the un-offset bases of all four arrays, and the chunk's first row
  return attention_rows_fp8kv_impl(c.q, ldq, Q8.k_q, Q8.vt_q, Q8.k_scale, Q8.v_scale, c.att, (int64_t)c.H * c.hd, pc, 1,
                                   s.src_row ? s.src_row + c.b0 : nullptr, s.shared ? s.shared + c.b0 : nullptr, s.pos_max + 1, c.nbr, c.b0,
                                   s.B, c.H, c.Hkv, c.hd, c.Smax, c.scratch, c.counters, c.stream);
}
}  // namespace

extern "C" int a3v_llama_decode_step_rows_kv8(const a3v_llama_layer* layers, const a3v_kv8_layer* kv8, int n_layers, void* h, void* xn,
                                              void* qkv, void* att, void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin,
                                              const int32_t* pos, const int32_t* src_row, const int32_t* shared, int pos_max, int B, int dim,
                                              int H, int Hkv, int hd, int ffn, int Smax, float eps, void* stream) {
  if (!layers || !kv8 || n_layers <= 0 || !h || !xn || !qkv || !att || !act || !attn_scratch || !skinny_ws || !cos_sin || !pos) return A3V_ERR_ARG;
  if (!src_row != !shared) return A3V_ERR_ARG;
  if (B <= 0 || B > 32 || pos_max < 0 || pos_max >= Smax || Smax % 64) return A3V_ERR_SHAPE;
  int rc, w8;
  if ((rc = a3v_decode_layer_table(layers, n_layers, false, &w8))) return rc;    // (the bf16 caches are not read)
  for (int i = 0; i < n_layers; ++i)
    if (!kv8[i].k_q || !kv8[i].vt_q || !kv8[i].k_scale || !kv8[i].v_scale) return A3V_ERR_ARG;
  // everything the stage's launches would refuse is refused here, before the first launch of the loop
  if (H <= 0 || Hkv <= 0 || H % Hkv || !al16(qkv)) return A3V_ERR_SHAPE;
  for (int i = 0; i < n_layers; ++i)
    if (!al16(kv8[i].k_q) || !al16(kv8[i].vt_q) || !al16(kv8[i].k_scale) || !al16(kv8[i].v_scale)) return A3V_ERR_SHAPE;
  if (a3v_llama_decode_step_rows_kv8_form(B, dim, H, Hkv, hd, ffn, w8) != 2) return A3V_ERR_SHAPE;    // nothing launched
  const RowsKv8Stage ctx{kv8, cos_sin, pos, src_row, shared, pos_max, B};
  const a3v_decode_stage stage{B > 16 ? (B + 1) / 2 : B, 1, nullptr, nullptr, nullptr, 0, 0, attend_rows_kv8, &ctx};   // 17..32 rows: two row chunks
  return a3v_decode_fused_layers(layers, n_layers, w8, h, qkv, att, act, attn_scratch, skinny_ws, B, dim, H, Hkv, hd, ffn, Smax, eps, stage, stream);
}
