// fp8 (OCP e4m3fn) KV cache for gfx950: the quantising cache write, its inverse, and decode attention on the fp8 bytes.
// Format (include/a3vlm_hip.h): K [B,Hkv,Smax,hd] and V^T [B,Hkv,hd,Smax] as e4m3 bytes in the layouts of the bf16 caches, one fp32
// scale per (batch, kv-head, position) for K and one for V, scale = max(amax, 1e-12) / 448 over the hd values of that head at that
// position, q = e4m3(x / scale) -- the arithmetic of rows_quant_fp8_kernel / oracle.quant_fp8 with a true division, so that the
// codes are the oracle's bit for bit.
//
//  * kv_quant_fp8_kernel<HD>      : one block per (64-position tile of the DESTINATION, kv-head, batch).  K rows are hd contiguous
//    values: HD/8 lanes per row, 16-B loads, 8-B stores.  V^T has the positions contiguous, so the S new bytes of a d row are a byte
//    run that starts anywhere: the tile goes through LDS (fp32, row pitch 65: column scans for the per-position maximum and row
//    reads for the stores are both conflict free), tiles are aligned to the destination, and a lane stores 16 whole bytes wherever
//    its 16 positions are all new; the two ragged edges are written byte by byte and nothing else is touched.
//  * kv_dequant_fp8_kernel        : element-wise inverse, bf16(float(q) * scale).
//  * attn_decode_fp8kv_kernel<HD> : attn_decode_wave_kernel (a3v_attn.hip) on fp8 bytes, see there.
#include "a3v_common.h"

namespace {

// two e4m3 bytes of a dword -> two floats (v_cvt_pk_f32_fp8: exact)
__device__ __forceinline__ void fp8x4_to_f32(unsigned w, float* o) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}
// four floats (already divided by the scale) -> four e4m3 bytes, round to nearest even, saturating at +-448
__device__ __forceinline__ unsigned f32x4_to_fp8(const float* t) {
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(t[e], -448.f), 448.f);
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
  return (unsigned)w;
}
__device__ __forceinline__ float kv8_scale(float amax) { return fmaxf(amax, 1e-12f) / 448.f; }

struct KvqArgs {
  const bf16_t* k_src; const bf16_t* vt_src;
  uint8_t* k_q; uint8_t* vt_q; float* k_scale; float* v_scale;
  int Hkv, S, Smax, Smax_src, src_pos, dst_pos;
};

template <int HD>
__global__ __launch_bounds__(256) void kv_quant_fp8_kernel(KvqArgs a) {
  constexpr int LPR = HD / 8;          // lanes per K row (8 bf16 = 16 B each)
  constexpr int RPP = 256 / LPR;       // K rows per pass of the block
  __shared__ float vs[HD][65];
  __shared__ float red[4][64];
  __shared__ float sc_s[64];
  const int tid = threadIdx.x;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int64_t bh = (int64_t)b * a.Hkv + hk;
  const int g0 = (a.dst_pos >> 6) + blockIdx.x;          // 64-position tile of the destination
  const int p_lo = max(g0 * 64, a.dst_pos), p_hi = min(g0 * 64 + 64, a.dst_pos + a.S);
  const int delta = a.src_pos - a.dst_pos;               // source position = destination position + delta

  // ---- K: rows [p_lo, p_hi)
  {
    const bf16_t* ks = a.k_src + bh * a.Smax_src * HD;
    uint8_t* kq = a.k_q + bh * a.Smax * HD;
    const int lr = tid / LPR, lc = (tid % LPR) * 8;
#pragma unroll
    for (int pass = 0; pass < 64 / RPP; ++pass) {
      const int p = g0 * 64 + pass * RPP + lr;
      const bool on = p >= p_lo && p < p_hi;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (on) load8(ks + (int64_t)(p + delta) * HD + lc, v);
      float amax = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      const float scale = kv8_scale(amax);
      if (on) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = v[e] / scale;
        u32x2 w;
        w[0] = f32x4_to_fp8(t);
        w[1] = f32x4_to_fp8(t + 4);
        *reinterpret_cast<u32x2*>(kq + (int64_t)p * HD + lc) = w;
        if (lc == 0) a.k_scale[bh * a.Smax + p] = scale;
      }
    }
  }

  // ---- V^T: columns [p_lo, p_hi) of HD rows, through LDS
  const bf16_t* vsrc = a.vt_src + bh * HD * a.Smax_src;
  const bool vec_ok = ((delta & 7) == 0) && ((a.Smax_src & 7) == 0);      // block-uniform: 16-B source loads are aligned
  if (vec_ok) {
    const int c = tid & 7;
    const int t0 = c * 8, p0 = g0 * 64 + t0;
#pragma unroll
    for (int i = 0; i < HD / 32; ++i) {
      const int d = (tid >> 3) + 32 * i;
      const bf16_t* src = vsrc + (int64_t)d * a.Smax_src + (p0 + delta);
      float v[8];
      if (p0 >= p_lo && p0 + 8 <= p_hi) {
        load8(src, v);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (p0 + e >= p_lo && p0 + e < p_hi) ? (float)src[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) vs[d][t0 + e] = v[e];
    }
  } else {
    const int t = tid & 63, p = g0 * 64 + t;
    const bool on = p >= p_lo && p < p_hi;
#pragma unroll 4
    for (int i = 0; i < HD / 4; ++i) {
      const int d = (tid >> 6) + 4 * i;
      vs[d][t] = on ? (float)vsrc[(int64_t)d * a.Smax_src + (p + delta)] : 0.f;
    }
  }
  __syncthreads();
  {
    const int t = tid & 63, part = tid >> 6;
    float amax = 0.f;
#pragma unroll 8
    for (int d = part * (HD / 4); d < (part + 1) * (HD / 4); ++d) amax = fmaxf(amax, fabsf(vs[d][t]));
    red[part][t] = amax;
  }
  __syncthreads();
  if (tid < 64) {
    const float scale = kv8_scale(fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid])));
    sc_s[tid] = scale;
    const int p = g0 * 64 + tid;
    if (p >= p_lo && p < p_hi) a.v_scale[bh * a.Smax + p] = scale;
  }
  __syncthreads();
  {
    uint8_t* vq = a.vt_q + bh * HD * a.Smax;
    const int c = tid & 3;
    const int t0 = c * 16, p0 = g0 * 64 + t0;
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) {
      const int d = (tid >> 2) + 64 * i;
      float t[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) t[e] = vs[d][t0 + e] / sc_s[t0 + e];
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = f32x4_to_fp8(t + 4 * j);
      uint8_t* dst = vq + (int64_t)d * a.Smax + p0;
      if (p0 >= p_lo && p0 + 16 <= p_hi) {
        *reinterpret_cast<u32x4*>(dst) = w;
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (p0 + e >= p_lo && p0 + e < p_hi) dst[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
      }
    }
  }
}

struct KvdArgs {
  const uint8_t* k_q; const uint8_t* vt_q; const float* k_scale; const float* v_scale;
  bf16_t* k_dst; bf16_t* vt_dst;
  int hd, n, Smax, Smax_dst;
};

// grid (chunks of 8 elements / 256, B*Hkv, 2): z = 0 the K rows, z = 1 the V^T rows
__global__ __launch_bounds__(256) void kv_dequant_fp8_kernel(KvdArgs a) {
  const int64_t bh = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int hd = a.hd;
  if (blockIdx.z == 0) {
    if (idx >= (int64_t)a.n * hd / 8) return;
    const int64_t e0 = idx * 8;                          // element of the [n, hd] block; one position per chunk (hd % 8 == 0)
    const u32x2 w = *reinterpret_cast<const u32x2*>(a.k_q + bh * a.Smax * hd + e0);
    const float s = a.k_scale[bh * a.Smax + e0 / hd];
    float v[8];
    fp8x4_to_f32(w[0], v);
    fp8x4_to_f32(w[1], v + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= s;
    store8(a.k_dst + bh * a.Smax_dst * hd + e0, v);
    return;
  }
  const int nch = (a.n + 7) / 8;
  if (idx >= (int64_t)nch * hd) return;
  const int d = (int)(idx / nch), p0 = (int)(idx % nch) * 8;
  const u32x2 w = *reinterpret_cast<const u32x2*>(a.vt_q + (bh * hd + d) * a.Smax + p0);     // p0 + 8 <= Smax (Smax % 64 == 0)
  float v[8], s[8];
  fp8x4_to_f32(w[0], v);
  fp8x4_to_f32(w[1], v + 4);
  load8(a.v_scale + bh * a.Smax + p0, s);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] *= s[e];
  bf16_t* dst = a.vt_dst + (bh * hd + d) * a.Smax_dst + p0;
  if (p0 + 8 <= a.n && (a.Smax_dst & 7) == 0) {
    store8(dst, v);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (p0 + e < a.n) dst[e] = f2bf(v[e]);
  }
}

// ------------------------------------------------------------------------------------
// Decode attention on the fp8 cache: the structure of attn_decode_wave_kernel -- grid (nsplit, H, B), eight waves, every eighth
// 64-key tile of the block's range per wave, K(t+1) and V^T(t) in flight together, non-temporal loads, wave-private online
// softmax, one merge of the eight waves through LDS, split-KV with the last-arriver combine.
// Lane geometry.  A 16-B load carries 16 elements, so a K row of HD bytes takes HD/16 lanes (8 at hd 128, 4 at hd 64) and a
// wave-wide load covers 64 / (HD/16) rows: a 64-key tile is HD/16 K loads -- the same number of lanes per row group as DPP can
// reduce without the LDS pipe (quad_perm, row_half_mirror).  On the V^T side 4 lanes x 16 keys cover the tile's 64 bytes of a d
// row and a load covers 16 d rows: HD/16 loads, each lane sums 16 keys of its rows and a quad is reduced once at the end.  The
// alternative, 128-key tiles (whole 128-B lines of V^T per request), doubles the registers a tile holds and leaves a context of
// ~1100 keys with 9 tiles for 8 waves; with 64-key tiles the other half of a V^T line is the next wave's tile, requested at the
// same time by the same block.  Per tile a wave has HD x 64 x 2 bytes in flight (16 KB at hd 128), half the bf16 kernel's.
// The scales: lane i fetches k_scale / v_scale of key t0 + i with the K rows, they go through the wave's LDS row next to the raw
// dot products; score = dot * k_scale * softmax_scale and p * v_scale are fp32 products on the 16 keys a lane owns.  Keys at or
// beyond the range are masked by SELECT on the score, on p * v_scale and on the V^T values (their bytes and scales may be
// NaN / inf); K rows and scales past the range are never read (the index is clamped to the last key).
// ------------------------------------------------------------------------------------
struct Kv8AttnArgs {
  const bf16_t* q; const uint8_t* k; const uint8_t* vt; const float* ks; const float* vs; bf16_t* out;
  int64_t ldq, ldo;
  int Sk, H, Hkv, Smax;
  float scale;
};

template <int HD>
__global__ __launch_bounds__(512) void attn_decode_fp8kv_kernel(Kv8AttnArgs p, float* part, int nsplit, int chunk, int* counters) {
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
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int n = min(p.Sk, kv_lo + chunk) - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * nsplit + sp) * (HD + 2);
  const int64_t bh = (int64_t)b * p.Hkv + hk;
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
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        const int r = min(t0 + u * RPW + lr, hi - 1);
        kk[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(K + (int64_t)r * HD + lc));   // read once per step by one block
      }
      const int ki = min(t0 + lane, hi - 1);
      ksc = KS[ki];
      vsc = VS[ki];
    };
    load_k(lo);
    for (int t0 = lo; t0 < hi; t0 += 512) {
      u32x4 vv[NVL];
      const int kvc = min(t0 + c16, last_vec);             // vectors past the wave's range re-read its last one (masked below)
#pragma unroll
      for (int j = 0; j < NVL; ++j)
        vv[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(VT + (int64_t)(j * 16 + dr) * p.Smax + kvc));
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
    if (nsplit == 1 && counters) {
      p.out[b * p.ldo + h * HD + tid] = f2bf(o / L);
    } else {
      po[tid] = o;
      if (tid == 0) { po[HD] = M; po[HD + 1] = L; }
    }
  }
  if (!counters || nsplit == 1) return;
  decode_combine_tail<HD>(p.out, p.ldo, (int64_t)HD, p.H, part, po, nsplit, counters, b, h, tid);
}

// the stand-alone form's merge of the split partials: the arithmetic of decode_combine_tail, value for value
template <int HD>
__global__ void attn_decode_fp8kv_combine_kernel(const float* part, bf16_t* out, int64_t ldo, int H, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const float* pp = part + (int64_t)(b * H + h) * nsplit * (HD + 2);
  float m = -INFINITY;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, pp[s * (HD + 2) + HD]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = pp[s * (HD + 2) + HD];
    const float w = (ms == -INFINITY) ? 0.f : __expf(ms - m);
    acc += w * pp[s * (HD + 2) + d];
    l += w * pp[s * (HD + 2) + HD + 1];
  }
  out[b * ldo + h * HD + d] = f2bf(acc / l);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int a3v_kv_quantize_fp8(const void* k_src, const void* vt_src, int Smax_src, int src_pos, void* k_q, void* vt_q, float* k_scale,
                                   float* v_scale, int B, int Hkv, int hd, int S, int Smax, int dst_pos, void* stream) {
  if (!k_src || !vt_src || !k_q || !vt_q || !k_scale || !v_scale || B <= 0 || Hkv <= 0 || S <= 0) return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (Smax <= 0 || Smax % 64 || Smax_src <= 0 || src_pos < 0 || dst_pos < 0 || src_pos + (int64_t)S > Smax_src || dst_pos + (int64_t)S > Smax)
    return A3V_ERR_SHAPE;
  if (!al16(k_src) || !al16(vt_src) || !al16(k_q) || !al16(vt_q) || !al16(k_scale) || !al16(v_scale)) return A3V_ERR_SHAPE;
  KvqArgs a{(const bf16_t*)k_src, (const bf16_t*)vt_src, (uint8_t*)k_q, (uint8_t*)vt_q, k_scale, v_scale, Hkv, S, Smax, Smax_src, src_pos, dst_pos};
  const int tiles = ((dst_pos + S - 1) >> 6) - (dst_pos >> 6) + 1;
  const dim3 grid(tiles, Hkv, B);
  if (hd == 128) hipLaunchKernelGGL(kv_quant_fp8_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv_quant_fp8_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_kv_dequantize_fp8(const void* k_q, const void* vt_q, const float* k_scale, const float* v_scale, int Smax, void* k_dst,
                                     void* vt_dst, int Smax_dst, int B, int Hkv, int hd, int n, void* stream) {
  if (!k_q || !vt_q || !k_scale || !v_scale || !k_dst || !vt_dst || B <= 0 || Hkv <= 0 || n <= 0) return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (Smax <= 0 || Smax % 64 || n > Smax || n > Smax_dst) return A3V_ERR_SHAPE;
  if (!al16(k_q) || !al16(vt_q) || !al16(k_scale) || !al16(v_scale) || !al16(k_dst) || !al16(vt_dst)) return A3V_ERR_SHAPE;
  KvdArgs a{(const uint8_t*)k_q, (const uint8_t*)vt_q, k_scale, v_scale, (bf16_t*)k_dst, (bf16_t*)vt_dst, hd, n, Smax, Smax_dst};
  const int64_t chunks = (int64_t)((n + 7) / 8) * hd;     // >= n * hd / 8: the V^T side's count covers the K side's
  hipLaunchKernelGGL(kv_dequant_fp8_kernel, dim3((unsigned)((chunks + 255) / 256), B * Hkv, 2), dim3(256), 0, (hipStream_t)stream, a);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_attention_decode_fp8kv_splits(int B, int H, int Sk) {
  if (B <= 0 || H <= 0 || Sk <= 0) return A3V_ERR_ARG;
  int ns, ch;
  a3v_decode_wave_plan(B, H, Sk, &ns, &ch);
  return ns;
}

extern "C" int a3v_attention_decode_fp8kv(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                                          const float* v_scale, void* out, int64_t ldo, int B, int Sk, int H, int Hkv, int hd, int Smax,
                                          float* scratch, int* counters, void* stream) {
  if (!q || !k_q || !vt_q || !k_scale || !v_scale || !out || !scratch || B <= 0 || Sk <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (hd != 64 && hd != 128) return A3V_ERR_SHAPE;
  if (H % Hkv || Smax <= 0 || Smax % 64 || Sk > Smax || ldq % 8 || ldq < (int64_t)H * hd || ldo < (int64_t)H * hd) return A3V_ERR_SHAPE;
  if (!al16(q) || !al16(k_q) || !al16(vt_q) || !al16(k_scale) || !al16(v_scale)) return A3V_ERR_SHAPE;
  Kv8AttnArgs p{(const bf16_t*)q, (const uint8_t*)k_q, (const uint8_t*)vt_q, k_scale, v_scale, (bf16_t*)out, ldq, ldo, Sk, H, Hkv, Smax,
                1.0f / sqrtf((float)hd)};
  int ns, ch;
  a3v_decode_wave_plan(B, H, Sk, &ns, &ch);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ns, H, B);
  if (hd == 128) hipLaunchKernelGGL(attn_decode_fp8kv_kernel<128>, grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  else hipLaunchKernelGGL(attn_decode_fp8kv_kernel<64>, grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  A3V_LAUNCH_CHECK();
  if (!counters) {
    if (hd == 128) hipLaunchKernelGGL(attn_decode_fp8kv_combine_kernel<128>, dim3(H, B), dim3(128), 0, st, scratch, (bf16_t*)out, ldo, H, ns);
    else hipLaunchKernelGGL(attn_decode_fp8kv_combine_kernel<64>, dim3(H, B), dim3(64), 0, st, scratch, (bf16_t*)out, ldo, H, ns);
    A3V_LAUNCH_CHECK();
  }
  return A3V_OK;
}
