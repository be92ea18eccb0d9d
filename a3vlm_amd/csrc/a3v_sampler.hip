// Sampling controls on the device: top-k and min-p beside top-p (a3v_sample_top_k_p; semantics in include/a3vlm_hip.h).
//
// One 1024-thread block per row, as a3v_sample_top_p (a3v_rowops.hip), and the same two mass selections (topp_select, a3v_common.h)
// -- run on MASKED values: a token a filter removed holds -1 in the LDS copy of e_i (every pass of the selection skips negative
// values: no atomic, no tie match, mass 0), or, above the cache's size (V > 32768, A3V_SAMPLER_CACHE=0), a cleared bit in an 8-KiB
// keep bitmap beside which e_i is recomputed per pass with the same expression.
//   top-k   the k-th largest logit by a radix descent over COUNT histograms (integer LDS atomics: exact, order-independent) on an
//           order-preserving 32-bit key of z_i, digits taken from key - min_key shifted so that the first digit spans the row's
//           range (at most 4 passes, fewer for a narrow range); per-wave histograms in the mass histograms' memory.  The mask is the
//           comparison key(z_i) >= key(t): the logits' own bits, all ties at t kept.
//   top-p   selection 1 on the masked values, target top_p * Z_K.
//   min-p   after selection 1: one more pass masks e_i < min_p and sums what is left in Z's summation order (a sum of a subset of
//           the same non-negative terms in the same order: never above Z); M = min(top-p mass, min-p mass).  Both sets are prefixes
//           of one ranking, so the smaller mass is the shorter prefix.
//   draw    selection 2 on the masked values at u * M.  With min-p on it builds its own first histogram (selection 1's still holds
//           the tokens min-p removed), so a draw can only land on a token every filter kept, whatever the rounding of M.
// With both filters off no mask is written and every statement that touches a float is a3v_sample_top_p's, in its order.
#include "a3v_common.h"
#include <math.h>

namespace {

// order-preserving key of a float (-0 ranks as +0, as the comparison z_i >= t does)
__device__ __forceinline__ unsigned zkey(float v) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}

// key of the k-th largest of r[0 .. V) counting duplicates, 1 <= k <= V; zmin / zmax: the smallest / largest key of the row
__device__ unsigned topk_threshold(const float* __restrict__ r, int V, int k, unsigned zmin, unsigned zmax, TopPShared& sh) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned* hist = reinterpret_cast<unsigned*>(&sh.hist[0][0]);      // [16][256] per-wave counts
  unsigned* bin = reinterpret_cast<unsigned*>(&sh.bin[0]);
  const unsigned range = zmax - zmin;
  const int nbits = range == 0 ? 0 : 32 - __clz((int)range);
  const int levels = (nbits + 7) / 8, lsh = levels * 8 - nbits;
  unsigned prefix = 0, remaining = (unsigned)k;
  for (int level = levels - 1; level >= 0; --level) {
    const int shift = level * 8;
    for (int b = tid; b < 16 * 256; b += 1024) hist[b] = 0u;
    __syncthreads();
    for (int i0 = tid; i0 < V; i0 += 4096) {
      float z4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * 1024;
        z4[q] = i < V ? r[i] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned kk = (zkey(z4[q]) - zmin) << lsh;
        if (i0 + q * 1024 < V && (level == levels - 1 || (kk >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&hist[wave * 256 + ((kk >> shift) & 255)], 1u);
      }
    }
    __syncthreads();
    if (tid < 256) {
      unsigned c = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) c += hist[w * 256 + tid];
      bin[tid] = c;
    }
    if (tid == 0) { sh.found = 0; sh.tie_n = 0; }
    __syncthreads();
    if (wave == 0) {
      // lane l owns bins 4 l .. 4 l + 3; the highest bin whose count together with everything above it reaches `remaining`
      unsigned c4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) c4[q] = bin[lane * 4 + q];
      const unsigned own = (c4[0] + c4[1]) + (c4[2] + c4[3]);
      unsigned suf = own;                                  // inclusive suffix over lanes >= l
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = (unsigned)__shfl_down((int)suf, o, 64);
        if (lane + o < 64) suf += v;
      }
      unsigned excl = suf - own;                           // elements in bins above 4 l + 3
      int hit = -1;
      unsigned hit_excl = 0;
#pragma unroll
      for (int q = 3; q >= 0; --q) {
        const unsigned incl = excl + c4[q];
        if (hit < 0 && incl >= remaining) { hit = lane * 4 + q; hit_excl = excl; }
        excl = incl;
      }
      int best = hit;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
      if (hit >= 0 && hit == best) { sh.found = hit; sh.tie_n = (int)hit_excl; }
    }
    __syncthreads();
    prefix |= (unsigned)sh.found << shift;
    remaining -= (unsigned)sh.tie_n;
    __syncthreads();
  }
  return (prefix >> lsh) + zmin;                           // (levels == 0: every logit of the row is the same value)
}

// MODE 1: e_i kept in LDS (V <= 32768), a removed token holds -1.  MODE 2: e_i recomputed per pass, keep bitmap in LDS (V <= 65536).
template <int MODE>
__global__ __launch_bounds__(1024) void sample_top_k_p_kernel(const float* __restrict__ logits, int64_t ld, int V, float T, int top_k, float top_p,
                                                              float min_p, const float* __restrict__ u, int64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char samp_lds[];
  TopPShared& sh = *reinterpret_cast<TopPShared*>(samp_lds);
  float* ec = reinterpret_cast<float*>(samp_lds + ((sizeof(TopPShared) + 15) & ~(size_t)15));     // MODE 1: [V]; MODE 2: the bitmap
  unsigned long long* keep = reinterpret_cast<unsigned long long*>(ec);                          // word j * 16 + wave = tokens j * 1024 + wave * 64 ..
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* r = logits + (int64_t)blockIdx.x * ld;
  const bool topk = top_k > 0;                             // (the host maps top_k >= V to 0)
  const int iters = (V + 1023) / 1024;
  // x_max (and the key range of the row for top-k), fixed order
  float xm = -INFINITY;
  unsigned zmin = 0xffffffffu, zmax = 0u;
  for (int i = tid; i < V; i += 1024) {
    const float zi = r[i];
    xm = fmaxf(xm, zi / T);
    if (topk) {
      const unsigned k = zkey(zi);
      zmin = min(zmin, k);
      zmax = max(zmax, k);
    }
  }
  xm = wave_max(xm);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    zmin = min(zmin, (unsigned)__shfl_xor((int)zmin, o, 64));
    zmax = max(zmax, (unsigned)__shfl_xor((int)zmax, o, 64));
  }
  if (lane == 0) { sh.red[wave] = xm; sh.ured[0][wave] = zmin; sh.ured[1][wave] = zmax; }
  __syncthreads();
  xm = sh.red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) xm = fmaxf(xm, sh.red[w]);
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    zmin = min(zmin, sh.ured[0][w]);
    zmax = max(zmax, sh.ured[1][w]);
  }
  __syncthreads();
  // 1. top-k: the threshold key, then the mask is one comparison per token
  unsigned tk = 0u;
  if (topk) tk = topk_threshold(r, V, top_k, zmin, zmax, sh);
  // Z_K and the key range of e over K; the masked e_i (MODE 1) or the keep bitmap (MODE 2) is written on the way
  float z = 0.f;
  unsigned kmin = 0xffffffffu, kmax = 0u;
  for (int j = 0; j < iters; ++j) {
    const int i = j * 1024 + tid;
    bool in = i < V;
    float e = -1.f;
    if (in) {
      const float zi = r[i];
      e = expf(zi / T - xm);
      in = !topk || zkey(zi) >= tk;
    }
    if (in) {
      z += e;
      const unsigned k = __float_as_uint(e);
      kmin = min(kmin, k);
      kmax = max(kmax, k);
    }
    if constexpr (MODE == 1) {
      if (i < V) ec[i] = in ? e : -1.f;
    } else {
      const unsigned long long bl = __ballot(in);
      if (lane == 0) keep[j * 16 + wave] = bl;
    }
  }
  z = wave_sum(z);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
  }
  if (lane == 0) { sh.red[wave] = z; sh.ured[0][wave] = kmin; sh.ured[1][wave] = kmax; }
  __syncthreads();
  z = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    z += sh.red[w];
    kmin = min(kmin, sh.ured[0][w]);
    kmax = max(kmax, sh.ured[1][w]);
  }
  __syncthreads();
  const unsigned range = kmax - kmin;
  const int nbits = range == 0 ? 0 : 32 - __clz((int)range);
  const int levels = (nbits + 7) / 8, lsh = levels * 8 - nbits;
  // 2. top-p on K: the last kept token is the one the cumulative mass passes top_p * Z_K on
  TopPSel cut, pick;
  topp_select<MODE>(r, ec, V, T, xm, kmin, levels, lsh, top_p * z, false, false, sh, cut);
  float M = cut.above < 0.f ? z : cut.above + (float)(cut.rank + 1) * __uint_as_float(cut.key);
  // 3. min-p: mask e_i < min_p, the mass of what is left in Z's summation order
  const bool minp = min_p > 0.f;
  if (minp) {
    float mp = 0.f;
    for (int j = 0; j < iters; ++j) {
      const int i = j * 1024 + tid;
      const float e = i < V ? topp_e<MODE>(r, ec, i, T, xm) : -1.f;
      const bool in = e >= min_p;                          // (a token removed before holds -1)
      if (in) mp += e;
      if constexpr (MODE == 1) {
        if (i < V && !in) ec[i] = -1.f;
      } else {
        const unsigned long long bl = __ballot(in);
        if (lane == 0) keep[j * 16 + wave] = bl;
      }
    }
    mp = wave_sum(mp);
    if (lane == 0) sh.red[wave] = mp;
    __syncthreads();
    mp = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) mp += sh.red[w];
    __syncthreads();
    M = fminf(M, mp);
  }
  // 4. one draw from what is kept: inverse CDF at u * M
  float uu = u[blockIdx.x];
  uu = uu < 0.f ? 0.f : (uu >= 1.f ? 0.99999994f : uu);
  topp_select<MODE>(r, ec, V, T, xm, kmin, levels, lsh, uu * M, true, !minp, sh, pick);
  if (tid == 0) {
    out[blockIdx.x] = pick.id < 0 ? 0 : pick.id;          // (id < 0 only for a row without any finite logit)
  }
}

}  // namespace

#define ST (hipStream_t)stream

extern "C" int a3v_sample_top_k_p(const float* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p, float min_p,
                                  const float* u, int64_t* out, void* stream) {
  if (!logits || !u || !out || B <= 0 || V <= 0 || top_k < 0 || !(min_p >= 0.f && min_p <= 1.f)) return A3V_ERR_ARG;
  if (V > 65536 || !(temperature > 0.f) || !(top_p > 0.f)) return A3V_ERR_SHAPE;
  const int k = top_k >= V ? 0 : top_k;                    // k >= V keeps every token: off
  const size_t base = (sizeof(TopPShared) + 15) & ~(size_t)15;
  if (V <= 32768 && A3V_ENV_INT("A3V_SAMPLER_CACHE", 1)) {
    static bool attr[A3V_MAX_DEV][1] = {};
    const int bytes = (int)(base + (size_t)V * 4);
    const int rc = a3v_dyn_lds_once(attr, 0, (const void*)sample_top_k_p_kernel<1>, 160 * 1024);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(sample_top_k_p_kernel<1>, dim3(B), dim3(1024), (size_t)bytes, ST, logits, ld, V, temperature, k, top_p, min_p, u, out);
  } else {
    hipLaunchKernelGGL(sample_top_k_p_kernel<2>, dim3(B), dim3(1024), base + 8192, ST, logits, ld, V, temperature, k, top_p, min_p, u, out);
  }
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
