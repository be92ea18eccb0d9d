// 8-bit AdamW moments for gfx950: blockwise e4m3 state (include/a3vlm_hip.h, "8-bit AdamW moments"), its quantiser, the inverse, and
// the AdamW step that reads and writes the codes.
// Format: a tensor of n elements (n % 256 == 0) is n / 256 blocks of 256 consecutive elements.  exp_avg m is stored as e4m3 codes m_q
// and one fp32 scale per block; exp_avg_sq v is stored as its square root r = sqrtf(v) in the same form (r_q, r_scale).  Per block
// scale = max(max|x|, 1e-30) / 448, q = e4m3(x / scale) with a true division, round to nearest even, saturating; a non-zero r whose
// quotient rounds to code 0 is stored as code 0x01.  Stored values: m^ = float(q) * scale, v^ = (float(q) * scale)^2.
//
//  * adam8_quant_kernel / adam8_dequant_kernel : one wave per block of 256, 4 elements per lane.
//  * adamw8_kernel : the sequence a3v_adam8_dequantize -> a3v_adamw_scaled -> a3v_adam8_quantize in one pass, value for value: the
//    three share the expressions below (adam8_widen, adamw_update of a3v_common.h, adam8_scale / adam8_codes), and none of them can be
//    contracted differently (the products of the widening are __fmul_rn).  One wave owns one block: per lane one 16-B load of p and
//    of g and one 4-B load of each code word, the update in fp32 registers, two wave reductions without the LDS pipe (wave_max) for
//    max|m'| and max r', then one 16-B parameter store, one 8-B bf16 store, two 4-B code stores; lane 0 stores the two scales.  18.06 B
//    per parameter with the image against the fp32 kernel's 30.  Every byte is touched once per step: the non-temporal policy of
//    adamw_kernel on loads and stores.  A wave walks blocks wave, wave + waves-in-grid, ...; the loads of its next block are issued
//    before the divisions and conversions of the current one, so a wave keeps two blocks' worth of requests in flight.
#include "a3v_common.h"

namespace {

constexpr int ADAM8_BLOCK = 256;           // elements per scale
constexpr int ADAM8_MAX_WG = 1024;         // 256 CUs x 4 workgroups x 4 waves: 16 waves per CU walk the blocks

__device__ __forceinline__ void fp8x4_to_f32(unsigned w, float* o) {       // v_cvt_pk_f32_fp8: exact
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}
// codes + block scales -> m^, v^ of the lane's 4 elements
__device__ __forceinline__ void adam8_widen(unsigned mw, float msc, unsigned rw, float rsc, float* m, float* v) {
  float a[4], b[4];
  fp8x4_to_f32(mw, a);
  fp8x4_to_f32(rw, b);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    m[e] = __fmul_rn(a[e], msc);
    const float r = __fmul_rn(b[e], rsc);
    v[e] = __fmul_rn(r, r);
  }
}
// the floor is 1e-30, not the KV cache's 1e-12: moments of small gradients are legitimately far below 1e-12
__device__ __forceinline__ float adam8_scale(float amax) { return fmaxf(amax, 1e-30f) / 448.f; }
// four values -> four e4m3 bytes: true division, round to nearest even, saturating at +-448.  keep_nonzero (r only): a non-zero
// value whose quotient rounds to code 0 becomes code 0x01, so an element that has seen a gradient never gets the denominator 0 + eps
template <bool KEEP_NONZERO>
__device__ __forceinline__ unsigned adam8_codes(const float* x, float scale) {
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(x[e] / scale, -448.f), 448.f);
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
  unsigned u = (unsigned)w;
  if (KEEP_NONZERO) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x[e] != 0.f && ((u >> (8 * e)) & 0x7fu) == 0u) u |= 1u << (8 * e);
  }
  return u;
}

// grid: waves walk the n / 256 blocks; either pair may be absent
__global__ __launch_bounds__(256) void adam8_quant_kernel(const float* __restrict__ m, const float* __restrict__ v, unsigned* __restrict__ mq,
                                                          float* __restrict__ ms, unsigned* __restrict__ rq, float* __restrict__ rs,
                                                          int64_t nblk) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += stride) {
    const int64_t i = b * 64 + lane;
    if (m) {
      const f32x4 x4 = reinterpret_cast<const f32x4*>(m)[i];
      float x[4], amax = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { x[e] = x4[e]; amax = fmaxf(amax, fabsf(x[e])); }
      const float sc = adam8_scale(wave_max(amax));
      mq[i] = adam8_codes<false>(x, sc);
      if (lane == 0) ms[b] = sc;
    }
    if (v) {
      const f32x4 x4 = reinterpret_cast<const f32x4*>(v)[i];
      float r[4], rmax = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { r[e] = sqrtf(x4[e]); rmax = fmaxf(rmax, r[e]); }
      const float sc = adam8_scale(wave_max(rmax));
      rq[i] = adam8_codes<true>(r, sc);
      if (lane == 0) rs[b] = sc;
    }
  }
}

__global__ __launch_bounds__(256) void adam8_dequant_kernel(const unsigned* __restrict__ mq, const float* __restrict__ ms,
                                                            const unsigned* __restrict__ rq, const float* __restrict__ rs,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t nblk) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += stride) {
    const int64_t i = b * 64 + lane;
    float mm[4], vv[4];
    adam8_widen(mq ? mq[i] : 0u, mq ? ms[b] : 0.f, rq ? rq[i] : 0u, rq ? rs[b] : 0.f, mm, vv);
    if (mq) reinterpret_cast<f32x4*>(m)[i] = f32x4{mm[0], mm[1], mm[2], mm[3]};
    if (rq) reinterpret_cast<f32x4*>(v)[i] = f32x4{vv[0], vv[1], vv[2], vv[3]};
  }
}

struct Adam8In { f32x4 p, g; unsigned mw, rw; float msc, rsc; };

__device__ __forceinline__ Adam8In adam8_load(const float* p, const float* g, const unsigned* mq, const float* ms, const unsigned* rq,
                                              const float* rs, int64_t b, int lane) {
  const int64_t i = b * 64 + lane;
  Adam8In x;
  x.p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
  x.g = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
  x.mw = __builtin_nontemporal_load(mq + i);
  x.rw = __builtin_nontemporal_load(rq + i);
  x.msc = ms[b];
  x.rsc = rs[b];
  return x;
}

__global__ __launch_bounds__(256) void adamw8_kernel(float* __restrict__ p, const float* __restrict__ g, unsigned* __restrict__ mq,
                                                     float* __restrict__ ms, unsigned* __restrict__ rq, float* __restrict__ rs,
                                                     int64_t nblk, float decay, float b1, float b2, float step_size, float inv_bc2_sqrt,
                                                     float eps, bf16_t* __restrict__ img, const float* __restrict__ gscale) {
  const float gs = gscale ? *gscale : 1.f;
  if (adamw_skip(gs)) return;                      // negative or NaN: no-op on the parameter, the codes, the scales and the image
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;
  Adam8In cur = adam8_load(p, g, mq, ms, rq, rs, b, lane);
  for (;;) {
    const int64_t nb = b + stride;
    const bool more = nb < nblk;                 // wave-uniform
    Adam8In nxt = cur;
    if (more) nxt = adam8_load(p, g, mq, ms, rq, rs, nb, lane);      // blocks are disjoint: nothing this wave stores below is read here
    float mm[4], vv[4], rr[4];
    adam8_widen(cur.mw, cur.msc, cur.rw, cur.rsc, mm, vv);
    f32x4 pp = cur.p;
    float amax = 0.f, rmax = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = __fmul_rn(cur.g[e], gs);
      float pe = pp[e];
      adamw_update(pe, ge, mm[e], vv[e], decay, b1, b2, step_size, inv_bc2_sqrt, eps);
      pp[e] = pe;
      rr[e] = sqrtf(vv[e]);
      amax = fmaxf(amax, fabsf(mm[e]));
      rmax = fmaxf(rmax, rr[e]);
    }
    const float msc = adam8_scale(wave_max(amax)), rsc = adam8_scale(wave_max(rmax));
    const int64_t i = b * 64 + lane;
    __builtin_nontemporal_store(pp, reinterpret_cast<f32x4*>(p) + i);
    if (img) {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(pp[e]);
      __builtin_nontemporal_store(o, reinterpret_cast<bf16x4*>(img) + i);
    }
    __builtin_nontemporal_store(adam8_codes<false>(mm, msc), mq + i);
    __builtin_nontemporal_store(adam8_codes<true>(rr, rsc), rq + i);
    if (lane == 0) { ms[b] = msc; rs[b] = rsc; }
    if (!more) break;
    cur = nxt;
    b = nb;
  }
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline unsigned adam8_grid(int64_t nblk) {
  const int64_t wg = (nblk + 3) / 4;
  return (unsigned)(wg < ADAM8_MAX_WG ? wg : ADAM8_MAX_WG);
}

}  // namespace

extern "C" int a3v_adam8_quantize(const float* m, const float* v, uint8_t* m_q, float* m_scale, uint8_t* r_q, float* r_scale, int64_t n,
                                  void* stream) {
  const bool has_m = m || m_q || m_scale, has_v = v || r_q || r_scale;
  if (n <= 0 || (!has_m && !has_v)) return A3V_ERR_ARG;
  if ((has_m && (!m || !m_q || !m_scale)) || (has_v && (!v || !r_q || !r_scale))) return A3V_ERR_ARG;
  if (n % ADAM8_BLOCK) return A3V_ERR_SHAPE;
  if (!al(m, 16) || !al(v, 16) || !al(m_q, 16) || !al(r_q, 16) || !al(m_scale, 4) || !al(r_scale, 4)) return A3V_ERR_SHAPE;
  const int64_t nblk = n / ADAM8_BLOCK;
  hipLaunchKernelGGL(adam8_quant_kernel, dim3(adam8_grid(nblk)), dim3(256), 0, (hipStream_t)stream, m, v, (unsigned*)m_q, m_scale,
                     (unsigned*)r_q, r_scale, nblk);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_adam8_dequantize(const uint8_t* m_q, const float* m_scale, const uint8_t* r_q, const float* r_scale, float* m, float* v,
                                    int64_t n, void* stream) {
  const bool has_m = m || m_q || m_scale, has_v = v || r_q || r_scale;
  if (n <= 0 || (!has_m && !has_v)) return A3V_ERR_ARG;
  if ((has_m && (!m || !m_q || !m_scale)) || (has_v && (!v || !r_q || !r_scale))) return A3V_ERR_ARG;
  if (n % ADAM8_BLOCK) return A3V_ERR_SHAPE;
  if (!al(m, 16) || !al(v, 16) || !al(m_q, 16) || !al(r_q, 16) || !al(m_scale, 4) || !al(r_scale, 4)) return A3V_ERR_SHAPE;
  const int64_t nblk = n / ADAM8_BLOCK;
  hipLaunchKernelGGL(adam8_dequant_kernel, dim3(adam8_grid(nblk)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)m_q, m_scale,
                     (const unsigned*)r_q, r_scale, m, v, nblk);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_adamw8_scaled(float* param, const float* grad, uint8_t* m_q, float* m_scale, uint8_t* r_q, float* r_scale, int64_t n,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* bf16_image,
                                 const float* grad_scale, void* stream) {
  if (!param || !grad || !m_q || !m_scale || !r_q || !r_scale || n <= 0 || step < 1) return A3V_ERR_ARG;
  if (n % ADAM8_BLOCK) return A3V_ERR_SHAPE;
  if (!al(param, 16) || !al(grad, 16) || !al(m_q, 16) || !al(r_q, 16) || !al(bf16_image, 16) || !al(m_scale, 4) || !al(r_scale, 4) ||
      !al(grad_scale, 4))
    return A3V_ERR_SHAPE;
  // the host scalars of a3v_adamw_scaled, derived the same way
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1), inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  const float decay = (float)(1.0 - (double)lr * (double)weight_decay);
  const int64_t nblk = n / ADAM8_BLOCK;
  hipLaunchKernelGGL(adamw8_kernel, dim3(adam8_grid(nblk)), dim3(256), 0, (hipStream_t)stream, param, grad, (unsigned*)m_q, m_scale,
                     (unsigned*)r_q, r_scale, nblk, decay, beta1, beta2, step_size, inv_bc2_sqrt, eps, (bf16_t*)bf16_image, grad_scale);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
