// MXFP4 weight images (OCP MX v1.0: e2m1 elements, one e8m0 scale per 32 consecutive k of a row) for decode: quantiser, dequantiser
// and the decode GEMV on v_mfma_scale_f32_16x16x128_f8f6f4 with fp4 weights and MXFP8 (e4m3fn + e8m0) activations.  The format is
// stated in include/a3vlm_hip.h ("MXFP4 weights") and restated on the CPU in tests/mx4_ref.py.
#include "a3v_common.h"

namespace {
typedef __attribute__((ext_vector_type(8))) int i32x8;

// floor(log2(x)) of a finite x > 0 (fp32 denormals included: v_frexp_exp_i32_f32 normalises them)
__device__ __forceinline__ int floor_log2(float x) { return __builtin_amdgcn_frexp_expf(x) - 1; }
__device__ __forceinline__ int clamp_e8m0(int e) { return e < -127 ? -127 : (e > 127 ? 127 : e); }

// e2m1 code of v = w / 2^E: nearest grid value (0 .5 1 1.5 2 3 4 6), ties to the even code, saturating at 6; -0 -> +0
__device__ __forceinline__ uint32_t e2m1_code(float v) {
  const float a = fabsf(v);
  const uint32_t c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return c | ((v < 0.f && c) ? 8u : 0u);
}

// One thread per 8 weights (one 16-B load, one packed 4-B store); the four lanes of a 32-k block share its maximum.
__global__ __launch_bounds__(256) void mx4_quant_kernel(const bf16_t* __restrict__ W, int64_t ldw, uint8_t* __restrict__ q, int64_t ldq,
                                                        uint8_t* __restrict__ s, int K, int64_t n8) {
  int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n8;
  t = live ? t : n8 - 1;                               // n8 % 16 == 0: a block's four lanes are live or dead together
  const int k8 = K >> 3;
  const int64_t n = t / k8;
  const int c = (int)(t - n * k8);
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(W + n * ldw + (int64_t)c * 8);
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[e]));
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  uint32_t o = 0;
  int E = 0;
  if (m > 0.f) {
    E = clamp_e8m0(floor_log2(m) - 2);
#pragma unroll
    for (int e = 0; e < 8; ++e) o |= e2m1_code(ldexpf((float)v[e], -E)) << (4 * e);     // element 2j in the low nibble of byte j
  }
  if (!live) return;
  *reinterpret_cast<uint32_t*>(q + n * ldq + (int64_t)c * 4) = o;
  if ((c & 3) == 0) s[n * (K >> 5) + (c >> 2)] = (uint8_t)(E + 127);
}

// 2^(s - 127) as the fp32 scale operand of the packed conversions (s = 0: the fp32 denormal 2^-127)
__device__ __forceinline__ float e8m0_value(uint32_t s) { return __builtin_bit_cast(float, s ? s << 23 : 0x00400000u); }

// Wd = e2m1(q) * 2^(s - 127), exact in bf16: v_cvt_scalef32_pk_bf16_fp4, two codes per instruction.  One thread per 8 codes.
__global__ __launch_bounds__(256) void mx4_dequant_kernel(const uint8_t* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ s,
                                                          bf16_t* __restrict__ out, int64_t ldo, int K, int64_t n8) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n8) return;
  const int k8 = K >> 3;
  const int64_t n = t / k8;
  const int c = (int)(t - n * k8);
  const uint32_t w = *reinterpret_cast<const uint32_t*>(q + n * ldq + (int64_t)c * 4);
  const float sc = e8m0_value(s[n * (K >> 5) + (c >> 2)]);
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
  const bf16x8 o = {p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  *reinterpret_cast<bf16x8*>(out + n * ldo + (int64_t)c * 8) = o;
}

// ------------------------------------------------------------------------------------
// MXFP4 decode GEMV, M <= 16, N % 16 == 0, K % 128 == 0:  C = epilogue(sum_blocks 2^(ea + ew) * sum_32 a_q * w_q), fp32 accumulation.
// It stands on gemv_dma_bf16_kernel (a3v_gemv.hip): 4 waves per block, all on K slice `sl` of one 64-row group of W, wave w on the
// 16-row tile 4 tg + w; W streamed once, non-temporally, by coalesced LDS-DMA through wave-private rings; no block barrier in the K
// loop; split-K partials merged in slice order by the wave that arrives last at its tile's counter (bit-identical run to run).
//
// Operands of one v_mfma_scale_f32_16x16x128_f8f6f4 (W is the first operand, fp4: four of the eight operand registers; the activations
// the second, fp8 e4m3), as measured on the device and pinned by the exact family of tests/test_gpu_mx4.py.  The instruction's k runs
// over four 32-k blocks c = 0..3.  fp4: lane (fr = lane & 15, fg = lane >> 4) holds block c = fg of row fr, 16 B of codes, element j in
// nibble j (low nibble first).  fp8: the same lane holds 16 B of block fg >> 1 (its half fg & 1) in registers 0-3 and 16 B of block
// 2 + (fg >> 1) (same half) in registers 4-7.  Scales: for BOTH operands the scale byte of block c is the one lane group c supplies.
// D[n = 4 fg + r][m = fr].  Which MX block of the row plays block c is free as long as both operands agree.
// The unit of the K loop is 512 k = 16 blocks = 4 MFMAs: lane group fg takes blocks 4 fg .. 4 fg + 3, so ONE dword per lane holds its
// four scale bytes (byte b shifted down for MFMA b) and its codes are 64 contiguous bytes of the row.  The K % 512 remainder (1..3 steps of 128 k, last slice only) takes blocks r fg + b of the
// remainder straight from global memory (issued before the ring starts).
//
// Bytes in flight.  A 16-row x 128-k MFMA step is 1 KB of codes + 64 scale bytes; a ring stage is one unit: 4 KB of codes (4 LDS-DMA
// instructions of 4 rows x 256 contiguous bytes, slot XOR row swizzle on the source side as the bf16 ring) + 256 B of scales (one
// 4-B-per-lane instruction: 16 rows x 16 B) = 4352 B.  The bf16 kernel keeps one 4-KB stage in flight per wave behind the one it
// consumes, and two blocks per CU: 32 KB per CU.  A 4-bit stage is consumed four times faster per byte (4 MFMAs per 4 KB against
// 16), so the ring has THREE slots: two stages (8.5 KB) in flight per wave, 34 KB per block, 68 KB per CU with two blocks resident.
// LDS: rings 4 x 3 x 4352 = 52224 B + the block's A slice as MXFP8 (8448 B per unit, at most 4 units = 2048 k per slice): 60672 ..
// 86016 B (+ 2 KB static): two blocks per CU (160 KB) up to 3 units, ONE at 4 units (7B w13 and LM head at two K slices).  The A
// slice is quantised by the block after its first ring stages are issued, but the overlap is small: the A loads are issued behind up
// to 15 LDS-DMA instructions and memory returns in order, so the wait for the first A data is also a wait for those stages, and the
// block barrier behind the quantisation stands in front of every wave's first MFMA (DESIGN 7e lists both among the suspected costs).
// ------------------------------------------------------------------------------------
struct Mx4Args {
  const bf16_t* A;
  const uint8_t* q;
  const uint8_t* s;
  void* C;
  const void* res;
  float* part;
  int* counters;
  int64_t lda, ldq, ldc, ldr;
  int M, N, K, epi, S, nun, tgs, tiles, maxun, tail;   // nun: 512-k units of K (the last may be partial: `tail` steps of 128 k, 0 = whole)
};

constexpr int MX_SLOT = 4352, MX_NSL = 3, MX_DPS = 5;   // bytes per ring slot, slots per wave, LDS-DMA instructions per stage
constexpr int MX_ACODES = 8192, MX_ASCALES = 256;       // bytes of A codes / scales per unit: [block 16][half 2][row 16][16 B], [row 16][block 16]
constexpr int MX_MAXUN = 4, MX_MAXS = 8;

__device__ __forceinline__ f32x4 mx_mfma(u32x4 w, u32x4 a0, u32x4 a1, f32x4 acc, uint32_t sw, uint32_t sa) {
  const i32x8 wv = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
  const i32x8 av = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv, av, acc, 4, 0, 0, (int)sw, 0, (int)sa);   // scale byte 0 of both operands
}

__device__ __forceinline__ void mx4_finish(const Mx4Args& p, f32x4 v, f32x4 u, int nt0, int lane, bool swiglu) {
  const int m = lane & 15;
  if (m >= p.M || nt0 >= p.N) return;
  if (swiglu) {
    const int oc = (nt0 >> 1) + (lane >> 4) * 4;
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(rbf(silu(rbf(v[r]))) * rbf(u[r]));
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + oc) = o;
    return;
  }
  const int n = nt0 + (lane >> 4) * 4;
  float o4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o4[r] = rbf(v[r]);
  if (p.epi & A3V_EPI_RESIDUAL) {
    const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] += bf2f(rr[r]);
  }
  if (p.epi & A3V_EPI_OUT_F32) {
    const f32x4 o = {o4[0], o4[1], o4[2], o4[3]};
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = o;
  } else {
    const bf16x4 o = {f2bf(o4[0]), f2bf(o4[1]), f2bf(o4[2]), f2bf(o4[3])};
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n) = o;
  }
}

__global__ __launch_bounds__(256) void gemv_mx4_kernel(Mx4Args p) {
  constexpr int WAUX = 2;                              // nt: the weights are streamed once per step
  extern __shared__ __attribute__((aligned(1024))) char mx_lds[];
  __shared__ f32x4 xch[2][64];                         // one-slice SwiGLU: the up tile's accumulators on their way to the gate tile's wave
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xq = blockIdx.x >> 3;                      // block -> (row group, slice): the slices of a row group share an XCD
  const int sl = xq % p.S;
  const int tg = (xq / p.S) * 8 + (blockIdx.x & 7);
  if (tg >= p.tgs) return;
  const int u0 = (int)(((int64_t)sl * p.nun) / p.S), u1 = (int)(((int64_t)(sl + 1) * p.nun) / p.S);
  const int r = (p.tail && u1 == p.nun) ? p.tail : 0;  // 128-k steps of the partial last unit (this slice owns it)
  const int nfull = u1 - u0 - (r ? 1 : 0);
  const int nkb = nfull * 16 + r * 4;                  // MX blocks of this slice
  char* Ac = mx_lds;
  char* As = mx_lds + p.maxun * MX_ACODES;
  char* Wring = As + p.maxun * MX_ASCALES + wave * (MX_NSL * MX_SLOT);
  const int tile = tg * 4 + wave;
  const bool live = tile < p.tiles;
  const int n0 = tile * 16;
  const int fr = lane & 15, fg = lane >> 4;
  const int64_t ldsc = p.K >> 5;

  // the remainder's weight fragments, straight from global memory
  u32x4 tw[3];
  uint32_t tsw[3];
  int wrf = n0 + fr;
  wrf = wrf < p.N ? wrf : p.N - 1;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    tw[b] = u32x4{0u, 0u, 0u, 0u};
    tsw[b] = 127u;
    if (b < r) {
      const int64_t gkb = (int64_t)(u0 + nfull) * 16 + r * fg + b;
      tw[b] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.q + (int64_t)wrf * p.ldq + gkb * 16));
      tsw[b] = p.s[(int64_t)wrf * ldsc + gkb];
    }
  }
  // ring: instruction i covers rows 4 i + (lane >> 4), 16-B slot lane & 15 of a 256-B stage row (chunk slot ^ row); scales: one
  // dword per lane, dword lane & 3 of the 16 scale bytes of row lane >> 2
  const char* wsrc[5];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * i + fg;
    int wr = n0 + row;
    wr = wr < p.N ? wr : p.N - 1;
    wsrc[i] = reinterpret_cast<const char*>(p.q) + (int64_t)wr * p.ldq + (int64_t)u0 * 256 + ((fr ^ row) & 15) * 16;
  }
  {
    int sr = n0 + (lane >> 2);
    sr = sr < p.N ? sr : p.N - 1;
    wsrc[4] = reinterpret_cast<const char*>(p.s) + (int64_t)sr * ldsc + (int64_t)u0 * 16 + (lane & 3) * 4;
  }
  auto dma_stage = [&](int st, int slot) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + st * 256),
                                       (__attribute__((address_space(3))) void*)(Wring + slot * MX_SLOT + i * 1024), 16, 0, WAUX);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[4] + st * 16),
                                     (__attribute__((address_space(3))) void*)(Wring + slot * MX_SLOT + 4096), 4, 0, WAUX);
  };
  if (live) {
    if (nfull > 0) dma_stage(0, 0);
    if (nfull > 1) dma_stage(1, 1);
    if (nfull > 2) dma_stage(2, 2);
  }
  // A slice -> MXFP8 in LDS: one (row, block) item per thread and pass; rows >= M are zero blocks
  for (int it = threadIdx.x; it < 16 * nkb; it += 256) {
    const int m = it / nkb, kb = it - m * nkb;
    u32x4 c0 = {0u, 0u, 0u, 0u}, c1 = {0u, 0u, 0u, 0u};
    uint32_t sb = 127u;
    if (m < p.M) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(p.A + (int64_t)m * p.lda + ((int64_t)u0 * 16 + kb) * 32);
      bf16x8 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = src[i];
      float mx = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf((float)v[i][e]));
      if (mx > 0.f) {
        const int E = clamp_e8m0(floor_log2(mx) - 8);
        sb = (uint32_t)(E + 127);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = fminf(fmaxf(ldexpf((float)v[i][e], -E), -448.f), 448.f);   // saturating; the conversion rounds to nearest even
          int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
          lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
          int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
          hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
          if (i < 2) { c0[2 * i] = (uint32_t)lo; c0[2 * i + 1] = (uint32_t)hi; }
          else { c1[2 * i - 4] = (uint32_t)lo; c1[2 * i - 3] = (uint32_t)hi; }
        }
      }
    }
    *reinterpret_cast<u32x4*>(Ac + (kb * 2 + 0) * 256 + m * 16) = c0;
    *reinterpret_cast<u32x4*>(Ac + (kb * 2 + 1) * 256 + m * 16) = c1;
    reinterpret_cast<uint8_t*>(As)[(kb >> 4) * 256 + m * 16 + (kb & 15)] = (uint8_t)sb;
  }
  __syncthreads();
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    for (int st = 0; st < nfull; ++st) {
      const int slot = st % MX_NSL;
      if (st + 3 <= nfull) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * MX_DPS) : "memory");   // stage st landed; up to two later stages in flight
      else if (st + 2 <= nfull) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MX_DPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const char* Ws = Wring + slot * MX_SLOT;
      u32x4 wq[4], a0[4], a1[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        wq[b] = *reinterpret_cast<const u32x4*>(Ws + fr * 256 + (((4 * fg + b) ^ fr) & 15) * 16);
        a0[b] = *reinterpret_cast<const u32x4*>(Ac + ((st * 16 + 4 * (fg >> 1) + b) * 2 + (fg & 1)) * 256 + fr * 16);
        a1[b] = *reinterpret_cast<const u32x4*>(Ac + ((st * 16 + 4 * (2 + (fg >> 1)) + b) * 2 + (fg & 1)) * 256 + fr * 16);
      }
      const uint32_t sw = *reinterpret_cast<const uint32_t*>(Ws + 4096 + fr * 16 + fg * 4);
      const uint32_t sa = *reinterpret_cast<const uint32_t*>(As + st * 256 + fr * 16 + fg * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // fragments are in registers: the slot may be overwritten
      if (st + MX_NSL < nfull) dma_stage(st + MX_NSL, slot);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b & 1) acc1 = mx_mfma(wq[b], a0[b], a1[b], acc1, sw >> (8 * b), sa >> (8 * b));
        else acc0 = mx_mfma(wq[b], a0[b], a1[b], acc0, sw >> (8 * b), sa >> (8 * b));
      }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if (b < r) {
        const int kb = nfull * 16 + b;                 // + r c: the block of lane group c
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(Ac + ((kb + r * (fg >> 1)) * 2 + (fg & 1)) * 256 + fr * 16);
        const u32x4 a1 = *reinterpret_cast<const u32x4*>(Ac + ((kb + r * (2 + (fg >> 1))) * 2 + (fg & 1)) * 256 + fr * 16);
        const uint32_t sa = reinterpret_cast<const uint8_t*>(As)[nfull * 256 + fr * 16 + r * fg + b];
        if (b & 1) acc1 = mx_mfma(tw[b], a0, a1, acc1, tsw[b], sa);
        else acc0 = mx_mfma(tw[b], a0, a1, acc0, tsw[b], sa);
      }
  }
  f32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = acc0[i] + acc1[i];
  const bool swiglu = (p.epi & A3V_EPI_SWIGLU) != 0;
  f32x4 u = {0.f, 0.f, 0.f, 0.f};
  int nt0 = n0;
  if (p.S == 1) {
    if (swiglu) {                                      // gate tile on the even wave, up tile on the odd one
      if (wave & 1) xch[wave >> 1][lane] = v;
      __syncthreads();
      if (wave & 1) return;
      u = xch[wave >> 1][lane];
    }
    if (live) mx4_finish(p, v, u, nt0, lane, swiglu);
    return;
  }
  if (!live) return;
  // Wave-granular split-K fix-up, as gemv_dma_bf16_kernel: partial out with agent-coherent stores, acknowledge, arrival counter of the
  // tile (of the gate / up pair with SwiGLU); the last arriver sums the S partials in slice order and leaves the counter at zero.
  float* mine = p.part + (((int64_t)(tg * p.S + sl) * 4 + wave) * 64 + lane) * 4;
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(mine), "v"(v) : "memory");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int* ctr = p.counters + (swiglu ? tg * 2 + (wave >> 1) : tg * 4 + wave);
  const int expect = swiglu ? 2 * p.S : p.S;
  int old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = __builtin_amdgcn_readfirstlane(old);
  if (old != expect - 1) return;
  if (lane == 0) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int w0 = swiglu ? (wave & ~1) : wave;
  nt0 = (tg * 4 + w0) * 16;
  const float* base = p.part + (((int64_t)tg * p.S * 4 + w0) * 64 + lane) * 4;
  f32x4 x[MX_MAXS], y[MX_MAXS];
#pragma unroll
  for (int s8 = 0; s8 < MX_MAXS; ++s8) {
    const float* src = base + (int64_t)(s8 < p.S ? s8 : p.S - 1) * 4 * 64 * 4;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(x[s8]) : "v"(src) : "memory");
  }
  if (swiglu) {
#pragma unroll
    for (int s8 = 0; s8 < MX_MAXS; ++s8) {
      const float* src = base + 64 * 4 + (int64_t)(s8 < p.S ? s8 : p.S - 1) * 4 * 64 * 4;
      asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(y[s8]) : "v"(src) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]), "+v"(y[6]), "+v"(y[7])::"memory");
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])::"memory");
  v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s8 = 0; s8 < MX_MAXS; ++s8)
    if (s8 < p.S) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += x[s8][i];
      if (swiglu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] += y[s8][i];
      }
    }
  mx4_finish(p, v, u, nt0, lane, swiglu);
}

bool mx4_shape_ok(int M, int N, int K, int epilogue) {
  if (M < 1 || M > 16 || N < 16 || N % 16 || N > 65536 || K < 128 || K % 128) return false;
  if (epilogue & ~(A3V_EPI_RESIDUAL | A3V_EPI_SWIGLU | A3V_EPI_OUT_F32)) return false;
  if ((epilogue & A3V_EPI_SWIGLU) && (epilogue != A3V_EPI_SWIGLU || N % 32)) return false;
  return true;
}

// plan[]: grid x, block size, K slices, W rows per block, dynamic LDS bytes, 512-k units of K, 64-row groups, units of A per slice
int mx4_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan) {
  if (!mx4_shape_ok(M, N, K, epilogue) || cus <= 0) return A3V_ERR_SHAPE;
  const int nun = (K + 511) / 512, tgs = (N / 16 + 3) / 4;
  const int smin = (nun + MX_MAXUN - 1) / MX_MAXUN, smax = nun < MX_MAXS ? nun : MX_MAXS;
  if (smin > MX_MAXS) return A3V_ERR_SHAPE;            // K > 16384: the block's A slice would not fit its LDS
  int S = (2 * cus + tgs - 1) / tgs;                   // two resident blocks per CU
  S = S < smin ? smin : (S > smax ? smax : S);
  const int maxun = (nun + S - 1) / S;
  plan[0] = (tgs + 7) / 8 * 8 * S;
  plan[1] = 256;
  plan[2] = S;
  plan[3] = 64;
  plan[4] = maxun * (MX_ACODES + MX_ASCALES) + 4 * MX_NSL * MX_SLOT;
  plan[5] = nun;
  plan[6] = tgs;
  plan[7] = maxun;
  return A3V_OK;
}
}  // namespace

extern "C" int a3v_mx4_gemv_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan) {
  if (!plan) return A3V_ERR_ARG;
  return mx4_plan(M, N, K, epilogue, cus, plan);
}

extern "C" int64_t a3v_gemm_skinny_mxfp4_ws_bytes(int M, int N, int K) {
  int32_t plan[A3V_MX4_PLAN_INTS];
  if (mx4_plan(M, N, K, 0, a3v_cu_count(), plan) != A3V_OK) return 0;
  return (int64_t)A3V_WS_PARTIALS + (int64_t)plan[6] * MX_MAXS * 4 * 64 * 4 * 4;    // any S the plan may pick for this shape
}

extern "C" int a3v_quantize_mxfp4(const void* w, int64_t ldw, void* q, int64_t ldq, void* s, int N, int K, void* stream) {
  if (!w || !q || !s) return A3V_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 128 || ldw < K || ldw % 8 || ldq < K / 2 || ldq % 16) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(q)) & 15) return A3V_ERR_SHAPE;
  const int64_t n8 = (int64_t)N * (K / 8);
  if ((n8 + 255) / 256 > 0x7fffffff) return A3V_ERR_SHAPE;
  hipLaunchKernelGGL(mx4_quant_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, ldw,
                     (uint8_t*)q, ldq, (uint8_t*)s, K, n8);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_dequantize_mxfp4(const void* q, int64_t ldq, const void* s, void* out, int64_t ldo, int N, int K, void* stream) {
  if (!q || !s || !out) return A3V_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 128 || ldo < K || ldo % 8 || ldq < K / 2 || ldq % 16) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(q)) & 15) return A3V_ERR_SHAPE;
  const int64_t n8 = (int64_t)N * (K / 8);
  if ((n8 + 255) / 256 > 0x7fffffff) return A3V_ERR_SHAPE;
  hipLaunchKernelGGL(mx4_dequant_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q, ldq,
                     (const uint8_t*)s, (bf16_t*)out, ldo, K, n8);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_gemm_skinny_mxfp4(const void* A, int64_t lda, const void* q, int64_t ldq, const void* s, void* C, int64_t ldc, int M,
                                     int N, int K, const void* residual, int64_t ldr, int epilogue, void* workspace, void* stream) {
  if (!A || !q || !s || !C || !workspace) return A3V_ERR_ARG;
  if ((epilogue & A3V_EPI_RESIDUAL) && !residual) return A3V_ERR_ARG;
  int32_t plan[A3V_MX4_PLAN_INTS];
  if (mx4_plan(M, N, K, epilogue, 256, plan) != A3V_OK) return A3V_ERR_SHAPE;      // shape refusals need no device
  const int ncol = (epilogue & A3V_EPI_SWIGLU) ? N / 2 : N;
  if (lda < K || lda % 8 || ldq < K / 2 || ldq % 16 || ldc < ncol || ldc % 4) return A3V_ERR_SHAPE;
  if ((epilogue & A3V_EPI_RESIDUAL) && (ldr < N || ldr % 4 || (reinterpret_cast<uintptr_t>(residual) & 7))) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return A3V_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(s) & 3) return A3V_ERR_SHAPE;
  if (mx4_plan(M, N, K, epilogue, a3v_cu_count(), plan) != A3V_OK) return A3V_ERR_SHAPE;
  Mx4Args p;
  p.A = (const bf16_t*)A; p.q = (const uint8_t*)q; p.s = (const uint8_t*)s; p.C = C; p.res = residual;
  p.counters = (int*)workspace;
  p.part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + A3V_WS_PARTIALS);
  p.lda = lda; p.ldq = ldq; p.ldc = ldc; p.ldr = ldr;
  p.M = M; p.N = N; p.K = K; p.epi = epilogue; p.S = plan[2]; p.nun = plan[5]; p.tgs = plan[6]; p.tiles = N / 16; p.maxun = plan[7];
  p.tail = (K / 128) % 4;
  static bool attr_done[A3V_MAX_DEV][1];
  const int rc = a3v_dyn_lds_once(attr_done, 0, (const void*)gemv_mx4_kernel, MX_MAXUN * (MX_ACODES + MX_ASCALES) + 4 * MX_NSL * MX_SLOT);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gemv_mx4_kernel, dim3((unsigned)plan[0]), dim3(256), (size_t)plan[4], (hipStream_t)stream, p);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
