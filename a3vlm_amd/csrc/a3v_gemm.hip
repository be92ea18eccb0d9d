// C[M,N] = epilogue(A[M,K] @ W[N,K]^T) for gfx950.
//
//  * gemm_nt_bf16_kernel : MFMA (v_mfma_f32_16x16x32_bf16) 128x128x64 tile, 4 waves (2x2),
//    each wave 64x64 = 4x4 MFMA tiles; both operands K-contiguous ("NT"), staged
//    HBM -> LDS with 16-byte LDS-DMA (global_load_lds_dwordx4), two LDS stages.
//    LDS image: [row][8 x 16-B slot], slot' = slot ^ ((row>>1)&7) -- the permutation is
//    applied on the per-lane SOURCE address (LDS-DMA destinations are lane-linear) and
//    again on the ds_read_b128 address; it makes every 16-lane ds_read_b128 group hit
//    16 distinct 16-B slots of the 256-B bank row (conflict-free).
//    MFMA is issued as D = W_frag x A_frag so a lane ends up with 4 CONSECUTIVE n for
//    one m: 8-byte bf16 / 16-byte fp32 row-contiguous stores and a lane-local epilogue
//    (bias, GELU, residual, SwiGLU on interleaved w1/w3 row blocks).
//    blockIdx -> tile map is XCD-aware (8 XCDs, private L2s): each XCD walks a
//    contiguous range of GROUP_M-tall tile groups.
//  * the decode GEMVs (M <= 16: a3v_gemm_skinny / _fp8 / _nf4, a3v_gemv_fused) and their planner live in a3v_gemv.hip.
//  * gemm_nt_f32_kernel : fp32 parity path (plain FMA, 64x64x16 tile).
#include "a3v_common.h"
#include <algorithm>
#include <cstring>
#include <type_traits>

namespace {

constexpr int BK = 64;
constexpr int GROUP_M = 8;
constexpr int GEMM_EPI_RAW = 1 << 20;     // internal: fp32 output without the bf16 rounding of the accumulator
constexpr int GEMM_EPI_SCALE = 1 << 22;   // internal: fp8 operands -- accumulator *= sa[m] * sw[n] (per-row scales of A and W) first
constexpr int GEMM_EPI_ROPEKV = 1 << 21;  // internal: fused-qkv epilogue (a3v_gemm_qkv_rope): RoPE on q / k, k -> K cache, v -> V^T cache

// destination of the fused-qkv epilogue: C row m = b*S + s; columns [q heads | k heads | v heads], hd = 1 << hd_shift each
struct RopeKvArgs {
  bf16_t* q_out;         // [rows][ldq], head-major columns (may alias nothing else the GEMM reads)
  bf16_t* k_cache;       // [B][Hkv][Smax][hd]
  bf16_t* vt_cache;      // [B][Hkv][hd][Smax]
  const float* cos_sin;  // [pos][hd/2][2]
  bf16_t* v_rows;        // optional [rows][ldv]: v also token-major (the attention backward reads it that way)
  int64_t ldq, ldv;
  int S, H, Hkv, hd_shift, Smax, start_pos, rope_pos0, m_off;
};

struct GemmArgs {
  const bf16_t* A;
  const bf16_t* W;
  void* C;
  const void* bias;
  const void* res;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K, epi;
  int tiles_m, tiles_n;
  int slow_epi;   // 1: interior tiles also take the general epilogue (A3V_GEMM_FAST_EPI=0; equality tests and A/B runs)
  int nt_store;   // fast epilogue forms: non-temporal stores of the output tile (A3V_GEMM_NT_STORE, read per launch)
  float* sumsq;   // fp32 outputs (weight gradients): slot (tile * 8 + wave) <- sum of squares of the values this wave stored (NULL: off)
  int64_t c_split;   // split-K (128x128 kernel, gridDim.y slices): byte stride between the slices' output planes
  RopeKvArgs rk;     // GEMM_EPI_ROPEKV only
  const float* sa;   // GEMM_EPI_SCALE: per-row dequantisation scales of A [M] and W [N]
  const float* sw;
  int xmap;          // ring kernel: 1 = every round of gridDim.x tiles is cut into eight runs, one per XCD (see tile_of)
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
// erf-GELU for the bf16 epilogues: Abramowitz-Stegun 7.1.26 (|erf error| < 1.5e-7, far below the bf16 rounding that follows)
// with one v_rcp and one v_exp instead of libm's branchy erff (the c_fc epilogue of the ViT cost 25 us of an 85-us GEMM)
__device__ __forceinline__ float gelu_erf_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float erf_abs = 1.f - poly * __expf(-z * z);
  return 0.5f * x * (1.f + copysignf(erf_abs, x));
}
// x * sigmoid(a x) with v_rcp_f32 (1 ulp) instead of the IEEE division sequence (~10 VALU instructions): the result is rounded to
// bf16 right after, and the SwiGLU epilogue of a 256x256 tile was VALU-bound on it (13 k cycles per tile)
__device__ __forceinline__ float quick_gelu(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * x)); }

// Stage one ROWS-row x 64-k bf16 tile with LDS-DMA.  Chunks of 8 rows (1 KiB = one wave
// instruction); lane -> (row = chunk*8 + lane/8, physical 16-B slot = lane%8).
template <int ROWS, int NWAVES>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ G, int64_t ld, int row0,
                                           int last_row, int k0, char* lds_tile, int wave, int lane) {
  constexpr int PER_WAVE = ROWS / 8 / NWAVES;
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int c = wave * PER_WAVE + i;
    const int r = c * 8 + (lane >> 3);
    const int s = (lane & 7) ^ ((r >> 1) & 7);
    int gr = row0 + r;
    gr = gr < last_row ? gr : last_row;
    const bf16_t* src = G + (int64_t)gr * ld + k0 + s * 8;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(lds_tile + c * 1024), 16, 0, 0);
  }
}

// Weight-gradient GEMMs can hand the global-norm clip its sum of squares for free: every wave adds up the squares of the fp32
// values it stores and writes ONE partial to slot (tile_m * tiles_n + tile_n) * 8 + (wave's position in the tile) -- a layout that
// depends only on the output coordinates, not on the block order (the caller zeroes the slots once per step and sums them).
__device__ __forceinline__ void sumsq_flush(const GemmArgs& p, float ss, int mbase, int nbase, int lane) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) p.sumsq[(((int64_t)(mbase >> 8) * p.tiles_n + (nbase >> 8)) << 3) + (((mbase >> 7) & 1) << 2) + ((nbase >> 6) & 3)] = ss;
}

// Compiler-level ordering point between the two halves of a wave-private LDS transpose (the hardware executes one wave's LDS
// instructions in order; what has to be prevented is the compiler moving a read of one vector type across writes of another)
#define LDS_ORDER() asm volatile("" ::: "memory")

// Fast forms of the epilogue for wave tiles that lie INSIDE C (16 TM x 64 outputs, no ragged edge) and the output kinds of the
// decoder's big linears: plain bf16, bf16 residual, fp32 residual stream, fp32 (raw or rounded, with or without accumulation),
// SwiGLU.  Same arithmetic as the general form below, bit for bit; what differs is the cost.  The general form tests the
// epilogue flags and both bounds per 16 x 16 tile and forms every address with a 64-bit multiply: its instruction stream for
// one 256 x 256 tile measured 21-25 k cycles where the stores alone need 3.5 k (one CU) to 8 k (all CUs storing at once,
// tools/ubench/stores.hip).  Here the kind is decided once per wave tile, addresses advance by a constant stride, residuals
// are read in the layout they are stored in (whole 128 / 256-byte row segments), and every value passes through the wave's
// private 4-KiB LDS patch so that it leaves as 16 bytes per lane.  Returns false when the tile is not eligible.
// SET selects which forms an instantiation carries: EPI_SET_COMMON the kinds of the decoder's linears, EPI_SET_PRE additionally
// bias / activation in front of them (the ViT), EPI_SET_ROPE the fused-qkv form alone.  The 256x256 kernels hold 128 accumulator
// registers and ~110 more across the k-loop; compiled together, the forms' peak pushed the k-loop's invariants into scratch
// (100 dwords per lane, 5-20 % of every kind's speed), so each big-tile kernel is instantiated per set and picked by the host.
constexpr int EPI_SET_COMMON = 1, EPI_SET_PRE = 2, EPI_SET_ROPE = 4, EPI_SET_SUMSQ = 8;   // SUMSQ: GemmArgs::sumsq honoured (weight-gradient kernels only)
template <int TM, int TN, int SET>
__device__ __forceinline__ bool gemm_epilogue_fast(f32x4 (&acc)[TM][TN], const GemmArgs& p, int mbase, int nbase, int lane, char* stage) {
  if constexpr (TN != 4 || ((TM % 4) != 0 && TM != 6)) {          // (TM = 6: the 192-row ring tiles)
    return false;
  } else {
    // opaque copies: everything below is recomputed per tile AFTER the k-loop instead of being hoisted out of the persistent tile
    // loop and kept (or spilled) across the k-loop, whose 244 live VGPRs leave no room
    int kind = p.epi & (0xffff | GEMM_EPI_RAW | GEMM_EPI_ROPEKV | GEMM_EPI_SCALE);
    int64_t ldc_ = p.ldc, ldr_ = p.ldr;
    uintptr_t c_ = reinterpret_cast<uintptr_t>(p.C), r_ = reinterpret_cast<uintptr_t>(p.res);
    asm volatile("" : "+s"(kind), "+s"(ldc_), "+s"(ldr_), "+s"(c_), "+s"(r_));
    if (!stage || p.slow_epi || mbase + TM * 16 > p.M || nbase + 64 > p.N || (c_ & 15)) return false;
    const int mrow = lane & 15, g = lane >> 4;
    float ss = 0.f;                                      // p.sumsq: squares of the fp32 values this wave stores
    const bool nts = p.nt_store != 0;                      // output tiles are written once and read by a later kernel: streaming stores
    auto st_c = [&](auto* ptr, auto val) { if (nts) __builtin_nontemporal_store(val, ptr); else *ptr = val; };
    const int pre = (SET & EPI_SET_PRE) ? kind & (A3V_EPI_BIAS | A3V_EPI_GELU | A3V_EPI_QUICKGELU) : 0;   // applied in the accumulator layout
    if (pre) kind &= ~pre;
    if constexpr ((SET & EPI_SET_COMMON) != 0) {
    if (kind == 0 || kind == A3V_EPI_RESIDUAL || kind == A3V_EPI_RES_F32 || kind == A3V_EPI_SWIGLU_BWD) {
      // bf16 staging: chunk = two 16-row tiles x 64 columns = 32 rows x 128 B; 8-byte slot s of row r at slot s ^ (r & 14),
      // read back as 16-byte pairs: pair q of row r from physical pair q ^ ((r >> 1) & 7) (see the general form)
      const bool f32 = kind == A3V_EPI_RES_F32;
      if (f32 ? ((ldc_ & 3) || (ldr_ & 3) || (r_ & 15)) : (ldc_ & 7)) return false;       // (before anything touches the accumulators)
      if ((kind == A3V_EPI_RESIDUAL || kind == A3V_EPI_SWIGLU_BWD) && ((ldr_ & 7) || (r_ & 15))) return false;
      if (kind == A3V_EPI_SWIGLU_BWD && (p.N & 7)) return false;
      uintptr_t b_ = reinterpret_cast<uintptr_t>(p.bias);
      asm volatile("" : "+s"(b_));
      if ((pre & A3V_EPI_BIAS) && (b_ & 7)) return false;
      // bias / activation in front (the ViT's linears): y = act(bf16(acc + bias)), each step rounded to bf16 as the general form
      // does; applied as the values are staged (a separate pass over the 128 accumulators kept the k-loop's state in scratch)
      float bv[4][4];
      if constexpr ((SET & EPI_SET_PRE) != 0) {
        if (pre) {
          if (f32) return false;                               // (fp32 stream with bias: not a shape of the path; general form)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bf16x4 b4 = {};
            if (pre & A3V_EPI_BIAS) b4 = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(b_) + nbase + j * 16 + g * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[j][e] = (pre & A3V_EPI_BIAS) ? bf2f(b4[e]) : 0.f;
          }
        }
      }
      auto pre_value = [&](float v, int j, int e) {
        v = rbf(v + bv[j][e]);
        if (pre & A3V_EPI_GELU) v = rbf(gelu_erf_fast(v));
        else if (pre & A3V_EPI_QUICKGELU) v = rbf(quick_gelu(v));
        return v;
      };
      const int l3 = lane >> 3, q = lane & 7;
      char* const wr = stage + mrow * 128;
      const int wx = mrow & 14;
      const char* const rd = stage + l3 * 128;
      const int rx = l3 >> 1;
      auto put = [&](int ic) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[2 * ic + ii][j][e];
              if constexpr ((SET & EPI_SET_PRE) != 0) { if (pre) v = pre_value(v, j, e); }
              o[e] = f2bf(v);
            }
            *reinterpret_cast<bf16x4*>(wr + ii * 2048 + (((j * 4 + g) ^ wx) << 3)) = o;
          }
        LDS_ORDER();        // the reads below are of another vector type: keep the compiler from moving them across these writes
      };
      auto get = [&](int it) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(rd + it * 1024 + ((q ^ rx ^ ((it & 1) << 2)) << 4));
        LDS_ORDER();        // ... and the next chunk's writes behind this read
        return v;
      };
      if (!f32) {
        bf16_t* cp = reinterpret_cast<bf16_t*>(c_) + (int64_t)(mbase + l3) * ldc_ + nbase + q * 8;
        const int64_t cstep = 8 * ldc_;
        if (kind == 0) {
#pragma unroll
          for (int ic = 0; ic < TM / 2; ++ic) {
            put(ic);
#pragma unroll
            for (int it = 0; it < 4; ++it) { st_c(reinterpret_cast<bf16x8*>(cp), get(it)); cp += cstep; }
          }
        } else if (kind == A3V_EPI_SWIGLU_BWD) {
          // the tile is d(act): gate / up read from `res` (gu [M, 2 N]) as whole 16-byte row segments, d(gate) -> C[., n], d(up) -> C[., N + n]
          const bf16_t* gp = reinterpret_cast<const bf16_t*>(r_) + (int64_t)(mbase + l3) * ldr_ + nbase + q * 8;
          const int64_t rstep = 8 * ldr_;
          int un = p.N;                                     // columns between the gate and the up half (gu and C alike)
          asm volatile("" : "+s"(un));
#pragma unroll
          for (int ic = 0; ic < TM / 2; ++ic) {             // one 32-row chunk's gate + up in flight at a time (32 VGPRs)
            bf16x8 gg[4], uu[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              gg[it] = *reinterpret_cast<const bf16x8*>(gp);
              uu[it] = *reinterpret_cast<const bf16x8*>(gp + un);
              gp += rstep;
            }
            put(ic);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const bf16x8 v = get(it);
              bf16x8 og, ou;
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                float dg, du;
                swiglu_bwd_pair(bf2f(gg[it][e]), bf2f(uu[it][e]), bf2f(v[e]), dg, du);
                og[e] = f2bf(dg);
                ou[e] = f2bf(du);
              }
              st_c(reinterpret_cast<bf16x8*>(cp), og);
              st_c(reinterpret_cast<bf16x8*>(cp + un), ou);
              cp += cstep;
            }
          }
        } else {
          const bf16_t* rp = reinterpret_cast<const bf16_t*>(r_) + (int64_t)(mbase + l3) * ldr_ + nbase + q * 8;
          const int64_t rstep = 8 * ldr_;
#pragma unroll
          for (int half = 0; half < (TM + 2) / 4; ++half) { // the loads of two 32-row chunks in flight at a time (32 VGPRs); TM = 6: 2 + 1
            bf16x8 rr[2][4];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
              for (int it = 0; it < 4; ++it) {
                if (half * 2 + c < TM / 2) { rr[c][it] = *reinterpret_cast<const bf16x8*>(rp); rp += rstep; }
              }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              if (half * 2 + c >= TM / 2) continue;
              put(half * 2 + c);
#pragma unroll
              for (int it = 0; it < 4; ++it) {
                const bf16x8 v = get(it);
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(rr[c][it][e]) + bf2f(v[e]));
                st_c(reinterpret_cast<bf16x8*>(cp), o);
                cp += cstep;
              }
            }
          }
        }
      } else {
        // fp32 residual stream: out = res + bf16(acc); a lane's 8 values of a row are 32 contiguous bytes of res / C
        float* cp = reinterpret_cast<float*>(c_) + (int64_t)(mbase + l3) * ldc_ + nbase + q * 8;
        const float* rp = reinterpret_cast<const float*>(r_) + (int64_t)(mbase + l3) * ldr_ + nbase + q * 8;
        const int64_t cstep = 8 * ldc_, rstep = 8 * ldr_;
#pragma unroll
        for (int ic = 0; ic < TM / 2; ++ic) {               // one 32-row chunk's residual in flight at a time (32 VGPRs)
          f32x4 rr[4][2];
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            rr[it][0] = *reinterpret_cast<const f32x4*>(rp);
            rr[it][1] = *reinterpret_cast<const f32x4*>(rp + 4);
            rp += rstep;
          }
          put(ic);
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            const bf16x8 v = get(it);
            f32x4 o0, o1;
#pragma unroll
            for (int e = 0; e < 4; ++e) { o0[e] = rr[it][0][e] + bf2f(v[e]); o1[e] = rr[it][1][e] + bf2f(v[4 + e]); }
            if constexpr ((SET & EPI_SET_SUMSQ) != 0) {
              if (p.sumsq) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = fmaf(o0[e], o0[e], fmaf(o1[e], o1[e], ss));
              }
            }
            st_c(reinterpret_cast<f32x4*>(cp), o0);
            st_c(reinterpret_cast<f32x4*>(cp + 4), o1);
            cp += cstep;
          }
        }
        if constexpr ((SET & EPI_SET_SUMSQ) != 0) { if (p.sumsq) sumsq_flush(p, ss, mbase, nbase, lane); }
      }
      return true;
    }
    if (kind == (A3V_EPI_RES_F32 | GEMM_EPI_RAW) || kind == (A3V_EPI_OUT_F32 | GEMM_EPI_RAW) || kind == A3V_EPI_OUT_F32) {
      // fp32 staging: chunk = one 16-row tile x 64 columns = 16 rows x 256 B, 16-byte slot s of row r at slot s ^ r
      const bool accum = (kind & A3V_EPI_RES_F32) != 0, raw = (kind & GEMM_EPI_RAW) != 0;
      if ((ldc_ & 3) || (accum && ((ldr_ & 3) || (r_ & 15)))) return false;
      const int q = lane & 15;
      char* const wr = stage + mrow * 256;
      const char* const rd = stage + g * 256;
      float* cp = reinterpret_cast<float*>(c_) + (int64_t)(mbase + g) * ldc_ + nbase + q * 4;
      const float* rp = accum ? reinterpret_cast<const float*>(r_) + (int64_t)(mbase + g) * ldr_ + nbase + q * 4 : nullptr;
      const int64_t cstep = 4 * ldc_, rstep = 4 * ldr_;
#pragma unroll
      for (int half = 0; half < TM / 2; ++half) {           // two 16-row tiles' worth of the accumulated-into rows in flight (32 VGPRs)
        f32x4 rr[2][4];
        if (accum) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int it = 0; it < 4; ++it) { rr[i][it] = *reinterpret_cast<const f32x4*>(rp); rp += rstep; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f32x4 v = acc[half * 2 + i][j];
            if (!raw) {
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
            }
            *reinterpret_cast<f32x4*>(wr + (((j * 4 + g) ^ mrow) << 4)) = v;
          }
          LDS_ORDER();
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            f32x4 v = *reinterpret_cast<const f32x4*>(rd + it * 1024 + ((q ^ (it * 4 + g)) << 4));
            LDS_ORDER();
            if (accum) {
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = rr[i][it][e] + v[e];
            }
            if constexpr ((SET & EPI_SET_SUMSQ) != 0) {
              if (p.sumsq) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = fmaf(v[e], v[e], ss);
              }
            }
            st_c(reinterpret_cast<f32x4*>(cp), v);
            cp += cstep;
          }
        }
      }
      if constexpr ((SET & EPI_SET_SUMSQ) != 0) { if (p.sumsq) sumsq_flush(p, ss, mbase, nbase, lane); }
      return true;
    }
    if (kind == A3V_EPI_SWIGLU && (TM % 4) == 0) {
      // 64 interleaved columns -> 32 output columns = 64 B per row.  chunk = four 16-row tiles = 64 rows x 64 B; 8-byte slot
      // s = 4 jp + g of row r at slot s ^ (((r >> 2) & 3) << 1) (rows r, r+4, r+8, r+12 share banks: the XOR separates them and keeps
      // 16-byte pairs together); read back as pairs, 16 rows x 64 B per store instruction
      if (ldc_ & 7) return false;
      const int rr_ = lane >> 2, qq = lane & 3;
      char* const wr = stage + mrow * 64;
      const int wx = ((mrow >> 2) & 3) << 1;
      const char* const rd = stage + rr_ * 64 + ((qq ^ ((rr_ >> 2) & 3)) << 4);
      bf16_t* cp = reinterpret_cast<bf16_t*>(c_) + (int64_t)(mbase + rr_) * ldc_ + (nbase >> 1) + qq * 8;
      const int64_t cstep = 16 * ldc_;
#pragma unroll
      for (int ic = 0; ic < TM / 4; ++ic) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jp = 0; jp < 2; ++jp) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float gt = rbf(acc[4 * ic + ii][2 * jp][e]);
              const float up = rbf(acc[4 * ic + ii][2 * jp + 1][e]);
              o[e] = f2bf(rbf(silu(gt)) * up);
            }
            *reinterpret_cast<bf16x4*>(wr + ii * 1024 + (((jp * 4 + g) ^ wx) << 3)) = o;
          }
        LDS_ORDER();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(rd + it * 1024);
          LDS_ORDER();
          st_c(reinterpret_cast<bf16x8*>(cp), v);
          cp += cstep;
        }
      }
      return true;
    }
    }
    if constexpr ((SET & EPI_SET_ROPE) != 0) {
    if (kind == GEMM_EPI_ROPEKV && !pre) {
      // Fused qkv epilogue.  The wave's 64 columns lie inside ONE head slot (hd >= 64), so the whole wave tile is q, k or v.
      //   q, k : rotated in the accumulator layout (cos / sin rows read there), then through the bf16 transpose: q as whole
      //          128-byte row segments of q_out, k as 128-byte segments of the token's K-cache row;
      //   v    : token-major rows of v_rows (training) through the same transpose, and the V^T cache through a TRANSPOSING
      //          stage ([64 d][32 tokens]): 16-byte stores of 8 consecutive tokens of one d (2-byte aligned: legal here,
      //          tools/ubench/unaligned.hip) instead of one 2-byte store per element.
      RopeKvArgs k = p.rk;                                   // opaque per-tile copy: none of it is hoisted out of the tile loop
      asm volatile("" : "+s"(k.q_out), "+s"(k.k_cache), "+s"(k.vt_cache), "+s"(k.cos_sin), "+s"(k.v_rows), "+s"(k.ldq), "+s"(k.ldv));
      asm volatile("" : "+s"(k.S), "+s"(k.H), "+s"(k.Hkv), "+s"(k.hd_shift), "+s"(k.Smax), "+s"(k.start_pos), "+s"(k.rope_pos0), "+s"(k.m_off));
      const int hd = 1 << k.hd_shift;
      if (k.hd_shift < 6 || k.S < 32 || (k.ldq & 7) || (reinterpret_cast<uintptr_t>(k.q_out) & 15) || (reinterpret_cast<uintptr_t>(k.k_cache) & 15) ||
          (k.v_rows && ((k.ldv & 7) || (reinterpret_cast<uintptr_t>(k.v_rows) & 15))))
        return false;
      int slot = nbase >> k.hd_shift, d0 = nbase & (hd - 1), mg0 = mbase + k.m_off, S_ = k.S;
      asm volatile("" : "+s"(slot), "+s"(d0), "+s"(mg0), "+s"(S_));
      const int l3 = lane >> 3, q = lane & 7;
      char* const wr = stage + mrow * 128;
      const int wx = mrow & 14;
      const char* const rd = stage + l3 * 128;
      const int rx = l3 >> 1;
      auto get = [&](int it) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(rd + it * 1024 + ((q ^ rx ^ ((it & 1) << 2)) << 4));
        LDS_ORDER();
        return v;
      };
      auto put_plain = [&](int ic) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[2 * ic + ii][j][e]);
            *reinterpret_cast<bf16x4*>(wr + ii * 2048 + (((j * 4 + g) ^ wx) << 3)) = o;
          }
        LDS_ORDER();
      };
      if (slot < k.H + k.Hkv) {
        // q / k: rotated as the chunk is staged.  The cos / sin rows of a 32-row chunk (8 x 16 B per lane) are requested one chunk
        // ahead -- before the previous chunk's stores, so the loads never queue behind them -- and nothing of the tile is copied.
        int sqr = (mg0 + mrow) % S_;                        // token position of this lane's row in tile i; +16 per tile
        const float* csb = k.cos_sin + ((d0 + g * 4) >> 1) * 2;
        f32x4 csA[2][4], csB[2][4];
        auto load_cs = [&](f32x4 (&cs)[2][4]) {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) {
            asm volatile("" : "+v"(sqr));
            const float* csr = csb + (((int64_t)(k.rope_pos0 + sqr)) << k.hd_shift);      // (pos << (hd_shift - 1)) * 2 floats
#pragma unroll
            for (int j = 0; j < 4; ++j) cs[ii][j] = *reinterpret_cast<const f32x4*>(csr + j * 16);
            sqr += 16;
            if (sqr >= S_) sqr -= S_;
          }
        };
        auto put_rot = [&](int ic, const f32x4 (&cs)[2][4]) {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int i = 2 * ic + ii;
              const float v0 = rbf(acc[i][j][0]), v1 = rbf(acc[i][j][1]), v2 = rbf(acc[i][j][2]), v3 = rbf(acc[i][j][3]);
              bf16x4 o;
              o[0] = f2bf(v0 * cs[ii][j][0] - v1 * cs[ii][j][1]);
              o[1] = f2bf(v0 * cs[ii][j][1] + v1 * cs[ii][j][0]);
              o[2] = f2bf(v2 * cs[ii][j][2] - v3 * cs[ii][j][3]);
              o[3] = f2bf(v2 * cs[ii][j][3] + v3 * cs[ii][j][2]);
              *reinterpret_cast<bf16x4*>(wr + ii * 2048 + (((j * 4 + g) ^ wx) << 3)) = o;
            }
          LDS_ORDER();
        };
        const bool isq = slot < k.H;
        bf16_t* cp = k.q_out + nbase + (int64_t)(mg0 + l3) * k.ldq + q * 8;
        const int64_t cstep = 8 * k.ldq;
        int b = (mg0 + l3) / S_, sq = (mg0 + l3) - b * S_;
        bf16_t* const kb = k.k_cache + d0 + q * 8;
        const int hk = slot - k.H;
        load_cs(csA);
#pragma unroll
        for (int ic = 0; ic < TM / 2; ++ic) {
          if (ic + 1 < TM / 2) { if (ic & 1) load_cs(csA); else load_cs(csB); }
          if (ic & 1) put_rot(ic, csB); else put_rot(ic, csA);
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            if (isq) {
              asm volatile("" : "+v"(cp));
              st_c(reinterpret_cast<bf16x8*>(cp), get(it));
              cp += cstep;
            } else {
              asm volatile("" : "+v"(sq), "+v"(b));
              *reinterpret_cast<bf16x8*>(kb + ((((int64_t)b * k.Hkv + hk) * k.Smax + k.start_pos + sq) << k.hd_shift)) = get(it);
              sq += 8;
              if (sq >= S_) { sq -= S_; ++b; }
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        return true;
      }
      if (k.v_rows) {
        bf16_t* cp = k.v_rows + (nbase - ((k.H + k.Hkv) << k.hd_shift)) + (int64_t)(mg0 + l3) * k.ldv + q * 8;
        const int64_t cstep = 8 * k.ldv;
#pragma unroll
        for (int ic = 0; ic < TM / 2; ++ic) {
          put_plain(ic);
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            asm volatile("" : "+v"(cp));
            st_c(reinterpret_cast<bf16x8*>(cp), get(it));
            cp += cstep;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // V^T cache: [64 d][32 tokens] bf16 per chunk; the 16-byte token group c of row d sits at group c ^ ((d >> 2) & 3)
      {
        const int hv = slot - k.H - k.Hkv;
        int b0 = mg0 / S_, sq0 = mg0 - b0 * S_;             // first token of the chunk (wave-uniform)
        const int dr = lane >> 2, c = lane & 3;
#pragma unroll
        for (int ic = 0; ic < TM / 2; ++ic) {
          asm volatile("" : "+s"(sq0), "+s"(b0));
          if (sq0 + 32 <= S_) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
              for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  *reinterpret_cast<bf16_t*>(stage + (j * 16 + g * 4 + e) * 64 + (((ii * 2 + (mrow >> 3)) ^ g) << 4) + (mrow & 7) * 2) =
                      f2bf(acc[2 * ic + ii][j][e]);
            LDS_ORDER();
            bf16_t* const vb = k.vt_cache + ((((int64_t)b0 * k.Hkv + hv) << k.hd_shift) + d0) * k.Smax + k.start_pos + sq0 + c * 8;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int d = it * 16 + dr;
              const bf16x8 v = *reinterpret_cast<const bf16x8*>(stage + d * 64 + ((c ^ ((d >> 2) & 3)) << 4));
              LDS_ORDER();
              bf16_t* const dst = vb + (int64_t)d * k.Smax;               // 2-byte-aligned 16-byte store: the compiler would split it
              // (s_nop 1 inside the statement: hipcc pads no hazards of an asm store, and a 16-byte store reads its data registers a
              //  couple of states after issue -- without it the next instruction the compiler places here may overwrite them first;
              //  seen as zeros / stale values in a few V^T rows per launch once a re-schedule put a register write right behind)
              asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
            }
          } else {
            // the chunk's 32 tokens straddle two batch elements: element-wise, as the general form does
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
              const int t = sq0 + ii * 16 + mrow;
              const int bb = t >= S_ ? b0 + 1 : b0, ss = t >= S_ ? t - S_ : t;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                bf16_t* dst = k.vt_cache + ((((int64_t)bb * k.Hkv + hv) << k.hd_shift) + d0 + j * 16 + g * 4) * k.Smax + k.start_pos + ss;
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(int64_t)e * k.Smax] = f2bf(acc[2 * ic + ii][j][e]);
              }
            }
          }
          sq0 += 32;
          if (sq0 >= S_) { sq0 -= S_; ++b0; }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      return true;
    }
    }
    return false;
  }
}

// Epilogue shared by the tile kernels.  The lane holds, for each (i, j) MFMA tile,
// C[m = mbase + 16 i + (lane&15)][n = nbase + 16 j + 4 (lane>>4) + 0..3].
// `stage`: optional wave-private 4-KiB LDS scratch for gemm_epilogue_fast (tiles inside C, the common output kinds); everything
// else takes the general form below, whose stores are 8 bytes per lane scattered over 16 rows.
template <int TM, int TN, bool F8 = false, int SET = EPI_SET_COMMON>
__device__ __forceinline__ void gemm_epilogue(f32x4 (&acc)[TM][TN], const GemmArgs& p, int mbase, int nbase, int lane, char* stage = nullptr) {
  // ---- epilogue: lane holds C[m][n..n+3], m = .. + (lane&15), n = .. + (lane>>4)*4 ----
  if constexpr (!F8) {
    if (gemm_epilogue_fast<TM, TN, SET>(acc, p, mbase, nbase, lane, stage)) return;
  }
  const int epi = p.epi;
  const int mrow = lane & 15;
  const int ncol = (lane >> 4) * 4;
  RopeKvArgs rk_ = p.rk;                                   // opaque per-tile copy (see gemm_epilogue_fast): not hoisted out of a persistent tile loop
  if (epi & GEMM_EPI_ROPEKV) {
    asm volatile("" : "+s"(rk_.q_out), "+s"(rk_.k_cache), "+s"(rk_.vt_cache), "+s"(rk_.cos_sin), "+s"(rk_.v_rows), "+s"(rk_.ldq), "+s"(rk_.ldv));
    asm volatile("" : "+s"(rk_.S), "+s"(rk_.H), "+s"(rk_.Hkv), "+s"(rk_.hd_shift), "+s"(rk_.Smax), "+s"(rk_.start_pos), "+s"(rk_.rope_pos0), "+s"(rk_.m_off));
  }
  if constexpr (F8) {
    // fp8 operands: the accumulator holds sum_k qa[m][k] qw[n][k]; the value of the product is that times sa[m] sw[n].
    // All scale loads are issued before the first store of the tile: a load behind a store would wait for the store to drain.
    f32x4 swv[TN];
    float sam[TM];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nbase + j * 16 + ncol;
      swv[j] = n < p.N ? *reinterpret_cast<const f32x4*>(p.sw + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = mbase + i * 16 + mrow;
      sam[i] = m < p.M ? p.sa[m] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] *= sam[i] * swv[j][r];
  }
  if (epi & A3V_EPI_SWIGLU) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = mbase + i * 16 + mrow;
      if (m >= p.M) continue;
      // W rows interleaved in blocks of 16: even 16-block = w1 (gate), odd = w3 (up)
#pragma unroll
      for (int j = 0; j < TN; j += 2) {
        const int n = nbase + j * 16;        // interleaved row of the gate block
        if (n >= p.N) continue;
        const int oc = (n >> 1) + ncol;             // output column
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = rbf(acc[i][j][r]);
          const float u = rbf(acc[i][j + 1][r]);
          o[r] = f2bf(rbf(silu(g)) * u);
        }
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + oc) = o;
      }
    }
    return;
  }
  if (epi & A3V_EPI_SWIGLU_BWD) {
    // the product is d(act): d(gate) / d(up) from the forward's gate / up (res = gu [M, 2 N]); loads of half the tile before its stores
    constexpr int HM = TM >= 2 ? TM / 2 : 1, NH = TM / HM;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      bf16x4 gg[HM][TN], uu[HM][TN];
#pragma unroll
      for (int ih = 0; ih < HM; ++ih) {
        const int m = mbase + (half * HM + ih) * 16 + mrow;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = nbase + j * 16 + ncol;
          gg[ih][j] = bf16x4{};
          uu[ih][j] = bf16x4{};
          if (m < p.M && n < p.N) {
            const bf16_t* gr = reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n;
            gg[ih][j] = *reinterpret_cast<const bf16x4*>(gr);
            uu[ih][j] = *reinterpret_cast<const bf16x4*>(gr + p.N);
          }
        }
      }
#pragma unroll
      for (int ih = 0; ih < HM; ++ih) {
        const int i = half * HM + ih, m = mbase + i * 16 + mrow;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = nbase + j * 16 + ncol;
          if (n >= p.N) continue;
          bf16x4 og, ou;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float dg, du;
            swiglu_bwd_pair(bf2f(gg[ih][j][r]), bf2f(uu[ih][j][r]), rbf(acc[i][j][r]), dg, du);
            og[r] = f2bf(dg);
            ou[r] = f2bf(du);
          }
          bf16_t* cr = reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n;
          *reinterpret_cast<bf16x4*>(cr) = og;
          *reinterpret_cast<bf16x4*>(cr + p.N) = ou;
        }
      }
    }
    return;
  }
  // Phase 1 -- values: bias, the bf16 rounding F.linear applies, activation, rotary embedding, residual; everything that LOADS
  // (bias, cos/sin rows, residual) happens here, before the tile's first store: on this ISA a load issued behind stores can
  // only be waited for together with them, and at the end of a tile round the whole chip's store burst takes microseconds to
  // drain.  The loads of half the tile (TM/2 x TN vectors) are in flight at a time; the results overwrite the accumulators.
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int i = half * (TM / 2); i < (half + 1) * (TM / 2); ++i) {
      const int m = mbase + i * 16 + mrow;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = nbase + j * 16 + ncol;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
        if (epi & A3V_EPI_BIAS) {
          const bf16x4 b = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.bias) + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bf2f(b[r]);
        }
        if (!(epi & GEMM_EPI_RAW)) {      // split-K planes keep the raw fp32 partial sums (rounded once by the reduce pass)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = rbf(v[r]);   // the bf16 value F.linear returns
        }
        if (epi & GEMM_EPI_ROPEKV) {
          // v[] = the bf16 qkv values of token (b, s), columns n..n+3 of head slot n >> hd_shift: rotate the two (even, odd)
          // pairs of q / k by the token's position (LLM/llama_ens5.py:123-135 apply_rotary_emb); v passes through
          const RopeKvArgs& k = rk_;
          if (epi & A3V_EPI_RESIDUAL) {      // an additive term of the projection (the LoRA branch, model/peft.py:89-95): the
            // reference adds it to the bf16 linear output and rounds, before the rotation
            const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rbf(bf2f(rr[r]) + v[r]);
          }
          const int mg = m + k.m_off;
          const int sq = mg - (mg / k.S) * k.S;
          const int slot = n >> k.hd_shift, d = n & ((1 << k.hd_shift) - 1);
          if (slot < k.H + k.Hkv) {
            const f32x4 cs = *reinterpret_cast<const f32x4*>(k.cos_sin + (((int64_t)(k.rope_pos0 + sq) << (k.hd_shift - 1)) + (d >> 1)) * 2);
            const float o0 = v[0] * cs[0] - v[1] * cs[1], o1 = v[0] * cs[1] + v[1] * cs[0];
            const float o2 = v[2] * cs[2] - v[3] * cs[3], o3 = v[2] * cs[3] + v[3] * cs[2];
            v[0] = o0; v[1] = o1; v[2] = o2; v[3] = o3;
          }
        } else {
          if (epi & A3V_EPI_GELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rbf(gelu_erf_fast(v[r]));
          } else if (epi & A3V_EPI_QUICKGELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rbf(quick_gelu(v[r]));
          }
          if (epi & A3V_EPI_RES_F32) {
            const f32x4 rr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rr[r] + v[r];
          } else if (epi & A3V_EPI_RESIDUAL) {
            const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = bf2f(rr[r]) + v[r];
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = v[r];
      }
    }
  }
  // Phase 2 -- stores only (ragged tiles and the rarer output kinds: 8 bytes per lane straight from the accumulator layout)
  float gss = 0.f;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = mbase + i * 16 + mrow;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nbase + j * 16 + ncol;
      if (n >= p.N) continue;
      if (epi & GEMM_EPI_ROPEKV) {
        // q in place of the qkv row, k into the K cache, v transposed into the V^T cache (and token-major into v_rows)
        const RopeKvArgs& k = rk_;
        const int mg = m + k.m_off;
        const int b = mg / k.S, sq = mg - b * k.S;
        const int slot = n >> k.hd_shift, d = n & ((1 << k.hd_shift) - 1);
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(acc[i][j][r]);
        if (slot < k.H + k.Hkv) {
          bf16_t* dst = slot < k.H ? k.q_out + (int64_t)mg * k.ldq + n
                                   : k.k_cache + ((((int64_t)b * k.Hkv + (slot - k.H)) * k.Smax + k.start_pos + sq) << k.hd_shift) + d;
          *reinterpret_cast<bf16x4*>(dst) = o;
        } else {
          bf16_t* dst = k.vt_cache + ((((int64_t)b * k.Hkv + (slot - k.H - k.Hkv)) << k.hd_shift) + d) * k.Smax + k.start_pos + sq;
#pragma unroll
          for (int r = 0; r < 4; ++r) dst[(int64_t)r * k.Smax] = o[r];
          if (k.v_rows) *reinterpret_cast<bf16x4*>(k.v_rows + (int64_t)mg * k.ldv + (n - ((k.H + k.Hkv) << k.hd_shift))) = o;
        }
        continue;
      }
      if (epi & (A3V_EPI_RES_F32 | A3V_EPI_OUT_F32)) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = acc[i][j];
        if constexpr ((SET & EPI_SET_SUMSQ) != 0) {
          if (p.sumsq) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gss = fmaf(acc[i][j][r], acc[i][j][r], gss);
          }
        }
      } else {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(acc[i][j][r]);
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n) = o;
      }
    }
  }
  if constexpr ((SET & EPI_SET_SUMSQ) != 0) { if (p.sumsq) sumsq_flush(p, gss, mbase, nbase, lane); }
}

// TBM x TBN block tile, WAVES_M x WAVES_N waves, each wave (TBM/WAVES_M) x (TBN/WAVES_N).
template <int TBM, int TBN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_nt_bf16_kernel(GemmArgs p) {
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int WTM = TBM / WAVES_M, WTN = TBN / WAVES_N;   // wave tile
  constexpr int TM = WTM / 16, TN = WTN / 16;               // MFMA tiles per wave
  constexpr int STAGE = (TBM + TBN) * BK * 2;
  static_assert(TN % 2 == 0, "SwiGLU pairing needs an even number of 16-column tiles per wave");
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // ---- XCD-aware tile map (bijective for any grid size) ----
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int per_group = GROUP_M * p.tiles_n;
  const int group = bid / per_group;
  const int first_m = group * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int in_g = bid - group * per_group;
  const int tm = first_m + in_g % gsz;
  const int tn = in_g / gsz;
  const int m0 = tm * TBM, n0 = tn * TBN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // split-K: slice z of gridDim.y takes the k-tiles [z nk/S, (z+1) nk/S) and writes its own output plane (summed by
  // splitk_reduce_kernel); skinny problems (N or M = 64) otherwise run as a few blocks with a long serial K loop
  int nk = p.K / BK;
  if (gridDim.y > 1) {
    const int z = blockIdx.y, S = gridDim.y;
    const int t0 = (int)(((int64_t)z * nk) / S), t1 = (int)(((int64_t)(z + 1) * nk) / S);
    p.A += (int64_t)t0 * BK;
    p.W += (int64_t)t0 * BK;
    p.C = reinterpret_cast<char*>(p.C) + (int64_t)z * p.c_split;
    nk = t1 - t0;
  }
  if (nk > 0) {
    stage_tile<TBM, NW>(p.A, p.lda, m0, p.M - 1, 0, lds, wave, lane);
    stage_tile<TBN, NW>(p.W, p.ldw, n0, p.N - 1, 0, lds + TBM * BK * 2, wave, lane);
  }
  __syncthreads();

  const int frow = lane & 15;            // row inside a 16-row MFMA tile
  const int fsw = (lane >> 1) & 7;       // ((row>>1)&7) -- tile bases are multiples of 16
  const int fks = lane >> 4;             // k-slot 0..3 inside a K=32 slice
  for (int t = 0; t < nk; ++t) {
    char* cur = lds + (t & 1) * STAGE;
    if (t + 1 < nk) {
      char* nxt = lds + ((t + 1) & 1) * STAGE;
      stage_tile<TBM, NW>(p.A, p.lda, m0, p.M - 1, (t + 1) * BK, nxt, wave, lane);
      stage_tile<TBN, NW>(p.W, p.ldw, n0, p.N - 1, (t + 1) * BK, nxt + TBM * BK * 2, wave, lane);
    }
    const char* At = cur + (wm * WTM + frow) * 128;
    const char* Wt = cur + TBM * BK * 2 + (wn * WTN + frow) * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((kk * 4 + fks) ^ fsw) << 4;
      bf16x8 af[TM], wf[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(Wt + j * 16 * 128 + off);
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(At + i * 16 * 128 + off);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // the loop's last __syncthreads() is behind every read of the stage buffers: a private 4 KiB per wave for whole-row stores
  gemm_epilogue<TM, TN, false, (TM > 4 ? EPI_SET_COMMON : EPI_SET_COMMON | EPI_SET_PRE)>(acc, p, m0 + wm * WTM, n0 + wn * WTN, lane, nk > 0 ? lds + wave * 4096 : nullptr);
}

// Adapter-sized products (N <= 64: t = x A^T, dt = dy B) stream one long operand once; what bounds them is how many of its bytes
// the chip has outstanding, not MFMA.  The two-stage kernel above keeps ONE 8-KiB k-tile of the streamed operand in flight per
// block (548 blocks x 8 KiB = 4.4 MB over the chip: 3.6 TB/s measured at 8728 x 64 x 22016).  Same 64 x 64 tile, same fragment
// reads and MFMA order -- bit-identical planes -- with NST stages: NST - 1 k-tiles stay in flight across the block barrier
// (counted waits: 4 LDS-DMA instructions per thread and stage), one barrier per k-tile.
template <int N> __device__ __forceinline__ void vm_wait_imm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// TBM rows of the streamed operand per block (4 waves x TBM / 4 rows), NST stages of (TBM + 64) x 128 B.
template <int TBM, int NST>
__global__ __launch_bounds__(256) void gemm_nt_skinny_kernel(GemmArgs p) {
  constexpr int TBN = 64, NW = 4, TN = 4, TM = TBM / 64, WTM = TBM / 4;
  constexpr int STAGE = (TBM + TBN) * BK * 2;            // 16 / 24 / 40 KiB
  constexpr int PER = TBM / 32 + 2;                      // LDS-DMA instructions per thread and stage
  static_assert(PER * (NST - 2) <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(1024))) char lds_dyn[];
  char* const lds = lds_dyn;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * TBM;
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int nk = p.K / BK;
  {
    const int z = blockIdx.y, S = gridDim.y;
    const int t0 = (int)(((int64_t)z * nk) / S), t1 = (int)(((int64_t)(z + 1) * nk) / S);
    p.A += (int64_t)t0 * BK;
    p.W += (int64_t)t0 * BK;
    p.C = reinterpret_cast<char*>(p.C) + (int64_t)z * p.c_split;
    nk = t1 - t0;
  }
  auto stage = [&](int t) __attribute__((always_inline)) {
    char* dst = lds + (t % NST) * STAGE;
    stage_tile<TBM, NW>(p.A, p.lda, m0, p.M - 1, t * BK, dst, wave, lane);
    stage_tile<TBN, NW>(p.W, p.ldw, 0, p.N - 1, t * BK, dst + TBM * BK * 2, wave, lane);
  };
#pragma unroll
  for (int s = 0; s < NST - 1; ++s)
    if (s < nk) stage(s);
  const int frow = lane & 15, fsw = (lane >> 1) & 7, fks = lane >> 4;
  for (int t = 0; t < nk; ++t) {
    // k-tile t has landed when at most the pieces of the k-tiles issued after it are outstanding
    const int ahead = min(NST - 2, nk - 1 - t);
    if (ahead >= 3) vm_wait_imm<3 * PER>();
    else if (ahead == 2) vm_wait_imm<2 * PER>();
    else if (ahead == 1) vm_wait_imm<PER>();
    else vm_wait_imm<0>();
    // every wave's pieces of k-tile t are in, every wave is done with k-tile t - 1.  A bare s_barrier: __syncthreads() carries a fence
    // that hipcc lowers to vmcnt(0), i.e. it would drain the k-tiles this loop exists to keep in flight
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + NST - 1 < nk) stage(t + NST - 1);            // into the buffer of k-tile t - 1
    const char* cur = lds + (t % NST) * STAGE;
    const char* At = cur + (wave * WTM + frow) * 128;
    const char* Wt = cur + TBM * BK * 2 + frow * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((kk * 4 + fks) ^ fsw) << 4;
      bf16x8 af[TM], wf[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(Wt + j * 16 * 128 + off);
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(At + i * 16 * 128 + off);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the epilogue's 4-KiB patches lie over the stage buffers
  gemm_epilogue<TM, TN, false, EPI_SET_COMMON | EPI_SET_PRE>(acc, p, m0 + wave * WTM, 0, lane, nk > 0 ? lds + wave * 4096 : nullptr);
}

// ------------------------------------------------------------------------------------
// 256x256x64 "ping-pong" schedule (the ring kernel below and the two-stage TN / NN kernels): 8 waves =
// 2 groups of 4 (wr = wave/4 owns 128 rows of A; the waves w and w+4 share a SIMD).  Each group
// alternates a LOAD interval (24 ds_read_b128 for a whole K-tile of its 128x64 wave tile, + its share
// of the LDS-DMA for a later K-tile) and an MFMA interval (64 v_mfma_f32_16x16x32_bf16 from registers);
// the groups run ONE barrier apart, so on every SIMD one wave feeds the matrix pipe while its partner
// reads LDS / issues DMA.  With two whole-tile stages:
//
//   interval:   1      2      3      4      5      6
//   group 0:   L(0)   M(0)   L(1)   M(1)   L(2)   M(2) ...      L(t): reads buf[t&1]
//   group 1:    -     L(0)   M(0)   L(1)   M(1)   L(2) ...
//   DMA issue:               t=2           t=3           ...    tile t+2 -> buf[t&1]: by group 0 in
//   DMA wait :                      t=2           t=3    ...    L(t+1), by group 1 in M(t) (same interval:
//                                                                 the first one after BOTH groups read tile t)
// Ordering rules used (guide: "read a staged buffer one phase AFTER the wait that retires it"):
// every wave waits for its own DMA pieces, then the interval barrier publishes them; readers start
// one barrier later.  A wave retires its own ds_reads (lgkmcnt(0)) BEFORE the barrier that ends its
// LOAD interval, so a buffer is only re-staged after every read of it has returned.
#define A3V_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define A3V_WAIT_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define A3V_BARRIER()                      \
  do {                                     \
    asm volatile("" ::: "memory");         \
    __builtin_amdgcn_s_barrier();          \
    asm volatile("" ::: "memory");         \
  } while (0)

typedef __attribute__((ext_vector_type(4))) int i32x4r;
// ------------------------------------------------------------------------------------
// "Ring" form of the ping-pong schedule: the LDS is cut into three rings that together use all 160 KiB of the CU, so every
// LDS-DMA piece has THREE OR FOUR intervals (1.5 - 2 K-tile periods) to land instead of two.  (With two whole-tile stages a
// wave waits ~2600 cycles for a stage that it issued one K-tile period -- 2176 cycles of MFMA -- earlier: the k-loop runs at
// the DMA's completion latency, not at the matrix pipe's rate.)
//
//   A_top ring : rows   0..127 of the A tile (only group 0 reads them), 2 slots x 16 KiB   slot(t) = t & 1
//   A_bot ring : rows 128..255 of the A tile (only group 1 reads them), 2 slots x 16 KiB   slot(t) = t & 1
//   W ring     : the 256 W rows (both groups read them),                3 slots x 32 KiB   slot(t) = t % 3
//
//   interval I:   2t             2t+1            2t+2            2t+3
//   group 0:      L(t)           M(t)            L(t+1)          M(t+1)
//   group 1:      M(t-1)         L(t)            M(t)            L(t+1)
//   freed at the barrier that ENDS the interval:
//                 A_top(t)       A_bot(t), W(t)
//   issued in L (the wave's partner on the SIMD is in its MFMA interval), 8 pieces per wave per K-tile:
//     group 0 in L(t)  : A_bot(t+1) -> needed I = 2t+3 (3 intervals),   W rows 0..127 of tile t+2   -> needed I = 2t+4 (4)
//     group 1 in L(t)  : W rows 128..255 of tile t+2 and A_top(t+2)     -> needed I = 2t+4 (3 intervals)
//   counted waits (loads retire in order; a wave only ever waits for its OWN pieces, the barrier publishes them):
//     group 0, top of L(t): vmcnt(16) = its W half of tile t (issued in L(t-2)) has landed.  The late W wait (r03 A/B +1 % on
//                           every shape, bit-equal): here and not between the group's last MFMA of M(t-1) and the barrier that
//                           hands the matrix pipe over
//              end of L(t): vmcnt(12) = A_bot(t), the first 4 pieces of its previous burst, has landed (group 1 reads it next)
//     group 1, end of L(t): vmcnt(8)  = its previous burst (W half and A_top of tile t+1) has landed
//   The last two K-tiles of a block's last tile issue shorter bursts, so their counts shrink accordingly.
//
// The DMA stream runs on ACROSS the block's tiles (r03): the last two LOAD intervals of a tile fetch K-tiles 0 / 1 of the
// block's next tile into the ring slots they would have used anyway, so there is no prologue burst, no pipeline drain / refill
// and no block-wide barrier between tiles (see the boundary notes in the body).
//
// Template parameters:
//   SET  : which fast epilogue forms are compiled in (gemm_epilogue_fast).
//   TBM_ : 256, or 192 (round 5) = a 192 x 256 tile (six 16-row MFMA tiles per wave, 12-KiB A halves, 7 instead of 8 DMA pieces
//          per wave and LOAD interval): M = 8728 x N = 4096 is 2.875 rounds of these instead of 2.19 rounds of 256 x 256 -- the
//          rows beyond whole rounds cost no split-K planes.
//   F8   : (round 5) OCP e4m3fn operands (the W8A8 prefill).  A K-tile is still 128 BYTES per row -- 128 elements -- so rings,
//          DMA pieces, swizzle and fragment reads are the bf16 kernel's; the two 16-byte fragments of a lane feed ONE
//          v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales) instead of two 16x16x32 bf16 MFMAs, and the per-row scales
//          sa[m] sw[n] are applied to the accumulators in front of the SAME staged epilogues.
// ------------------------------------------------------------------------------------
template <int SET = EPI_SET_COMMON, int TBM_ = 256, bool F8 = false>
__global__ __launch_bounds__(512) void gemm_nt_bf16_ring_kernel(GemmArgs p) {
  static_assert(TBM_ == 256 || TBM_ == 192, "256- or 192-row tiles");
  constexpr int EB = F8 ? 1 : 2;                        // bytes per operand element
  constexpr int BKE = 128 / EB;                         // elements per K-tile (128 bytes per row either way)
  constexpr int TBM = TBM_, TBN = 256, WTM = TBM / 2, WTN = 64, TM = WTM / 16, TN = 4;
  constexpr int AH = WTM * BK * 2;                      // 16 KiB (12 KiB): one group's half of an A K-tile
  constexpr int APW = WTM / 32;                         // 1-KiB pieces (8 rows) of an A half per wave of a group: 4 (3)
  constexpr int BURST = APW + 4;                        // pieces per wave and LOAD interval: A half + W half
  constexpr int WT = TBN * BK * 2;                      // 32 KiB: a W K-tile
  constexpr int ATOP = 0, ABOT = 2 * AH, WB = 4 * AH;   // ring bases
  __shared__ __attribute__((aligned(1024))) char lds[4 * AH + 3 * WT];   // 163840 B = all of the CU's LDS (147456 B with 192-row tiles)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int ntiles = p.tiles_m * p.tiles_n;
  auto tile_of = [&](int vb, int& tm0, int& tn0) {
    int bid;
    const int G = (int)gridDim.x, full = ntiles / G, rnd = vb / G;
    if (p.xmap & 4) {
      // super-tile walk (host sets it when G == 256 and both tile counts are multiples of 16): a round is ONE 16 x 16 block of tiles
      // (32 operand panels from HBM instead of the 40 of an 8 x 32 strip), XCD x takes its 8 x 4 sub-block (still 12 panels per L2)
      const int x = vb & 7, i = (vb & 255) >> 3, nsc = p.tiles_n >> 4;
      tm0 = ((rnd / nsc) * 16 + (x >> 2) * 8 + (i & 7)) * TBM;
      tn0 = ((rnd % nsc) * 16 + (x & 3) * 4 + (i >> 3)) * TBN;
      return;
    }
    if (p.xmap && rnd < full) {
      // round-major: the eight XCDs work on the SAME run of G consecutive tiles (8 tile rows x G/8 columns), XCD x on columns
      // [x G/64, (x+1) G/64) of it -- the A panels of the row group are shared by all XCDs through the Infinity Cache instead of
      // every XCD streaming its own eight panels from HBM
      bid = rnd * G + (vb & 7) * (G >> 3) + ((vb - rnd * G) >> 3);
    } else {
      const int base = p.xmap ? full * G : 0, R = ntiles - base, v = vb - base;
      const int xcd = v & 7, q = R >> 3, r = R & 7;
      bid = base + (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (v >> 3);
    }
    const int per_group = GROUP_M * p.tiles_n;
    const int group = bid / per_group;
    const int first_m = group * GROUP_M;
    const int gsz = min(p.tiles_m - first_m, GROUP_M);
    const int in_g = bid - group * per_group;
    tm0 = (first_m + in_g % gsz) * TBM;
    const int tn = in_g / gsz;
    // xmap & 2: odd row groups walk the columns backwards, so a new group starts on the W panels the last one ended on (still in the
    // Infinity Cache) instead of on the ones evicted longest ago
    tn0 = (((p.xmap & 2) && (group & 1)) ? p.tiles_n - 1 - tn : tn) * TBN;
  };
  int m0, n0, sm0, sn0;     // tile being computed / tile being staged
  tile_of(blockIdx.x, m0, n0);
  sm0 = m0; sn0 = n0;
  f32x4 acc[TM][TN];

  // split-K (gridDim.y slices; the tail rows of the hybrid dispatch): slice z takes the k-tiles [z nk/S, (z+1) nk/S) and writes
  // its own raw fp32 plane (summed, rounded and finished by splitk_epilogue_kernel)
  if (gridDim.y > 1) {
    const int nk_all = p.K / BKE, z = blockIdx.y, S = gridDim.y;
    const int t0 = (int)(((int64_t)z * nk_all) / S), t1 = (int)(((int64_t)(z + 1) * nk_all) / S);
    p.A = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(p.A) + (int64_t)t0 * 128);
    p.W = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(p.W) + (int64_t)t0 * 128);
    p.K = (t1 - t0) * BKE;
    p.C = reinterpret_cast<char*>(p.C) + (int64_t)z * p.c_split;
  }
  const int nk = p.K / BKE;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)(((int64_t)(p.M - 1) * p.lda + p.K) * EB), 0x00020000);
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)(((int64_t)(p.N - 1) * p.ldw + p.K) * EB), 0x00020000);
  // per-lane byte offset inside an 8-row chunk: row = lane/8, 16-B slot = (lane%8) ^ ((chunk*4 + lane/16) & 7)
  const unsigned lr = lane >> 3;
  unsigned voA[2], voW[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const unsigned sl = (lane & 7) ^ ((par * 4 + (lane >> 4)) & 7);
    voA[par] = (unsigned)(lr * p.lda * EB + sl * 16);
    voW[par] = (unsigned)(lr * p.ldw * EB + sl * 16);
  }
  // one 1-KiB piece = 8 rows x 128 B; `row` = first row inside the A (W) tile, `par` = its chunk index & 1 (swizzle key)
  // (`tm0` / `tn0`: first row of the tile the K-tile belongs to -- the tile being computed, or, at the end of a k-loop, the block's next one)
  auto piece_a = [&](int tm0, int row, int t, int par, char* dst) {
    const unsigned so = (unsigned)((int64_t)(tm0 + row) * p.lda * EB + t * 128);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)dst, 16, voA[par] + so, 0, 0, 0);
  };
  auto piece_w = [&](int tn0, int row, int t, int par, char* dst) {
    const unsigned so = (unsigned)((int64_t)(tn0 + row) * p.ldw * EB + t * 128);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)dst, 16, voW[par] + so, 0, 0, 0);
  };
  // tile prologue (all 8 waves, 14 pieces each): K-tile 0 whole, A_top and W of K-tile 1
  auto prologue = [&]() {
#pragma unroll
    for (int c = 0; c < APW; ++c) {
      const int ch = (wave & 3) * APW + c;              // chunks of A(0): waves 0-3 -> A_top, waves 4-7 -> A_bot (chunk parity = swizzle key)
      piece_a(sm0, wr * WTM + ch * 8, 0, ch & 1, lds + (wr ? ABOT : ATOP) + ch * 1024);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) piece_w(sn0, (wave * 4 + c) * 8, 0, c & 1, lds + WB + (wave * 4 + c) * 1024);
    if (nk > 1) {
      if constexpr (TBM == 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) piece_a(sm0, (wave * 2 + c) * 8, 1, c & 1, lds + ATOP + AH + (wave * 2 + c) * 1024);
      } else {                                          // 12 chunks over 8 waves: waves 0-3 two each, waves 4-7 one each
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int ch = wave < 4 ? wave * 2 + c : 8 + (wave - 4);
          if (c == 0 || wave < 4) piece_a(sm0, ch * 8, 1, ch & 1, lds + ATOP + AH + ch * 1024);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) piece_w(sn0, (wave * 4 + c) * 8, 1, c & 1, lds + WB + WT + (wave * 4 + c) * 1024);
    }
  };
  prologue();

  // fragments: lane -> row (lane&15), 16-B slots (lane>>4) and 4 + (lane>>4) of the 64-k row (two MFMAs per tile): 24 ds_read_b128
  const int frow = lane & 15, fsw = (lane >> 1) & 7;
  constexpr int NKK = 2;
  int offk[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) offk[kk] = ((kk * 4 + (lane >> 4)) ^ fsw) << 4;
  const int a_base = frow * 128;                        // inside the group's own A ring slot
  const int w_base = (wc * WTN + frow) * 128;
  constexpr int TSTRIDE = 16 * 128;       // bytes between the row tiles of a fragment set
  bf16x8 af[NKK][TM], wf[NKK][TN];

#define RG_READ_FRAGS(aslot, wslot)                                                                  \
  do {                                                                                               \
    const char* At_ = (aslot) + a_base;                                                              \
    const char* Wt_ = (wslot) + w_base;                                                              \
    _Pragma("unroll") for (int kk = 0; kk < NKK; ++kk)                                               \
      _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
        wf[kk][j] = *reinterpret_cast<const bf16x8*>(Wt_ + j * TSTRIDE + offk[kk]);                  \
    _Pragma("unroll") for (int kk = 0; kk < NKK; ++kk)                                               \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                 \
        af[kk][i] = *reinterpret_cast<const bf16x8*>(At_ + i * TSTRIDE + offk[kk]);                  \
  } while (0)

#define RG_MFMA()                                                                          \
  do {                                                                                               \
    if constexpr (F8) {                                                                              \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                 \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                               \
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                              \
              __builtin_shufflevector(__builtin_bit_cast(i32x4r, wf[0][j]), __builtin_bit_cast(i32x4r, wf[1][j]), 0, 1, 2, 3, 4, 5, 6, 7), \
              __builtin_shufflevector(__builtin_bit_cast(i32x4r, af[0][i]), __builtin_bit_cast(i32x4r, af[1][i]), 0, 1, 2, 3, 4, 5, 6, 7), \
              acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);                                        \
    } else                                                                                           \
    _Pragma("unroll") for (int kk = 0; kk < NKK; ++kk)                                               \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                 \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                               \
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kk][j], af[kk][i], acc[i][j], 0, 0, 0); \
  } while (0)
#define RG_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

  const int g4 = wave & 3;
  // Tile boundaries (cont: the block has a next tile and nk >= 2).  The ping-pong keeps its two barriers per K-tile,
  //   X(t) = [group 0: end of L(t) | group 1: end of M(t-1)]      Y(t) = [group 0: end of M(t) | group 1: end of L(t)]
  // and the boundary only stretches the interval between Y(nk-1) and X(0') of the next tile:
  //   group 0:  ... M(nk-1) Y(nk-1) [store tile]          L(0') X(0') M(0') ...
  //   group 1:  ... L(nk-1) Y(nk-1) M(nk-1) [store tile]        X(0') L(0') ...
  // * the pieces of K-tiles 0' / 1' are issued by the LOAD intervals nk-2 / nk-1 exactly as those of t+1 / t+2 inside a tile (same
  //   slots, same counts: the A parity `pa` of K-tile 0 and the W slot `wcur` simply run on), so the counted waits stay the steady ones;
  // * the epilogue's staging patches live in the W slot of K-tile nk-1: every read of it is behind Y(nk-1), and it is the slot W(2')
  //   goes to -- each wave's pieces of W(2') land in that wave's OWN 4-KiB patch (rows 8 (4 g4 + c) .. of its group's half), issued
  //   after the wave's own epilogue, so no block-wide barrier is needed before the slot is reused;
  // * the stores of the epilogue count in vmcnt like the DMA pieces: one vmcnt(0) behind them (they were issued thousands of cycles
  //   after the last pieces) and the next k-loop's counted waits see DMA pieces only.
  // Without cont (nk == 1): prologue burst for the next tile before the epilogue, vmcnt(0) + block barrier at the k-loop entry.
  int wcur = 0, pa = 0;                                  // W ring slot / A parity of K-tile 0 of the current tile
  bool fresh = true;                                     // the tile's K-tiles 0 / 1 come from a prologue burst (first tile, or nk == 1)
  for (int vb = blockIdx.x;;) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{};
    const int nb = vb + (int)gridDim.x;
    const bool more = nb < ntiles;
    const bool cont = more && nk >= 2;                   // K-tiles nk, nk+1 of this k-loop are K-tiles 0, 1 of the block's next tile
    if (cont) tile_of(nb, sm0, sn0);                     // (sm0, sn0): the tile being staged = the next one from here on
    if (fresh) {
      A3V_WAIT_VM0();
      A3V_BARRIER();
      wcur = 0; pa = 0;
    }
    // The k-loop is split into its steady part (t + 2 < nk: every piece belongs to this tile, no condition, addresses advance by a
    // constant) and the last two iterations, which may stage the next tile (TAIL): with the selects in every iteration the LOAD
    // interval grew from ~900 to ~1140 cycles and the whole K-tile period with it (the two intervals are co-critical).
    if (wr == 0) {
      auto iter = [&](int t, auto tailc) {
        constexpr bool TAIL = decltype(tailc)::value;
        const int wn2 = wcur == 0 ? 2 : wcur - 1;        // slot of K-tile t + 2
        if (!TAIL || t + 1 < nk || cont) {
          const bool nx = TAIL && t + 1 >= nk;
          const int tm = nx ? sm0 : m0, tk = nx ? t + 1 - nk : t + 1;
#pragma unroll
          for (int c = 0; c < APW; ++c) piece_a(tm, WTM + (g4 * APW + c) * 8, tk, (g4 * APW + c) & 1, lds + ABOT + ((pa ^ (t + 1)) & 1) * AH + (g4 * APW + c) * 1024);
        }
        if (!TAIL || t + 2 < nk || cont) {
          const bool nx = TAIL && t + 2 >= nk;
          const int tn = nx ? sn0 : n0, tk = nx ? t + 2 - nk : t + 2;
#pragma unroll
          for (int c = 0; c < 4; ++c) piece_w(tn, (g4 * 4 + c) * 8, tk, c & 1, lds + WB + wn2 * WT + (g4 * 4 + c) * 1024);
        }
        // everything older than the bursts of L(t-1) and L(t) has landed: in particular this group's W half of tile t (the reads
        // below); in steady state 8 + 8 pieces may stay in flight, the last two tiles of the block's last k-loop issue shorter bursts
        if (!TAIL || t + 2 < nk || cont) vm_wait_imm<2 * BURST>();            // (16 with 256-row tiles)
        else if (t + 2 == nk) vm_wait_imm<BURST + APW>();                        // L(t-1): A + W, L(t): A only (12)
        else vm_wait_imm<APW>();                                                  // only A_bot(nk-1) of L(nk-2) may be in flight (4)
        RG_READ_FRAGS(lds + ATOP + ((pa ^ t) & 1) * AH, lds + WB + wcur * WT);
        A3V_WAIT_LGKM0();
        if (!TAIL || t + 2 < nk || cont) vm_wait_imm<BURST + 4>();                // this burst + the W half of the previous one (12)
        else if (t + 2 == nk) vm_wait_imm<APW + 4>();                            // this burst (A only) + the W half of L(t-1) (8)
        else RG_VMCNT(0);
        A3V_BARRIER();
        __builtin_amdgcn_s_setprio(1);
        RG_MFMA();
        __builtin_amdgcn_s_setprio(0);                 // never wait (vmcnt / barrier) at raised priority: measured -20 %
        A3V_BARRIER();
        wcur = wcur == 2 ? 0 : wcur + 1;
      };
      int t = 0;
      for (; t + 2 < nk; ++t) iter(t, std::false_type{});
      for (; t < nk; ++t) iter(t, std::true_type{});
      if (!cont) A3V_BARRIER();                          // (with cont the other group's matching barrier is X(0') of the next tile)
    } else {
      if (fresh) A3V_BARRIER();
      auto iter = [&](int t, auto tailc) {
        constexpr bool TAIL = decltype(tailc)::value;
        const int wn2 = wcur == 0 ? 2 : wcur - 1;
        if (!TAIL || t + 2 < nk || cont) {
          const bool nx = TAIL && t + 2 >= nk;
          const int tn = nx ? sn0 : n0, tm = nx ? sm0 : m0, tk = nx ? t + 2 - nk : t + 2;
#pragma unroll
          for (int c = 0; c < 4; ++c) piece_w(tn, 128 + (g4 * 4 + c) * 8, tk, c & 1, lds + WB + wn2 * WT + WT / 2 + (g4 * 4 + c) * 1024);
#pragma unroll
          for (int c = 0; c < APW; ++c) piece_a(tm, (g4 * APW + c) * 8, tk, (g4 * APW + c) & 1, lds + ATOP + ((pa ^ t) & 1) * AH + (g4 * APW + c) * 1024);
        }
        RG_READ_FRAGS(lds + ABOT + ((pa ^ t) & 1) * AH, lds + WB + wcur * WT);
        A3V_WAIT_LGKM0();
        if (!TAIL || t + 2 < nk || cont) vm_wait_imm<BURST>();                   // its previous burst (W half + A_top of tile t+1) has landed (8)
        else RG_VMCNT(0);
        A3V_BARRIER();
        __builtin_amdgcn_s_setprio(1);
        RG_MFMA();
        __builtin_amdgcn_s_setprio(0);                 // never wait (vmcnt / barrier) at raised priority: measured -20 %
        if (!TAIL || t + 1 < nk || !cont) A3V_BARRIER();          // X(t+1) (or the block barrier that ends a k-loop without cont); with cont X(0') follows the epilogue
        wcur = wcur == 2 ? 0 : wcur + 1;
      };
      int t = 0;
      for (; t + 2 < nk; ++t) iter(t, std::false_type{});
      for (; t < nk; ++t) iter(t, std::true_type{});
    }
    // every read of the rings is behind the last barrier.  No cont: stage the next tile now (prologue burst), store this one after.
    if (more && !cont) {
      tile_of(nb, sm0, sn0);
      prologue();
    }
    {
      int lane_e = lane;
      asm volatile("" : "+v"(lane_e));
      // staging patches: the W slot of K-tile nk - 1 (cont: the one slot no piece of the next tile is in flight to); the slot behind the
      // prologue's two otherwise
      const int wst = cont ? (wcur == 0 ? 2 : wcur - 1) : 2;
      if constexpr (F8) {
        // acc = sum_k qa[m][k] qw[n][k]: the product's value is that times sa[m] sw[n] (what the general epilogue's F8 form applies);
        // done here so that the staged forms run on fp8 tiles too (the host leaves GEMM_EPI_SCALE out of p.epi for this kernel)
        const int mr_ = m0 + wr * WTM + (lane_e & 15), nc_ = n0 + wc * WTN + (lane_e >> 4) * 4;
        f32x4 swv[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) swv[j] = nc_ + j * 16 < p.N ? *reinterpret_cast<const f32x4*>(p.sw + nc_ + j * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float sam = mr_ + i * 16 < p.M ? p.sa[mr_ + i * 16] : 0.f;
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] *= sam * swv[j][r];
        }
      }
      gemm_epilogue<TM, TN, false, SET>(acc, p, m0 + wr * WTM, n0 + wc * WTN, lane_e, lds + WB + wst * WT + wave * 4096);
    }
    if (!more) break;
    if (cont) {
      A3V_WAIT_LGKM0();                                  // the wave's own patch reads are done: its next pieces may land in the patch
      A3V_WAIT_VM0();                                    // stores (and every older piece) retired: the counted waits count pieces again
      if (wr == 1) A3V_BARRIER();                        // X(0')
      pa ^= nk & 1;
      fresh = false;
    } else {
      fresh = true;
    }
    vb = nb; m0 = sm0; n0 = sn0;
  }
#undef RG_VMCNT
#undef RG_READ_FRAGS
#undef RG_MFMA
}

// ------------------------------------------------------------------------------------
// fp8 (OCP e4m3fn) form of the 256x256 ping-pong kernel: A [M][K] and W [N][K] are fp8 bytes, one k-tile is 128 elements =
// the same 128-byte LDS rows, DMA pieces and swizzle as the bf16 kernel's 64-element tile, and the two 16-byte fragment reads
// of a lane (16-B chunks g and 4 + g of its row) feed ONE v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales) instead of
// two 16x16x32 bf16 MFMAs: the same cycles per k-tile for twice the k.  Which 32 of the 128 k a lane group holds does not
// matter as long as A and W agree (tools/ubench/mxfp8.hip).  Per-row dequantisation scales are applied in the epilogue.
// ------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
__global__ __launch_bounds__(512) void gemm_nt_fp8_pp_kernel(GemmArgs p) {
  constexpr int TBM = 256, TBN = 256, WTM = 128, WTN = 64, TM = 8, TN = 4, KT = 128;
  constexpr int STAGE = (TBM + TBN) * KT;   // 64 KiB
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int per_group = GROUP_M * p.tiles_n;
  const int group = bid / per_group;
  const int first_m = group * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int in_g = bid - group * per_group;
  const int tm = first_m + in_g % gsz;
  const int tn = in_g / gsz;
  const int m0 = tm * TBM, n0 = tn * TBN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // split-K (gridDim.y slices -> raw fp32 planes, the tail rows of the hybrid dispatch): this block's k-tile range [kt0, nk)
  const int nk_all = p.K / KT;
  const int kt0 = (int)((int64_t)nk_all * blockIdx.y / gridDim.y), nk = (int)((int64_t)nk_all * (blockIdx.y + 1) / gridDim.y);
  if (gridDim.y > 1) p.C = reinterpret_cast<char*>(p.C) + (int64_t)blockIdx.y * p.c_split;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)((int64_t)(p.M - 1) * p.lda + p.K), 0x00020000);
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)((int64_t)(p.N - 1) * p.ldw + p.K), 0x00020000);
  const unsigned lr = lane >> 3;
  unsigned voA[2], voW[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const unsigned sl = (lane & 7) ^ ((par * 4 + (lane >> 4)) & 7);
    voA[par] = (unsigned)(lr * p.lda + sl * 16);
    voW[par] = (unsigned)(lr * p.ldw + sl * 16);
  }
  auto stage = [&](int t) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int ch = wave * 4 + (c & 3);
      char* dst = lds + (t & 1) * STAGE + (c >= 4 ? TBM * KT : 0) + ch * 1024;
      if (c < 4) {
        const unsigned so = (unsigned)((int64_t)(m0 + ch * 8) * p.lda + t * KT);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)dst, 16, voA[c & 1] + so, 0, 0, 0);
      } else {
        const unsigned so = (unsigned)((int64_t)(n0 + ch * 8) * p.ldw + t * KT);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)dst, 16, voW[c & 1] + so, 0, 0, 0);
      }
    }
  };
  stage(kt0);
  if (nk > kt0 + 1) stage(kt0 + 1);
  A3V_WAIT_VM0();
  A3V_BARRIER();

  const int frow = lane & 15, fsw = (lane >> 1) & 7, fks = lane >> 4;
  const int off0 = ((0 * 4 + fks) ^ fsw) << 4, off1 = ((1 * 4 + fks) ^ fsw) << 4;
  const int a_base = (wr * WTM + frow) * 128;
  const int w_base = TBM * KT + (wc * WTN + frow) * 128;
  i32x4 alo[TM], ahi[TM], wlo[TN], whi[TN];
#define F8_READ_FRAGS(cur)                                                                           \
  do {                                                                                               \
    const char* At_ = (cur) + a_base;                                                                \
    const char* Wt_ = (cur) + w_base;                                                                \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                 \
      wlo[j] = *reinterpret_cast<const i32x4*>(Wt_ + j * 2048 + off0);                               \
      whi[j] = *reinterpret_cast<const i32x4*>(Wt_ + j * 2048 + off1);                               \
    }                                                                                                \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                 \
      alo[i] = *reinterpret_cast<const i32x4*>(At_ + i * 2048 + off0);                               \
      ahi[i] = *reinterpret_cast<const i32x4*>(At_ + i * 2048 + off1);                               \
    }                                                                                                \
  } while (0)
#define F8_MFMA_ALL()                                                                                \
  do {                                                                                               \
    __builtin_amdgcn_s_setprio(1);                                                                   \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                   \
      _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_shufflevector(wlo[j], whi[j], 0, 1, 2, 3, 4, 5, 6, 7), \
            __builtin_shufflevector(alo[i], ahi[i], 0, 1, 2, 3, 4, 5, 6, 7), acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);    \
    __builtin_amdgcn_s_setprio(0);                                                                   \
  } while (0)
  if (wr == 0) {
    for (int t = kt0; t < nk; ++t) {
      F8_READ_FRAGS(lds + (t & 1) * STAGE);
      if (t >= kt0 + 1 && t + 1 < nk) stage(t + 1);
      A3V_WAIT_LGKM0();
      A3V_BARRIER();
      F8_MFMA_ALL();
      A3V_WAIT_VM0();
      A3V_BARRIER();
    }
    A3V_BARRIER();
  } else {
    A3V_BARRIER();
    for (int t = kt0; t < nk; ++t) {
      F8_READ_FRAGS(lds + (t & 1) * STAGE);
      A3V_WAIT_LGKM0();
      A3V_WAIT_VM0();
      A3V_BARRIER();
      if (t + 2 < nk) stage(t + 2);
      F8_MFMA_ALL();
      A3V_BARRIER();
    }
  }
#undef F8_READ_FRAGS
#undef F8_MFMA_ALL
  gemm_epilogue<TM, TN, true>(acc, p, m0 + wr * WTM, n0 + wc * WTN, lane);
}

// ------------------------------------------------------------------------------------
// "TN" form of the 256x256 ping-pong kernel: C[M,N] = At^T . Wt with BOTH operands K-major, At [K][lda] (m contiguous)
// and Wt [K][ldw] (n contiguous) -- the weight-gradient product dW = dY^T . X on the activations as they sit in memory
// (token-major), without materialising dY^T and X^T.  A stage tile is [64 k][256 m] (512-B rows, LDS-DMA of two k-rows
// per instruction); MFMA fragments come from ds_read_b64_tr_b16 (gfx950 transpose read: the 16 lanes of a group pass the
// addresses of a 4 x 16 block -- lane i: row i>>2, columns 4 (i&3).. -- and lane c receives column c), two reads per
// 8-k operand.  The 32-B column chunks of a row are XOR-swizzled on the DMA source side with key(k) = (k>>3 & 3)*4 + (k & 3):
// the 16 k-rows one read instruction touches (k = 8g + 4jj + r over lane groups g and r = 0..3) get 16 different keys, and
// the 8 rows of either wave half 8 different keys mod 8 -- 512 B over all 64 banks twice, conflict-free.  K need not be
// a tile multiple: rows past K are out of the buffer descriptor's range and read as zero.
// ------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) short s16x4;
template <bool A_ROWS>
__global__ __launch_bounds__(512) void gemm_tn_bf16_pp_kernel(GemmArgs p) {
  constexpr int TBM = 256, TBN = 256, WTM = 128, WTN = 64, TM = 8, TN = 4;
  constexpr int STAGE = (TBM + TBN) * BK * 2;   // 64 KiB
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  if (p.xmap && bid < (nwg & ~255)) {
    // blocks are dispatched in index order, 256 (one per CU) at a time: within each such round XCD x takes the x-th run of 32
    // consecutive tiles, so all eight XCDs share the round's row-group panels through the Infinity Cache (see the ring kernel)
    bid = (bid & ~255) + (bid & 7) * 32 + ((bid & 255) >> 3);
  } else {
    const int base = p.xmap ? (nwg & ~255) : 0, R = nwg - base, v = bid - base;
    const int xcd = v & 7, q = R >> 3, r = R & 7;
    bid = base + (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (v >> 3);
  }
  const int per_group = GROUP_M * p.tiles_n;
  const int group = bid / per_group;
  const int first_m = group * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int in_g = bid - group * per_group;
  int tm = first_m + in_g % gsz;
  int tn = ((p.xmap & 2) && (group & 1)) ? p.tiles_n - 1 - in_g / gsz : in_g / gsz;   // serpentine over the row groups (see the ring kernel)
  if (p.xmap & 4) {                          // super-tile walk (see the ring kernel): 256 consecutive blocks = one 16 x 16 block of tiles
    const int b = blockIdx.x, rnd = b >> 8, x = b & 7, i = (b & 255) >> 3, nsc = p.tiles_n >> 4;
    tm = (rnd / nsc) * 16 + (x >> 2) * 8 + (i & 7);
    tn = (rnd % nsc) * 16 + (x & 3) * 4 + (i >> 3);
  }
  const int m0 = tm * TBM, n0 = tn * TBN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // split-K: gridDim.y slices of the k-tile range, slice z -> output plane z (raw fp32 partial sums, a3v_splitk_reduce adds them)
  const int nk_all = (p.K + BK - 1) / BK;
  const int kt0 = (int)((int64_t)nk_all * blockIdx.y / gridDim.y), nk = (int)((int64_t)nk_all * (blockIdx.y + 1) / gridDim.y);
  if (gridDim.y > 1) p.C = reinterpret_cast<char*>(p.C) + (int64_t)blockIdx.y * p.c_split;
  // waves whose 128 x 64 part of the tile lies outside C (adapter-sized M or N) keep the barriers but skip reads and MFMAs
  const bool active = (m0 + wr * WTM < p.M) && (n0 + wc * WTN < p.N);
  // A_ROWS ("NN" form, C = A . Wt): A is [M][K] row-major and takes the NT kernel's staging (8-row chunks of 128-B rows, 16-B slot
  // swizzle) and ds_read_b128 fragments; only Wt [K][N] goes through the transpose reads.  K % 64 == 0 there (host-checked).
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, A_ROWS ? (int)(((int64_t)(p.M - 1) * p.lda + p.K) * 2)
                                                                           : (int)(((int64_t)(p.K - 1) * p.lda + p.M) * 2), 0x00020000);
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)(((int64_t)(p.K - 1) * p.ldw + p.N) * 2), 0x00020000);
  // piece c of this wave: DMA instruction q = wave*4 + c of the tile (k-rows 2q, 2q+1); lane -> row 2q + (lane>>5),
  // 16-B position lane&31 of the 512-B row, which holds source chunk ((pos>>1) ^ key(k)) * 32 B + (pos&1) * 16 B
  unsigned voA[4], voW[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned kin = 2 * (wave * 4 + c) + (lane >> 5);
    const unsigned col = (((((unsigned)lane & 31) >> 1) ^ (((kin >> 3) & 3) * 4 + (kin & 3))) << 5) + (lane & 1) * 16;
    voA[c] = (unsigned)(kin * p.lda * 2) + col;
    voW[c] = (unsigned)(kin * p.ldw * 2) + col;
    if constexpr (A_ROWS) {   // row = lane/8 of the 8-row chunk, 16-B slot = (lane%8) ^ ((chunk*4 + lane/16) & 7); chunk parity = c & 1
      const unsigned sl = (lane & 7) ^ (((c & 1) * 4 + (lane >> 4)) & 7);
      voA[c] = (unsigned)(((lane >> 3) * p.lda + sl * 8) * 2);
    }
  }
  auto stage_piece = [&](int t, int c) {
    char* dst = lds + (t & 1) * STAGE + (c >= 4 ? TBM * BK * 2 : 0) + (wave * 4 + (c & 3)) * 1024;
    if (c < 4) {
      const unsigned so = A_ROWS ? (unsigned)(((int64_t)(m0 + (wave * 4 + c) * 8) * p.lda + t * BK) * 2)
                                 : (unsigned)(((int64_t)t * BK * p.lda + m0) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)dst, 16, voA[c & 3] + so, 0, 0, 0);
    } else {
      const unsigned so = (unsigned)(((int64_t)t * BK * p.ldw + n0) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)dst, 16, voW[c & 3] + so, 0, 0, 0);
    }
  };
  auto stage = [&](int t) {
#pragma unroll
    for (int c = 0; c < 8; ++c) stage_piece(t, c);
  };
  stage(kt0);
  if (nk > kt0 + 1) stage(kt0 + 1);
  A3V_WAIT_VM0();
  A3V_BARRIER();

  // fragment addressing: lane (g = lane>>4, il = lane&15); k sub-block (ks, jj): rows ks*32 + 8g + 4jj + (il>>2)
  const int fg = lane >> 4, il = lane & 15;
  int kro[2][2], kxo[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int k = ks * 32 + 8 * fg + 4 * jj + (il >> 2);
      kro[ks][jj] = k * 512 + (il & 3) * 8;
      kxo[ks][jj] = ((k >> 3) & 3) * 4 + (k & 3);
    }
  const int off0 = ((0 * 4 + fg) ^ ((lane >> 1) & 7)) << 4, off1 = ((1 * 4 + fg) ^ ((lane >> 1) & 7)) << 4;   // A_ROWS fragment slots
  const int a_base = (wr * WTM + il) * 128;
  bf16x8 af0[TM], af1[TM], wf0[TN], wf1[TN];
  auto tr8 = [&](const char* tile, int blk16, int ks) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(tile + kro[ks][0] + ((blk16 ^ kxo[ks][0]) << 5)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(tile + kro[ks][1] + ((blk16 ^ kxo[ks][1]) << 5)));
    bf16x8 r;
    const short v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    __builtin_memcpy(&r, v, 16);
    return r;
  };
#define TN_READ_FRAGS(cur)                                                                           \
  do {                                                                                               \
    const char* At_ = (cur);                                                                         \
    const char* Wt_ = (cur) + TBM * BK * 2;                                                          \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                 \
      wf0[j] = tr8(Wt_, wc * 4 + j, 0);                                                              \
      wf1[j] = tr8(Wt_, wc * 4 + j, 1);                                                              \
    }                                                                                                \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                 \
      if constexpr (A_ROWS) {                                                                        \
        af0[i] = *reinterpret_cast<const bf16x8*>(At_ + a_base + i * 2048 + off0);                   \
        af1[i] = *reinterpret_cast<const bf16x8*>(At_ + a_base + i * 2048 + off1);                   \
      } else {                                                                                       \
        af0[i] = tr8(At_, wr * 8 + i, 0);                                                            \
        af1[i] = tr8(At_, wr * 8 + i, 1);                                                            \
      }                                                                                              \
    }                                                                                                \
  } while (0)
#define TN_MFMA_ALL()                                                                                \
  do {                                                                                               \
    __builtin_amdgcn_s_setprio(1);                                                                   \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                   \
      _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[j], af0[i], acc[i][j], 0, 0, 0);     \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                   \
      _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[j], af1[i], acc[i][j], 0, 0, 0);     \
    __builtin_amdgcn_s_setprio(0);                                                                   \
  } while (0)
  if (wr == 0) {
    for (int t = kt0; t < nk; ++t) {
      if (active) TN_READ_FRAGS(lds + (t & 1) * STAGE);
      if (t >= kt0 + 1 && t + 1 < nk) stage(t + 1);
      A3V_WAIT_LGKM0();
      A3V_BARRIER();
      if (active) TN_MFMA_ALL();
      A3V_WAIT_VM0();
      A3V_BARRIER();
    }
    A3V_BARRIER();
  } else {
    A3V_BARRIER();
    for (int t = kt0; t < nk; ++t) {
      if (active) TN_READ_FRAGS(lds + (t & 1) * STAGE);
      A3V_WAIT_LGKM0();
      A3V_WAIT_VM0();
      A3V_BARRIER();
      if (t + 2 < nk) stage(t + 2);
      if (active) TN_MFMA_ALL();
      A3V_BARRIER();
    }
  }
#undef TN_READ_FRAGS
#undef TN_MFMA_ALL
  // every read of the stage buffers is behind the last barrier: each wave takes a private 4 KiB of them for the row-contiguous stores
  // (sums of squares only in the TN form: the NN form computes input gradients)
  if (active) gemm_epilogue<TM, TN, false, (A_ROWS ? EPI_SET_COMMON : EPI_SET_COMMON | EPI_SET_SUMSQ)>(acc, p, m0 + wr * WTM, n0 + wc * WTN, lane, lds + wave * 4096);
}

// A ring form of this kernel (A_top / A_bot / W rings over all 160 KiB as in gemm_nt_bf16_ring_kernel; for TN the A halves as
// [64 k][128 m] tiles with 256-B rows and key(k) & 7) was built and measured in round 2: bit-identical, but NN +1..3 % and TN -7..9 %
// against this two-stage form (gpurun_out/tn_ring_b.log) -- the transpose-read L interval, not the DMA flight time, paces these
// loops -- so it was not kept.  One finding worth keeping: with ds_read_tr builtins in the loop, hipcc orders every fragment read
// behind ALL outstanding LDS-DMA builtins (a compiler-inserted s_waitcnt vmcnt(0)); LDS-DMA that must stay in flight across
// transpose reads has to be issued from inline asm (s_mov_b32 m0 / buffer_load_dwordx4 ... offen lds).
// Same schedule with v_mfma_f32_32x32x16_bf16 (8-pass, higher sustained rate than 16x16x32):
// wave tile 128x64 = 4x2 tiles of 32x32, 4 k-steps of 16 per K-tile, 32 MFMAs per interval.

// ------------------------------------------------------------------------------------
// fp32 parity GEMM: 64(m) x 64(tile rows of W) x 16, 256 threads, 4x4 outputs per thread.
// A thread owns tile columns {2tx, 2tx+1, 32+2tx, 33+2tx}; with SWIGLU the tile's rows
// 0..31 are gate rows and 32..63 the matching up rows, so the pairing is thread-local.
// ------------------------------------------------------------------------------------
struct GemmF32Args {
  const float* A;
  const float* W;
  float* C;
  const float* bias;
  const float* res;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K, epi;
};

__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(GemmF32Args p) {
  __shared__ float As[16][64 + 4];
  __shared__ float Ws[16][64 + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const bool swi = (p.epi & A3V_EPI_SWIGLU) != 0;
  const int m0 = blockIdx.y * 64;
  const int c0 = blockIdx.x * (swi ? 32 : 64);  // first output column of the tile
  // loader mapping: thread -> (tile row lr, 4 consecutive k)
  const int lr = tid >> 2, lk = (tid & 3) * 4;
  int arow = m0 + lr;
  arow = arow < p.M ? arow : p.M - 1;
  int wrow;
  if (swi) {
    const int c = c0 + (lr & 31);
    wrow = (c >> 4) * 32 + (c & 15) + 16 * (lr >> 5);
  } else {
    wrow = c0 + lr;
  }
  wrow = wrow < p.N ? wrow : p.N - 1;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < p.K; k0 += 16) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p.A + (int64_t)arow * p.lda + k0 + lk);
    const f32x4 w = *reinterpret_cast<const f32x4*>(p.W + (int64_t)wrow * p.ldw + k0 + lk);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) { As[lk + e][lr] = a[e]; Ws[lk + e][lr] = w[e]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float av[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = As[k][ty * 4 + i];
      wv[0] = Ws[k][2 * tx]; wv[1] = Ws[k][2 * tx + 1];
      wv[2] = Ws[k][32 + 2 * tx]; wv[3] = Ws[k][33 + 2 * tx];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], wv[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= p.M) continue;
    if (swi) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = c0 + 2 * tx + j;
        if (c >= p.N / 2) continue;
        const float g = acc[i][j], u = acc[i][j + 2];
        p.C[(int64_t)m * p.ldc + c] = (g / (1.f + expf(-g))) * u;
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = c0 + (j < 2 ? 2 * tx + j : 32 + 2 * tx + (j - 2));
      if (n >= p.N) continue;
      float v = acc[i][j];
      if (p.epi & A3V_EPI_BIAS) v += p.bias[n];
      if (p.epi & A3V_EPI_GELU) v = gelu_erf(v);
      else if (p.epi & A3V_EPI_QUICKGELU) v = v / (1.f + expf(-1.702f * v));
      if (p.epi & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) v = p.res[(int64_t)m * p.ldr + n] + v;
      p.C[(int64_t)m * p.ldc + n] = v;
    }
  }
}

}  // namespace

extern "C" int a3v_version(void) { return 100; }

// environment switches: see A3V_ENV_INT (a3v_common.h)
static int g_env_generation = 0;
int a3v_env_generation() { return g_env_generation; }
extern "C" int a3v_reload_env(void) { return ++g_env_generation; }

// Optional scratch for the split-K forms of the hybrid dispatch (tail rows, few-tile problems): the library never allocates, so without
// it those rows run as plain launches.  Registrations are keyed by (device, stream): two streams that run GEMMs concurrently must not
// share split-K planes (round 3 kept ONE process-global pointer: a second stream, model or device raced through it silently).
//   a3v_gemm_set_workspace_for(stream, ptr, bytes)   the scratch of GEMM calls issued on `stream` of the current device
//   a3v_gemm_set_workspace(ptr, bytes)               legacy form: a scratch for callers that never name a stream; it is BOUND to the
//                                                    first (device, stream) that uses it -- any other stream without a registration
//                                                    of its own gets none (plain launches), never somebody else's planes
#include <mutex>
#include <vector>
namespace {
struct GemmWs { float* p; int64_t bytes; };
struct GemmWsEntry { int dev; hipStream_t st; float* p; int64_t bytes; };
std::mutex g_ws_mu;
std::vector<GemmWsEntry> g_ws_tab;
GemmWsEntry g_ws_legacy = {-1, nullptr, nullptr, 0};
bool g_ws_legacy_bound = false;
GemmWs gemm_ws_for(hipStream_t st) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g_ws_mu);
  for (const GemmWsEntry& e : g_ws_tab)
    if (e.dev == dev && e.st == st) return {e.p, e.bytes};
  if (g_ws_legacy.p) {
    if (!g_ws_legacy_bound) { g_ws_legacy.dev = dev; g_ws_legacy.st = st; g_ws_legacy_bound = true; }
    if (g_ws_legacy.dev == dev && g_ws_legacy.st == st) return {g_ws_legacy.p, g_ws_legacy.bytes};
  }
  return {nullptr, 0};
}
}  // namespace
extern "C" int a3v_gemm_set_workspace_for(void* stream, void* ptr, int64_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g_ws_mu);
  for (size_t i = 0; i < g_ws_tab.size(); ++i)
    if (g_ws_tab[i].dev == dev && g_ws_tab[i].st == (hipStream_t)stream) {
      if (ptr) { g_ws_tab[i].p = (float*)ptr; g_ws_tab[i].bytes = bytes; } else g_ws_tab.erase(g_ws_tab.begin() + i);
      return A3V_OK;
    }
  if (ptr) g_ws_tab.push_back({dev, (hipStream_t)stream, (float*)ptr, bytes});
  return A3V_OK;
}
extern "C" int a3v_gemm_set_workspace(void* ptr, int64_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  g_ws_legacy = {-1, nullptr, (float*)ptr, ptr ? bytes : 0};
  g_ws_legacy_bound = false;
  return A3V_OK;
}

namespace {
// sum of S raw fp32 planes [M][N] -> rounded once to bf16 ("the value F.linear returns") -> residual / output forms of gemm_epilogue
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const float* __restrict__ part, int S, int64_t plane, int M, int N, void* __restrict__ C,
                                                              int64_t ldc, const void* __restrict__ res, int64_t ldr, int epi,
                                                              const bf16_t* __restrict__ bias = nullptr, float* __restrict__ sumsq = nullptr) {
  const int64_t n4 = (int64_t)M * (N / 4);
  float ss = 0.f;                                        // sumsq: squares of the fp32 values this block stores -> slot blockIdx.x
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / (N / 4)), c = (int)(i % (N / 4)) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(part + (int64_t)s * plane + (int64_t)r * N + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += x[e];
    }
    if (bias) {
      const bf16x4 b4 = *reinterpret_cast<const bf16x4*>(bias + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += bf2f(b4[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = rbf(a[e]);
    if (epi & A3V_EPI_RES_F32) {
      const f32x4 rr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(res) + (int64_t)r * ldr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += rr[e];
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(C) + (int64_t)r * ldc + c) = a;
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(a[e], a[e], ss);
      continue;
    }
    if (epi & A3V_EPI_RESIDUAL) {
      const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(res) + (int64_t)r * ldr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += bf2f(rr[e]);
    }
    if (epi & A3V_EPI_OUT_F32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(C) + (int64_t)r * ldc + c) = a;
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(a[e], a[e], ss);
    } else {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(a[e]);
      *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(C) + (int64_t)r * ldc + c) = o;
    }
  }
  if (sumsq) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) sumsq[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}
}  // namespace

int a3v_cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v & ~7;
    if (n <= 0) n = 256;
  }
  return n;
}
static bool pp_persistent() { return A3V_ENV_INT("A3V_GEMM_PERSISTENT", 1) != 0; }   // 0: one block per tile (A/B runs)
static int nt_store_env() { return A3V_ENV_INT("A3V_GEMM_NT_STORE", 0); }
static int slow_epi_env() { return A3V_ENV_INT("A3V_GEMM_FAST_EPI", 1) == 0 ? 1 : 0; }   // 0: every tile through the general epilogue

// ------------------------------------------------------------------------------------
// GEMM dispatch: a pure function per family decides (the plan), one executor launches it.
//
// A plan is at most three steps: the tiles that run as one launch, the rows beyond whole rounds of the CUs ("tail") and, when the
// tail is split over K into raw fp32 planes, the reduce pass that sums the planes and applies the epilogue.  The plan functions take
// values only (no pointer, no HIP call; the A3V_* switches through A3V_ENV_INT, each at one call site); a3v_gemm_plan returns the
// same plan to a caller without a GPU, and profiles/gemm_dispatch_*.tsv + tests/test_gemm_plan_cpu.py pin it for the product shapes.
//
// Known, kept (each is today's behaviour; changing one is a behaviour change with its own measurement):
//  - NT cost model against NT launch: the hybrid tail is priced as a ring split when S >= 3, the epilogue is plain / residual / fp32
//    and a workspace is registered -- without the workspace-size check and without A3V_GEMM_TAIL_SLICES / A3V_GEMM_RING_TAIL.  The
//    launch applies all three, so it may run the 128 x 128 split-K tail or the plain 128 x 128 tail under a price it did not get.
//  - NT counts floor(M / 256) tile rows against rounds of 256 tiles; fp8 / TN / NN count ceil(M / 256) against rounds of the CU count.
//  - slice rules: slices_nt_ring (min(8, cus / tiles), K/64 >= 8 S, used only when S >= 3), slices_tn_nn (the same with >= 16 S, TN
//    on ceil(K/64), NN on K/64), slices_fp8 (powers of two, 2 S rem <= cus, K/128 >= 8 S), and the NT small-tile tail's own
//    slices_nt_small (powers of two up to 512 blocks, K/64 >= 16 S).  Their values differ for the same tail; they are not merged.
//  - xmap (ring kernels): 0 when grid_x & 63 and for every split launch (grid_y > 1); bit 2 cleared unless grid_x == 256 and both
//    tile counts are 16-aligned.  TN / NN read A3V_GEMM_XMAP_TN, also for the split tail, bit 2 on the tile counts alone.
//  - fp8: bias / GELU epilogues have no ring instantiation and take the two-stage kernel; the 192-row form is tried before the tail
//    form and without looking at the workspace, and when the ring kernel is off it falls through to the other forms.
//  - the reduce pass adds the bias only for the NT whole-problem ring split (no tail form accepts a bias epilogue); the TN reduce
//    pass writes its sumsq partials behind the tile slots, from slot ceil(M/256) * ceil(N/256) * 8.
// ------------------------------------------------------------------------------------
struct GemmStep { int32_t kernel, grid_x, grid_y, block, xmap, row0, rows, slices; };   // the A3V_GEMM_STEP_INTS fields of a3v_gemm_plan
static_assert(sizeof(GemmStep) == A3V_GEMM_STEP_INTS * sizeof(int32_t), "a3v_gemm_plan copies steps as int32 fields");
struct GemmPlan { int n; GemmStep step[A3V_GEMM_MAX_STEPS]; };
struct GemmShape {      // the value inputs of a plan
  int M, N, K;
  int64_t lda, ldw;
  int epilogue, dtype;  // the caller's epilogue word (A3V_EPI_TILE_* included)
  bool rope, bias_al8, sumsq, ws;   // fused rope / cache write; bias 8-byte aligned; sumsq requested (no decision reads it); a workspace is registered
  int64_t ws_bytes;
  int cus;
};
struct KernelShape { int tbm, tbn, block; };
static KernelShape kernel_shape(int kernel) {
  switch (kernel) {
    case A3V_GEMM_K_NT_128: return {128, 128, 256};
    case A3V_GEMM_K_RING_192: case A3V_GEMM_K_RING_PRE_192: case A3V_GEMM_K_RING_192_F8: return {192, 256, 512};
    case A3V_GEMM_K_F32: return {64, 64, 256};
    default: return {256, 256, 512};
  }
}
static void add_step(GemmPlan& pl, int kernel, int gx, int gy, int xmap, int row0, int rows, int slices) {
  pl.step[pl.n++] = GemmStep{kernel, gx, gy, kernel_shape(kernel).block, xmap, row0, rows, slices};
}
static int tiles_of(int kernel, int rows, int N) {
  const KernelShape k = kernel_shape(kernel);
  return ((rows + k.tbm - 1) / k.tbm) * ((N + k.tbn - 1) / k.tbn);
}
// rows [row0, row0 + rows) split S ways over K into fp32 planes on `kernel`, and the reduce pass over them
static void add_split(GemmPlan& pl, int kernel, int xmap, int S, int row0, int rows, int N) {
  add_step(pl, kernel, tiles_of(kernel, rows, N), S, xmap, row0, rows, S);
  const int64_t n4 = (int64_t)rows * (N / 4);
  pl.step[pl.n++] = GemmStep{A3V_GEMM_K_REDUCE, (int)std::min<int64_t>(2048, (n4 + 255) / 256), 1, 256, 0, row0, rows, S};
}

// tile rows (of `tiles_m`, each `tiles_n` tiles wide) that make whole rounds of `round` concurrent tiles, and what lies beyond them
struct Rounds { long mt_h, rem_tiles; int m_big; };
static Rounds whole_rounds(long tiles_m, long tiles_n, int round) {
  const long total = tiles_m * tiles_n;
  const long mt_h = (total / round) * round / tiles_n;
  return {mt_h, total - mt_h * tiles_n, (int)(mt_h * 256)};
}
// as many K-slices as fill the CUs once, at most 8, each at least 8 k-tiles long (the caller takes the split only for S >= 3)
static int slices_nt_ring(long tiles, int K, int cus) {
  int S = tiles > 0 ? (int)(cus / tiles) : 0;
  if (S > 8) S = 8;
  while (S > 1 && K / 64 < 8 * S) --S;
  return S;
}
// the NT tail on 128 x 128 tiles: powers of two while the blocks stay under one round of 512
static int slices_nt_small(int tblocks, int K) {
  int S = 1;
  while (tblocks * S < 512 && S < 8 && K / 64 >= 16 * S) S *= 2;
  return S;
}
// TN / NN: as slices_nt_ring with at least 16 k-tiles per slice (round 2: was the largest power of two with 2 S rem_tiles <= CUs, i.e.
// 96 blocks for the 48 tail tiles of a [8728, 4096] output; 5 slices = 240 blocks finish the tail in 1/5 of a tile time instead of 1/2)
static int slices_tn_nn(long rem_tiles, int ktiles, int cus) {
  int S = rem_tiles > 0 ? (int)std::min<long>(8, cus / rem_tiles) : 1;
  while (S > 1 && ktiles < 16 * S) --S;
  return S < 1 ? 1 : S;
}
// fp8: measured on wo / w2 of 7B: S = 2 (96 blocks) beat S = 8 (384 blocks)
static int slices_fp8(long rem_tiles, int K, int cus) {
  int S = 1;
  while (rem_tiles * S * 2 <= cus && S < 8 && (K / 128) >= 8 * S) S *= 2;
  return S;
}

// ring kernels: 1 = every round of gridDim.x tiles is cut into eight runs, one per XCD; =0: one contiguous run of tiles per XCD (A/B)
static int ring_xmap(int gx, int tiles_m, int tiles_n) {
  int xmap = (gx & 63) ? 0 : A3V_ENV_INT("A3V_GEMM_XMAP", 1);
  if (!((xmap & 4) && gx == 256 && (tiles_m & 15) == 0 && (tiles_n & 15) == 0)) xmap &= ~4;
  return xmap;
}
// TN / NN: =0: one contiguous run of tiles per XCD (A/B); 1: round-major; +2: serpentine; +4: 16 x 16 super-tiles where they fit
static int tn_xmap(int tiles_m, int tiles_n) {
  int xmap = A3V_ENV_INT("A3V_GEMM_XMAP_TN", 1);
  if (!((xmap & 4) && (tiles_m & 15) == 0 && (tiles_n & 15) == 0)) xmap &= ~4;
  return xmap;
}

// One NT launch of rows [row0, row0 + rows) on one tile form: 256x256 ping-pong ring (8 waves, 1 block/CU, persistent: one block per
// CU walks its tiles; A3V_GEMM_PERSISTENT=0: one block per tile), its 192 x 256 form (the fused-qkv form has no instantiation
// there), the plain 256 x 256 kernel or the 128x128 kernel (4 waves, 2 blocks/CU).  The ring kernel is instantiated per set of fast
// epilogue forms.
// `tile`: A3V_GEMM_K_NT_128, _NT_256, _RING or _RING_192; the ring forms are refined by the epilogue here.
static void add_nt(GemmPlan& pl, int tile, int epi, bool rope, int row0, int rows, int N, int cus) {
  if (tile == A3V_GEMM_K_NT_128 || tile == A3V_GEMM_K_NT_256) {
    add_step(pl, tile, tiles_of(tile, rows, N), 1, 0, row0, rows, 1);
    return;
  }
  const bool pre = (epi & (A3V_EPI_BIAS | A3V_EPI_GELU | A3V_EPI_QUICKGELU)) != 0;
  const int k = tile == A3V_GEMM_K_RING_192 ? (pre ? A3V_GEMM_K_RING_PRE_192 : A3V_GEMM_K_RING_192)
                : rope              ? A3V_GEMM_K_RING_ROPE
                                    : (pre ? A3V_GEMM_K_RING_PRE : A3V_GEMM_K_RING);
  const KernelShape ks = kernel_shape(k);
  const int tiles_m = (rows + ks.tbm - 1) / ks.tbm, tiles_n = (N + 255) / 256, nt = tiles_m * tiles_n;
  const int gx = pp_persistent() ? std::min(nt, cus) : nt;
  add_step(pl, k, gx, 1, ring_xmap(gx, tiles_m, tiles_n), row0, rows, 1);
}

// a3v_gemm_nt / a3v_gemm_qkv_rope
static int plan_nt(const GemmShape& s, GemmPlan& pl) {
  const int M = s.M, N = s.N, K = s.K, cus = s.cus, epi = s.epilogue & 0xffff;
  if (s.dtype == A3V_F32) {
    const int ncols = (epi & A3V_EPI_SWIGLU) ? N / 2 : N;
    const int tile_c = (epi & A3V_EPI_SWIGLU) ? 32 : 64;
    add_step(pl, A3V_GEMM_K_F32, (ncols + tile_c - 1) / tile_c, (M + 63) / 64, 0, 0, M, 1);
    return A3V_OK;
  }
  if (s.dtype != A3V_BF16) return A3V_ERR_DTYPE;
  const int64_t bytesA = ((int64_t)(M - 1) * s.lda + K) * 2, bytesW = ((int64_t)(N - 1) * s.ldw + K) * 2;
  const bool desc_ok = bytesA < (1LL << 31) && bytesW < (1LL << 31);   // buffer descriptors: 32-bit offsets
  // A3V_EPI_TILE_* force one configuration for the whole problem (tuning / tests)
  if (s.epilogue & (A3V_EPI_TILE_256PP | A3V_EPI_TILE_256 | A3V_EPI_TILE_128 | A3V_EPI_TILE_192PP)) {
    const int tile = (s.epilogue & A3V_EPI_TILE_192PP) ? A3V_GEMM_K_RING_192 : (s.epilogue & A3V_EPI_TILE_256PP) ? A3V_GEMM_K_RING
                     : (s.epilogue & A3V_EPI_TILE_256) ? A3V_GEMM_K_NT_256 : A3V_GEMM_K_NT_128;
    if (tile >= A3V_GEMM_K_RING && !desc_ok) return A3V_ERR_SHAPE;
    add_nt(pl, tile, epi, s.rope, 0, M, N, cus);
    return A3V_OK;
  }
  // Cost model in units of one 256x256 tile's time on one CU (T256): a "round" is 256 concurrent big tiles or
  // 512 concurrent 128x128 tiles (2 blocks/CU, each ~0.65 T256 at the small kernel's lower rate); a second launch
  // costs ~0.1.  Candidates: small kernel for everything, big kernel for everything, or big kernel on the M-tile rows
  // that fill whole rounds + small kernel on the remaining rows.
  const long tn256 = (N + 255) / 256, tn128 = (N + 127) / 128;
  const bool eligible = desc_ok && M >= 512 && N >= 512;
  const int simple = A3V_EPI_RESIDUAL | A3V_EPI_RES_F32 | A3V_EPI_OUT_F32;
  // (round 2 recalibration, tools/hybrid_vs_ring.py: with the ring kernel at 1.35-1.45 PF and the small kernel at ~0.6 PF a round
  // of 512 small tiles costs ~1.15 T256, and a split-K tail adds its reduce pass: the 7B qkv shape (6.56 rounds) went to the
  // hybrid under the old 0.65 and lost 11 % to the all-ring launch)
  auto small_cost = [&](long rows) { return rows <= 0 ? 0.0 : 1.15 * std::max(0.5, (double)((rows + 127) / 128) * tn128 / 512.0); };
  const double round_us = 12.0 + 0.0206 * K;          // one round of 256 tiles of 256 x 256 on the ring kernel (M = 8192, N = 4096: 98 us at K = 4096, 476 at 22016)
  const double c_small = small_cost(M);
  const double c_big = eligible ? (double)((((long)(M + 255) / 256) * tn256 + 255) / 256) : 1e30;
  const Rounds r = whole_rounds(M / 256, tn256, 256);
  double c_hyb = 1e30;
  if (eligible && r.mt_h >= 1 && r.m_big < M) {
    // tail rows: on the ring kernel split over K when that fills the CUs (1/S of a tile time + the reduce pass), else small tiles
    const long tail_rows = M - r.m_big;
    const int S2 = slices_nt_ring(((tail_rows + 255) / 256) * tn256, K, cus);
    const bool simple_epi = !(epi & ~simple) && !s.rope && s.ws && N % 4 == 0;
    // (round 5 recalibration, tools/ring192_ab.py) the split-K tail costs its 1 / S of a tile time plus ~32 us that do not depend on K
    // (plane traffic + two launches): 0.30 of a round at K = 4096, 0.07 at K = 22016, where a round of 256 tiles takes ~12 + 0.0206 K us
    const double tail = (S2 >= 3 && simple_epi && pp_persistent()) ? 1.0 / S2 + 32.0 / round_us : small_cost(tail_rows) + 0.25;
    c_hyb = (double)((r.mt_h * tn256 + 255) / 256) + tail;
  }
  // (round 5) the whole problem on 192 x 256 ring tiles: a round of them takes 0.79 of a 256 x 256 round (48 instead of 64 MFMAs per
  // wave and K-tile on 7 / 8 of the LDS-DMA pieces); 8728 x 4096 is 2.875 rounds of these against 2 rounds + a split-K tail
  double c_192 = 1e30;
  if (eligible && !s.rope && pp_persistent() && A3V_ENV_INT("A3V_GEMM_RING_192", 1) != 0 && !(epi & A3V_EPI_SWIGLU))
    c_192 = 0.79 * (double)((((long)(M + 191) / 192) * tn256 + 255) / 256) + 0.02;
  // few big tiles (small N or M: the ViT's output projections, 76 tiles): the whole problem on the ring kernel split over K
  double c_spl = 1e30;
  const int S3 = slices_nt_ring(((long)(M + 255) / 256) * tn256, K, cus);
  if (A3V_ENV_INT("A3V_GEMM_RING_SPLIT", 1) != 0 && eligible && S3 >= 3 && !(epi & ~(A3V_EPI_BIAS | simple)) && !s.rope && pp_persistent() && s.ws &&
      N % 4 == 0 && (int64_t)S3 * M * N * 4 <= s.ws_bytes && (!(epi & A3V_EPI_BIAS) || s.bias_al8))
    c_spl = 1.0 / S3 + 0.2;
  if (c_192 < c_spl && c_192 < c_small && c_192 < c_big && c_192 < c_hyb) {
    add_nt(pl, A3V_GEMM_K_RING_192, epi, s.rope, 0, M, N, cus);
  } else if (c_spl < c_small && c_spl < c_big && c_spl < c_hyb) {
    add_split(pl, A3V_GEMM_K_RING, 0, S3, 0, M, N);
  } else if (c_big <= c_small && c_big <= c_hyb) {
    add_nt(pl, A3V_GEMM_K_RING, epi, s.rope, 0, M, N, cus);
  } else if (c_hyb < c_small) {
    add_nt(pl, A3V_GEMM_K_RING, epi, s.rope, 0, r.m_big, N, cus);
    // tail rows: a few hundred rows x N on 128x128 tiles = ~160 blocks with a serial K loop (50 us at K = 4096, 135 us at
    // K = 11008).  With a registered workspace the K loop is split into S planes (more blocks, 1/S the latency) and a
    // reduce pass applies the epilogue; only the plain / residual / fp32 forms are handled there.
    const int rows = M - r.m_big;
    const int S = slices_nt_small(tiles_of(A3V_GEMM_K_NT_128, rows, N), K);
    // (round 2) the same tail on the ring kernel: its ceil(rows / 256) x tn256 big tiles split S ways over K so that they fill the
    // CUs once -- a fraction 1/S of a tile time instead of ~0.6 on the small kernel (wo: 257 -> ~235 us)
    int S2 = slices_nt_ring(tiles_of(A3V_GEMM_K_RING, rows, N), K, cus);
    { const int e = A3V_ENV_INT("A3V_GEMM_TAIL_SLICES", 0); if (e >= 3 && e <= 16 && K / 64 >= 2 * e) S2 = e; }      // sweeps (tools/tail_cost.py)
    const bool ring_tail = A3V_ENV_INT("A3V_GEMM_RING_TAIL", 1) != 0;
    const bool can_split = !(epi & ~simple) && !s.rope && s.ws && N % 4 == 0;
    if (ring_tail && pp_persistent() && S2 >= 3 && can_split && (int64_t)S2 * rows * N * 4 <= s.ws_bytes) {
      add_split(pl, A3V_GEMM_K_RING, 0, S2, r.m_big, rows, N);
    } else if (S > 1 && can_split && (int64_t)S * rows * N * 4 <= s.ws_bytes) {
      add_split(pl, A3V_GEMM_K_NT_128, 0, S, r.m_big, rows, N);
    } else {
      add_nt(pl, A3V_GEMM_K_NT_128, epi, s.rope, r.m_big, rows, N, cus);
    }
  } else {
    add_nt(pl, A3V_GEMM_K_NT_128, epi, s.rope, 0, M, N, cus);
  }
  return A3V_OK;
}

// a3v_gemm_tn / a3v_gemm_tn_sumsq (nn = false) and a3v_gemm_nn (nn = true): 256 x 256 tiles.  Rows of C beyond whole tile rounds (e.g.
// dW of w1|w3: 86 x 16 tiles = 5.4 rounds) are split over the contracted index into fp32 planes + the reduce epilogue (needs the
// registered workspace; otherwise one plain launch).
static int plan_tn_nn(const GemmShape& s, bool nn, GemmPlan& pl) {
  const int M = s.M, N = s.N, cus = s.cus, k = nn ? A3V_GEMM_K_NN : A3V_GEMM_K_TN;
  const int tiles_n = (N + 255) / 256, tm_all = (M + 255) / 256;
  const Rounds r = whole_rounds(tm_all, tiles_n, cus);
  const int S = slices_tn_nn(r.rem_tiles, nn ? s.K / 64 : (s.K + 63) / 64, cus);
  const bool tail_on = nn ? s.epilogue != A3V_EPI_SWIGLU_BWD : A3V_ENV_INT("A3V_TN_TAIL", 1) != 0;
  const int rows = M - r.m_big;
  if (tail_on && r.mt_h >= 1 && r.m_big < M && S > 1 && r.rem_tiles * 4 < 3 * cus && s.ws && (int64_t)S * rows * N * 4 <= s.ws_bytes) {
    add_step(pl, k, (int)r.mt_h * tiles_n, 1, tn_xmap((int)r.mt_h, tiles_n), 0, r.m_big, 1);
    add_split(pl, k, tn_xmap((rows + 255) / 256, tiles_n), S, r.m_big, rows, N);
  } else {
    add_step(pl, k, tm_all * tiles_n, 1, tn_xmap(tm_all, tiles_n), 0, M, 1);
  }
  return A3V_OK;
}

// a3v_gemm_nt_fp8 / a3v_gemm_qkv_rope_fp8.  (round 5) the fp8 product runs on the ring kernel: persistent tile walk, three LDS rings,
// staged epilogues; bias / activation kinds keep the two-stage kernel (no fp8 instantiation of that epilogue set).
// A3V_GEMM_FP8_RING=0: the two-stage kernel for everything (A/B runs, equality tests).
static int plan_nt_fp8(const GemmShape& s, GemmPlan& pl) {
  const int M = s.M, N = s.N, K = s.K, cus = s.cus, epi = s.epilogue;
  const bool ring_on = A3V_ENV_INT("A3V_GEMM_FP8_RING", 1) != 0 && pp_persistent();
  // one launch of rows [row0, row0 + rows) on the ring kernel (one block per CU), or on the two-stage kernel (one block per tile)
  auto add_fp8 = [&](int ring_kernel, int row0, int rows) {
    const bool ring = ring_on && !(epi & (A3V_EPI_BIAS | A3V_EPI_GELU | A3V_EPI_QUICKGELU));
    const int k = ring ? ring_kernel : A3V_GEMM_K_FP8_PP;
    const KernelShape ks = kernel_shape(k);
    const int tiles_m = (rows + ks.tbm - 1) / ks.tbm, tiles_n = (N + 255) / 256, nt = tiles_m * tiles_n;
    const int gx = ring ? std::min(nt, cus) : nt;
    add_step(pl, k, gx, 1, ring ? ring_xmap(gx, tiles_m, tiles_n) : 0, row0, rows, 1);
  };
  // when the last round would be mostly empty (e.g. 35 x 16 = 560 tiles on 256 CUs: a third round at 19 %), the rows beyond whole rounds
  // are split over K -- S times the blocks at 1/S the length (needs the registered workspace; otherwise one plain launch)
  const int tiles_n = (N + 255) / 256;
  const Rounds r = whole_rounds((M + 255) / 256, tiles_n, cus);
  const long total = (long)((M + 255) / 256) * tiles_n;
  const int S = slices_fp8(r.rem_tiles, K, cus);
  const int simple = A3V_EPI_RESIDUAL | A3V_EPI_RES_F32 | A3V_EPI_OUT_F32;
  const bool tail_form = !s.rope && !(epi & ~simple) && r.mt_h >= 1 && r.m_big < M && S > 1 && r.rem_tiles * 4 < 3 * cus;
  // (round 5) 192 x 256 ring tiles where they cost fewer rounds than whole 256-row rounds + a split-K tail (a round of them is 0.79 of a
  // 256-row round; the tail's ~32 us do not shrink with the fp8 round time ~12 + 0.0103 K us): A3V_GEMM_FP8_192 = 0 never, 2 always
  const int e192 = A3V_ENV_INT("A3V_GEMM_FP8_192", 1);
  const double round_us = 12.0 + 0.0103 * K;
  const double c_now = tail_form ? (double)(r.mt_h * tiles_n / cus) + 1.0 / S + 32.0 / round_us : (double)((total + cus - 1) / cus);
  const long t192 = (long)((M + 191) / 192) * tiles_n;
  const double c_192 = 0.79 * (double)((t192 + cus - 1) / cus) + 0.02;
  if (e192 && !s.rope && !(epi & (A3V_EPI_SWIGLU | A3V_EPI_BIAS | A3V_EPI_GELU | A3V_EPI_QUICKGELU)) && M >= 512 && N >= 512 &&
      (e192 == 2 || c_192 < c_now) && ring_on) {
    add_fp8(A3V_GEMM_K_RING_192_F8, 0, M);
    return A3V_OK;
  }
  const int rows = M - r.m_big;
  if (tail_form && s.ws && (int64_t)S * rows * N * 4 <= s.ws_bytes) {
    add_fp8(A3V_GEMM_K_RING_F8, 0, r.m_big);
    add_split(pl, ring_on ? A3V_GEMM_K_RING_F8 : A3V_GEMM_K_FP8_PP, 0, S, r.m_big, rows, N);
  } else {
    add_fp8(s.rope ? A3V_GEMM_K_RING_ROPE_F8 : A3V_GEMM_K_RING_F8, 0, M);
  }
  return A3V_OK;
}

static int gemm_plan(int family, const GemmShape& s, GemmPlan& pl) {
  pl.n = 0;
  return family == A3V_GEMM_NT ? plan_nt(s, pl) : family == A3V_GEMM_NT_FP8 ? plan_nt_fp8(s, pl)
         : family == A3V_GEMM_TN || family == A3V_GEMM_NN ? plan_tn_nn(s, family == A3V_GEMM_NN, pl) : A3V_ERR_ARG;
}

extern "C" int a3v_gemm_plan(int family, int M, int N, int K, int64_t lda, int64_t ldw, int epilogue, int dtype, int rope,
                             int bias_aligned, int sumsq, int64_t workspace_bytes, int cus, int32_t* steps) {
  if (M <= 0 || N <= 0 || K <= 0 || cus <= 0 || !steps) return A3V_ERR_ARG;
  const GemmShape s{M, N, K, lda, ldw, epilogue, dtype, rope != 0, bias_aligned != 0, sumsq != 0, workspace_bytes > 0, workspace_bytes, cus};
  GemmPlan pl;
  const int rc = gemm_plan(family, s, pl);
  if (rc != A3V_OK) return rc;
  memcpy(steps, pl.step, sizeof(GemmStep) * pl.n);
  return pl.n;
}

// ---- the executor: the only code that fills GemmArgs for, and launches, the kernels of a plan ----
static GemmArgs gemm_args(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, const void* res, int64_t ldr,
                          int M, int N, int K, int epi) {
  GemmArgs p{};
  p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.C = C; p.res = res;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr;
  p.M = M; p.N = N; p.K = K; p.epi = epi;
  return p;
}

// rows [row0, row0 + rows) of the problem `p` as a problem of its own
static GemmArgs gemm_rows(const GemmArgs& p, int family, int row0, int rows) {
  GemmArgs q = p;
  q.M = rows;
  // A: rows of lda bf16 (NT, NN) or of lda bytes (fp8); TN's At is [K][lda] with the C-row index contiguous: columns row0.. of At
  const int64_t a_bytes = family == A3V_GEMM_TN ? (int64_t)row0 * 2 : (int64_t)row0 * p.lda * (family == A3V_GEMM_NT_FP8 ? 1 : 2);
  q.A = (const bf16_t*)((const char*)p.A + a_bytes);
  if (p.sa) q.sa = p.sa + row0;
  q.rk.m_off = p.rk.m_off + row0;
  const int esz = (p.epi & (A3V_EPI_OUT_F32 | A3V_EPI_RES_F32)) ? 4 : 2;
  q.C = (char*)p.C + (int64_t)row0 * p.ldc * esz;
  if (p.res) q.res = (const char*)p.res + (int64_t)row0 * p.ldr * ((p.epi & A3V_EPI_RES_F32) ? 4 : 2);
  return q;
}

static void launch_step(const GemmStep& s, GemmArgs q, hipStream_t st) {
  const KernelShape ks = kernel_shape(s.kernel);
  const dim3 g(s.grid_x, s.grid_y), b(s.block);
  q.tiles_m = (q.M + ks.tbm - 1) / ks.tbm; q.tiles_n = (q.N + ks.tbn - 1) / ks.tbn;
  q.xmap = s.xmap;
  if (s.kernel != A3V_GEMM_K_FP8_PP) { q.slow_epi = slow_epi_env(); q.nt_store = nt_store_env(); }
  switch (s.kernel) {
    case A3V_GEMM_K_NT_128: hipLaunchKernelGGL((gemm_nt_bf16_kernel<128, 128, 2, 2>), g, b, 0, st, q); break;
    case A3V_GEMM_K_NT_256: hipLaunchKernelGGL((gemm_nt_bf16_kernel<256, 256, 2, 4>), g, b, 0, st, q); break;
    case A3V_GEMM_K_RING: hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON>), g, b, 0, st, q); break;
    case A3V_GEMM_K_RING_PRE: hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON | EPI_SET_PRE>), g, b, 0, st, q); break;
    case A3V_GEMM_K_RING_ROPE: hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_ROPE>), g, b, 0, st, q); break;
    case A3V_GEMM_K_RING_192: hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON, 192>), g, b, 0, st, q); break;
    case A3V_GEMM_K_RING_PRE_192: hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON | EPI_SET_PRE, 192>), g, b, 0, st, q); break;
    case A3V_GEMM_K_TN: hipLaunchKernelGGL(gemm_tn_bf16_pp_kernel<false>, g, b, 0, st, q); break;
    case A3V_GEMM_K_NN: hipLaunchKernelGGL(gemm_tn_bf16_pp_kernel<true>, g, b, 0, st, q); break;
    case A3V_GEMM_K_FP8_PP: hipLaunchKernelGGL(gemm_nt_fp8_pp_kernel, g, b, 0, st, q); break;
    case A3V_GEMM_K_F32: {
      GemmF32Args f{(const float*)q.A, (const float*)q.W, (float*)q.C, (const float*)q.bias, (const float*)q.res,
                    q.lda, q.ldw, q.ldc, q.ldr, q.M, q.N, q.K, q.epi};
      hipLaunchKernelGGL(gemm_nt_f32_kernel, g, b, 0, st, f);
      break;
    }
    default:      // the fp8 ring kernel scales its accumulators itself, in front of the staged epilogues
      q.epi &= ~GEMM_EPI_SCALE;
      if (s.kernel == A3V_GEMM_K_RING_192_F8) hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON, 192, true>), g, b, 0, st, q);
      else if (s.kernel == A3V_GEMM_K_RING_ROPE_F8) hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_ROPE, 256, true>), g, b, 0, st, q);
      else hipLaunchKernelGGL((gemm_nt_bf16_ring_kernel<EPI_SET_COMMON, 256, true>), g, b, 0, st, q);
  }
}

// The split-K tail of every family: `tail.slices` slices of the K loop of the rows `q` (of the whole problem `p`) write raw fp32
// planes into the workspace; one reduce pass sums them in order and applies the epilogue (the bias, if any, there) on the way to
// q's output.
static void launch_split(const GemmStep& tail, const GemmStep& reduce, const GemmArgs& p, const GemmArgs& q, float* ws, hipStream_t st) {
  GemmArgs t = q;
  t.C = ws; t.ldc = q.N; t.res = nullptr; t.bias = nullptr; t.sumsq = nullptr;
  t.epi = A3V_EPI_OUT_F32 | GEMM_EPI_RAW | (q.epi & GEMM_EPI_SCALE);
  t.c_split = (int64_t)q.M * q.N * 4;
  launch_step(tail, t, st);
  const int64_t tile_slots = (int64_t)((p.M + 255) / 256) * ((p.N + 255) / 256) * 8;   // a3v_gemm_tn_sumsq_slots: the reduce blocks' slots follow
  hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(reduce.grid_x), dim3(reduce.block), 0, st, ws, reduce.slices, (int64_t)q.M * q.N, q.M, q.N,
                     q.C, q.ldc, q.res, q.ldr, q.epi & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32 | A3V_EPI_OUT_F32),
                     (q.epi & A3V_EPI_BIAS) ? (const bf16_t*)q.bias : nullptr, q.sumsq ? q.sumsq + tile_slots : nullptr);
}

// plan the problem `p` (epilogue / dtype: the caller's words) with the stream's workspace and this device's CUs, and launch the plan
static int gemm_run(int family, const GemmArgs& p, int epilogue, int dtype, bool rope, hipStream_t st) {
  const GemmWs gws = gemm_ws_for(st);
  const GemmShape s{p.M, p.N, p.K, p.lda, p.ldw, epilogue, dtype, rope, !(reinterpret_cast<uintptr_t>(p.bias) & 7), p.sumsq != nullptr,
                    gws.p != nullptr, gws.bytes, a3v_cu_count()};
  GemmPlan pl;
  const int rc = gemm_plan(family, s, pl);
  if (rc != A3V_OK) return rc;
  for (int i = 0; i < pl.n; ++i) {
    const GemmStep& step = pl.step[i];
    const GemmArgs q = gemm_rows(p, family, step.row0, step.rows);
    if (i + 1 < pl.n && pl.step[i + 1].kernel == A3V_GEMM_K_REDUCE) launch_split(step, pl.step[++i], p, q, gws.p, st);
    else launch_step(step, q, st);
  }
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

static int gemm_nt_impl(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                        int M, int N, int K, const void* bias, const void* residual, int64_t ldr,
                        int epilogue, int dtype, void* stream, const RopeKvArgs* rk) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !W || !C) return A3V_ERR_ARG;
  if (epilogue & (1 << 19)) return A3V_ERR_ARG;   // the retired 32x32x16-MFMA tile switch: an error, not some other tile
  if ((epilogue & A3V_EPI_BIAS) && !bias) return A3V_ERR_ARG;
  if ((epilogue & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) && !residual) return A3V_ERR_ARG;
  if (epilogue & A3V_EPI_SWIGLU_BWD) {     // alone (no bias / activation / residual kinds), bf16, gate / up rows in `residual`
    if (!residual || dtype != A3V_BF16 || (epilogue & 0xffff & ~A3V_EPI_SWIGLU_BWD)) return A3V_ERR_ARG;
    if ((N % 8) || (ldr % 4) || ldr < 2 * (int64_t)N || ldc < 2 * (int64_t)N) return A3V_ERR_SHAPE;
  }
  if (dtype == A3V_F32) {
    if (K % 16 || lda % 4 || ldw % 4) return A3V_ERR_SHAPE;
    if ((epilogue & A3V_EPI_SWIGLU) && (N % 32)) return A3V_ERR_SHAPE;
  } else {
    if (dtype != A3V_BF16) return A3V_ERR_DTYPE;
    if (K % BK || lda % 8 || ldw % 8 || N % 4 || ldc % 4) return A3V_ERR_SHAPE;
    if ((epilogue & A3V_EPI_SWIGLU) && (N % 32)) return A3V_ERR_SHAPE;
    if ((epilogue & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) && (ldr % 4)) return A3V_ERR_SHAPE;
  }
  GemmArgs p = gemm_args(A, lda, W, ldw, C, ldc, residual, ldr, M, N, K, dtype == A3V_F32 ? epilogue : epilogue & 0xffff);
  p.bias = bias;
  if (rk && dtype == A3V_BF16) { p.rk = *rk; p.epi |= GEMM_EPI_ROPEKV; }
  return gemm_run(A3V_GEMM_NT, p, epilogue, dtype, rk != nullptr, (hipStream_t)stream);
}

extern "C" int a3v_gemm_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                           int M, int N, int K, const void* bias, const void* residual, int64_t ldr,
                           int epilogue, int dtype, void* stream) {
  return gemm_nt_impl(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, epilogue, dtype, stream, nullptr);
}

// qkv = A . Wqkv^T with the rotary embedding and the KV-cache write in the GEMM epilogue (prefill: LLM/llama_ens5.py:155-176
// xq, xk, xv = wq(x), wk(x), wv(x); apply_rotary_emb; cache_k / cache_v[:bsz, start_pos:start_pos+seqlen] = xk / xv).
// Same values as a3v_gemm_nt followed by a3v_rope_kvcache (the accumulator is rounded to the bf16 qkv value first).
extern "C" int a3v_gemm_qkv_rope(const void* A, int64_t lda, const void* W, int64_t ldw, int K, void* q_out, int64_t ldq,
                                 void* k_cache, void* vt_cache, void* v_rows, int64_t ldv, const void* delta, int64_t ldd,
                                 const float* cos_sin, int B, int S, int H, int Hkv, int hd, int Smax, int start_pos, int rope_pos0,
                                 void* stream) {
  if (!q_out || !k_cache || !vt_cache || !cos_sin || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if ((hd != 64 && hd != 128) || ldq % 4 || (v_rows && ldv % 4) || (delta && ldd % 4) || start_pos < 0 || start_pos + S > Smax) return A3V_ERR_SHAPE;
  RopeKvArgs rk;
  rk.q_out = (bf16_t*)q_out; rk.k_cache = (bf16_t*)k_cache; rk.vt_cache = (bf16_t*)vt_cache; rk.cos_sin = cos_sin;
  rk.v_rows = (bf16_t*)v_rows; rk.ldv = ldv;
  rk.ldq = ldq; rk.S = S; rk.H = H; rk.Hkv = Hkv; rk.hd_shift = hd == 128 ? 7 : 6; rk.Smax = Smax;
  rk.start_pos = start_pos; rk.rope_pos0 = rope_pos0; rk.m_off = 0;
  return gemm_nt_impl(A, lda, W, ldw, q_out, ldq, B * S, (H + 2 * Hkv) * hd, K, nullptr, delta, ldd, delta ? A3V_EPI_RESIDUAL : 0, A3V_BF16,
                      stream, &rk);
}

// ------------------------------------------------------------------------------------
// Split-K skinny GEMM for the LoRA adapter products (N or M = 64 with K in the thousands): S slices of the K loop run
// as gridDim.y planes of the 128x128 kernel writing fp32 partial outputs; a3v_splitk_reduce sums the planes in slice
// order (deterministic), optionally accumulates into the destination, and rounds once -- the same fp32-accumulate,
// round-once arithmetic as the un-split kernel.
// ------------------------------------------------------------------------------------
namespace {
template <typename TO>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int S, int64_t plane, int M, int N, TO* __restrict__ out,
                                                            int64_t ldo, int accumulate) {
  const int64_t n4 = (int64_t)M * (N / 4);
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / (N / 4)), c = (int)(i % (N / 4)) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(part + (int64_t)s * plane + (int64_t)r * N + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += x[e];
    }
    TO* o = out + (int64_t)r * ldo + c;
    // the product is rounded to bf16 exactly once, like the un-split kernel's epilogue (the value autocast's bf16 matmul
    // returns), also when it is then accumulated into an fp32 gradient
#pragma unroll
    for (int e = 0; e < 4; ++e) Cvt<TO>::st(o + e, accumulate ? Cvt<TO>::ld(o + e) + rbf(a[e]) : rbf(a[e]));
  }
}
}  // namespace

extern "C" int a3v_gemm_nt_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, float* partial, int M, int N, int K, int S,
                                  void* stream) {
  if (!A || !W || !partial || M <= 0 || N <= 0 || K <= 0 || S < 1 || S > 64) return A3V_ERR_ARG;
  if (K % 64 || lda % 8 || ldw % 8 || N % 4 || S > K / 64) return A3V_ERR_SHAPE;
  GemmArgs p = gemm_args(A, lda, W, ldw, partial, N, nullptr, 0, M, N, K, A3V_EPI_OUT_F32 | GEMM_EPI_RAW);
  p.c_split = (int64_t)M * N * 4;
  // Rows of the streamed operand per block and LDS stages (tools/skinny_stages_bench.py, operands rotating through 700 MB, us incl.
  // the reduce pass at 8728 x 64 x K = 4096 / 11008 / 12288 / 22016):
  //   64 rows, 2 stages, S = 4 (rounds 2-3)   24.0  54.5  60.0  112.1     half of the LDS-DMA traffic is the 64-row second operand
  //   64 rows, 4 stages, S = 3                23.1  52.8  56.4   96.9     k-tiles in flight across the barrier: +2..14 %
  //  256 rows, 3 stages, S = 7                23.5  46.3  49.0   82.9     35 row tiles x 7 slices = 245 blocks: ONE resident block per CU
  //  256 rows, 3 stages, S = 8                31.2  63.0  66.1  114.0     280 blocks: the 24 that wait for a CU double the time
  // so the 256-row form is taken when its blocks fill between half and all of the CUs (the caller picks S for that: train._skinny),
  // the 64-row form otherwise.  A3V_SKINNY_NARROW = 1 / 2 / 3 forces 256 / 128 / 64 rows, A3V_SKINNY_STAGES = 2 the two-stage kernels.
  const int narrow_env = A3V_ENV_INT("A3V_SKINNY_NARROW", 0);
  const int nst_env = A3V_ENV_INT("A3V_SKINNY_STAGES", 0);
  const int blocks256 = ((M + 255) / 256) * S;
  const bool wide = narrow_env ? narrow_env == 1 : (blocks256 <= a3v_cu_count() && 2 * blocks256 > a3v_cu_count());
  const int narrow = narrow_env ? narrow_env : (wide ? 1 : 3);
  if (N <= 64 && M >= 512 && narrow) {
    p.tiles_n = 1;
    const int nst = nst_env ? nst_env : (narrow == 1 ? 3 : 4);
    const int rows = narrow == 3 ? 64 : narrow == 2 ? 128 : 256;
    p.tiles_m = (M + rows - 1) / rows;
    static bool attr[A3V_MAX_DEV][9] = {};
    int attr_rc = 0;
    auto go = [&](auto kern, int bytes, int ai) {
      attr_rc = a3v_dyn_lds_once(attr, ai, (const void*)kern, bytes);
      if (attr_rc == 0) hipLaunchKernelGGL(kern, dim3(p.tiles_m, S), dim3(256), (size_t)bytes, (hipStream_t)stream, p);
    };
    // the library carries the two forms the rule above picks (and the two-stage kernels below)
    const int bytes = (rows + 64) * 128 * nst;
    if (rows == 64 && nst == 4) go(gemm_nt_skinny_kernel<64, 4>, bytes, 1);
    else if (rows == 256 && nst == 3) go(gemm_nt_skinny_kernel<256, 3>, bytes, 6);
    else if (nst != 2) return A3V_ERR_ARG;               // a rows / stages pair the library does not carry
    else if (narrow == 3) {
      hipLaunchKernelGGL((gemm_nt_bf16_kernel<64, 64, 4, 1>), dim3(p.tiles_m, S), dim3(256), 0, (hipStream_t)stream, p);
    } else if (narrow == 2) {
      hipLaunchKernelGGL((gemm_nt_bf16_kernel<128, 64, 4, 1>), dim3(p.tiles_m, S), dim3(256), 0, (hipStream_t)stream, p);
    } else {
      hipLaunchKernelGGL((gemm_nt_bf16_kernel<256, 64, 4, 1>), dim3(p.tiles_m, S), dim3(256), 0, (hipStream_t)stream, p);
    }
    if (attr_rc != 0) return attr_rc;
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  p.tiles_m = (M + 127) / 128; p.tiles_n = (N + 127) / 128;
  p.slow_epi = slow_epi_env(); p.nt_store = nt_store_env();
  hipLaunchKernelGGL((gemm_nt_bf16_kernel<128, 128, 2, 2>), dim3(p.tiles_m * p.tiles_n, S), dim3(256), 0, (hipStream_t)stream, p);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_splitk_reduce(const float* partial, int S, int M, int N, void* out, int64_t ldo, int out_dtype, int accumulate, void* stream) {
  if (!partial || !out || S < 1 || M <= 0 || N <= 0) return A3V_ERR_ARG;
  if (N % 4) return A3V_ERR_SHAPE;
  const int64_t n4 = (int64_t)M * (N / 4);
  const int blocks = (int)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
  if (out_dtype == A3V_BF16) hipLaunchKernelGGL(splitk_reduce_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, partial, S, (int64_t)M * N, M, N, (bf16_t*)out, ldo, accumulate);
  else if (out_dtype == A3V_F32) hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, partial, S, (int64_t)M * N, M, N, (float*)out, ldo, accumulate);
  else return A3V_ERR_DTYPE;
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

// C[M,N] = epilogue(At^T . Wt): At [K, M] (row stride lda), Wt [K, N] (row stride ldw), both bf16 with the CONTRACTED index
// as the row index -- dW = dY^T . X straight from the token-major activations (no a3v_transpose of either operand).
// 256x256 tiles only (M, N >= 256 recommended); plain / residual / fp32 epilogues as a3v_gemm_nt; any K >= 1.
extern "C" int64_t a3v_gemm_tn_sumsq_slots(int M, int N) {
  return (int64_t)((M + 255) / 256) * ((N + 255) / 256) * 8 + 2048;      // 8 waves per 256 x 256 tile + the split-K reduce pass' blocks
}

static int gemm_tn_impl(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                        const void* residual, int64_t ldr, int epilogue, void* stream, float* sumsq, int64_t sumsq_cap) {
  if (!At || !Wt || !C || M <= 0 || N <= 0 || K <= 0) return A3V_ERR_ARG;
  if (sumsq && (!(epilogue & (A3V_EPI_OUT_F32 | A3V_EPI_RES_F32)) || sumsq_cap < a3v_gemm_tn_sumsq_slots(M, N))) return A3V_ERR_ARG;
  if (lda % 8 || ldw % 8 || N % 4 || ldc % 4 || M % 8) return A3V_ERR_SHAPE;
  if (epilogue & ~(A3V_EPI_RESIDUAL | A3V_EPI_RES_F32 | A3V_EPI_OUT_F32)) return A3V_ERR_ARG;
  if ((epilogue & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) && !residual) return A3V_ERR_ARG;
  if (((int64_t)(K - 1) * lda + M) * 2 >= (1LL << 31) || ((int64_t)(K - 1) * ldw + N) * 2 >= (1LL << 31)) return A3V_ERR_SHAPE;
  GemmArgs p = gemm_args(At, lda, Wt, ldw, C, ldc, residual, ldr, M, N, K, epilogue);
  p.sumsq = sumsq;
  return gemm_run(A3V_GEMM_TN, p, epilogue, A3V_BF16, false, (hipStream_t)stream);
}

extern "C" int a3v_gemm_tn(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                           const void* residual, int64_t ldr, int epilogue, void* stream) {
  return gemm_tn_impl(At, lda, Wt, ldw, C, ldc, M, N, K, residual, ldr, epilogue, stream, nullptr, 0);
}

// a3v_gemm_tn with fp32 output that also leaves the sum of squares of what it stored, as a3v_gemm_tn_sumsq_slots(M, N) partial
// sums in `sumsq` (every slot it owns is written or was zeroed by the caller; slots of tiles outside C stay untouched = 0).
extern "C" int a3v_gemm_tn_sumsq(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                                 const void* residual, int64_t ldr, int epilogue, float* sumsq, int64_t sumsq_cap, void* stream) {
  if (!sumsq) return A3V_ERR_ARG;
  return gemm_tn_impl(At, lda, Wt, ldw, C, ldc, M, N, K, residual, ldr, epilogue, stream, sumsq, sumsq_cap);
}

// split-K form of a3v_gemm_tn for adapter-sized outputs (M or N of a few dozen, long K: the LoRA weight gradients
// dB = dY^T . t and dA = dt^T . X): S slices of the contracted index write raw fp32 planes partial[s][M][N]; a3v_splitk_reduce
// sums them in slice order.  Waves of the 256 x 256 tile that fall outside C idle.
extern "C" int a3v_gemm_tn_splitk(const void* At, int64_t lda, const void* Wt, int64_t ldw, float* partial, int M, int N, int K, int S,
                                  void* stream) {
  if (!At || !Wt || !partial || M <= 0 || N <= 0 || K <= 0 || S < 1 || S > 64) return A3V_ERR_ARG;
  if (lda % 8 || ldw % 8 || N % 4 || M % 8 || S > (K + 63) / 64) return A3V_ERR_SHAPE;
  if (((int64_t)(K - 1) * lda + M) * 2 >= (1LL << 31) || ((int64_t)(K - 1) * ldw + N) * 2 >= (1LL << 31)) return A3V_ERR_SHAPE;
  GemmArgs p = gemm_args(At, lda, Wt, ldw, partial, N, nullptr, 0, M, N, K, A3V_EPI_OUT_F32 | GEMM_EPI_RAW);
  p.tiles_m = (M + 255) / 256; p.tiles_n = (N + 255) / 256;
  p.c_split = (int64_t)M * N * 4;
  p.slow_epi = slow_epi_env(); p.nt_store = nt_store_env();
  p.xmap = tn_xmap(p.tiles_m, p.tiles_n);
  hipLaunchKernelGGL(gemm_tn_bf16_pp_kernel<false>, dim3(p.tiles_m * p.tiles_n, S), dim3(512), 0, (hipStream_t)stream, p);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

// C = epilogue((Aq . Wq^T) * sa[m] * sw[n]): fp8 (OCP e4m3fn) activations and weights with per-row fp32 scales, MX-scaled
// MFMA at twice the bf16 rate.  K % 128 == 0; 256 x 256 tiles for the whole problem; epilogues as a3v_gemm_nt (bf16 C).
static int gemm_nt_fp8_impl(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, void* C,
                            int64_t ldc, int M, int N, int K, const void* bias, const void* residual, int64_t ldr, int epilogue,
                            void* stream, const RopeKvArgs* rk) {
  if (!Aq || !sa || !Wq || !sw || !C || M <= 0 || N <= 0 || K <= 0) return A3V_ERR_ARG;
  if (K % 128 || lda % 16 || ldw % 16 || N % 4 || ldc % 4) return A3V_ERR_SHAPE;
  if (epilogue & ~(A3V_EPI_BIAS | A3V_EPI_GELU | A3V_EPI_QUICKGELU | A3V_EPI_RESIDUAL | A3V_EPI_SWIGLU | A3V_EPI_OUT_F32 | A3V_EPI_RES_F32)) return A3V_ERR_ARG;
  if ((epilogue & A3V_EPI_BIAS) && !bias) return A3V_ERR_ARG;
  if ((epilogue & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) && (!residual || ldr % 4)) return A3V_ERR_ARG;
  if ((epilogue & A3V_EPI_SWIGLU) && (N % 32)) return A3V_ERR_SHAPE;
  if ((int64_t)(M - 1) * lda + K >= (1LL << 31) || (int64_t)(N - 1) * ldw + K >= (1LL << 31)) return A3V_ERR_SHAPE;
  GemmArgs p = gemm_args(Aq, lda, Wq, ldw, C, ldc, residual, ldr, M, N, K, epilogue | GEMM_EPI_SCALE);
  p.bias = bias; p.sa = sa; p.sw = sw;
  if (rk) { p.rk = *rk; p.epi |= GEMM_EPI_ROPEKV; }
  return gemm_run(A3V_GEMM_NT_FP8, p, epilogue, A3V_BF16, rk != nullptr, (hipStream_t)stream);
}

extern "C" int a3v_gemm_nt_fp8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, void* C,
                               int64_t ldc, int M, int N, int K, const void* bias, const void* residual, int64_t ldr, int epilogue,
                               void* stream) {
  return gemm_nt_fp8_impl(Aq, lda, sa, Wq, ldw, sw, C, ldc, M, N, K, bias, residual, ldr, epilogue, stream, nullptr);
}

extern "C" int a3v_gemm_qkv_rope_fp8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, int K,
                                     void* q_out, int64_t ldq, void* k_cache, void* vt_cache, const float* cos_sin, int B, int S,
                                     int H, int Hkv, int hd, int Smax, int start_pos, int rope_pos0, void* stream) {
  if (!q_out || !k_cache || !vt_cache || !cos_sin || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if ((hd != 64 && hd != 128) || ldq % 4 || start_pos < 0 || start_pos + S > Smax) return A3V_ERR_SHAPE;
  RopeKvArgs rk{};
  rk.q_out = (bf16_t*)q_out; rk.k_cache = (bf16_t*)k_cache; rk.vt_cache = (bf16_t*)vt_cache; rk.cos_sin = cos_sin;
  rk.ldq = ldq; rk.S = S; rk.H = H; rk.Hkv = Hkv; rk.hd_shift = hd == 128 ? 7 : 6; rk.Smax = Smax;
  rk.start_pos = start_pos; rk.rope_pos0 = rope_pos0; rk.m_off = 0;
  return gemm_nt_fp8_impl(Aq, lda, sa, Wq, ldw, sw, q_out, ldq, B * S, (H + 2 * Hkv) * hd, K, nullptr, nullptr, 0, 0, stream, &rk);
}

// The training form: a3v_gemm_qkv_rope_fp8 with the two operands of a3v_gemm_qkv_rope the training forward needs -- v_rows and delta,
// through the same epilogue code (the fp8 kernels scale their accumulators in front of the bf16 kernels' epilogues).
extern "C" int a3v_gemm_qkv_rope_fp8_train(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, int K,
                                           void* q_out, int64_t ldq, void* k_cache, void* vt_cache, void* v_rows, int64_t ldv,
                                           const void* delta, int64_t ldd, const float* cos_sin, int B, int S, int H, int Hkv, int hd,
                                           int Smax, int start_pos, int rope_pos0, void* stream) {
  if (!q_out || !k_cache || !vt_cache || !cos_sin || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if ((hd != 64 && hd != 128) || ldq % 4 || (v_rows && ldv % 4) || (delta && ldd % 4) || start_pos < 0 || start_pos + S > Smax) return A3V_ERR_SHAPE;
  RopeKvArgs rk{};
  rk.q_out = (bf16_t*)q_out; rk.k_cache = (bf16_t*)k_cache; rk.vt_cache = (bf16_t*)vt_cache; rk.cos_sin = cos_sin;
  rk.v_rows = (bf16_t*)v_rows; rk.ldv = ldv;
  rk.ldq = ldq; rk.S = S; rk.H = H; rk.Hkv = Hkv; rk.hd_shift = hd == 128 ? 7 : 6; rk.Smax = Smax;
  rk.start_pos = start_pos; rk.rope_pos0 = rope_pos0; rk.m_off = 0;
  return gemm_nt_fp8_impl(Aq, lda, sa, Wq, ldw, sw, q_out, ldq, B * S, (H + 2 * Hkv) * hd, K, nullptr, delta, ldd,
                          delta ? A3V_EPI_RESIDUAL : 0, stream, &rk);
}

// "NN" GEMM: C[M,N] = epilogue(A . Wt) with A [M, K] row-major and Wt [K, N] row-major (the contracted index is Wt's ROW index) --
// the input gradient dX = dY . W on the weight image the forward pass uses, without a transposed copy of W.  K % 64 == 0.
extern "C" int a3v_gemm_nn(const void* A, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                           const void* residual, int64_t ldr, int epilogue, void* stream) {
  if (!A || !Wt || !C || M <= 0 || N <= 0 || K <= 0) return A3V_ERR_ARG;
  if (K % 64 || lda % 8 || ldw % 8 || N % 8 || ldc % 4) return A3V_ERR_SHAPE;
  const int simple = A3V_EPI_RESIDUAL | A3V_EPI_RES_F32 | A3V_EPI_OUT_F32;
  const bool swb = epilogue == A3V_EPI_SWIGLU_BWD;     // the product is d(act): `residual` = the forward's [gate | up] rows, C = [d gate | d up] (see a3v_gemm_nt)
  if (swb) {
    if (!residual || (ldr % 4) || ldr < 2 * (int64_t)N || ldc < 2 * (int64_t)N) return A3V_ERR_ARG;
  } else if (epilogue & ~simple) {
    return A3V_ERR_ARG;
  }
  if ((epilogue & (A3V_EPI_RESIDUAL | A3V_EPI_RES_F32)) && (!residual || ldr % 4)) return A3V_ERR_ARG;
  if (((int64_t)(M - 1) * lda + K) * 2 >= (1LL << 31) || ((int64_t)(K - 1) * ldw + N) * 2 >= (1LL << 31)) return A3V_ERR_SHAPE;
  return gemm_run(A3V_GEMM_NN, gemm_args(A, lda, Wt, ldw, C, ldc, residual, ldr, M, N, K, epilogue), epilogue, A3V_BF16, false, (hipStream_t)stream);
}

