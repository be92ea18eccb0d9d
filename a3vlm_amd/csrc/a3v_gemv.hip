// Decode GEMVs for gfx950: C[M,N] = epilogue(A[M,K] @ W[N,K]^T) with M <= 16 rows of activations, W in bf16, fp8 or NF4.
//
//  * gemv_dma_bf16_kernel : K % 128 == 0 (fp8 / NF4: % 256).  W streamed once from HBM by coalesced LDS-DMA through wave-private
//    rings, A slice shared per block in LDS, split-K across blocks with an in-kernel last-block fix-up (one launch).
//  * gemv_kq_bf16_kernel : M <= 8, bf16 weights: the K slices are the waves of one block, the partials meet in LDS.
//  * gemm_skinny1_bf16_kernel : the direct-to-VGPR form for every other K % 32 == 0 (bf16 weights only).
//  * gemv_plan / gemv_execute / gemv_run (below the kernels): which of them a call launches, the launch, the argument check.
// The LoRA adapter products (gemm_nt_skinny_kernel, a3v_gemm_nt_splitk) are tile GEMMs and live in a3v_gemm.hip.
#include "a3v_common.h"
#include <cstring>

namespace {

// ------------------------------------------------------------------------------------
// Skinny GEMM, single launch: one 8-wave block per 16 (or 32 with SwiGLU: gate block + up block)
// rows of W.  The block's waves split K, each streams its slice of the W rows straight into MFMA
// operand registers (8 independent 16-B non-temporal loads in flight per lane), the eight partial
// 16x16 accumulators are summed through LDS and wave 0 applies the epilogue.  W is read from HBM
// exactly once, nothing is written but C: algorithmic bytes = 2 N K (+ M K x re-reads from L2).
// ------------------------------------------------------------------------------------
struct Skinny1Args {
  const bf16_t* A;
  const bf16_t* W;
  void* C;
  const void* res;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K, epi, kslice;
};

template <int TILES>   // 1: 16 rows per block; 2: 32 rows (interleaved gate/up pair)
__global__ __launch_bounds__(512) void gemm_skinny1_bf16_kernel(Skinny1Args p) {
  __shared__ float red[8][TILES][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16 * TILES;
  const int row = lane & 15, kq = (lane >> 4) * 8;
  const int ar = row < p.M ? row : p.M - 1;
  const bf16_t* ap = p.A + (int64_t)ar * p.lda + wave * p.kslice + kq;
  const bf16_t* wp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    int wr = n0 + t * 16 + row;
    wr = wr < p.N ? wr : p.N - 1;
    wp[t] = p.W + (int64_t)wr * p.ldw + wave * p.kslice + kq;
  }
  f32x4 acc[TILES][2];
#pragma unroll
  for (int t = 0; t < TILES; ++t) { acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int kend = min(p.kslice, p.K - wave * p.kslice);     // the last wave may own a shorter (or empty) slice
  constexpr int U = TILES == 1 ? 8 : 4;                      // 32-k steps per unrolled iteration
  int k = 0;
  for (; k + U * 32 <= kend; k += U * 32) {
    bf16x8 w[TILES][U], a[U];
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int q = 0; q < U; ++q) w[t][q] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp[t] + k + q * 32));
#pragma unroll
    for (int q = 0; q < U; ++q) a[q] = *reinterpret_cast<const bf16x8*>(ap + k + q * 32);
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int q = 0; q < U; ++q) acc[t][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t][q], a[q], acc[t][q & 1], 0, 0, 0);
  }
  for (; k < kend; k += 32) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + k);
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const bf16x8 w = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp[t] + k));
      acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, acc[t][0], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][lane][r] = acc[t][0][r] + acc[t][1][r];
  __syncthreads();
  if (wave != 0) return;
  float v[TILES][4];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float a = 0.f;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) a += red[w8][t][lane][r];
      v[t][r] = a;
    }
  // D[n = (lane>>4)*4 + r][m = lane&15]
  const int m = lane & 15;
  if (m >= p.M) return;
  if (TILES == 2) {        // SwiGLU: tile 0 = gate rows, tile 1 = up rows of the same 16 output columns
    const int oc = (n0 >> 1) + (lane >> 4) * 4;
    if (n0 >= p.N) return;
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(rbf(silu(rbf(v[0][r]))) * rbf(v[TILES - 1][r]));
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + oc) = o;
    return;
  }
  const int n = n0 + (lane >> 4) * 4;
  if (n >= p.N) return;
  float o4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o4[r] = rbf(v[0][r]);
  if (p.epi & A3V_EPI_RESIDUAL) {
    const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] += bf2f(rr[r]);
  }
  if (p.epi & A3V_EPI_OUT_F32) {
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = o4[r];
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = o;
  } else {
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(o4[r]);
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n) = o;
  }
}

// ------------------------------------------------------------------------------------
// Decode GEMV, M <= 16, K % 128 == 0: W streamed ONCE from HBM by LDS-DMA.
//   * block = 4 waves, all on K-slice `sl` of row group `tg` (64 W rows); wave w owns the 16-row tile tg*4 + w.
//   * the A slice [AROWS][slice] is DMA'd once per block into LDS and shared by the 4 waves (AROWS = 8 when
//     M <= 8: MFMA columns m >= 8 read row m & 7 and are never stored), so activations cost no VGPR traffic.
//   * each wave streams its 16 rows through a private 2-stage ring of 16 rows x 128 k (4 KB = 4 DMA instructions
//     of 4 rows x 256 contiguous bytes); MFMA fragments by ds_read_b128, slot XOR row swizzle applied on the DMA
//     source side (conflict-free).  No block barrier in the K loop (the ring is wave-private).
//   * split-K across blocks: partial accumulators go to the workspace; the WAVE that arrives last at its tile's
//     (agent-scope) counter sums the S partials in slice order (deterministic), runs the epilogue and leaves the
//     counter at zero -- no block barrier, no second launch.  Blocks of one row group share an XCD (same L2).
// Measured (tools/ubench/skinny.hip, weights rotating through 3 GB): 5.0-5.5 TB/s vs 3.5-4.3 for the direct-to-VGPR form.
// ------------------------------------------------------------------------------------
struct GemvArgs {
  const bf16_t* A;
  const bf16_t* W;
  void* C;
  const void* res;
  float* part;
  int* counters;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K, epi, S, nkb, tgs, maxkb;
  // fused decode-step forms (a3v_gemv_fused): RMSNorm prologue, RoPE + KV-cache epilogue, sum-of-squares side output
  const bf16_t* norm_w;     // PRO: A holds the un-normalised rows h; the block normalises its K slice while staging it
  const float* ssq_in;      // PRO: [ssq_tiles][16] per-16-column partial sums of squares of the rows of A
  float* ssq_out;           // GEMV_EPI_SSQ: the same quantity for the rows this GEMV writes (residual stream)
  const float* cos_sin;     // GEMV_EPI_ROPEKV: fp32 [pos][hd/2][2]
  bf16_t* k_cache;          //   [M, Hkv, Smax, hd]
  bf16_t* vt_cache;         //   [M, Hkv, hd, Smax]
  const float* wscale;      // W8: per-row dequantisation scales (W rows are fp8 e4m3fn bytes, ldw in BYTES); N4: [N, K/64] block scales
  float eps;
  int ssq_tiles, H, Hkv, hd, Smax, pos;
  int n4;                   // N4: W rows are NF4 nibbles (a3v_quantize_nf4 image, ldw in BYTES)
};

constexpr int GEMV_EPI_ROPEKV = 1 << 24;
constexpr int GEMV_EPI_SSQ = 1 << 25;

// Epilogue of the decode GEMVs for one finished 16-row tile (SwiGLU: one gate / up tile pair): v[r] = D[n = nt0 + 4 (lane>>4) + r][m = lane & 15]
// (u: the matching up-projection rows).  Shared by the split-K-across-blocks kernel above and the split-K-inside-the-block kernel below.
__device__ __forceinline__ void gemv_finish(const GemvArgs& p, f32x4 v, f32x4 u, int nt0, int lane, bool swiglu) {
  const int m = lane & 15;
  if (swiglu) {
    if (m >= p.M || nt0 >= p.N) return;
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
  if (p.epi & GEMV_EPI_ROPEKV) {
    // fused apply_rotary_emb + KV-cache write of the decode step (llama_ens5.py:118,124-129; a3v_rope_kvcache at S == 1):
    // rows n are [q heads | k heads | v heads] x hd; a lane holds two interleaved pairs of one head, batch row m.
    if (m >= p.M || n >= p.N) return;
    const int slot = n / p.hd, d = n % p.hd, half = p.hd >> 1;
    if (slot < p.H + p.Hkv) {
      const float* cs = p.cos_sin + ((int64_t)p.pos * half + (d >> 1)) * 2;
      const f32x4 t = *reinterpret_cast<const f32x4*>(cs);          // (cos, sin) of the two pairs
      bf16x4 o;
      o[0] = f2bf(o4[0] * t[0] - o4[1] * t[1]);
      o[1] = f2bf(o4[0] * t[1] + o4[1] * t[0]);
      o[2] = f2bf(o4[2] * t[2] - o4[3] * t[3]);
      o[3] = f2bf(o4[2] * t[3] + o4[3] * t[2]);
      bf16_t* dst = slot < p.H ? reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n
                               : p.k_cache + (((int64_t)m * p.Hkv + (slot - p.H)) * p.Smax + p.pos) * p.hd + d;
      *reinterpret_cast<bf16x4*>(dst) = o;
    } else {
      bf16_t* dst = p.vt_cache + (((int64_t)m * p.Hkv + (slot - p.H - p.Hkv)) * p.hd + d) * (int64_t)p.Smax + p.pos;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(int64_t)r * p.Smax] = f2bf(o4[r]);
    }
    return;
  }
  const bool live = m < p.M && n < p.N;
  if (live && (p.epi & A3V_EPI_RESIDUAL)) {
    const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p.res) + (int64_t)m * p.ldr + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] += bf2f(rr[r]);
  }
  if (p.epi & GEMV_EPI_SSQ) {
    // sum of squares of the 16 bf16 values this tile contributes to row m (consumed by the next GEMV's RMSNorm prologue)
    float sq = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float hb = rbf(o4[r]); sq = fmaf(hb, hb, sq); }
    if (!live) sq = 0.f;
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    if (lane < 16 && nt0 < p.N) p.ssq_out[(nt0 >> 4) * 16 + lane] = sq;
  }
  if (!live) return;
  if (p.epi & A3V_EPI_OUT_F32) {
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = o4[r];
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = o;
  } else {
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(o4[r]);
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n) = o;
  }
}

// Eight NF4 codes (one dword: byte j holds elements 2j (high nibble) and 2j+1 (low nibble)) -> their code-book values as bf16x8.
// v_perm_b32 picks bytes out of 8-byte tables: the high and the low bytes of the bf16 code book, entries 0..7 and 8..15 apart
// (bf16 bits: bf80 bf32 bf06 beca be92 be3d bdba 0000 3da3 3e25 3e7c 3ead 3ee2 3f10 3f39 3f80); bit 3 of a code selects the
// half by a byte mask.  29 VALU operations per 8 weights.
__device__ __forceinline__ bf16x8 nf4_bf16x8(uint32_t x) {
  const uint32_t io = x & 0x07070707u, ie = (x >> 4) & 0x07070707u;           // odd / even elements, low 3 bits
  const uint32_t mo = ((x >> 3) & 0x01010101u) * 0xFFu, me = ((x >> 7) & 0x01010101u) * 0xFFu;   // bit 3 -> byte masks
  auto look = [](uint32_t i, uint32_t m, uint32_t t0a, uint32_t t0b, uint32_t t1a, uint32_t t1b) {
    return (__builtin_amdgcn_perm(t1b, t1a, i) & m) | (__builtin_amdgcn_perm(t0b, t0a, i) & ~m);
  };
  const uint32_t he = look(ie, me, 0xbebfbfbfu, 0x00bdbebeu, 0x3e3e3e3du, 0x3f3f3f3eu);
  const uint32_t le = look(ie, me, 0xca063280u, 0x00ba3d92u, 0xad7c25a3u, 0x803910e2u);
  const uint32_t ho = look(io, mo, 0xbebfbfbfu, 0x00bdbebeu, 0x3e3e3e3du, 0x3f3f3f3eu);
  const uint32_t lo = look(io, mo, 0xca063280u, 0x00ba3d92u, 0xad7c25a3u, 0x803910e2u);
  const uint32_t e01 = __builtin_amdgcn_perm(he, le, 0x05010400u), e23 = __builtin_amdgcn_perm(he, le, 0x07030602u);   // elements 0,2 | 4,6
  const uint32_t o01 = __builtin_amdgcn_perm(ho, lo, 0x05010400u), o23 = __builtin_amdgcn_perm(ho, lo, 0x07030602u);   // elements 1,3 | 5,7
  u32x4 r;
  r[0] = __builtin_amdgcn_perm(o01, e01, 0x05040100u);
  r[1] = __builtin_amdgcn_perm(o01, e01, 0x07060302u);
  r[2] = __builtin_amdgcn_perm(o23, e23, 0x05040100u);
  r[3] = __builtin_amdgcn_perm(o23, e23, 0x07060302u);
  return __builtin_bit_cast(bf16x8, r);
}

// W8: the weight rows are OCP fp8 e4m3fn (weight-only quantisation, one fp32 scale per row applied to the summed
// accumulator).  A ring stage is still 16 rows x 256 B, i.e. 256 k instead of 128; fragments are read 8 B per lane and
// widened fp8 -> f32 -> bf16 in registers (exact), so the arithmetic is the bf16 MFMA on dequantised weights.
//
// N4: the weight rows are NF4 nibbles (a3v_quantize_nf4: two codes per byte, earlier element high, one fp32 scale per 64-k block).
// A ring stage is 16 rows x 128 B of nibbles (256 k, so K % 256 == 0 as for W8) plus the 16 rows x 16 B of the stage's four block
// scales (2 x 16-B + 1 x 4-B LDS-DMA instructions, 2304 B); a stage holds half the bytes of a bf16 / fp8 stage, so the wave's ring
// has THREE slots of 2304 B in the same 8 KiB (two stages in flight behind the one being consumed instead of one).  The codes are looked up as bf16 by v_perm_b32 from byte tables held in
// registers (nf4_bf16x8), each 64-k block is accumulated by its own two MFMAs and its scale is applied once per accumulator element:
// acc += s_b * (codes . a).  Rounding differs from the bf16 GEMV on Wd = bf16(NF4[q] * s_b): the codes are rounded to bf16 and the
// scale is applied in fp32 to the block sums.
template <int AROWS, bool PRO, bool W8, bool N4 = false>
__global__ __launch_bounds__(256) void gemv_dma_bf16_kernel(GemvArgs p) {
  constexpr int WAUX = 2;   // cache-policy bits of the weight-stream LDS-DMA: nt (the weights are streamed once per step by ONE CU each)
  extern __shared__ __attribute__((aligned(1024))) char gemv_lds[];
  __shared__ float rinv_s[16];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // block -> (row group, slice): all slices of a row group on one XCD (blockIdx % 8)
  const int xq = blockIdx.x >> 3;
  const int sl = xq % p.S;
  const int tg = (xq / p.S) * 8 + (blockIdx.x & 7);
  if (tg >= p.tgs) return;
  constexpr int APB = (W8 || N4) ? 2 : 1;              // 128-k blocks of A per ring stage of W
  constexpr int DPS = N4 ? 3 : 4;                      // LDS-DMA instructions per ring stage
  constexpr int NSL = N4 ? 3 : 2;                      // ring slots per wave
  constexpr int SSTR = N4 ? 2304 : 4096;               // bytes per ring slot
  const int nst_all = p.nkb / APB;
  const int st0 = (int)(((int64_t)sl * nst_all) / p.S), st1 = (int)(((int64_t)(sl + 1) * nst_all) / p.S);
  const int nst = st1 - st0;                           // ring stages of this slice
  const int kb0 = st0 * APB, nkb = nst * APB;          // ... in 128-k blocks of A
  constexpr int ABLK = AROWS * 256;                    // bytes of A per 128-k block
  char* Alds = gemv_lds;
  char* Wring = gemv_lds + p.maxkb * ABLK + wave * 2 * 4096;
  const int n0 = (tg * 4 + wave) * 16;
  const int dr = lane >> 4, dslot = lane & 15;
  if (!PRO) {
    constexpr int IPB = AROWS / 4;                     // DMA instructions per k-block
    for (int j = wave; j < nkb * IPB; j += 4) {
      const int kb = j / IPB, i = j % IPB;
      const int row = 4 * i + dr;
      const int ar = row < p.M ? row : p.M - 1;
      const bf16_t* src = p.A + (int64_t)ar * p.lda + (int64_t)(kb0 + kb) * 128 + ((dslot ^ row) & 15) * 8;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(Alds + kb * ABLK + i * 1024), 16, 0, 0);
    }
  }
  const char* wrow[4];                                 // a stage row is 256 B in the bf16 and fp8 formats
  if constexpr (N4) {
    // nibbles: instruction i covers rows 8 i + (lane >> 3), 16-B slot lane & 7 of a 128-B stage row (chunk slot ^ row);
    // scales: one 4-B piece per lane, scale (lane & 3) of the stage's four of row lane >> 2 (16 rows x 16 B = 256 B)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = 8 * i + (lane >> 3);
      int wr = n0 + row;
      wr = wr < p.N ? wr : p.N - 1;
      wrow[i] = reinterpret_cast<const char*>(p.W) + (int64_t)wr * p.ldw + (int64_t)st0 * 128 + (((lane & 7) ^ row) & 7) * 16;
    }
    int sr = n0 + (lane >> 2);
    sr = sr < p.N ? sr : p.N - 1;
    wrow[2] = reinterpret_cast<const char*>(p.wscale + (int64_t)sr * (p.K / 64) + (int64_t)st0 * 4 + (lane & 3));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * i + dr;
      int wr = n0 + row;
      wr = wr < p.N ? wr : p.N - 1;
      wrow[i] = reinterpret_cast<const char*>(p.W) + (int64_t)wr * p.ldw * (W8 ? 1 : 2) + (int64_t)st0 * 256 + ((dslot ^ row) & 15) * 16;
    }
  }
  auto dma_stage = [&](int st, int slot) {
    if constexpr (N4) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wrow[i] + st * 128),
                                         (__attribute__((address_space(3))) void*)(Wring + slot * SSTR + i * 1024), 16, 0, WAUX);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wrow[2] + st * 16),
                                       (__attribute__((address_space(3))) void*)(Wring + slot * SSTR + 2048), 4, 0, WAUX);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wrow[i] + st * 256),
                                         (__attribute__((address_space(3))) void*)(Wring + slot * 4096 + i * 1024), 16, 0, WAUX);
    }
  };
  if (PRO) {
    // RMSNorm of the block's K slice of A (model/components.py:39,52-53 rounding: fp32 x*rinv -> bf16 -> * weight -> bf16),
    // 1/rms from the producer's per-tile sums of squares.  All prologue loads (L2 hits) are issued BEFORE the weight
    // ring's first DMAs: memory returns in order, so the normalisation runs while the first weight stages are in flight.
    __shared__ float ssq_w[4][16];
    constexpr int NQ = AROWS / 4;                      // float4 per tile row of the ssq table
    f32x4 sq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) sq[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = threadIdx.x; t < p.ssq_tiles; t += 256) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p.ssq_in + t * 16 + q * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) sq[q][r] += x[r];
      }
    }
    const int per_row = nkb * 16, total = p.M * per_row;
    constexpr int CH = 4;                              // items (16-B chunks of A) per thread per pass
    bf16x8 xa[CH], ga[CH];
    auto issue = [&](int base) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        int it = base + j * 256 + threadIdx.x;
        it = it < total ? it : total - 1;
        const int m = it / per_row, cc = it % per_row;
        const int64_t k = (int64_t)(kb0 + (cc >> 4)) * 128 + (cc & 15) * 8;
        xa[j] = *reinterpret_cast<const bf16x8*>(p.A + (int64_t)m * p.lda + k);
        ga[j] = *reinterpret_cast<const bf16x8*>(p.norm_w + k);
      }
    };
    auto finish = [&](int base) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int it = base + j * 256 + threadIdx.x;
        if (it < total) {
          const int m = it / per_row, cc = it % per_row;
          const int kb = cc >> 4, c = cc & 15;
          const float ri = rinv_s[m];
          bf16x8 y;
#pragma unroll
          for (int e = 0; e < 8; ++e) y[e] = f2bf(rbf((float)xa[j][e] * ri) * (float)ga[j][e]);
          *reinterpret_cast<bf16x8*>(Alds + kb * ABLK + m * 256 + ((c ^ m) & 15) * 16) = y;
        }
      }
    };
    issue(0);
    dma_stage(0, 0);
    if (nst > 1) dma_stage(1, 1);
    if constexpr (NSL > 2) {
      if (nst > 2) dma_stage(2, 2);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = wave_sum(sq[q][r]);
        if (lane == 0) ssq_w[wave][q * 4 + r] = t;
      }
    __syncthreads();
    if (threadIdx.x < AROWS)
      rinv_s[threadIdx.x] = rsqrtf((ssq_w[0][threadIdx.x] + ssq_w[1][threadIdx.x] + ssq_w[2][threadIdx.x] + ssq_w[3][threadIdx.x]) / (float)p.K + p.eps);
    __syncthreads();
    finish(0);
    for (int base = CH * 256; base < total; base += CH * 256) {
      issue(base);
      finish(base);
    }
  } else if constexpr (NSL > 2) {
    dma_stage(0, 0);
    if (nst > 2) {
      dma_stage(1, 1);
      dma_stage(2, 2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * DPS) : "memory");   // in-order completion: the A pieces issued before the ring prologue
    } else if (nst > 1) {
      dma_stage(1, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DPS) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS) : "memory");
    }
  } else {
    dma_stage(0, 0);
    if (nst > 1) {
      dma_stage(1, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DPS) : "memory");   // in-order completion: the A pieces issued before the ring prologue
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS) : "memory");
    }
  }
  __syncthreads();
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fg = lane >> 4;
  const int arow = AROWS == 8 ? (fr & 7) : fr;
  int foff[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) foff[s4] = (((4 * s4 + fg) ^ fr) & 15) * 16;
  int aoff[4];
#pragma unroll
  // AROWS == 8: lanes fr >= 8 feed accumulator columns 8..15, which are never stored.  Pointing them at the SAME address as lane
  // fr - 8 made every A fragment read a 2-way bank conflict (b128 reads do not merge duplicates: PMC conflict cycles = 2x the
  // active LDS cycles); with the lane's own fr in the swizzle they read the other half-row of the same row instead (any finite
  // data will do) and the 16 lanes of a group cover 16 distinct slots.
  for (int s4 = 0; s4 < 4; ++s4) aoff[s4] = (((4 * s4 + fg) ^ fr) & 15) * 16;
  for (int st = 0; st < nst; ++st) {
    const int slot = NSL > 2 ? st % NSL : st & 1;
    if constexpr (NSL > 2) {                            // stage st landed; up to two later stages may still be in flight
      if (st + 3 <= nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DPS) : "memory");
      else if (st + 2 <= nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (st + 2 <= nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const char* Ws = Wring + slot * 4096 + fr * 256;
    if constexpr (N4) {
      // 8 MFMA steps per stage, two per 64-k block: step s covers k = 32 s .. 32 s + 31; the lane's 8 codes are dword fg of
      // 16-B chunk s of its row.  Block scales of rows 4 (lane >> 4) + r: 16 B per row at +2048 of the slot.
      const char* Wn = Wring + slot * SSTR + fr * 128;
      const char* Sc = Wring + slot * SSTR + 2048 + (lane >> 4) * 64;
      uint32_t wq[8];
      bf16x8 af[8];
      f32x4 sc[4];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        wq[s8] = *reinterpret_cast<const uint32_t*>(Wn + ((s8 ^ fr) & 7) * 16 + fg * 4);
        af[s8] = *reinterpret_cast<const bf16x8*>(Alds + (st * 2 + (s8 >> 2)) * ABLK + arow * 256 + aoff[s8 & 3]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = *reinterpret_cast<const f32x4*>(Sc + r * 16);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (st + NSL < nst) dma_stage(st + NSL, slot);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf4_bf16x8(wq[2 * b]), af[2 * b], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nf4_bf16x8(wq[2 * b + 1]), af[2 * b + 1], t, 0, 0, 0);
        if (b & 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc1[r] = fmaf(t[r], sc[r][b], acc1[r]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc0[r] = fmaf(t[r], sc[r][b], acc0[r]);
        }
      }
    } else if (!W8) {
      const char* As = Alds + st * ABLK + arow * 256;
      bf16x8 wf[4], af[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        wf[s4] = *reinterpret_cast<const bf16x8*>(Ws + foff[s4]);
        af[s4] = *reinterpret_cast<const bf16x8*>(As + aoff[s4]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // fragments are in registers: the slot may be overwritten
      if (st + 2 < nst) dma_stage(st + 2, slot);
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        if (s4 & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s4], af[s4], acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s4], af[s4], acc0, 0, 0, 0);
      }
    } else {
      // 8 MFMA steps per stage: step s8 covers k = 32 s8 .. 32 s8 + 31; the lane's 8 bytes sit in 16-B chunk 2 s8 + (fg >> 1)
      u32x2 wq[8];
      bf16x8 af[8];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        wq[s8] = *reinterpret_cast<const u32x2*>(Ws + (((2 * s8 + (fg >> 1)) ^ fr) & 15) * 16 + (fg & 1) * 8);
        af[s8] = *reinterpret_cast<const bf16x8*>(Alds + (st * 2 + (s8 >> 2)) * ABLK + arow * 256 + aoff[s8 & 3]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (st + 2 < nst) dma_stage(st + 2, slot);
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        bf16x8 wf;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          // (round 5) v_cvt_scalef32_pk_bf16_fp8 (gfx950): two e4m3 bytes -> two bf16 in ONE VALU op (scale 1: exact, as the fp8 -> f32
          // -> bf16 pair of ops it replaces)
          const bf16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(wq[s8][h2], 1.0f, false);
          const bf16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(wq[s8][h2], 1.0f, true);
          wf[4 * h2 + 0] = lo[0]; wf[4 * h2 + 1] = lo[1]; wf[4 * h2 + 2] = hi[0]; wf[4 * h2 + 3] = hi[1];
        }
        if (s8 & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[s8], acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[s8], acc0, 0, 0, 0);
      }
    }
  }
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = acc0[r] + acc1[r];
  const bool swiglu = (p.epi & A3V_EPI_SWIGLU) != 0;     // launcher guarantees S > 1 with SwiGLU
  f32x4 u = {0.f, 0.f, 0.f, 0.f};
  int nt0 = n0;                                          // first W row of the tile this wave finishes
  if (p.S > 1) {
    // Wave-granular split-K fix-up, no block barrier: the wave writes its partial accumulator (sc0 sc1 = agent-coherent
    // access, no cache-wide write-back / invalidate), waits for the acknowledge, then bumps the arrival counter of its
    // tile (of its gate/up tile PAIR with SwiGLU).  The wave that arrives last reloads all partials in one round trip,
    // sums them in slice order (bit-identical whichever wave is last), resets the counter and runs the epilogue.
    float* mine = p.part + (((int64_t)(tg * p.S + sl) * 4 + wave) * 64 + lane) * 4;
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(mine), "v"(v) : "memory");   // (s_nop: the store's data registers, see the V^T store of the fused-qkv epilogue)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int* ctr = p.counters + (swiglu ? tg * 2 + (wave >> 1) : tg * 4 + wave);
    const int expect = swiglu ? 2 * p.S : p.S;
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != expect - 1) return;
    if (lane == 0) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int w0 = swiglu ? (wave & ~1) : wave;          // gate tile (or own tile)
    nt0 = (tg * 4 + w0) * 16;
    const float* base = p.part + (((int64_t)tg * p.S * 4 + w0) * 64 + lane) * 4;
    f32x4 x[8], y[8];
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const float* src = base + (int64_t)(s8 < p.S ? s8 : p.S - 1) * 4 * 64 * 4;
      asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(x[s8]) : "v"(src) : "memory");
    }
    if (swiglu) {
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        const float* src = base + 64 * 4 + (int64_t)(s8 < p.S ? s8 : p.S - 1) * 4 * 64 * 4;
        asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(y[s8]) : "v"(src) : "memory");
      }
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]), "+v"(y[6]), "+v"(y[7])::"memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])::"memory");
    v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8)
      if (s8 < p.S) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += x[s8][r];
        if (swiglu) {
#pragma unroll
          for (int r = 0; r < 4; ++r) u[r] += y[s8][r];
        }
      }
  }
  if (W8) {                 // per-row dequantisation scale on the summed accumulator (rows clamp: the stores are masked)
    const int nr = nt0 + (lane >> 4) * 4;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(p.wscale + (nr + 4 <= p.N ? nr : 0));
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= sc[r];
    if (swiglu) {
      const f32x4 su = *reinterpret_cast<const f32x4*>(p.wscale + (nr + 20 <= p.N ? nr + 16 : 0));
#pragma unroll
      for (int r = 0; r < 4; ++r) u[r] *= su[r];
    }
  }
  gemv_finish(p, v, u, nt0, lane, swiglu);
}

// ------------------------------------------------------------------------------------
// Decode GEMV with the K split INSIDE the block (round 4; M <= 8, bf16 weights): the block owns ONE 16-row tile of W (with SwiGLU a
// gate / up tile pair) and its waves are the K slices -- the same number of waves streaming the same 16 rows x (K / slices) through
// the same private 2-stage rings as gemv_dma_bf16_kernel, but the partial accumulators meet in LDS behind one block barrier instead
// of in HBM behind store -> acknowledge -> arrival counter -> reload (three dependent memory round trips per launch: 0.42 ms of the
// 3.85-ms decode step, profiles/r04g_decode_fixup_and_rope_epilogue.txt).  What the shared LDS slice of A gave up for that: a wave
// reads ITS K slice of the 8 activation rows straight from L2 into registers in MFMA operand layout (4 x 16 B per lane and stage,
// two stages ahead; with the RMSNorm prologue the norm weights the same way and the normalisation in registers), so a block needs
// only its rings + a 1-KiB reduce patch per wave and 5-6 blocks fit a CU.
// ------------------------------------------------------------------------------------
template <bool PRO>
__global__ __launch_bounds__(768) void gemv_kq_bf16_kernel(GemvArgs p) {
  extern __shared__ __attribute__((aligned(1024))) char kq_lds[];
  __shared__ float rinv_s[8];
  __shared__ float ssq_w[12][8];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
  const bool swiglu = (p.epi & A3V_EPI_SWIGLU) != 0;
  // tile and K slice of this wave
  const int tiles_pb = swiglu ? 2 : 1;
  const int slices = nw / tiles_pb;
  const int tile = blockIdx.x * tiles_pb + (swiglu ? (wave & 1) : 0);
  const int sl = swiglu ? (wave >> 1) : wave;
  const int n0 = tile * 16;
  const int st0 = (int)(((int64_t)sl * p.nkb) / slices), st1 = (int)(((int64_t)(sl + 1) * p.nkb) / slices);
  const int nst = st1 - st0;
  char* Wring = kq_lds + wave * 2 * 4096;
  float* red = reinterpret_cast<float*>(kq_lds + nw * 2 * 4096);          // [nw][64 lanes][4] partial accumulators
  const int dr = lane >> 4, dslot = lane & 15;
  const char* wrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * i + dr;
    int wr = n0 + row;
    wr = wr < p.N ? wr : p.N - 1;
    wrow[i] = reinterpret_cast<const char*>(p.W) + (int64_t)wr * p.ldw * 2 + (int64_t)st0 * 256 + ((dslot ^ row) & 15) * 16;
  }
  auto dma_stage = [&](int st, int slot) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wrow[i] + st * 256),
                                       (__attribute__((address_space(3))) void*)(Wring + slot * 4096 + i * 1024), 16, 0, 2);
  };
  // A fragments (B operand): lane (fr = lane & 15 -> activation row fr & 7, fg = lane >> 4): k = 128 stage + 32 s4 + 8 fg + 0..7
  const int fr = lane & 15, fg = lane >> 4;
  const int arow = (fr & 7) < p.M ? (fr & 7) : p.M - 1;
  const bf16_t* arp = p.A + (int64_t)arow * p.lda + (int64_t)st0 * 128 + fg * 8;
  const bf16_t* gp = PRO ? p.norm_w + (int64_t)st0 * 128 + fg * 8 : nullptr;
  bf16x8 ax[2][4], ag[2][4];
  auto load_a = [&](int st, int set) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      ax[set][s4] = *reinterpret_cast<const bf16x8*>(arp + st * 128 + s4 * 32);
      if (PRO) ag[set][s4] = *reinterpret_cast<const bf16x8*>(gp + st * 128 + s4 * 32);
    }
  };
  if (nst > 0) { load_a(0, 0); dma_stage(0, 0); }
  if (nst > 1) { load_a(1, 1); dma_stage(1, 1); }
  float ri = 1.f;
  if (PRO) {
    // 1/rms of the 8 rows from the producer's per-16-column sums of squares (model/components.py:39,52-53); issued behind the first
    // stages, so the reduction runs while they are in flight
    f32x4 sq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int t = threadIdx.x; t < p.ssq_tiles; t += blockDim.x) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p.ssq_in + t * 16 + q * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) sq[q][r] += x[r];
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = wave_sum(sq[q][r]);
        if (lane == 0) ssq_w[wave][q * 4 + r] = t;
      }
    __syncthreads();
    if (threadIdx.x < 8) {
      float t = 0.f;
      for (int w = 0; w < nw; ++w) t += ssq_w[w][threadIdx.x];
      rinv_s[threadIdx.x] = rsqrtf(t / (float)p.K + p.eps);
    }
    __syncthreads();
    ri = rinv_s[fr & 7];
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int foff[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) foff[s4] = (((4 * s4 + fg) ^ fr) & 15) * 16;
  auto stage_body = [&](int st, auto setc) {
    constexpr int SET = decltype(setc)::value;
    // W(st) and A(st) have landed when at most the next stage's pieces are outstanding (in-order completion)
    if (st + 1 < nst) { if (PRO) asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* Ws = Wring + SET * 4096 + fr * 256;
    bf16x8 wf[4], af[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) wf[s4] = *reinterpret_cast<const bf16x8*>(Ws + foff[s4]);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      if (PRO) {
#pragma unroll
        for (int e = 0; e < 8; ++e) af[s4][e] = f2bf(rbf((float)ax[SET][s4][e] * ri) * (float)ag[SET][s4][e]);
      } else {
        af[s4] = ax[SET][s4];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // fragments are in registers: the slot may be overwritten
    if (st + 2 < nst) { load_a(st + 2, SET); dma_stage(st + 2, SET); }
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      if (s4 & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s4], af[s4], acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s4], af[s4], acc0, 0, 0, 0);
    }
  };
  {
    int st = 0;
    for (; st + 1 < nst; st += 2) {
      stage_body(st, std::integral_constant<int, 0>{});
      stage_body(st + 1, std::integral_constant<int, 1>{});
    }
    if (st < nst) stage_body(st, std::integral_constant<int, 0>{});
  }
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = acc0[r] + acc1[r];
  f32x4 u = {0.f, 0.f, 0.f, 0.f};
  if (nw > 1) {
    // the K slices meet in LDS: the tile's first wave sums them in slice order (deterministic) and finishes the tile
    *reinterpret_cast<f32x4*>(red + (wave * 64 + lane) * 4) = v;
    __syncthreads();
    if (wave != 0) return;
    v = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s8 = 0; s8 < slices; ++s8) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(red + ((s8 * tiles_pb) * 64 + lane) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += x[r];
      if (swiglu) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(red + ((s8 * 2 + 1) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] += y[r];
      }
    }
  }
  gemv_finish(p, v, u, blockIdx.x * tiles_pb * 16, lane, swiglu);
}

}  // namespace

// ------------------------------------------------------------------------------------
// Decode GEMV dispatch: one pure function decides (the plan), one executor launches it.
//
// gemv_plan takes values only -- shape, epilogue (with the internal GEMV_EPI_* bits), weight format, RMSNorm prologue, whether the
// in-block form can address the caller's pointers, the CU count -- and names the one launch of the problem: kernel, template form,
// grid, block, dynamic LDS and the split values the executor copies into the kernel arguments; or no kernel at all.  a3v_gemv_plan
// is the same function as a C-ABI query.  gemv_execute is the only code that launches the family's kernels, gemv_run the only code
// that checks an entry point's arguments.  The plan is pinned, row for row, to what commit de04e97 -- the last one that decided and
// launched in one piece -- launched (profiles/gemv_dispatch_de04e97.tsv, tests/test_gemv_plan_cpu.py).
//
// Where the entry points genuinely differ (kept as they were, return codes included):
//   * bf16 (a3v_gemm_skinny) takes any K % 32 == 0: what the LDS-DMA kernels cannot run (K % 128, N > 65536, more than 150 KiB of
//     LDS, SwiGLU without a split) falls back to the direct-to-VGPR kernel, which ignores the workspace;
//   * fp8 / NF4 need K % 256 == 0 and ldw % 16 == 0 (ldw in bytes) and have no fallback: A3V_ERR_SHAPE where no kernel can run;
//   * NF4 additionally needs ldw >= K / 2 and Wq, scales and A 16-byte aligned (the scale DMA and the 8-byte fragment reads);
//   * the fused decode-step form (a3v_gemv_fused) needs K % 128 == 0 and N % 16 == 0, checks neither strides nor epilogue bits (its
//     one caller passes its own buffers), has no fallback either -- the direct kernel has no prologue / RoPE / SSQ form -- and
//     answers A3V_ERR_SHAPE where the public forms answer A3V_ERR_ARG for M or a missing workspace;
//   * a failed opt-in to more than 64 KiB of LDS is a fallback for bf16 and A3V_ERR_SHAPE for the others.
// ------------------------------------------------------------------------------------
struct GemvPlan {       // the A3V_GEMV_PLAN_INTS fields of a3v_gemv_plan
  int32_t kernel;       // A3V_GEMV_K_*, or GEMV_K_NONE
  int32_t arows, pro, format;          // template form: gemv_dma_bf16_kernel<arows, pro, fp8, nf4>, gemv_kq_bf16_kernel<pro>
  int32_t grid_x, block, lds_bytes;
  int32_t S, nkb, tgs, maxkb;          // GemvArgs: K slices of the across-blocks plan, 128-k blocks, 64-row groups, 128-k blocks of A per slice
  int32_t slices;                      // K slices inside the block (KQ), else S
  int32_t kslice;                      // Skinny1Args: k elements per wave (direct kernels)
};
static_assert(sizeof(GemvPlan) == A3V_GEMV_PLAN_INTS * sizeof(int32_t), "a3v_gemv_plan copies the plan as int32 fields");
constexpr int GEMV_K_NONE = -1;
constexpr int GEMV_LDS_LIMIT = 150 * 1024;

// k elements per ring stage of W: a stage is 16 rows x 256 B of bf16, x 256 B of fp8 or x 128 B of nibbles
static int gemv_kst(int format) { return format == A3V_GEMV_BF16 ? 128 : 256; }
static int gemv_tgs(int N) { return (N + 63) / 64; }

// split-K factor of the DMA GEMV: enough blocks (row groups x S >= A3V_GEMV_BLOCKS) for 256 CUs, S <= 8, S <= number of ring stages
static int gemv_split(int N, int K, int kst) {
  const int tgs = gemv_tgs(N), nst = K / kst;
  // block target of the split: 768 measured best in the decode bench of the 7B geometry (qkv: 4 slices instead of 8, LM head 2 instead
  // of 4; +2-3 % decode tok/s, +6 % with fp8 weights; 640 / 896 / 1024 / 1536 all slower)
  constexpr int A3V_GEMV_BLOCKS = 768;
  constexpr int A3V_GEMV_MAXS = 8;      // the fix-up reloads at most eight partials in one round trip
  int S = 1;
  while (S < A3V_GEMV_MAXS && tgs * S < A3V_GEMV_BLOCKS && S * 2 <= nst) S *= 2;
  return S;
}

// the direct-to-VGPR form (bf16 weights, any K % 32 == 0, no fused form): 8 waves split K in 32-element granules, LDS reduction
static GemvPlan gemv_plan_direct(int M, int N, int K, int epi, int format, bool pro) {
  GemvPlan pl{};
  pl.kernel = GEMV_K_NONE; pl.format = format; pl.pro = pro;
  if (format != A3V_GEMV_BF16 || pro || (epi & (GEMV_EPI_ROPEKV | GEMV_EPI_SSQ)) || K % 32 || M > 16) return pl;
  const bool sw = (epi & A3V_EPI_SWIGLU) != 0;
  pl.kernel = sw ? A3V_GEMV_K_DIRECT2 : A3V_GEMV_K_DIRECT1;
  pl.grid_x = sw ? (N + 31) / 32 : (N + 15) / 16; pl.block = 512;
  pl.kslice = ((K / 32 + 7) / 8) * 32;
  return pl;
}

static GemvPlan gemv_plan(int M, int N, int K, int epi, int format, bool pro, bool inblock_ok, int cus) {
  const int kst = gemv_kst(format);
  // can the LDS-DMA GEMV take this problem (else: the direct-to-VGPR kernel, which has no fused decode / fp8 / NF4 forms)
  if (K % kst || K < kst || N > 65536 || M > 16) return gemv_plan_direct(M, N, K, epi, format, pro);
  GemvPlan pl{};
  pl.format = format; pl.pro = pro; pl.arows = M <= 8 ? 8 : 16;
  pl.S = gemv_split(N, K, kst); pl.nkb = K / 128; pl.tgs = gemv_tgs(N);
  pl.maxkb = ((K / kst + pl.S - 1) / pl.S) * (kst / 128);
  pl.slices = pl.S;
  const bool sw = (epi & A3V_EPI_SWIGLU) != 0;
  const size_t ldsb = (size_t)pl.maxkb * pl.arows * 256 + 4 * 2 * 4096;     // the block's A slice + four wave rings of two 4-KiB stages
  if (ldsb > (size_t)GEMV_LDS_LIMIT || (sw && pl.S == 1)) return gemv_plan_direct(M, N, K, epi, format, pro);
  // M <= 8, bf16 weights: the K slices as the waves of ONE block per 16-row tile (gemv_kq_bf16_kernel: the partials meet in LDS,
  // no split-K fix-up through HBM); same slice count as the across-blocks plan.  A3V_GEMV_KQ=0: the across-blocks kernel (A/B runs)
  // A3V_GEMV_KQ: 1 (default) = where it was measured to win: no RMSNorm prologue, no SwiGLU, and the 16-row tiles spread EVENLY over the
  // CUs (one or two blocks each: 7B wo / w2 = 256 tiles: 11.5 -> 10.4 us, 19.4 -> 19.6) -- a block of 8 waves is a coarse unit, 320
  // tiles (13B wo / w2) leave a quarter of the CUs with twice the work (15.1 -> 18.0 us, 32.0 -> 38.8: tools/ab_gemv_kq.py);
  // 2 = every bf16 GEMV with M <= 8 (A/B runs); 0 = none
  const int kq_mode = A3V_ENV_INT("A3V_GEMV_KQ", 1);
  const int tiles = N / 16;
  const bool kq_even = !pro && !sw && tiles % cus == 0 && tiles <= 2 * cus;
  if (format == A3V_GEMV_BF16 && pl.arows == 8 && (kq_mode == 2 || (kq_mode == 1 && kq_even)) && N % 16 == 0 && inblock_ok &&
      (!sw || tiles % 2 == 0)) {
    int slices = pl.S;
    if (sw && slices > 6) slices = 6;       // 12 waves = the kernel's launch bound of 768 threads
    while (slices > 1 && pl.nkb < 2 * slices) --slices;
    const int nw = slices * (sw ? 2 : 1);
    pl.kernel = A3V_GEMV_K_KQ; pl.slices = slices;
    pl.grid_x = sw ? tiles / 2 : tiles; pl.block = nw * 64; pl.lds_bytes = nw * (2 * 4096 + 1024);
    return pl;
  }
  pl.kernel = A3V_GEMV_K_DMA;
  pl.grid_x = ((pl.tgs + 7) / 8) * 8 * pl.S; pl.block = 256; pl.lds_bytes = (int32_t)ldsb;
  return pl;
}

extern "C" int a3v_gemv_plan(int M, int N, int K, int epilogue, int format, int prologue, int rope, int ssq, int inblock_ok, int cus,
                             int32_t* plan) {
  if (M <= 0 || M > 16 || N <= 0 || K <= 0 || cus <= 0 || format < A3V_GEMV_BF16 || format > A3V_GEMV_NF4 || !plan) return A3V_ERR_ARG;
  const int epi = epilogue | (rope ? GEMV_EPI_ROPEKV : 0) | (ssq ? GEMV_EPI_SSQ : 0);
  const GemvPlan pl = gemv_plan(M, N, K, epi, format, prologue != 0, inblock_ok != 0, cus);
  if (pl.kernel == GEMV_K_NONE) return A3V_ERR_SHAPE;
  memcpy(plan, &pl, sizeof(pl));
  return pl.kernel;
}

// can the LDS-DMA GEMV take this problem: what a3v_llama_decode_step asks before it commits to the fused form (w8: fp8 or NF4 images)
bool a3v_gemv_supported(int M, int N, int K, int epilogue, int w8) {
  const int k = gemv_plan(M, N, K, epilogue, w8 ? A3V_GEMV_FP8 : A3V_GEMV_BF16, false, false, a3v_cu_count()).kernel;
  return k == A3V_GEMV_K_DMA || k == A3V_GEMV_K_KQ;
}

extern "C" int a3v_gemm_skinny_split(int M, int N, int K) {
  (void)M;
  const int kst = gemv_kst(A3V_GEMV_BF16);
  return (K % kst == 0 && K >= kst) ? gemv_split(N, K, kst) : 1;
}

extern "C" int64_t a3v_gemm_skinny_ws_bytes(int M, int N, int K) {
  (void)M;
  const int kst = gemv_kst(A3V_GEMV_BF16);
  if (K % kst || K < kst) return A3V_WS_PARTIALS;
  return A3V_WS_PARTIALS + (int64_t)gemv_tgs(N) * 8 * 4 * 1024;     // sized for the largest split of either weight format
}

// ---- the executor: the only code that launches the kernels of the family.  `g` holds the caller's pointers, strides, shape and
// epilogue; the split values and the workspace pointers come from the plan.  false: the opt-in to the plan's LDS failed. ----
static bool gemv_execute(const GemvPlan& pl, GemvArgs g, void* ws, hipStream_t st) {
  const dim3 grid(pl.grid_x), block(pl.block);
  if (pl.kernel == A3V_GEMV_K_DIRECT1 || pl.kernel == A3V_GEMV_K_DIRECT2) {
    Skinny1Args q{};
    q.A = g.A; q.W = g.W; q.C = g.C; q.res = g.res;
    q.lda = g.lda; q.ldw = g.ldw; q.ldc = g.ldc; q.ldr = g.ldr;
    q.M = g.M; q.N = g.N; q.K = g.K; q.epi = g.epi; q.kslice = pl.kslice;
    if (pl.kernel == A3V_GEMV_K_DIRECT2) hipLaunchKernelGGL(gemm_skinny1_bf16_kernel<2>, grid, block, 0, st, q);
    else hipLaunchKernelGGL(gemm_skinny1_bf16_kernel<1>, grid, block, 0, st, q);
    return true;
  }
  g.counters = (int*)ws;
  g.part = (float*)((char*)ws + A3V_WS_PARTIALS);
  g.S = pl.S; g.nkb = pl.nkb; g.tgs = pl.tgs; g.maxkb = pl.maxkb;
  static bool attr_done[A3V_MAX_DEV][14] = {};
  void (*kern)(GemvArgs);
  int slot = (pl.arows == 16 ? 2 : 0) + (pl.pro ? 1 : 0);
  if (pl.kernel == A3V_GEMV_K_KQ) {
    kern = pl.pro ? gemv_kq_bf16_kernel<true> : gemv_kq_bf16_kernel<false>;
    slot += 12;
  } else {
    switch (pl.format * 4 + slot) {
      case 0: kern = gemv_dma_bf16_kernel<8, false, false>; break;
      case 1: kern = gemv_dma_bf16_kernel<8, true, false>; break;
      case 2: kern = gemv_dma_bf16_kernel<16, false, false>; break;
      case 3: kern = gemv_dma_bf16_kernel<16, true, false>; break;
      case 4: kern = gemv_dma_bf16_kernel<8, false, true>; break;
      case 5: kern = gemv_dma_bf16_kernel<8, true, true>; break;
      case 6: kern = gemv_dma_bf16_kernel<16, false, true>; break;
      case 7: kern = gemv_dma_bf16_kernel<16, true, true>; break;
      case 8: kern = gemv_dma_bf16_kernel<8, false, false, true>; break;
      case 9: kern = gemv_dma_bf16_kernel<8, true, false, true>; break;
      case 10: kern = gemv_dma_bf16_kernel<16, false, false, true>; break;
      default: kern = gemv_dma_bf16_kernel<16, true, false, true>; break;
    }
    slot += pl.format * 4;
  }
  if (a3v_dyn_lds_once(attr_done, slot, (const void*)kern, GEMV_LDS_LIMIT) != 0) return false;
  hipLaunchKernelGGL(kern, grid, block, pl.lds_bytes, st, g);
  return true;
}

// what a3v_gemv_fused adds to a public call (see there)
struct GemvFused {
  const void* norm_w; const float* ssq_in; float eps; float* ssq_out;
  int rope; const float* cos_sin; void* k_cache; void* vt_cache;
  int H, Hkv, hd, Smax, pos;
};

// the one argument check, plan and launch behind a3v_gemm_skinny / _fp8 / _nf4 (fx == NULL) and a3v_gemv_fused
static int gemv_run(int format, const void* A, int64_t lda, const void* W, int64_t ldw, const float* wscale, void* C, int64_t ldc,
                    int M, int N, int K, const void* residual, int64_t ldr, int epilogue, const GemvFused* fx, void* ws, void* stream) {
  const bool quant = format != A3V_GEMV_BF16;
  if (fx) {
    if (M <= 0 || M > 16 || K % 128 || N % 16 || N > 65536 || !ws) return A3V_ERR_SHAPE;
    if (format == A3V_GEMV_NF4 && (!wscale || K % 256)) return A3V_ERR_ARG;
    if (fx->rope && (fx->hd % 16 || !fx->cos_sin || !fx->k_cache || !fx->vt_cache)) return A3V_ERR_ARG;
  } else {
    if (M <= 0 || M > 16 || N <= 0 || K <= 0 || !A || !W || (quant && !wscale) || !C || !ws) return A3V_ERR_ARG;
    if (K % (quant ? 256 : 32) || lda % 8 || ldw % (quant ? 16 : 8) || N % 4 || ldc % 4) return A3V_ERR_SHAPE;
    if (format == A3V_GEMV_NF4 && (ldw < K / 2 || ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(wscale) |
                                                    reinterpret_cast<uintptr_t>(A)) & 15))) return A3V_ERR_SHAPE;
    if ((epilogue & A3V_EPI_SWIGLU) && (N % 32)) return A3V_ERR_SHAPE;
    if (epilogue & ~(A3V_EPI_RESIDUAL | A3V_EPI_SWIGLU | A3V_EPI_OUT_F32)) return A3V_ERR_ARG;
    if ((epilogue & A3V_EPI_RESIDUAL) && (!residual || (ldr % 4))) return A3V_ERR_ARG;
  }
  GemvArgs g{};
  g.A = (const bf16_t*)A; g.W = (const bf16_t*)W; g.C = C; g.res = residual;
  g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr;
  g.M = M; g.N = N; g.K = K; g.epi = epilogue;
  g.wscale = wscale; g.n4 = format == A3V_GEMV_NF4;
  if (fx) {
    g.epi |= (fx->rope ? GEMV_EPI_ROPEKV : 0) | (fx->ssq_out ? GEMV_EPI_SSQ : 0);
    g.norm_w = (const bf16_t*)fx->norm_w; g.ssq_in = fx->ssq_in; g.eps = fx->eps; g.ssq_tiles = K / 16; g.ssq_out = fx->ssq_out;
    g.cos_sin = fx->cos_sin; g.k_cache = (bf16_t*)fx->k_cache; g.vt_cache = (bf16_t*)fx->vt_cache;
    g.H = fx->H; g.Hkv = fx->Hkv; g.hd = fx->hd; g.Smax = fx->Smax; g.pos = fx->pos;
  }
  // the in-block form reads A (and the norm weights) 16 bytes per lane straight from memory
  const bool inblock_ok = (reinterpret_cast<uintptr_t>(A) & 15) == 0 && lda % 8 == 0 && (reinterpret_cast<uintptr_t>(g.norm_w) & 15) == 0;
  const bool fallback = !quant && !fx;
  GemvPlan pl = gemv_plan(M, N, K, g.epi, format, g.norm_w != nullptr, inblock_ok, a3v_cu_count());
  const bool direct = pl.kernel == A3V_GEMV_K_DIRECT1 || pl.kernel == A3V_GEMV_K_DIRECT2;
  if (pl.kernel == GEMV_K_NONE || (direct && !fallback)) return A3V_ERR_SHAPE;
  if (!gemv_execute(pl, g, ws, (hipStream_t)stream)) {
    if (!fallback) return A3V_ERR_SHAPE;
    gemv_execute(gemv_plan_direct(M, N, K, g.epi, format, false), g, ws, (hipStream_t)stream);
  }
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_gemm_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                               int M, int N, int K, const void* residual, int64_t ldr, int epilogue,
                               void* partial, void* stream) {
  return gemv_run(A3V_GEMV_BF16, A, lda, W, ldw, nullptr, C, ldc, M, N, K, residual, ldr, epilogue, nullptr, partial, stream);
}

// Decode-step forms of the GEMV (the building block of a3v_llama_decode_step; contract in include/a3vlm_hip.h):
//   norm_w != NULL : A is the un-normalised residual rows h; RMSNorm(h) is applied while the A slice is staged (ssq_in)
//   rope != 0      : [q|k|v] rows get RoPE and go to C (q) / the KV cache at `pos` (no separate rope kernel)
//   ssq_out != NULL: with a residual epilogue, also emit the per-tile sums of squares of the new rows
extern "C" int a3v_gemv_fused(const void* A, int64_t lda, const void* W, int64_t ldw, const float* wscale, int n4, void* C, int64_t ldc, int M, int N,
                   int K, const void* residual, int64_t ldr, int epilogue, const void* norm_w, const float* ssq_in, float eps,
                   float* ssq_out, int rope, const float* cos_sin, void* k_cache, void* vt_cache, int H, int Hkv, int hd,
                   int Smax, int pos, void* ws, void* stream) {
  const GemvFused fx{norm_w, ssq_in, eps, ssq_out, rope, cos_sin, k_cache, vt_cache, H, Hkv, hd, Smax, pos};
  return gemv_run(n4 ? A3V_GEMV_NF4 : wscale ? A3V_GEMV_FP8 : A3V_GEMV_BF16, A, lda, W, ldw, wscale, C, ldc, M, N, K, residual, ldr, epilogue,
                  &fx, ws, stream);
}

// Weight-only fp8 (OCP e4m3fn) form of a3v_gemm_skinny: Wq [N, K] bytes (row stride ldw BYTES), wscale [N] fp32;
// C = epilogue((A . dequant(Wq)^T) * wscale).  K % 256 == 0.  BASELINE config 5 / SURVEY 8(a) row Q: no reference oracle
// exists for this path (the reference's quantised path is bitsandbytes NF4, util/quant.py); parity is stated against
// the bf16 GEMV on the dequantised weights.
extern "C" int a3v_gemm_skinny_fp8(const void* A, int64_t lda, const void* Wq, int64_t ldw, const float* wscale, void* C, int64_t ldc,
                                   int M, int N, int K, const void* residual, int64_t ldr, int epilogue, void* workspace, void* stream) {
  return gemv_run(A3V_GEMV_FP8, A, lda, Wq, ldw, wscale, C, ldc, M, N, K, residual, ldr, epilogue, nullptr, workspace, stream);
}

// Weight-only NF4 form of a3v_gemm_skinny (the decode GEMV of the reference's 4-bit mode, util/quant.py:95-163): Wq [N, K/2] nibbles
// (row stride ldw BYTES), scales [N, K/64] fp32 (contiguous rows) as a3v_quantize_nf4 writes them; C = epilogue(sum over 64-k blocks of
// s_b * (A . NF4[q])^T).  K % 256 == 0.
extern "C" int a3v_gemm_skinny_nf4(const void* A, int64_t lda, const void* Wq, int64_t ldw, const float* scales, void* C, int64_t ldc,
                                   int M, int N, int K, const void* residual, int64_t ldr, int epilogue, void* workspace, void* stream) {
  return gemv_run(A3V_GEMV_NF4, A, lda, Wq, ldw, scales, C, ldc, M, N, K, residual, ldr, epilogue, nullptr, workspace, stream);
}
