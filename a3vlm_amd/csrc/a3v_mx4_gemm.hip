// W4A8 GEMM on the MXFP4 weight images (include/a3vlm_hip.h "MXFP4 weights"): the MXFP8 row quantiser that runs once per product and
// the GEMM for any M on v_mfma_scale_f32_16x16x128_f8f6f4 with the e8m0 block scales of BOTH operands handed to the instruction.
// Restated on the CPU in tests/mx4_gemm_ref.py.  The operand lane map is the one gemv_mx4_kernel (a3v_mx4.hip) measured.
#include "a3v_common.h"

namespace {
typedef __attribute__((ext_vector_type(8))) int i32x8;

// floor(log2(x)) of a finite x > 0 (fp32 denormals included: v_frexp_exp_i32_f32 normalises them)
__device__ __forceinline__ int floor_log2(float x) { return __builtin_amdgcn_frexp_expf(x) - 1; }
__device__ __forceinline__ int clamp_e8m0(int e) { return e < -127 ? -127 : (e > 127 ? 127 : e); }

// ------------------------------------------------------------------------------------
// Rows -> MXFP8: y = the bf16 rows x (NORM = false) or the bf16 RMSNorm output of x (NORM = true: the values rmsnorm_kernel<bf16, bf16,
// bf16> stores -- the same statements in the same order, so the same bits -- never written to memory).  One block per row; a thread
// keeps 8 consecutive k per step, so the four lanes 4 j .. 4 j + 3 hold one 32-k block: its maximum is two lane exchanges, its eight
// codes one 8-byte store, its exponent byte one store of the first lane.
// ------------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(256) void rows_quant_mxfp8_kernel(const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ w,
                                                               uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ ex, int dim,
                                                               float eps) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const bf16_t* xr = x + (int64_t)row * ldx;
  constexpr int MAXV = 8;  // dim <= 256*8*8 = 16384
  float v[MAXV][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (tid + i * 256) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    if (c < dim) {
      load8(xr + c, v[i]);
      if (NORM) {
#pragma unroll
        for (int e = 0; e < 8; ++e) ss = fmaf(v[i][e], v[i][e], ss);
      }
    }
  }
  if (NORM) {
    ss = block_sum<256>(ss, red);
    const float inv = rsqrtf(ss / (float)dim + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = (tid + i * 256) * 8;
      if (c < dim) {
        float wv[8];
        load8(w + c, wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = rbf(rbf(v[i][e] * inv) * wv[e]);
      }
    }
  }
  uint8_t* qr = q + (int64_t)row * ldq;
  uint8_t* er = ex + (int64_t)row * (dim >> 5);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (tid + i * 256) * 8;          // dim % 32 == 0: the four lanes of a block are inside the row or beyond it together
    float mx = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(v[i][e]));
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    if (c < dim) {
      int lo = 0, hi = 0, E = 0;
      if (mx > 0.f) {
        E = clamp_e8m0(floor_log2(mx) - 8);
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = fminf(fmaxf(ldexpf(v[i][e], -E), -448.f), 448.f);   // saturating; the conversion rounds to nearest even
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], hi, true);
      }
      *reinterpret_cast<int2*>(qr + c) = make_int2(lo, hi);
      if ((tid & 3) == 0) er[c >> 5] = (uint8_t)(E + 127);
    }
  }
}

// ------------------------------------------------------------------------------------
// C = epilogue(sum_blocks 2^(ea + ew) * sum_32 a_q * w_q), any M, N % 16 == 0, K % 128 == 0.
// One v_mfma_scale_f32_16x16x128_f8f6f4 takes 128 consecutive k = the four MX blocks c = 0..3 of a 16-row tile of W (first operand, fp4)
// and of a 16-row tile of A (second operand, e4m3).  Lane (fr = lane & 15, fg = lane >> 4): W row fr, block fg: the 16 code bytes at k/2
// = 64 step + 16 fg; A row fr: 16 bytes of block fg >> 1 (half fg & 1) in registers 0-3 and of block 2 + (fg >> 1) in 4-7, i.e. bytes
// 128 step + 16 fg and + 64 of the row: both operands are read in their natural order, 64 contiguous bytes of a row per load
// instruction.  The scale byte of block c of either operand is the one lane group c supplies.  D[n = 4 fg + r][m = fr].
//
// Block = 4 waves, no LDS, no barrier: wave w owns NT 16-row tiles of W (the columns of C) over the whole K and MT 16-row tiles of A,
// MT x NT accumulators.  A tile row of C is MT x 16 <= 128 rows, so up to 128 rows the image is streamed from HBM exactly once; the
// A codes (M x K bytes, L2-resident) are re-read by every wave.  The row tiles of one column tile are neighbours in the grid: above
// 128 rows they meet W in L2.  NT = 2 only with SwiGLU: the wave holds the gate tile and the up tile of its output columns.
// K loop: stages of 512 k (four MFMA steps per accumulator, their loads issued together), then the K % 512 remainder step by step;
// every accumulator sums its steps in k order, so the result depends on (M, N, K, epilogue) alone.  No split-K form.
// ------------------------------------------------------------------------------------
struct Mx4GemmArgs {
  const uint8_t* A;
  const uint8_t* ea;
  const uint8_t* q;
  const uint8_t* s;
  void* C;
  const void* res;
  int64_t lda, ldq, ldc, ldr;
  int M, N, K, epi, mtiles;
};

constexpr int MXG_STAGE = 512, MXG_MAXROWS = 128, MXG_WAVES = 4;

__device__ __forceinline__ f32x4 mxg_mfma(u32x4 w, u32x4 a0, u32x4 a1, f32x4 acc, uint32_t sw, uint32_t sa) {
  const i32x8 wv = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
  const i32x8 av = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv, av, acc, 4, 0, 0, (int)sw, 0, (int)sa);   // scale byte 0 of both operands
}

template <int MT, int NT>
__device__ __forceinline__ void mxg_step(f32x4 (&acc)[MT][NT], const uint8_t* const (&wq)[NT], const uint8_t* const (&ws)[NT],
                                         const uint8_t* const (&aq)[MT], const uint8_t* const (&as)[MT], int step, int fg) {
  u32x4 w[NT];
  uint32_t sw[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    w[j] = *reinterpret_cast<const u32x4*>(wq[j] + (int64_t)step * 64 + fg * 16);
    sw[j] = ws[j][step * 4 + fg];
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const u32x4 a0 = *reinterpret_cast<const u32x4*>(aq[i] + (int64_t)step * 128 + fg * 16);
    const u32x4 a1 = *reinterpret_cast<const u32x4*>(aq[i] + (int64_t)step * 128 + 64 + fg * 16);
    const uint32_t sa = as[i][step * 4 + fg];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = mxg_mfma(w[j], a0, a1, acc[i][j], sw[j], sa);
  }
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void gemm_mx4_kernel(Mx4GemmArgs p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int bm = blockIdx.x % p.mtiles, bn = blockIdx.x / p.mtiles;
  const int n0 = (bn * MXG_WAVES + wave) * 16 * NT;
  if (n0 >= p.N) return;                               // N % (16 NT) == 0: a wave's tiles are inside W or beyond it together
  const int m0 = bm * 16 * MT;
  const int64_t ldsc = p.K >> 5;
  const uint8_t* wq[NT];
  const uint8_t* ws[NT];
  const uint8_t* aq[MT];
  const uint8_t* as[MT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    wq[j] = p.q + (int64_t)(n0 + 16 * j + fr) * p.ldq;
    ws[j] = p.s + (int64_t)(n0 + 16 * j + fr) * ldsc;
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    int m = m0 + 16 * i + fr;
    m = m < p.M ? m : p.M - 1;                         // rows beyond M: row M - 1 again, never stored
    aq[i] = p.A + (int64_t)m * p.lda;
    as[i] = p.ea + (int64_t)m * ldsc;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = p.K >> 7, whole = steps & ~3;
  for (int st = 0; st < whole; st += 4) {
#pragma unroll
    for (int b = 0; b < 4; ++b) mxg_step<MT, NT>(acc, wq, ws, aq, as, st + b, fg);
  }
  for (int st = whole; st < steps; ++st) mxg_step<MT, NT>(acc, wq, ws, aq, as, st, fg);

  // epilogues: the rounding sequences of a3v_gemm_skinny_mxfp4
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + fr;
    if (m >= p.M) continue;
    if (NT == 2) {                                     // SwiGLU: tile 0 the gate rows, tile 1 the up rows of output columns n0 / 2 ..
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f2bf(rbf(silu(rbf(acc[i][0][r]))) * rbf(acc[i][NT - 1][r]));
      *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + (n0 >> 1) + fg * 4) = o;
      continue;
    }
    const int n = n0 + fg * 4;
    float o4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] = rbf(acc[i][0][r]);
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
}

bool mxg_shape_ok(int M, int N, int K, int epilogue) {
  if (M < 1 || N < 16 || N % 16 || N > 65536 || K < 128 || K % 128 || K > 16384) return false;
  if (epilogue & ~(A3V_EPI_RESIDUAL | A3V_EPI_SWIGLU | A3V_EPI_OUT_F32)) return false;
  if ((epilogue & A3V_EPI_SWIGLU) && (epilogue != A3V_EPI_SWIGLU || N % 32)) return false;
  return true;
}

// plan[]: tile rows, tile columns (rows of W per block), K stage in k, grid x, block size, LDS bytes, K slices, K stages of a slice
int mxg_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan) {
  if (!mxg_shape_ok(M, N, K, epilogue) || cus <= 0) return A3V_ERR_SHAPE;
  int rows = 16;                                       // the smallest of 16, 32, 64, 128 rows that holds M: W is read once up to 128 rows
  while (rows < M && rows < MXG_MAXROWS) rows *= 2;
  const int cols = MXG_WAVES * 16 * ((epilogue & A3V_EPI_SWIGLU) ? 2 : 1);
  const int64_t grid = (((int64_t)M + rows - 1) / rows) * ((N + cols - 1) / cols);
  if (grid > 0x7fffffff) return A3V_ERR_SHAPE;
  plan[0] = rows;
  plan[1] = cols;
  plan[2] = MXG_STAGE;
  plan[3] = (int32_t)grid;
  plan[4] = 64 * MXG_WAVES;
  plan[5] = 0;
  plan[6] = 1;
  plan[7] = (K + MXG_STAGE - 1) / MXG_STAGE;
  return A3V_OK;
}

template <int NT>
void mxg_launch(int rows, dim3 g, hipStream_t st, const Mx4GemmArgs& p) {
  switch (rows) {
    case 16: hipLaunchKernelGGL((gemm_mx4_kernel<1, NT>), g, dim3(64 * MXG_WAVES), 0, st, p); break;
    case 32: hipLaunchKernelGGL((gemm_mx4_kernel<2, NT>), g, dim3(64 * MXG_WAVES), 0, st, p); break;
    case 64: hipLaunchKernelGGL((gemm_mx4_kernel<4, NT>), g, dim3(64 * MXG_WAVES), 0, st, p); break;
    default: hipLaunchKernelGGL((gemm_mx4_kernel<8, NT>), g, dim3(64 * MXG_WAVES), 0, st, p); break;
  }
}
}  // namespace

extern "C" int a3v_mx4_gemm_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan) {
  if (!plan) return A3V_ERR_ARG;
  return mxg_plan(M, N, K, epilogue, cus, plan);
}

extern "C" int a3v_quantize_rows_mxfp8(const void* x, int64_t ldx, const void* norm_w, float eps, void* q, int64_t ldq, void* e, int rows,
                                       int K, void* stream) {
  if (!x || !q || !e) return A3V_ERR_ARG;
  if (rows <= 0 || K < 128 || K % 128 || K > 16384 || ldx < K || ldx % 8 || ldq < K || ldq % 8) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(norm_w)) & 15 || reinterpret_cast<uintptr_t>(q) & 7) return A3V_ERR_SHAPE;
  const dim3 g(rows), b(256);
  if (norm_w)
    hipLaunchKernelGGL(rows_quant_mxfp8_kernel<true>, g, b, 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (const bf16_t*)norm_w, (uint8_t*)q,
                       ldq, (uint8_t*)e, K, eps);
  else
    hipLaunchKernelGGL(rows_quant_mxfp8_kernel<false>, g, b, 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (const bf16_t*)nullptr,
                       (uint8_t*)q, ldq, (uint8_t*)e, K, eps);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_gemm_nt_mxfp4(const void* Aq, int64_t lda, const void* ea, const void* q, int64_t ldq, const void* s, void* C, int64_t ldc,
                                 int M, int N, int K, const void* residual, int64_t ldr, int epilogue, void* stream) {
  if (!Aq || !ea || !q || !s || !C) return A3V_ERR_ARG;
  if ((epilogue & A3V_EPI_RESIDUAL) && !residual) return A3V_ERR_ARG;
  int32_t plan[A3V_MX4_GEMM_PLAN_INTS];
  if (mxg_plan(M, N, K, epilogue, a3v_cu_count(), plan) != A3V_OK) return A3V_ERR_SHAPE;
  const int ncol = (epilogue & A3V_EPI_SWIGLU) ? N / 2 : N;
  if (lda < K || lda % 16 || ldq < K / 2 || ldq % 16 || ldc < ncol || ldc % 4) return A3V_ERR_SHAPE;
  if ((epilogue & A3V_EPI_RESIDUAL) && (ldr < N || ldr % 4 || (reinterpret_cast<uintptr_t>(residual) & 7))) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(Aq) | reinterpret_cast<uintptr_t>(q)) & 15) return A3V_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(C) & ((epilogue & A3V_EPI_OUT_F32) ? 15 : 7)) return A3V_ERR_SHAPE;
  Mx4GemmArgs p;
  p.A = (const uint8_t*)Aq; p.ea = (const uint8_t*)ea; p.q = (const uint8_t*)q; p.s = (const uint8_t*)s; p.C = C; p.res = residual;
  p.lda = lda; p.ldq = ldq; p.ldc = ldc; p.ldr = ldr;
  p.M = M; p.N = N; p.K = K; p.epi = epilogue; p.mtiles = (int)(((int64_t)M + plan[0] - 1) / plan[0]);
  const dim3 g((unsigned)plan[3]);
  if (epilogue & A3V_EPI_SWIGLU) mxg_launch<2>(plan[0], g, (hipStream_t)stream, p);
  else mxg_launch<1>(plan[0], g, (hipStream_t)stream, p);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
