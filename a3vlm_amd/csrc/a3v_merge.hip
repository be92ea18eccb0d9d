// LoRA merge (a3v_lora_merge): out = round( base + lora_b . lora_a ), the adapters of a fine-tuned model folded into its base matrices
// once, so that the result is a plain model for every inference path.  The arithmetic is stated in include/a3vlm_hip.h and restated in
// fp64 in tests/lora_merge_ref.py.
//
// The kernel streams the base: it reads every base element once and writes it once (HBM bound); lora_b and lora_a are tiny and stay in
// L2 / LDS.  One workgroup (4 waves) owns 64 k-columns and MG_ROWS rows.  The 64-column slice of lora_a [R, K] -- contraction index
// strided -- is parked in LDS transposed ([k][r], r contiguous) once per workgroup; a wave then takes 16 rows x 64 columns per pass with
// v_mfma_f32_16x16x32_bf16 in the orientation   D[k][n] = sum_r  At[k][r] . B[n][r] :
//   A operand (16 k x 32 r)  <- LDS, one 16-B read per lane;     B operand (32 r x 16 n)  <- lora_b rows, one 16-B global load per lane;
//   D: lane (g = lane >> 4, n = lane & 15) holds rows 4g .. 4g+3 of the k axis.
// Which k a D row stands for is the kernel's choice (it only picks the LDS row the A operand is read from): MFMA t of 4 maps D row
// 4g + i to k = 16 g + 4 t + i, so after the four MFMAs a lane holds 16 CONSECUTIVE k of ONE row n: the base is loaded and the result
// stored in 16-B pieces, and the four lane groups of a row cover 128 contiguous bytes.  (The natural mapping k = 16 t + 4 g + i would
// leave 8-B pieces.)  The LDS image is stored in the order it is read -- LDS row 16 t + 4 (k >> 4) + (k & 3) -- so the 16 lanes of a
// group read 16 consecutive LDS rows; with the 16-B row pad these are 16 distinct 16-B bank slots.
// R is padded to a multiple of 32 with zero fragments (R = 8, 16, 24: part of the only contraction step).
// Every output element is read (as base) and written by the same lane and by no other: out == W is safe.
#include "a3v_common.h"

namespace {
constexpr int MG_TK = 64;        // k columns per workgroup (= one NF4 scale block per row)
constexpr int MG_PASSES = 2;     // 16-row passes per wave
constexpr int MG_ROWS = 4 * 16 * MG_PASSES;

__host__ __device__ constexpr int mg_rpad(int R) { return (R + 31) & ~31; }
__host__ __device__ constexpr int mg_pitch(int R) { return mg_rpad(R) + 8; }      // LDS row pitch in elements (+16 B: bank spread)

template <bool NF4>
__global__ __launch_bounds__(256) void lora_merge_bf16_kernel(const bf16_t* W, int64_t ldw, const uint8_t* __restrict__ q,
                                                              const float* __restrict__ scales, const bf16_t* __restrict__ Bm, int64_t ldb,
                                                              const bf16_t* __restrict__ A, int64_t lda, bf16_t* out, int64_t ldo, int N,
                                                              int K, int R) {
  extern __shared__ __attribute__((aligned(16))) bf16_t sAt[];      // [MG_TK][pitch]: lora_a slice, transposed, rows in read order
  __shared__ float tab[16];
  const int t = threadIdx.x;
  const int Rp = mg_rpad(R), pitch = mg_pitch(R);
  const int k0 = blockIdx.x * MG_TK;
  if (NF4 && t < 16) tab[t] = nf4_value(t);
  // stage: lanes run along r (consecutive 2-B LDS addresses of one row per store); rows r >= R and columns k >= K are zeros
  for (int p = t; p < Rp * (MG_TK / 8); p += 256) {
    const int r = p % Rp, c = p / Rp;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16_t)0.f;
    if (r < R && k0 + c * 8 < K) v = *reinterpret_cast<const bf16x8*>(A + (int64_t)r * lda + k0 + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kk = c * 8 + e;
      sAt[(16 * ((kk >> 2) & 3) + 4 * (kk >> 4) + (kk & 3)) * pitch + r] = v[e];
    }
  }
  __syncthreads();
  const int wave = t >> 6, l = t & 63, g = l >> 4, m = l & 15;
#pragma unroll 1
  for (int pass = 0; pass < MG_PASSES; ++pass) {
    const int nb = blockIdx.y * MG_ROWS + (pass * 4 + wave) * 16;     // wave-uniform
    if (nb >= N) break;
    const int n = nb + m;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < Rp; r0 += 32) {                           // ascending r, whatever the base format
      bf16x8 bf;
#pragma unroll
      for (int e = 0; e < 8; ++e) bf[e] = (bf16_t)0.f;
      if (n < N && r0 + 8 * g < R) bf = *reinterpret_cast<const bf16x8*>(Bm + (int64_t)n * ldb + r0 + 8 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(&sAt[(16 * i + m) * pitch + r0 + 8 * g]);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[i], 0, 0, 0);
      }
    }
    if (n >= N) continue;
    const int k = k0 + 16 * g;                                      // this lane: row n, columns k .. k + 15
    float sc = 0.f;
    u32x2 codes = {0u, 0u};
    if (NF4) {                                                      // K % 64 == 0: the whole tile is inside the matrix
      codes = *reinterpret_cast<const u32x2*>(q + (int64_t)n * (K >> 1) + (k >> 1));
      sc = scales[(int64_t)n * (K >> 6) + (k0 >> 6)];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = k + 8 * h;
      if (kk >= K) break;                                           // K % 8 == 0: whole 8-element pieces
      float v[8];
      if (NF4) {
        const uint32_t w = codes[h];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                               // Wd = bf16(NF4[q] * s_b), the bits of a3v_dequantize_nf4
          v[2 * j] = rbf(__fmul_rn(tab[(w >> (8 * j + 4)) & 15], sc));
          v[2 * j + 1] = rbf(__fmul_rn(tab[(w >> (8 * j)) & 15], sc));
        }
      } else {
        load8(W + (int64_t)n * ldw + kk, v);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += acc[2 * h + (e >> 2)][e & 3];
      store8(out + (int64_t)n * ldo + kk, v);                       // the one rounding
    }
  }
}

// fp32 parity form: one thread per 4 consecutive k of one row, r ascending
__global__ __launch_bounds__(256) void lora_merge_f32_kernel(const float* W, int64_t ldw, const float* __restrict__ Bm, int64_t ldb,
                                                             const float* __restrict__ A, int64_t lda, float* out, int64_t ldo, int N, int K,
                                                             int R) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k4 = K >> 2;
  if (idx >= (int64_t)N * k4) return;
  const int64_t n = idx / k4;
  const int k = (int)(idx % k4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    const float b = Bm[n * ldb + r];
    const f32x4 a = *reinterpret_cast<const f32x4*>(A + (int64_t)r * lda + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(b, a[e], acc[e]);
  }
  const f32x4 w = *reinterpret_cast<const f32x4*>(W + n * ldw + k);
  *reinterpret_cast<f32x4*>(out + n * ldo + k) = w + acc;
}

inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
}  // namespace

extern "C" int a3v_lora_merge(const void* W, int64_t ldw, const void* q, const float* scales, const void* B, int64_t ldb, const void* A,
                              int64_t lda, void* out, int64_t ldo, int N, int K, int R, int dtype, void* stream) {
  if (!B || !A || !out) return A3V_ERR_ARG;
  if ((W != nullptr) == (q != nullptr)) return A3V_ERR_ARG;        // exactly one base
  if ((q != nullptr) != (scales != nullptr)) return A3V_ERR_ARG;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  if (q && dtype != A3V_BF16) return A3V_ERR_ARG;                   // the fp32 parity form has no NF4 base
  if (N <= 0 || K <= 0) return A3V_ERR_SHAPE;
  if (R % 8 || R < 8 || R > 256) return A3V_ERR_SHAPE;
  if (K % (q ? 64 : 8)) return A3V_ERR_SHAPE;
  if (ldo % 8 || lda % 8 || ldb % 8 || ldo < K || lda < K || ldb < R) return A3V_ERR_SHAPE;
  if (W && (ldw % 8 || ldw < K)) return A3V_ERR_SHAPE;
  if (misaligned16(B) || misaligned16(A) || misaligned16(out) || (W && misaligned16(W)) || (q && (misaligned16(q) || misaligned16(scales))))
    return A3V_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_F32) {
    const int64_t blocks = ((int64_t)N * (K / 4) + 255) / 256;
    if (blocks > 0x7fffffff) return A3V_ERR_SHAPE;
    hipLaunchKernelGGL(lora_merge_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)W, ldw, (const float*)B, ldb,
                       (const float*)A, lda, (float*)out, ldo, N, K, R);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  const int64_t rows = ((int64_t)N + MG_ROWS - 1) / MG_ROWS;
  if (rows > 65535) return A3V_ERR_SHAPE;
  const dim3 grid((unsigned)((K + MG_TK - 1) / MG_TK), (unsigned)rows);
  const size_t lds = (size_t)MG_TK * mg_pitch(R) * sizeof(bf16_t);  // <= 33 KB at R = 256
  if (q)
    hipLaunchKernelGGL((lora_merge_bf16_kernel<true>), grid, dim3(256), lds, st, (const bf16_t*)nullptr, (int64_t)0, (const uint8_t*)q, scales,
                       (const bf16_t*)B, ldb, (const bf16_t*)A, lda, (bf16_t*)out, ldo, N, K, R);
  else
    hipLaunchKernelGGL((lora_merge_bf16_kernel<false>), grid, dim3(256), lds, st, (const bf16_t*)W, ldw, (const uint8_t*)nullptr,
                       (const float*)nullptr, (const bf16_t*)B, ldb, (const bf16_t*)A, lda, (bf16_t*)out, ldo, N, K, R);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
