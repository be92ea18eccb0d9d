// NF4 weight-only quantisation (the reference's quantised inference mode: bitsandbytes Linear4bit, quant_type "nf4", blocksize 64,
// compress_statistics=True; reference util/quant.py:95-163).  The format is stated in include/a3vlm_hip.h (a3v_quantize_nf4) and restated
// on the CPU in tests/nf4_ref.py.  Quantiser and dequantiser live here; the decode GEMV is the NF4 form of gemv_dma_bf16_kernel
// (a3v_gemm.hip).  Quantisation runs once per model at load time: these kernels are written for clarity, not speed.
#include "a3v_common.h"

namespace {
// bitsandbytes create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8), sorted (exact fp32 values)
__constant__ float kDynMap[256] = {
    -0x1.fc66660000000p-1f, -0x1.f533340000000p-1f, -0x1.ee00000000000p-1f, -0x1.e6cccc0000000p-1f, -0x1.df999a0000000p-1f, -0x1.d866660000000p-1f, -0x1.d133340000000p-1f, -0x1.ca00000000000p-1f,
    -0x1.c2cccc0000000p-1f, -0x1.bb999a0000000p-1f, -0x1.b466660000000p-1f, -0x1.ad33340000000p-1f, -0x1.a600000000000p-1f, -0x1.9ecccc0000000p-1f, -0x1.97999a0000000p-1f, -0x1.9066660000000p-1f,
    -0x1.8933340000000p-1f, -0x1.8200000000000p-1f, -0x1.7acccc0000000p-1f, -0x1.73999a0000000p-1f, -0x1.6c66680000000p-1f, -0x1.6533340000000p-1f, -0x1.5e00000000000p-1f, -0x1.56cccc0000000p-1f,
    -0x1.4f999a0000000p-1f, -0x1.4866680000000p-1f, -0x1.4133340000000p-1f, -0x1.3a00000000000p-1f, -0x1.32cccc0000000p-1f, -0x1.2b999a0000000p-1f, -0x1.2466680000000p-1f, -0x1.1d33340000000p-1f,
    -0x1.1600000000000p-1f, -0x1.0ecccc0000000p-1f, -0x1.0799980000000p-1f, -0x1.0066660000000p-1f, -0x1.f266640000000p-2f, -0x1.e400000000000p-2f, -0x1.d599980000000p-2f, -0x1.c733340000000p-2f,
    -0x1.b8cccc0000000p-2f, -0x1.aa66660000000p-2f, -0x1.9c00000000000p-2f, -0x1.8d99980000000p-2f, -0x1.7f33340000000p-2f, -0x1.70cccc0000000p-2f, -0x1.6266660000000p-2f, -0x1.5400000000000p-2f,
    -0x1.4599980000000p-2f, -0x1.3733340000000p-2f, -0x1.28cccc0000000p-2f, -0x1.1a66680000000p-2f, -0x1.0c00000000000p-2f, -0x1.fb33320000000p-3f, -0x1.de66660000000p-3f, -0x1.c1999a0000000p-3f,
    -0x1.a4cccc0000000p-3f, -0x1.8800000000000p-3f, -0x1.6b33340000000p-3f, -0x1.4e66660000000p-3f, -0x1.31999a0000000p-3f, -0x1.14cccc0000000p-3f, -0x1.f000000000000p-4f, -0x1.b666680000000p-4f,
    -0x1.93d70a0000000p-4f, -0x1.8851ee0000000p-4f, -0x1.7cccce0000000p-4f, -0x1.7147ae0000000p-4f, -0x1.65c2900000000p-4f, -0x1.5a3d700000000p-4f, -0x1.4eb8540000000p-4f, -0x1.4333340000000p-4f,
    -0x1.37ae140000000p-4f, -0x1.2c28f60000000p-4f, -0x1.20a3d60000000p-4f, -0x1.151eba0000000p-4f, -0x1.09999a0000000p-4f, -0x1.fc28f60000000p-5f, -0x1.e51eba0000000p-5f, -0x1.ce147a0000000p-5f,
    -0x1.b70a3e0000000p-5f, -0x1.a000000000000p-5f, -0x1.88f5c20000000p-5f, -0x1.71eb860000000p-5f, -0x1.5ae1460000000p-5f, -0x1.43d70a0000000p-5f, -0x1.2cccce0000000p-5f, -0x1.15c2900000000p-5f,
    -0x1.fd70a40000000p-6f, -0x1.cf5c2a0000000p-6f, -0x1.a147ae0000000p-6f, -0x1.7333340000000p-6f, -0x1.451eba0000000p-6f, -0x1.170a3e0000000p-6f, -0x1.d1eb860000000p-7f, -0x1.75c2900000000p-7f,
    -0x1.3e76c80000000p-7f, -0x1.2c08300000000p-7f, -0x1.19999a0000000p-7f, -0x1.072b020000000p-7f, -0x1.e978d40000000p-8f, -0x1.c49ba60000000p-8f, -0x1.9fbe760000000p-8f, -0x1.7ae1480000000p-8f,
    -0x1.56041a0000000p-8f, -0x1.3126e80000000p-8f, -0x1.0c49ba0000000p-8f, -0x1.ced9140000000p-9f, -0x1.851eb80000000p-9f, -0x1.3b645a0000000p-9f, -0x1.e353f80000000p-10f, -0x1.4fdf3a0000000p-10f,
    -0x1.eecbfe0000000p-11f, -0x1.b3d07c0000000p-11f, -0x1.78d5000000000p-11f, -0x1.3dd9820000000p-11f, -0x1.02de020000000p-11f, -0x1.8fc5060000000p-12f, -0x1.19ce0a0000000p-12f, -0x1.47ae160000000p-13f,
    -0x1.743e960000000p-14f, -0x1.15df660000000p-14f, -0x1.6f00680000000p-15f, -0x1.64840c0000000p-16f, -0x1.040bfe0000000p-17f, -0x1.b435280000000p-19f, -0x1.27476e0000000p-21f, 0x0.0p+0f,
    0x1.27476e0000000p-21f, 0x1.b435280000000p-19f, 0x1.040bfe0000000p-17f, 0x1.64840c0000000p-16f, 0x1.6f00680000000p-15f, 0x1.15df660000000p-14f, 0x1.743e960000000p-14f, 0x1.47ae160000000p-13f,
    0x1.19ce0a0000000p-12f, 0x1.8fc5060000000p-12f, 0x1.02de020000000p-11f, 0x1.3dd9820000000p-11f, 0x1.78d5000000000p-11f, 0x1.b3d07c0000000p-11f, 0x1.eecbfe0000000p-11f, 0x1.4fdf3a0000000p-10f,
    0x1.e353f80000000p-10f, 0x1.3b645a0000000p-9f, 0x1.851eb80000000p-9f, 0x1.ced9140000000p-9f, 0x1.0c49ba0000000p-8f, 0x1.3126e80000000p-8f, 0x1.56041a0000000p-8f, 0x1.7ae1480000000p-8f,
    0x1.9fbe760000000p-8f, 0x1.c49ba60000000p-8f, 0x1.e978d40000000p-8f, 0x1.072b020000000p-7f, 0x1.19999a0000000p-7f, 0x1.2c08300000000p-7f, 0x1.3e76c80000000p-7f, 0x1.75c2900000000p-7f,
    0x1.d1eb860000000p-7f, 0x1.170a3e0000000p-6f, 0x1.451eba0000000p-6f, 0x1.7333340000000p-6f, 0x1.a147ae0000000p-6f, 0x1.cf5c2a0000000p-6f, 0x1.fd70a40000000p-6f, 0x1.15c2900000000p-5f,
    0x1.2cccce0000000p-5f, 0x1.43d70a0000000p-5f, 0x1.5ae1460000000p-5f, 0x1.71eb860000000p-5f, 0x1.88f5c20000000p-5f, 0x1.a000000000000p-5f, 0x1.b70a3e0000000p-5f, 0x1.ce147a0000000p-5f,
    0x1.e51eba0000000p-5f, 0x1.fc28f60000000p-5f, 0x1.09999a0000000p-4f, 0x1.151eba0000000p-4f, 0x1.20a3d60000000p-4f, 0x1.2c28f60000000p-4f, 0x1.37ae140000000p-4f, 0x1.4333340000000p-4f,
    0x1.4eb8540000000p-4f, 0x1.5a3d700000000p-4f, 0x1.65c2900000000p-4f, 0x1.7147ae0000000p-4f, 0x1.7cccce0000000p-4f, 0x1.8851ee0000000p-4f, 0x1.93d70a0000000p-4f, 0x1.b666680000000p-4f,
    0x1.f000000000000p-4f, 0x1.14cccc0000000p-3f, 0x1.31999a0000000p-3f, 0x1.4e66660000000p-3f, 0x1.6b33340000000p-3f, 0x1.8800000000000p-3f, 0x1.a4cccc0000000p-3f, 0x1.c1999a0000000p-3f,
    0x1.de66660000000p-3f, 0x1.fb33320000000p-3f, 0x1.0c00000000000p-2f, 0x1.1a66680000000p-2f, 0x1.28cccc0000000p-2f, 0x1.3733340000000p-2f, 0x1.4599980000000p-2f, 0x1.5400000000000p-2f,
    0x1.6266660000000p-2f, 0x1.70cccc0000000p-2f, 0x1.7f33340000000p-2f, 0x1.8d99980000000p-2f, 0x1.9c00000000000p-2f, 0x1.aa66660000000p-2f, 0x1.b8cccc0000000p-2f, 0x1.c733340000000p-2f,
    0x1.d599980000000p-2f, 0x1.e400000000000p-2f, 0x1.f266640000000p-2f, 0x1.0066660000000p-1f, 0x1.0799980000000p-1f, 0x1.0ecccc0000000p-1f, 0x1.1600000000000p-1f, 0x1.1d33340000000p-1f,
    0x1.2466680000000p-1f, 0x1.2b999a0000000p-1f, 0x1.32cccc0000000p-1f, 0x1.3a00000000000p-1f, 0x1.4133340000000p-1f, 0x1.4866680000000p-1f, 0x1.4f999a0000000p-1f, 0x1.56cccc0000000p-1f,
    0x1.5e00000000000p-1f, 0x1.6533340000000p-1f, 0x1.6c66680000000p-1f, 0x1.73999a0000000p-1f, 0x1.7acccc0000000p-1f, 0x1.8200000000000p-1f, 0x1.8933340000000p-1f, 0x1.9066660000000p-1f,
    0x1.97999a0000000p-1f, 0x1.9ecccc0000000p-1f, 0x1.a600000000000p-1f, 0x1.ad33340000000p-1f, 0x1.b466660000000p-1f, 0x1.bb999a0000000p-1f, 0x1.c2cccc0000000p-1f, 0x1.ca00000000000p-1f,
    0x1.d133340000000p-1f, 0x1.d866660000000p-1f, 0x1.df999a0000000p-1f, 0x1.e6cccc0000000p-1f, 0x1.ee00000000000p-1f, 0x1.f533340000000p-1f, 0x1.fc66660000000p-1f, 0x1.0000000000000p+0f,
};

// nearest NF4 code of x (first minimum on ties, as argmin)
__device__ __forceinline__ int nf4_nearest(float x) {
  int best = 0;
  float bd = fabsf(x - nf4_value(0));
#pragma unroll
  for (int i = 1; i < 16; ++i) {
    const float d = fabsf(x - nf4_value(i));
    if (d < bd) { bd = d; best = i; }
  }
  return best;
}

// one thread per 64-weight block: absmax and the 32 bytes of codes
__global__ __launch_bounds__(256) void nf4_codes_kernel(const bf16_t* __restrict__ W, int64_t nblk, uint8_t* __restrict__ q,
                                                        float* __restrict__ absmax) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  const bf16x8* src = reinterpret_cast<const bf16x8*>(W + b * 64);
  bf16x8 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = src[i];
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)v[i][e]));
  absmax[b] = am;
  const float r = am > 0.f ? 1.0f / am : 0.f;        // correctly rounded fp32 reciprocal, then a product (kQuantizeBlockwise)
  u32x4 o[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int hi = am > 0.f ? nf4_nearest(__fmul_rn((float)v[i][2 * j], r)) : 7;
      const int lo = am > 0.f ? nf4_nearest(__fmul_rn((float)v[i][2 * j + 1], r)) : 7;
      w |= (uint32_t)((hi << 4) | lo) << (8 * j);     // earlier element in the high nibble
    }
    o[i >> 2][i & 3] = w;
  }
  u32x4* dst = reinterpret_cast<u32x4*>(q + b * 32);
  dst[0] = o[0];
  dst[1] = o[1];
}

// offset = mean(absmax) over the module: one workgroup, fp64 sum in a fixed order (deterministic), rounded once to fp32
__global__ __launch_bounds__(1024) void nf4_offset_kernel(const float* __restrict__ absmax, int64_t nblk, float* __restrict__ offset) {
  __shared__ double part[1024];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += 1024) s += (double)absmax[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *offset = (float)(part[0] / (double)nblk);
}

// second level: one workgroup per group of 256 blocks -> effective scale s_b = map[qa_b] * absmax2_g + offset
__global__ __launch_bounds__(256) void nf4_scales_kernel(const float* __restrict__ absmax, const float* __restrict__ offset, int64_t nblk,
                                                         float* __restrict__ scales) {
  __shared__ float wmax[4];
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float off = *offset;
  const float am = b < nblk ? absmax[b] : 0.f;
  const float d = b < nblk ? __fsub_rn(am, off) : 0.f;
  float m = fabsf(d);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  const float a2 = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const float r = a2 > 0.f ? 1.0f / a2 : 0.f;
  const float x = __fmul_rn(d, r);
  int best = 0;
  float bd = fabsf(x - kDynMap[0]);
  for (int i = 1; i < 256; ++i) {
    const float e = fabsf(x - kDynMap[i]);
    if (e < bd) { bd = e; best = i; }
  }
  if (b < nblk) scales[b] = am == 0.f ? 0.f : __fadd_rn(__fmul_rn(kDynMap[best], a2), off);   // no fma: dequantize_4bit rounds twice
}

// Wd = bf16(NF4[q] * s_b): one thread per 8 codes
__global__ __launch_bounds__(256) void nf4_dequant_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scales,
                                                          bf16_t* __restrict__ Wd, int64_t ldd, int K, int64_t n8) {
  __shared__ float tab[16];
  if (threadIdx.x < 16) tab[threadIdx.x] = nf4_value(threadIdx.x);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n8) return;
  const int64_t e0 = t * 8;
  const int64_t n = e0 / K, k = e0 % K;
  const uint32_t w = reinterpret_cast<const uint32_t*>(q)[t];
  const float s = scales[e0 / 64];
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[2 * j] = f2bf(__fmul_rn(tab[(w >> (8 * j + 4)) & 15], s));
    o[2 * j + 1] = f2bf(__fmul_rn(tab[(w >> (8 * j)) & 15], s));
  }
  *reinterpret_cast<bf16x8*>(Wd + n * ldd + k) = o;
}

// ---- streaming dequantiser of the QLoRA training step (a3v_dequantize_nf4_images): runs two to three times per layer per step.
// One workgroup owns a 64-row x 128-k tile: every thread reads 16 B of codes (32 weights of one row, inside one scale block) and one
// scale, rounds exactly as nf4_dequant_kernel (__fmul_rn of the fp32 code-book value, then f2bf: the bf16 v_perm tables of the decode
// GEMV hold the code book ROUNDED to bf16 and cannot give these bits, so the 16 fp32 entries sit in LDS: one ds_read_b32 per weight,
// 16 distinct dwords whatever the codes), and parks the tile in LDS twice: row-major (272-B pitch) for Wd and transposed (144-B
// pitch) for Wt.  Both are then stored with 16-B pieces that are contiguous along the destination's rows (256 B per Wd row, 128 B
// per Wt row).  The transposed tile is written with 2-byte LDS stores (32 per thread); lanes of one store differ in the k-segment s
// (k rows 32 s apart: the same bank at every pitch) and in the row, so the column is XOR-ed with 16 s (whole 16-B pieces move, banks
// shift by 8 s); two lanes still share each dword.  By the bank rule that layout should not serialise; no counter has been read and
// the kernel has not been timed (tools/qlora_bench.py).  If it comes in under the copy rate, the 2-byte stores are the first suspect:
// pack row pairs into ds_write_b32.  The algorithm needs ~2.56 B of HBM traffic per weight for both images.
constexpr int QI_TN = 64, QI_TK = 128, QI_DP = QI_TK + 8, QI_TP = QI_TN + 8;     // tile and LDS pitches (elements)

template <bool HAS_D, bool HAS_T>
__global__ __launch_bounds__(256) void nf4_images_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scales,
                                                         bf16_t* __restrict__ Wd, int64_t ldd, bf16_t* __restrict__ Wt, int64_t ldt,
                                                         int N, int K) {
  __shared__ float tab[16];
  __shared__ __attribute__((aligned(16))) bf16_t sD[HAS_D ? QI_TN * QI_DP : 8];
  __shared__ __attribute__((aligned(16))) bf16_t sT[HAS_T ? QI_TK * QI_TP : 8];
  const int t = threadIdx.x;
  if (t < 16) tab[t] = nf4_value(t);
  __syncthreads();
  const int n0 = blockIdx.x * QI_TN, k0 = blockIdx.y * QI_TK;
  const int r = t >> 2, s = t & 3;                     // tile row, 32-wide k segment
  const int n = n0 + r, k = k0 + s * 32;
  bf16x8 v[4];
  if (n < N && k < K) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(q + (int64_t)n * (K >> 1) + (k >> 1));
    const float sc = scales[(int64_t)n * (K >> 6) + (k >> 6)];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[d][2 * j] = f2bf(__fmul_rn(tab[(w[d] >> (8 * j + 4)) & 15], sc));
        v[d][2 * j + 1] = f2bf(__fmul_rn(tab[(w[d] >> (8 * j)) & 15], sc));
      }
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[d][e] = (bf16_t)0.f;
  }
  if (HAS_D) {
#pragma unroll
    for (int d = 0; d < 4; ++d) *reinterpret_cast<bf16x8*>(&sD[r * QI_DP + s * 32 + d * 8]) = v[d];
  }
  if (HAS_T) {
    const int col = r ^ (s << 4);
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 8; ++e) sT[(s * 32 + d * 8 + e) * QI_TP + col] = v[d][e];
  }
  __syncthreads();
  if (HAS_D) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 16 + (t >> 4), c = t & 15;
      const int nn = n0 + row, kk = k0 + c * 8;
      if (nn < N && kk < K) *reinterpret_cast<bf16x8*>(Wd + (int64_t)nn * ldd + kk) = *reinterpret_cast<const bf16x8*>(&sD[row * QI_DP + c * 8]);
    }
  }
  if (HAS_T) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int kr = it * 32 + (t >> 3), c = t & 7;
      const int kk = k0 + kr, nn = n0 + c * 8;
      if (kk < K && nn < N) {
        const bf16x8 o = *reinterpret_cast<const bf16x8*>(&sT[kr * QI_TP + ((c ^ ((kr >> 5) << 1)) << 3)]);
        bf16_t* dst = Wt + (int64_t)kk * ldt + nn;
        if (nn + 8 <= N) {
          *reinterpret_cast<bf16x8*>(dst) = o;
        } else {                                       // ragged last piece of a row: only the N columns of the window are written
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (nn + e < N) dst[e] = o[e];
        }
      }
    }
  }
}
}  // namespace

extern "C" int64_t a3v_quantize_nf4_ws_bytes(int N, int K) {
  if (N <= 0 || K <= 0 || K % 64) return 0;
  return 256 + (int64_t)N * (K / 64) * 4;
}

extern "C" int a3v_quantize_nf4(const void* W, int N, int K, void* q, float* scales, float* ws, void* stream) {
  if (!W || !q || !scales || !ws) return A3V_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 64) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(ws)) & 15) return A3V_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = (int64_t)N * (K / 64);
  float* offset = ws;                  // ws[0]: the module offset (read back by the tests)
  float* absmax = ws + 64;
  const unsigned grid = (unsigned)((nblk + 255) / 256);
  hipLaunchKernelGGL(nf4_codes_kernel, dim3(grid), dim3(256), 0, st, (const bf16_t*)W, nblk, (uint8_t*)q, absmax);
  A3V_LAUNCH_CHECK();
  hipLaunchKernelGGL(nf4_offset_kernel, dim3(1), dim3(1024), 0, st, (const float*)absmax, nblk, offset);
  A3V_LAUNCH_CHECK();
  hipLaunchKernelGGL(nf4_scales_kernel, dim3(grid), dim3(256), 0, st, (const float*)absmax, (const float*)offset, nblk, scales);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_dequantize_nf4(const void* q, const float* scales, void* Wd, int64_t ldd, int N, int K, void* stream) {
  if (!q || !scales || !Wd) return A3V_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 64 || ldd < K || ldd % 8) return A3V_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(Wd) & 15) || (reinterpret_cast<uintptr_t>(q) & 3)) return A3V_ERR_SHAPE;
  const int64_t n8 = (int64_t)N * K / 8;
  hipLaunchKernelGGL(nf4_dequant_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q, scales,
                     (bf16_t*)Wd, ldd, K, n8);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_dequantize_nf4_images(const void* q, const float* scales, int N, int K, void* Wd, int64_t ldd, void* Wt, int64_t ldt,
                                         void* stream) {
  if (!q || !scales || (!Wd && !Wt)) return A3V_ERR_ARG;
  if (N <= 0 || K <= 0 || K % 64 || (K + QI_TK - 1) / QI_TK > 65535) return A3V_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(q) & 15) return A3V_ERR_SHAPE;
  if (Wd && (ldd < K || ldd % 8 || (reinterpret_cast<uintptr_t>(Wd) & 15))) return A3V_ERR_SHAPE;
  if (Wt && (ldt < N || ldt % 8 || (reinterpret_cast<uintptr_t>(Wt) & 15))) return A3V_ERR_SHAPE;
  const dim3 grid((unsigned)((N + QI_TN - 1) / QI_TN), (unsigned)((K + QI_TK - 1) / QI_TK));
  hipStream_t st = (hipStream_t)stream;
  if (Wd && Wt)
    hipLaunchKernelGGL((nf4_images_kernel<true, true>), grid, dim3(256), 0, st, (const uint8_t*)q, scales, (bf16_t*)Wd, ldd, (bf16_t*)Wt, ldt, N, K);
  else if (Wd)
    hipLaunchKernelGGL((nf4_images_kernel<true, false>), grid, dim3(256), 0, st, (const uint8_t*)q, scales, (bf16_t*)Wd, ldd, (bf16_t*)nullptr, (int64_t)0, N, K);
  else
    hipLaunchKernelGGL((nf4_images_kernel<false, true>), grid, dim3(256), 0, st, (const uint8_t*)q, scales, (bf16_t*)nullptr, (int64_t)0, (bf16_t*)Wt, ldt, N, K);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
