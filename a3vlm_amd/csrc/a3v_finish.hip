// One launch that finishes every fp32 gradient partial of a LoRA backward (a3v_grad_finish_multi).
//
// A LoRA step leaves ~450 small partial results behind: the split-K planes of the adapter weight gradients (dA strips, dB^T strips)
// and the per-block partial rows of the RMSNorm weight gradients.  Finishing each of them where it is produced costs one or two tiny
// dependent launches per product (a3v_splitk_reduce, a3v_lora_gb_scatter, colsum_add_kernel: 1 - 17 MB each, at the launch floor).
// Nobody reads the finished gradients before the clip and the optimizer, so the producers can leave their partials in a step-long
// arena and ONE launch at the end of the backward walks a device-resident table of jobs (the pattern of a3v_adamw_multi):
//
//   A3V_FINISH_PLANES   dst[r][c] (+)= rbf(sum_s plane[s][r][c])              -- a3v_splitk_reduce<float>, element for element
//   A3V_FINISH_SCATTER  dst_j[n][c] += rbf(sum_s plane[s][j r + c][row0_j + n])   -- a3v_splitk_reduce<float> (store) + a3v_lora_gb_scatter
//   A3V_FINISH_COLSUM   dst[c] += sum_r part[r][c] in 16 row chunks, one atomic per column and chunk   -- colsum_add_kernel
//
// The planes are summed in ascending s from 0.f, rounded to bf16 once and added with one fp32 add; the column sums keep the four
// interleaved accumulators and the (a0 + a1) + (a2 + a3) combine of colsum_add_kernel: every job gives what the kernels it replaces
// give (the plane jobs bit for bit; the column sums up to the order in which the 16 chunk atomics land, as before).
//
// Work units (the table carries each job's first unit; the host computes the same counts, a3vlm_amd/grad_finish.py):
//   PLANES   256 threads x 4 consecutive elements of the row-major [R][N] result            ceil(R (N / 4) / 256)
//   SCATTER  module j, 64 consecutive n: an [r][64] tile goes through LDS and leaves transposed   sum_j ceil(nj / 64)
//   COLSUM   1024 columns x one of the 16 row chunks                                         16 ceil(cols / 1024)
// Blocks stride over the units of the whole table; every global access but the column sums' atomics is 16 bytes wide.
#include "a3v_common.h"

namespace {
constexpr int FIN_TN = 64;          // n per scatter unit
constexpr int FIN_CHUNKS = 16;      // row chunks of a column sum (gridDim.y of colsum_add_kernel)

__device__ __forceinline__ f32x4 plane_sum(const float* __restrict__ p, int64_t plane, int S) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p + (int64_t)s * plane);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += x[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = rbf(a[e]);
  return a;
}

__global__ __launch_bounds__(256) void grad_finish_multi_kernel(const a3v_finish_job* __restrict__ tab, int n_jobs, int64_t total_units) {
  __shared__ float tile[64][FIN_TN + 1];
  const int tid = threadIdx.x;
  for (int64_t u = blockIdx.x; u < total_units; u += gridDim.x) {
    int lo = 0, hi = n_jobs - 1;           // the last job whose first unit is <= u
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].unit0 <= u) lo = mid; else hi = mid - 1;
    }
    const a3v_finish_job* jb = tab + lo;
    const int64_t lu = u - jb->unit0;
    const int kind = (int)jb->kind;
    if (kind == A3V_FINISH_PLANES) {
      const int S = (int)jb->S, R = (int)jb->R, N = (int)jb->N;
      const int64_t n4 = (int64_t)R * (N / 4), i = lu * 256 + tid;
      if (i < n4) {
        const int r = (int)(i / (N / 4)), c = (int)(i % (N / 4)) * 4;
        const f32x4 a = plane_sum(jb->src + (int64_t)r * N + c, (int64_t)R * N, S);
        f32x4* o = reinterpret_cast<f32x4*>(jb->dst[0] + (int64_t)r * jb->ldo + c);
        if (jb->accumulate) {
          f32x4 v = *o;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += a[e];
          *o = v;
        } else {
          *o = a;
        }
      }
    } else if (kind == A3V_FINISH_SCATTER) {
      const int S = (int)jb->S, R = (int)jb->R, N = (int)jb->N, r = (int)jb->r;
      int j = 0;
      int64_t first = 0;                   // first unit of module j inside the job
      for (; j + 1 < (int)jb->n_mods; ++j) {
        const int64_t uj = (jb->nj[j] + FIN_TN - 1) / FIN_TN;
        if (lu < first + uj) break;
        first += uj;
      }
      const int nj = (int)jb->nj[j], n0 = (int)(lu - first) * FIN_TN;
      const int cnt = min(FIN_TN, nj - n0);                    // n of this tile (nj is a multiple of 4)
      const float* src = jb->src + (int64_t)(j * r) * N + jb->row0[j] + n0;
      for (int i = tid; i < r * (FIN_TN / 4); i += 256) {
        const int c = i / (FIN_TN / 4), nn = (i % (FIN_TN / 4)) * 4;
        if (nn < cnt) {
          const f32x4 a = plane_sum(src + (int64_t)c * N + nn, (int64_t)R * N, S);
#pragma unroll
          for (int e = 0; e < 4; ++e) tile[c][nn + e] = a[e];
        }
      }
      __syncthreads();
      float* d = jb->dst[j] + (int64_t)n0 * r;                 // [cnt][r] of the module's gradient: contiguous
      for (int i = tid; i < cnt * r / 4; i += 256) {
        const int nn = (4 * i) / r, c = (4 * i) % r;
        f32x4 v = *reinterpret_cast<f32x4*>(d + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += tile[c + e][nn];
        *reinterpret_cast<f32x4*>(d + 4 * i) = v;
      }
      __syncthreads();                     // the tile is free for this block's next unit
    } else {
      const int nrows = (int)jb->R, cols = (int)jb->N;
      const int ctiles = (cols + 1023) / 1024;
      const int c = (int)(lu % ctiles) * 1024 + tid * 4, chunk = (int)(lu / ctiles);
      if (c < cols) {
        const int per = (nrows + FIN_CHUNKS - 1) / FIN_CHUNKS;
        const int r0 = chunk * per, r1 = min(nrows, r0 + per);
        const float* part = jb->src + c;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
          const f32x4 x0 = *reinterpret_cast<const f32x4*>(part + (int64_t)r * cols);
          const f32x4 x1 = *reinterpret_cast<const f32x4*>(part + (int64_t)(r + 1) * cols);
          const f32x4 x2 = *reinterpret_cast<const f32x4*>(part + (int64_t)(r + 2) * cols);
          const f32x4 x3 = *reinterpret_cast<const f32x4*>(part + (int64_t)(r + 3) * cols);
#pragma unroll
          for (int e = 0; e < 4; ++e) { a0[e] += x0[e]; a1[e] += x1[e]; a2[e] += x2[e]; a3[e] += x3[e]; }
        }
        for (; r < r1; ++r) {
          const f32x4 x0 = *reinterpret_cast<const f32x4*>(part + (int64_t)r * cols);
#pragma unroll
          for (int e = 0; e < 4; ++e) a0[e] += x0[e];
        }
        if (r1 > r0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) atomicAdd(jb->dst[0] + c + e, (a0[e] + a1[e]) + (a2[e] + a3[e]));
        }
      }
    }
  }
}
}  // namespace

extern "C" int a3v_grad_finish_multi(const a3v_finish_job* table_dev, int n_jobs, int64_t total_units, int max_blocks, void* stream) {
  if (!table_dev || n_jobs <= 0 || total_units <= 0 || max_blocks < 0) return A3V_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(table_dev) & 7) || total_units >= (1LL << 31)) return A3V_ERR_SHAPE;
  // a few blocks per CU stride over the units (the table of a 7B step holds ~30 K of them)
  int64_t blocks = max_blocks > 0 ? max_blocks : 4 * (int64_t)a3v_cu_count();
  if (blocks > total_units) blocks = total_units;
  hipLaunchKernelGGL(grad_finish_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n_jobs, total_units);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
