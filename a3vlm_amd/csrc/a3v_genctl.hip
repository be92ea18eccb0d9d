// Generation controls on the device (include/a3vlm_hip.h, "Generation controls"): the seen-token bitmap of the repetition
// penalty, the penalised logits row, the raw log-sum-exp of the row and the log-probability of the chosen token.  Opt-in: nothing
// here runs unless MetaModel.generate / generate_many / stream_generate are called with repetition_penalty != 1 or
// return_logprobs=True.
//  * seen_mark_kernel        : tokens[b, 0 .. lens[b]) -> bits of seen[b] (vector atomicOr: several lanes can hit one word).
//  * seen_clear_rows_kernel  : zero the bitmap rows of a device row list.
//  * logits_prepare_kernel   : one 1024-thread block per row, ONE pass with 16-byte loads: out = penalised row (if a bitmap is
//                              given), lse = logsumexp of the RAW row (if asked), an online (max, sum) per thread.
//  * generate_record_kernel  : after the step kernel has written the chosen id: lp = z[id] - lse, bit of id set.
#include "a3v_common.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void seen_mark_kernel(const int64_t* __restrict__ tokens, int64_t ld_tok, const int32_t* __restrict__ lens,
                                                        uint32_t* __restrict__ seen, int64_t wpr, int V) {
  const int b = blockIdx.x;
  int64_t n = lens[b];
  if (n > ld_tok) n = ld_tok;                          // never past the row
  const int64_t* t = tokens + (int64_t)b * ld_tok;
  uint32_t* s = seen + (int64_t)b * wpr;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const int64_t id = t[i];
    if (id >= 0 && id < V) atomicOr(s + (id >> 5), 1u << (id & 31));
  }
}

__global__ __launch_bounds__(256) void seen_clear_rows_kernel(uint32_t* __restrict__ seen, const int32_t* __restrict__ rows, int64_t wpr,
                                                              int64_t n_words, int R) {
  const int row = rows[blockIdx.y];
  if (row < 0 || row >= R) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_words) seen[(int64_t)row * wpr + i] = 0u;
}

// the HF RepetitionPenaltyLogitsProcessor rule on one logit; a true fp32 division (hipcc's default: correctly rounded), torch's bits
__device__ __forceinline__ float penalise(float z, bool seen, float p) { return seen ? (z > 0.f ? z / p : z * p) : z; }

// exponent offset of a running maximum: the maximum itself, 0 when it is infinite (so that inf - inf never appears)
__device__ __forceinline__ float safe_max(float m) { return (m == INFINITY || m == -INFINITY) ? 0.f : m; }
// factor that carries a sum taken at offset safe_max(m) to the offset ms of a maximum >= m; an empty sum (m = -inf) stays 0
__device__ __forceinline__ float rescale(float m, float ms) { return m == -INFINITY ? 0.f : expf(safe_max(m) - ms); }

// Reduction order of lse (the bound of tests/genctl_ref.py: lse_bound is derived from exactly this):
//   thread t owns the 4-element vectors t, t + 1024, t + 2048, ... of the row in ascending order (rows whose address is not
//   16-byte aligned: single elements t, t + 1024, ... as one-element "vectors"; the V % 4 tail likewise, after the vectors).
//   Per vector: M = max(m, max of the vector); s = s * exp(m - M) + (((e0 + e1) + e2) + e3), e_j = exp(x_j - M); m = M.
//   Wave: M_w = butterfly max of m (wave_max); s *= exp(m - M_w); S_w = butterfly sum of s (wave_sum: ^32 ^16 ^8 ^4 ^2 ^1).
//   Block: M = max over the 16 waves; S = sum over w = 0 .. 15 in order of S_w * exp(M_w - M);  lse = M + log(S).
//   expf / logf are the full-precision library functions (<= 1 ulp), not the fast intrinsics.
template <bool PEN, bool LSE>
__global__ __launch_bounds__(1024) void logits_prepare_kernel(const float* __restrict__ logits, int64_t ld, const uint32_t* __restrict__ seen,
                                                              int64_t wpr, float p, float* __restrict__ out, int64_t ld_out,
                                                              float* __restrict__ lse, int V) {
  __shared__ float wm[16];
  __shared__ float ws[16];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* r = logits + (int64_t)row * ld;
  const uint32_t* sr = PEN ? seen + (int64_t)row * wpr : nullptr;
  float* o = PEN ? out + (int64_t)row * ld_out : nullptr;
  float m = -INFINITY, s = 0.f;
  auto fold4 = [&](const f32x4& x) {
    const float M = fmaxf(m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    const float ms = safe_max(M);
    const float t = ((expf(x[0] - ms) + expf(x[1] - ms)) + expf(x[2] - ms)) + expf(x[3] - ms);
    s = s * rescale(m, ms) + t;
    m = M;
  };
  auto fold1 = [&](float x) {
    const float M = fmaxf(m, x);
    const float ms = safe_max(M);
    s = s * rescale(m, ms) + expf(x - ms);
    m = M;
  };
  bool vec = (reinterpret_cast<uintptr_t>(r) & 15) == 0;
  if (PEN) vec = vec && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
  const int V4 = vec ? V / 4 : 0;
  for (int i0 = tid; i0 < V4; i0 += 4 * 1024) {
    f32x4 x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 1024;
      if (i < V4) x[q] = reinterpret_cast<const f32x4*>(r)[i];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 1024;
      if (i >= V4) break;
      if (LSE) fold4(x[q]);
      if (PEN) {
        const uint32_t w = sr[i >> 3] >> ((i & 7) * 4);      // elements 4 i .. 4 i + 3: four bits of word i / 8
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = penalise(x[q][e], (w >> e) & 1u, p);
        reinterpret_cast<f32x4*>(o)[i] = y;
      }
    }
  }
  for (int i = V4 * 4 + tid; i < V; i += 1024) {
    const float x = r[i];
    if (LSE) fold1(x);
    if (PEN) o[i] = penalise(x, (sr[i >> 5] >> (i & 31)) & 1u, p);
  }
  if (!LSE) return;
  const float Mw = wave_max(m);
  s = wave_sum(s * rescale(m, safe_max(Mw)));
  if ((tid & 63) == 0) { wm[tid >> 6] = Mw; ws[tid >> 6] = s; }
  __syncthreads();
  if (tid != 0) return;
  float M = wm[0];
  for (int w = 1; w < 16; ++w) M = fmaxf(M, wm[w]);
  const float ms = safe_max(M);
  float S = 0.f;
  for (int w = 0; w < 16; ++w) S += ws[w] * rescale(wm[w], ms);
  lse[row] = M + logf(S);
}

// One thread per row.  Column convention: uniform step (cur == NULL): column `col`.  Ragged (cur != NULL): generate_step_rows_kernel
// has written tokens[b, c] and advanced cur[b] to c + 1, so the column is cur[b] - 1; a row that kernel did not touch (stopped on entry)
// still has its old cur[b], which is why the caller hands in the snapshot of `stopped` taken BEFORE the step.
__global__ __launch_bounds__(64) void generate_record_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                             const int64_t* __restrict__ tokens, int64_t ld_tok, int col,
                                                             const int32_t* __restrict__ cur, const uint8_t* __restrict__ stopped_before,
                                                             uint32_t* __restrict__ seen, int64_t wpr, float* __restrict__ logprob,
                                                             int64_t ld_lp, int n_lp, int idx, const int32_t* __restrict__ prompt_len, int B,
                                                             int V) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (stopped_before && stopped_before[b]) return;
  const int64_t c = cur ? (int64_t)cur[b] - 1 : (int64_t)col;
  if (c < 0 || c >= ld_tok) return;                      // idle ragged row, or nothing written yet
  const int64_t g = prompt_len ? c - prompt_len[b] : (int64_t)idx;
  if (g < 0) return;                                     // a teacher-forced prompt position: marked up front, never scored
  const int64_t id = tokens[(int64_t)b * ld_tok + c];
  if (id < 0 || id >= V) return;
  if (logprob && g < n_lp) logprob[(int64_t)b * ld_lp + g] = logits[(int64_t)b * ld + id] - lse[b];
  if (seen) atomicOr(seen + (int64_t)b * wpr + (id >> 5), 1u << (id & 31));
}

}  // namespace

#define ST (hipStream_t)stream

extern "C" int a3v_seen_mark(const int64_t* tokens, int64_t ld_tok, const int32_t* lens, uint32_t* seen, int64_t words_per_row, int B,
                             int V, void* stream) {
  if (!tokens || !lens || !seen) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld_tok <= 0 || words_per_row < ((int64_t)V + 31) / 32) return A3V_ERR_ARG;
  hipLaunchKernelGGL(seen_mark_kernel, dim3(B), dim3(256), 0, ST, tokens, ld_tok, lens, seen, words_per_row, V);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_seen_clear_rows(uint32_t* seen, const int32_t* rows, int n_rows, int64_t words_per_row, int64_t n_words, int R,
                                   void* stream) {
  if (!seen || !rows) return A3V_ERR_ARG;
  if (n_rows <= 0 || n_rows > 65535 || R <= 0 || n_words <= 0 || n_words > words_per_row || n_words > (int64_t)1 << 36) return A3V_ERR_ARG;
  hipLaunchKernelGGL(seen_clear_rows_kernel, dim3((unsigned)((n_words + 255) / 256), n_rows), dim3(256), 0, ST, seen, rows, words_per_row,
                     n_words, R);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_logits_prepare(const float* logits, int64_t ld, const uint32_t* seen, int64_t words_per_row, float penalty, float* out,
                                  int64_t ld_out, float* lse, int B, int V, void* stream) {
  if (!logits || (!seen && !lse)) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld < V) return A3V_ERR_ARG;
  if (seen && (!out || out == logits || ld_out < V || !(penalty > 0.f) || words_per_row < ((int64_t)V + 31) / 32)) return A3V_ERR_ARG;
  if (seen && lse)
    hipLaunchKernelGGL((logits_prepare_kernel<true, true>), dim3(B), dim3(1024), 0, ST, logits, ld, seen, words_per_row, penalty, out, ld_out, lse, V);
  else if (seen)
    hipLaunchKernelGGL((logits_prepare_kernel<true, false>), dim3(B), dim3(1024), 0, ST, logits, ld, seen, words_per_row, penalty, out, ld_out, lse, V);
  else
    hipLaunchKernelGGL((logits_prepare_kernel<false, true>), dim3(B), dim3(1024), 0, ST, logits, ld, seen, words_per_row, penalty, out, ld_out, lse, V);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_generate_record(const float* logits, int64_t ld, const float* lse, const int64_t* tokens, int64_t ld_tok, int col,
                                   const int32_t* cur, const uint8_t* stopped_before, uint32_t* seen, int64_t words_per_row,
                                   float* logprob, int64_t ld_lp, int n_lp, int idx, const int32_t* prompt_len, int B, int V,
                                   void* stream) {
  if (!tokens || (!seen && !logprob)) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld_tok <= 0 || (!cur && (col < 0 || col >= ld_tok))) return A3V_ERR_ARG;
  if (logprob && (!logits || !lse || ld < V || n_lp <= 0 || ld_lp < n_lp || (!prompt_len && (idx < 0 || idx >= n_lp)))) return A3V_ERR_ARG;
  if (seen && words_per_row < ((int64_t)V + 31) / 32) return A3V_ERR_ARG;
  hipLaunchKernelGGL(generate_record_kernel, dim3((B + 63) / 64), dim3(64), 0, ST, logits, ld, lse, tokens, ld_tok, col, cur, stopped_before,
                     seen, words_per_row, logprob, ld_lp, n_lp, idx, prompt_len, B, V);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
