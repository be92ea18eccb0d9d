// Lookup decoding under sampling, penalty, log-probs and constraints (include/a3vlm_hip.h, "Lookup decoding: sample and match").
// Opt-in: nothing here runs unless MetaModel.generate_many is called with lookup=D and lookup_verify="choice".  The verify step
// itself (a3v_spec.hip) is unchanged; these entries sit between its logits and the token write.  Virtual row m = b * Q + j is query j
// of cache row b, as there.
//  * verify_prepare_kernel<PEN, CON, LSE> : one 1024-thread block per virtual row, ONE pass with 16-byte loads and stores over the raw
//    fp32 row: out = the row as the plain loop would prepare it if drafts 1..j had been emitted -- the repetition penalty over
//    seen[b] plus the drafts x[b, 1..j] (kept in registers, compared per vector; no [B*Q, words] bitmap), then the automaton's mask
//    in the state reached by walking those drafts (8-byte loads of the int16 row) -- and lse = logsumexp of the RAW row in the
//    reduction order of logits_prepare_kernel (a3v_genctl.hip), statement for statement.
//  * accept_rows_chosen_kernel : accept_rows_kernel (a3v_spec.hip) with the per-query choice handed in, one thread per cache row, plus
//    per emission what generate_record_kernel and constrain_advance_kernel do behind the plain loop's token write.
//  * verify_uniforms_kernel    : u[m] = uni[row_base[b] + (cur[b] - prompt_len[b]) + j], the plain loop's uniform of that emission.
#include "a3v_common.h"
#include <math.h>

namespace {

constexpr unsigned NEG_INF_BITS = 0xff800000u;

typedef __attribute__((ext_vector_type(4))) short i16x4;

// a3v_genctl.hip's rule and helpers, the same expressions (the bits of the penalised row and of lse are that file's)
__device__ __forceinline__ float penalise(float z, bool seen, float p) { return seen ? (z > 0.f ? z / p : z * p) : z; }
__device__ __forceinline__ float safe_max(float m) { return (m == INFINITY || m == -INFINITY) ? 0.f : m; }
__device__ __forceinline__ float rescale(float m, float ms) { return m == -INFINITY ? 0.f : expf(safe_max(m) - ms); }

template <bool PEN, bool CON, bool LSE>
__global__ __launch_bounds__(1024) void verify_prepare_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ x,
                                                              const int32_t* __restrict__ nq, const int32_t* __restrict__ pos, int Q,
                                                              const uint32_t* __restrict__ seen, int64_t wpr, float p,
                                                              const int16_t* __restrict__ trans, int n_states,
                                                              const int32_t* __restrict__ state, float* __restrict__ lse,
                                                              float* __restrict__ out, int64_t ld_out, int V) {
  __shared__ float wm[16];
  __shared__ float ws[16];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int b = m / Q, j = m - b * Q;
  const float* r = logits + (int64_t)m * ld;
  float* o = out + (int64_t)m * ld_out;
  const bool ovec = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
  if (pos[b] < 0 || j >= min(max(nq[b], 1), Q)) {          // idle query (block-uniform): zeros, the raw row is not read
    const int Z4 = ovec ? V / 4 : 0;
    for (int i = tid; i < Z4; i += 1024) reinterpret_cast<f32x4*>(o)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = Z4 * 4 + tid; i < V; i += 1024) o[i] = 0.f;
    if (LSE && tid == 0) lse[m] = 0.f;
    return;
  }
  const int64_t* xr = x + (int64_t)b * Q;
  // the drafts in front of this query: block-uniform registers; an id outside [0, V) is -1 and matches no element
  int d[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    d[k] = -1;
    if (PEN && k < j) {
      const int64_t id = xr[k + 1];
      if (id >= 0 && id < V) d[k] = (int)id;
    }
  }
  // the automaton state behind drafts 1..j, walked once (block-uniform loads).  dead: a draft the automaton forbids, the whole row -inf
  bool masked = false, dead = false;
  const int16_t* t = trans;
  if (CON) {
    int s = state[b];
    masked = s >= 0 && s < n_states;                        // any other value: an unconstrained row, for every j
    if (masked) {
      for (int k = 1; k <= j && !dead; ++k) {
        const int64_t id = xr[k];
        if (id < 0 || id >= V) { dead = true; break; }
        s = trans[(int64_t)s * V + id];
        dead = s < 0 || s >= n_states;
      }
      if (!dead) t = trans + (int64_t)s * V;
    }
  }
  const uint32_t* sr = PEN ? seen + (int64_t)b * wpr : nullptr;
  float mx = -INFINITY, s = 0.f;
  auto fold4 = [&](const f32x4& x) {
    const float M = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    const float ms = safe_max(M);
    const float t = ((expf(x[0] - ms) + expf(x[1] - ms)) + expf(x[2] - ms)) + expf(x[3] - ms);
    s = s * rescale(mx, ms) + t;
    mx = M;
  };
  auto fold1 = [&](float x) {
    const float M = fmaxf(mx, x);
    const float ms = safe_max(M);
    s = s * rescale(mx, ms) + expf(x - ms);
    mx = M;
  };
  // the alignment cases of logits_prepare_kernel with an out row: both rows on a 16-byte boundary, else element by element
  const bool vec = (reinterpret_cast<uintptr_t>(r) & 15) == 0 && ovec;
  const int V4 = vec ? V / 4 : 0;
  const bool tvec = (reinterpret_cast<uintptr_t>(t) & 7) == 0;
  for (int i0 = tid; i0 < V4; i0 += 4 * 1024) {
    f32x4 xv[4];
    i16x4 mk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 1024;
      if (i < V4) {
        xv[q] = reinterpret_cast<const f32x4*>(r)[i];
        if (CON && masked && !dead) {
          if (tvec) {
            mk[q] = reinterpret_cast<const i16x4*>(t)[i];
          } else {
            const int16_t* te = t + 4 * (int64_t)i;
            mk[q] = i16x4{te[0], te[1], te[2], te[3]};
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 1024;
      if (i >= V4) break;
      if (LSE) fold4(xv[q]);
      f32x4 y = xv[q];
      if (PEN) {
        uint32_t w = sr[i >> 3] >> ((i & 7) * 4);          // elements 4 i .. 4 i + 3: four bits of word i / 8
#pragma unroll
        for (int k = 0; k < 7; ++k)
          if ((d[k] >> 2) == i) w |= 1u << (d[k] & 3);       // a draft in this vector joins the seen set
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = penalise(xv[q][e], (w >> e) & 1u, p);
      }
      u32x4 yb = __builtin_bit_cast(u32x4, y);               // the select moves bit patterns: a kept value keeps its bits
      if (CON && masked) {
#pragma unroll
        for (int e = 0; e < 4; ++e) yb[e] = (!dead && mk[q][e] >= 0) ? yb[e] : NEG_INF_BITS;
      }
      reinterpret_cast<u32x4*>(o)[i] = yb;
    }
  }
  for (int i = V4 * 4 + tid; i < V; i += 1024) {
    const float xe = r[i];
    if (LSE) fold1(xe);
    float y = xe;
    if (PEN) {
      bool sn = (sr[i >> 5] >> (i & 31)) & 1u;
#pragma unroll
      for (int k = 0; k < 7; ++k) sn = sn || d[k] == i;
      y = penalise(xe, sn, p);
    }
    uint32_t yb = __float_as_uint(y);
    if (CON && masked) yb = (!dead && t[i] >= 0) ? yb : NEG_INF_BITS;
    reinterpret_cast<uint32_t*>(o)[i] = yb;
  }
  if (!LSE) return;
  const float Mw = wave_max(mx);
  s = wave_sum(s * rescale(mx, safe_max(Mw)));
  if ((tid & 63) == 0) { wm[tid >> 6] = Mw; ws[tid >> 6] = s; }
  __syncthreads();
  if (tid != 0) return;
  float M = wm[0];
  for (int w = 1; w < 16; ++w) M = fmaxf(M, wm[w]);
  const float ms = safe_max(M);
  float S = 0.f;
  for (int w = 0; w < 16; ++w) S += ws[w] * rescale(wm[w], ms);
  lse[m] = M + logf(S);
}

struct AcceptBook {                      // the optional bookkeeping of an emission; every pointer may be NULL on its own
  const float* logits; int64_t ld; int V; const float* lse;
  float* logprob; int64_t ld_lp; int n_lp;
  const int32_t* prompt_len;
  uint32_t* seen; int64_t wpr;
  const int16_t* trans; int n_states; int32_t* state;
};

// One thread per cache row: accept_rows_kernel's thread-0 part with t_j = chosen[b * Q + j].
__global__ __launch_bounds__(64) void accept_rows_chosen_kernel(const int64_t* __restrict__ chosen, int B, int Q, const int64_t* __restrict__ x,
                                                                const int32_t* __restrict__ nq, int64_t* __restrict__ tokens, int64_t ld_tok,
                                                                int32_t* __restrict__ cur, const int32_t* __restrict__ limit, int pos_base,
                                                                const int64_t* __restrict__ stop_seq, const int32_t* __restrict__ stop_off,
                                                                int n_stop, uint8_t* __restrict__ stopped, int64_t* __restrict__ stop_pos,
                                                                int64_t* __restrict__ next_tok, int32_t* __restrict__ pos,
                                                                unsigned long long* __restrict__ stats, AcceptBook k) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  if (stopped[row]) {                  // a stopped row is not touched
    next_tok[row] = 0;
    pos[row] = -1;
    return;
  }
  const int nd = min(max(nq[row], 1), Q) - 1;
  int c = cur[row];
  const int lim = limit[row];
  if (c < 0 || c >= lim || c >= ld_tok) {            // nothing writable: the row stops where it is
    stopped[row] = 1;
    next_tok[row] = 0;
    pos[row] = -1;
    return;
  }
  int64_t* trow = tokens + (int64_t)row * ld_tok;
  const int64_t* xr = x + (int64_t)row * Q;
  const int64_t* tj = chosen + (int64_t)row * Q;
  bool st = false;
  int64_t sp = 0, next = 0;
  int emitted = 0;
  for (int j = 0; j <= nd && !st; ++j) {
    if (j > 0 && tj[j - 1] != xr[j]) break;            // a draft the choice did not produce ends the run
    if (c >= ld_tok) { st = true; break; }
    next = tj[j];
    trow[c] = next;
    sp = (int64_t)c + 1;
    for (int s = 0; s < n_stop; ++s) {
      const int o = stop_off[s], n = stop_off[s + 1] - o;
      if (c + 1 - n < 0 || st) continue;
      bool hit = true;
      for (int e = 0; e < n && hit; ++e) hit = trow[c + 1 - n + e] == stop_seq[o + e];
      if (hit) { sp = c + 1 - n; st = true; }
    }
    // the plain loop's record and advance of this emission (the one that stops the row included): column c, the RAW row of query j
    const int64_t g = k.prompt_len ? (int64_t)c - k.prompt_len[row] : 0;
    if (g >= 0 && next >= 0 && next < k.V) {
      const int64_t m = (int64_t)row * Q + j;
      if (k.logprob && g < k.n_lp) k.logprob[(int64_t)row * k.ld_lp + g] = k.logits[m * k.ld + next] - k.lse[m];
      if (k.seen) atomicOr(k.seen + (int64_t)row * k.wpr + (next >> 5), 1u << (next & 31));
      if (k.state) {
        const int s = k.state[row];
        if (s >= 0 && s < k.n_states) k.state[row] = (int32_t)k.trans[(int64_t)s * k.V + next];
      }
    }
    c += 1;
    if (c >= lim) st = true;                           // the last writable index is written: stop_pos stays c
    ++emitted;
  }
  cur[row] = c;
  stopped[row] = st ? 1 : 0;
  stop_pos[row] = sp;
  next_tok[row] = st ? 0 : next;
  pos[row] = st ? -1 : pos_base + c - 1;
  if (stats) {
    atomicAdd(stats, (unsigned long long)nd);
    atomicAdd(stats + 1, (unsigned long long)(emitted - 1));
  }
}

__global__ __launch_bounds__(256) void verify_uniforms_kernel(const float* __restrict__ uni, int64_t n_uni, const int64_t* __restrict__ row_base,
                                                              const int32_t* __restrict__ cur, const int32_t* __restrict__ prompt_len,
                                                              int B, int Q, float* __restrict__ u) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= B * Q) return;
  const int b = m / Q, j = m - b * Q;
  int64_t i = row_base[b] + ((int64_t)cur[b] - prompt_len[b]) + j;
  i = i < 0 ? 0 : (i > n_uni - 1 ? n_uni - 1 : i);       // clamped into the array: an idle row's index means nothing
  u[m] = uni[i];
}

}  // namespace

#define ST (hipStream_t)stream

extern "C" int a3v_verify_prepare(const float* logits, int64_t ld, int B, int Q, int V, const int64_t* x, const int32_t* nq,
                                  const int32_t* pos, const uint32_t* seen, int64_t words_per_row, float penalty, const int16_t* trans,
                                  int n_states, const int32_t* state, float* lse, float* out, int64_t ld_out, void* stream) {
  if (!logits || !x || !nq || !pos || !out || out == logits) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld < V || ld_out < V) return A3V_ERR_ARG;
  if (seen && (!(penalty > 0.f) || words_per_row < ((int64_t)V + 31) / 32)) return A3V_ERR_ARG;
  if (trans && (!state || n_states <= 0 || n_states > 32767)) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8 || (int64_t)B * Q > 65535) return A3V_ERR_SHAPE;
#define A3V_VP(PEN, CON, LSE)                                                                                                              \
  hipLaunchKernelGGL((verify_prepare_kernel<PEN, CON, LSE>), dim3(B * Q), dim3(1024), 0, ST, logits, ld, x, nq, pos, Q, seen, words_per_row, \
                     penalty, trans, n_states, state, lse, out, ld_out, V)
  const int form = (seen ? 4 : 0) | (trans ? 2 : 0) | (lse ? 1 : 0);
  switch (form) {
    case 0: A3V_VP(false, false, false); break;
    case 1: A3V_VP(false, false, true); break;
    case 2: A3V_VP(false, true, false); break;
    case 3: A3V_VP(false, true, true); break;
    case 4: A3V_VP(true, false, false); break;
    case 5: A3V_VP(true, false, true); break;
    case 6: A3V_VP(true, true, false); break;
    default: A3V_VP(true, true, true); break;
  }
#undef A3V_VP
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_accept_rows_chosen(const int64_t* chosen, int B, int Q, const int64_t* x, const int32_t* nq, int64_t* tokens,
                                      int64_t ld_tok, int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq,
                                      const int32_t* stop_off, int n_stop, uint8_t* stopped, int64_t* stop_pos, int64_t* next_tok,
                                      int32_t* pos, int64_t* stats, const float* logits, int64_t ld, int V, const float* lse,
                                      float* logprob, int64_t ld_lp, int n_lp, const int32_t* prompt_len, uint32_t* seen,
                                      int64_t words_per_row, const int16_t* trans, int n_states, int32_t* state, void* stream) {
  if (!chosen || !x || !nq || !tokens || !cur || !limit || !stopped || !stop_pos || !next_tok || !pos) return A3V_ERR_ARG;
  if (B <= 0 || ld_tok <= 0 || pos_base < 0 || n_stop < 0 || (n_stop > 0 && (!stop_seq || !stop_off))) return A3V_ERR_ARG;
  if ((logprob || seen || state) && (V <= 0 || !prompt_len)) return A3V_ERR_ARG;
  if (logprob && (!logits || !lse || ld < V || n_lp <= 0 || ld_lp < n_lp)) return A3V_ERR_ARG;
  if (seen && words_per_row < ((int64_t)V + 31) / 32) return A3V_ERR_ARG;
  if (state && (!trans || n_states <= 0 || n_states > 32767)) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8) return A3V_ERR_SHAPE;
  const AcceptBook k{logits, ld, (logprob || seen || state) ? V : 0, lse, logprob, ld_lp, n_lp, prompt_len, seen, words_per_row, trans, n_states, state};
  hipLaunchKernelGGL(accept_rows_chosen_kernel, dim3((B + 63) / 64), dim3(64), 0, ST, chosen, B, Q, x, nq, tokens, ld_tok, cur, limit, pos_base,
                     stop_seq, stop_off, n_stop, stopped, stop_pos, next_tok, pos, (unsigned long long*)stats, k);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_verify_uniforms(const float* uni, int64_t n_uni, const int64_t* row_base, const int32_t* cur, const int32_t* prompt_len,
                                   int B, int Q, float* u, void* stream) {
  if (!uni || !row_base || !cur || !prompt_len || !u || n_uni <= 0 || B <= 0) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8) return A3V_ERR_SHAPE;
  hipLaunchKernelGGL(verify_uniforms_kernel, dim3((B * Q + 255) / 256), dim3(256), 0, ST, uni, n_uni, row_base, cur, prompt_len, B, Q, u);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
