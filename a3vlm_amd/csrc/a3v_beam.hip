// Beam search on the ragged decode path (include/a3vlm_hip.h, "Beam search"; tests/beam_ref.py is the restatement).  Opt-in: nothing
// here runs unless MetaModel.beam_search is called.  Groups of K = num_beams consecutive cache rows, group g = rows [gK, gK + K).
//  * beam_select_kernel<N2>   : one 1024-thread block per group: the best N2 = 2K candidates (beam b, token v) of the group's live
//                               beams, ordered by score descending, then flat index b V + v ascending.  Every thread keeps a sorted
//                               list of N2 in registers (compare-exchange chains with constant indices: no scratch), a wave takes
//                               its best N2 by N2 rounds of (butterfly arg-best over the list heads, the winner pops), wave 0 does
//                               the same over the 16 wave lists in LDS.  The result depends only on the (score, index) order.
//  * beam_advance_kernel      : one block per group: thread 0 walks the candidates (integer work and one division per finished
//                               hypothesis) and leaves a list of token-row copies, which the block then carries out.
//  * kv_permute_tails_kernel  : the generated keys of a parent beam into its children's cache rows, every layer in one launch.  A
//                               thread owns ONE 16-byte vector offset for all K rows of a group: it reads the K rows' vectors into
//                               its LDS column, then writes each row from its parent's copy.  OWNERSHIP is what removes the hazard:
//                               nobody else touches that offset, so a parent that is itself overwritten, or named by several rows,
//                               is read before it is written, by the one thread that does both.  LDS is used only so that the
//                               parent can index the K copies dynamically without scratch; the barrier between the two phases is
//                               the contract's (include/a3vlm_hip.h) and orders nothing a thread does not already order itself.
#include "a3v_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int BEAM_MAX = 8;

// (s, f) ranks before (s2, f2): the higher score, then the lower flat index.  A NaN score ranks before nothing.
__device__ __forceinline__ bool ranks_before(float s, int f, float s2, int f2) { return s > s2 || (s == s2 && f < f2); }

template <int N2>
struct TopList {
  float s[N2];
  int f[N2];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < N2; ++j) { s[j] = -INFINITY; f[j] = INT_MAX; }
  }
  // -inf and NaN are never taken
  __device__ __forceinline__ void insert(float x, int i) {
    if (!(x > -INFINITY) || !ranks_before(x, i, s[N2 - 1], f[N2 - 1])) return;
    s[N2 - 1] = x; f[N2 - 1] = i;
#pragma unroll
    for (int j = N2 - 1; j > 0; --j) {
      const bool up = ranks_before(s[j], f[j], s[j - 1], f[j - 1]);
      const float ts = s[j]; const int tf = f[j];
      s[j] = up ? s[j - 1] : ts; f[j] = up ? f[j - 1] : tf;
      s[j - 1] = up ? ts : s[j - 1]; f[j - 1] = up ? tf : f[j - 1];
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j < N2 - 1; ++j) { s[j] = s[j + 1]; f[j] = f[j + 1]; }
    s[N2 - 1] = -INFINITY; f[N2 - 1] = INT_MAX;
  }
};

// the best head of the wave's 64 lists, in every lane (flat indices are unique, so every lane ends on the same pair)
__device__ __forceinline__ void wave_best(float& bs, int& bf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int of = __shfl_xor(bf, o, 64);
    if (ranks_before(os, of, bs, bf)) { bs = os; bf = of; }
  }
}

template <int N2>
__global__ __launch_bounds__(1024) void beam_select_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                           const float* __restrict__ cum, const uint8_t* __restrict__ alive,
                                                           const int16_t* __restrict__ trans, int n_states,
                                                           const int32_t* __restrict__ state, int K, int V,
                                                           float* __restrict__ cand_score, int32_t* __restrict__ cand_beam,
                                                           int32_t* __restrict__ cand_tok) {
  __shared__ float ws[16][N2];
  __shared__ int wf[16][N2];
  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  TopList<N2> top;
  top.clear();
  for (int b = 0; b < K; ++b) {
    const int row = g * K + b;
    if (!alive[row]) continue;                                   // block-uniform
    const float c = cum[row], l = lse[row];
    const float* r = logits + (int64_t)row * ld;
    const int16_t* t = nullptr;                                  // the row of the automaton; NULL: every token is allowed
    if (trans) {
      const int st = state[row];
      if (st >= 0 && st < n_states) t = trans + (int64_t)st * V; // the kernel bounds the state: the host cannot see it
    }
    const int base = b * V;
    // the alignment rule of logits_prepare_kernel: 16-byte vectors of a 16-byte aligned row, else (and for the V % 4 tail) single elements
    const int V4 = (reinterpret_cast<uintptr_t>(r) & 15) == 0 ? V / 4 : 0;
    for (int i = tid; i < V4; i += 1024) {
      const f32x4 x = reinterpret_cast<const f32x4*>(r)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * i + e;
        if (t && t[v] < 0) continue;
        top.insert(c + (x[e] - l), base + v);                    // two fp32 operations in this order, on the raw logit
      }
    }
    for (int v = V4 * 4 + tid; v < V; v += 1024) {
      if (t && t[v] < 0) continue;
      top.insert(c + (r[v] - l), base + v);
    }
  }
  for (int k = 0; k < N2; ++k) {
    float bs = top.s[0];
    int bf = top.f[0];
    wave_best(bs, bf);
    if (bf != INT_MAX && top.f[0] == bf) top.pop();
    if (lane == 0) { ws[wave][k] = bs; wf[wave][k] = bf; }
  }
  __syncthreads();
  if (wave != 0) return;
  top.clear();
  for (int e = lane; e < 16 * N2; e += 64) top.insert((&ws[0][0])[e], (&wf[0][0])[e]);
  for (int k = 0; k < N2; ++k) {
    float bs = top.s[0];
    int bf = top.f[0];
    wave_best(bs, bf);
    if (bf != INT_MAX && top.f[0] == bf) top.pop();
    if (lane == 0) {
      const bool filled = bf != INT_MAX;
      cand_score[(int64_t)g * N2 + k] = filled ? bs : -INFINITY;
      cand_beam[(int64_t)g * N2 + k] = filled ? bf / V : -1;
      cand_tok[(int64_t)g * N2 + k] = filled ? bf % V : -1;
    }
  }
}

struct AdvanceArgs {
  const float* cand_score; const int32_t* cand_beam; const int32_t* cand_tok;
  int K, V, eos, early, n_div, n_states, pos_cap;
  const float* len_div; const int16_t* trans;
  const int32_t* base; const int32_t* limit;
  float* cum; uint8_t* alive; int32_t* state; int32_t* glen; uint8_t* done; int32_t* parent; int64_t* next_tok; int32_t* pos;
  const int64_t* tokens_in; int64_t* tokens_out; int64_t ld_tok;
  int32_t* pool_n; int32_t* pool_added; float* pool_score; float* pool_cum; int32_t* pool_len; int32_t* pool_seq; int64_t* pool_ids;
};

constexpr int ADV_ACTS = 3 * BEAM_MAX;               // <= K finished at rank < K, K new token rows, K hypotheses at the limit

__global__ __launch_bounds__(256) void beam_advance_kernel(AdvanceArgs a) {
  __shared__ int64_t* act_dst[ADV_ACTS];
  __shared__ const int64_t* act_src[ADV_ACTS];
  __shared__ int act_n[ADV_ACTS];
  __shared__ int64_t act_extra[ADV_ACTS];
  __shared__ int n_act;
  __shared__ int old_state[BEAM_MAX], nb[BEAM_MAX], nt[BEAM_MAX], pq[BEAM_MAX];
  __shared__ float ns[BEAM_MAX], ps[BEAM_MAX];
  const int g = blockIdx.x, tid = threadIdx.x, K = a.K, row0 = g * K;
  if (tid == 0) {
    int na = 0;
    if (!a.done[g]) {
      const int L = a.glen[g], b0 = a.base[g];
      int64_t lim = a.limit[g];
      if (lim > a.ld_tok) lim = a.ld_tok;
      if (lim > a.n_div - 1) lim = a.n_div - 1;
      if (b0 < 0) lim = 0;
      else if (lim > a.pos_cap - b0) lim = a.pos_cap - b0;
      bool dn = false;
      if (L < 0 || L >= lim) {
        dn = true;                                               // nothing may be written behind the limit: the group just ends
      } else {
        int np = a.pool_n[g], added = a.pool_added[g];
        if (np < 0) np = 0;
        if (np > K) np = K;
        for (int j = 0; j < K; ++j) { old_state[j] = a.state[row0 + j]; ps[j] = a.pool_score[row0 + j]; pq[j] = a.pool_seq[row0 + j]; }
        // a full pool keeps the best K; a tie keeps the earlier entry
        auto pool_add = [&](float score, float cumv, int len, const int64_t* src) {
          int slot;
          if (np < K) {
            slot = np++;
          } else {
            slot = 0;
            for (int j = 1; j < K; ++j)
              if (ps[j] < ps[slot] || (ps[j] == ps[slot] && pq[j] > pq[slot])) slot = j;
            if (!(score > ps[slot])) return;
          }
          ps[slot] = score; pq[slot] = added;
          a.pool_score[row0 + slot] = score; a.pool_cum[row0 + slot] = cumv; a.pool_len[row0 + slot] = len; a.pool_seq[row0 + slot] = added++;
          act_dst[na] = a.pool_ids + (int64_t)(row0 + slot) * a.ld_tok; act_src[na] = src; act_n[na] = len; act_extra[na] = -1;
          ++na;
        };
        int taken = 0;
        for (int rank = 0; rank < 2 * K; ++rank) {
          const float s = a.cand_score[(int64_t)g * 2 * K + rank];
          const int b = a.cand_beam[(int64_t)g * 2 * K + rank], t = a.cand_tok[(int64_t)g * 2 * K + rank];
          if (!(s > -INFINITY) || b < 0 || b >= K || t < 0 || t >= a.V) continue;      // an unfilled slot, or not a candidate
          if (t == a.eos) {
            if (rank < K) pool_add(s / a.len_div[L], s, L, a.tokens_in + (int64_t)(row0 + b) * a.ld_tok);
            continue;
          }
          if (taken < K) { nb[taken] = b; nt[taken] = t; ns[taken] = s; ++taken; }
        }
        const int G1 = L + 1;
        a.glen[g] = G1;
        for (int j = 0; j < K; ++j) {
          const int r = row0 + j;
          if (j < taken) {
            const int st = old_state[nb[j]];
            a.parent[r] = row0 + nb[j]; a.next_tok[r] = nt[j]; a.cum[r] = ns[j]; a.alive[r] = 1; a.pos[r] = b0 + L;
            a.state[r] = (a.trans && st >= 0 && st < a.n_states) ? (int32_t)a.trans[(int64_t)st * a.V + nt[j]] : st;
            act_dst[na] = a.tokens_out + (int64_t)r * a.ld_tok; act_src[na] = a.tokens_in + (int64_t)(row0 + nb[j]) * a.ld_tok;
            act_n[na] = L; act_extra[na] = nt[j];
            ++na;
          } else {
            a.parent[r] = r; a.next_tok[r] = 0; a.cum[r] = -INFINITY; a.alive[r] = 0; a.pos[r] = -1;
          }
        }
        if (taken == 0) {
          dn = true;
        } else if (G1 >= lim) {                                  // the limit: every live beam is a hypothesis at its current sum
          for (int j = 0; j < taken; ++j) pool_add(ns[j] / a.len_div[G1], ns[j], G1, a.tokens_out + (int64_t)(row0 + j) * a.ld_tok);
          dn = true;
        } else if (np == K) {
          if (a.early) {
            dn = true;
          } else {
            float worst = ps[0];
            for (int j = 1; j < K; ++j) worst = fminf(worst, ps[j]);
            dn = ns[0] / a.len_div[G1] <= worst;                 // the live beams are in rank order: beam 0 has the best sum
          }
        }
        a.pool_n[g] = np; a.pool_added[g] = added;
      }
      if (dn) {
        for (int j = 0; j < K; ++j) { const int r = row0 + j; a.parent[r] = r; a.next_tok[r] = 0; a.alive[r] = 0; a.pos[r] = -1; }
        a.done[g] = 1;
      }
    }
    n_act = na;
  }
  __syncthreads();
  const int na = n_act;
  // in order: a hypothesis at the limit is read from the token row written just before it, and a slot may be written twice
  for (int i = 0; i < na; ++i) {
    int64_t* d = act_dst[i];
    const int64_t* s = act_src[i];
    const int n = act_n[i];
    for (int j = tid; j < n; j += 256) d[j] = s[j];
    if (tid == 0 && act_extra[i] >= 0) d[n] = act_extra[i];
    __threadfence_block();
    __syncthreads();
  }
}

constexpr int PT_THREADS = 256, PT_CHUNK = 64;       // cache positions per block

// grid (chunks, Hkv, layers * G).  Chunk c of group g covers the positions [o + 64 c, o + 64 c + 64), o = the smallest tail_lo of the
// group's moved rows rounded down to 8 (so that every V^T vector of a chunk is 16-byte aligned: Smax is a multiple of 8).
template <typename T>
__global__ __launch_bounds__(PT_THREADS) void kv_permute_tails_kernel(const void* const* __restrict__ k_ptrs, const void* const* __restrict__ vt_ptrs,
                                                                      const int32_t* __restrict__ parent, const int32_t* __restrict__ tail_lo,
                                                                      const int32_t* __restrict__ pos, int G, int K, int Hkv, int hd, int Smax) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ u32x4 stage[BEAM_MAX][PT_THREADS];
  __shared__ int par[BEAM_MAX], lo[BEAM_MAX], hi[BEAM_MAX];
  const int tid = threadIdx.x, hk = blockIdx.y, layer = blockIdx.z / G, g = blockIdx.z % G, row0 = g * K;
  if (tid < K) {
    const int r = row0 + tid;
    int p = parent[r], l = tail_lo[r], h = pos[r];
    if (p < row0 || p >= row0 + K) p = r;                        // a parent outside the group is read as the identity
    if (l < 0) l = 0;
    if (h > Smax) h = Smax;
    if (h <= l) p = r;                                           // an empty span moves nothing
    par[tid] = p - row0; lo[tid] = l; hi[tid] = h;
  }
  __syncthreads();
  int lo_min = INT_MAX, hi_max = 0;
  for (int j = 0; j < K; ++j)
    if (par[j] != j) { lo_min = min(lo_min, lo[j]); hi_max = max(hi_max, hi[j]); }
  if (lo_min == INT_MAX) return;                                 // every parent is the identity (block-uniform)
  const int p0 = (lo_min & ~7) + blockIdx.x * PT_CHUNK;          // this block's positions [p0, p1)
  const int p1 = min(p0 + PT_CHUNK, Smax);
  if (p0 >= hi_max || p0 >= p1) return;
  T* kb = (T*)k_ptrs[layer];
  T* vb = (T*)vt_ptrs[layer];
  // K: the chunk of a (row, head) is one contiguous run of (p1 - p0) * hd elements; vector i lies wholly in position p0 + i / (hd / VEC)
  {
    const int vpp = hd / VEC, nvec = (p1 - p0) * vpp;
    for (int i0 = 0; i0 < nvec; i0 += PT_THREADS) {              // uniform trip count, for the contract's barrier inside
      const int i = i0 + tid;
      const bool on = i < nvec;
      const int p = p0 + i / vpp;
      const int64_t off = (int64_t)p0 * hd + (int64_t)i * VEC;
      if (on)
        for (int j = 0; j < K; ++j)
          stage[j][tid] = *reinterpret_cast<const u32x4*>(kb + ((int64_t)(row0 + j) * Hkv + hk) * Smax * hd + off);
      __syncthreads();
      if (on)
        for (int j = 0; j < K; ++j)
          if (par[j] != j && p >= lo[j] && p < hi[j])
            *reinterpret_cast<u32x4*>(kb + ((int64_t)(row0 + j) * Hkv + hk) * Smax * hd + off) = stage[par[j]][tid];
      __syncthreads();
    }
  }
  // V^T: per d row the chunk is (p1 - p0) / VEC aligned vectors (p0 and Smax are multiples of 8); a vector wholly inside a row's span
  // is one 16-byte store, one that straddles an edge of the span is stored element by element
  {
    const int vpd = (p1 - p0) / VEC, nvec = hd * vpd;
    for (int i0 = 0; i0 < nvec; i0 += PT_THREADS) {
      const int i = i0 + tid;
      const bool on = i < nvec;
      const int d = i / vpd, p = p0 + (i % vpd) * VEC;
      if (on)
        for (int j = 0; j < K; ++j)
          stage[j][tid] = *reinterpret_cast<const u32x4*>(vb + (((int64_t)(row0 + j) * Hkv + hk) * hd + d) * Smax + p);
      __syncthreads();
      if (on)
        for (int j = 0; j < K; ++j) {
          if (par[j] == j || p + VEC <= lo[j] || p >= hi[j]) continue;
          T* dst = vb + (((int64_t)(row0 + j) * Hkv + hk) * hd + d) * Smax + p;
          const u32x4 x = stage[par[j]][tid];
          if (p >= lo[j] && p + VEC <= hi[j]) {
            *reinterpret_cast<u32x4*>(dst) = x;
          } else {
            const T* e = reinterpret_cast<const T*>(&stage[par[j]][tid]);
            for (int q = 0; q < VEC; ++q)
              if (p + q >= lo[j] && p + q < hi[j]) dst[q] = e[q];
          }
        }
      __syncthreads();
    }
  }
}

}  // namespace

#define ST (hipStream_t)stream

extern "C" int a3v_beam_select(const float* logits, int64_t ld, const float* lse, const float* cum, const uint8_t* alive,
                               const int16_t* trans, int n_states, const int32_t* state, int G, int K, int V, float* cand_score,
                               int32_t* cand_beam, int32_t* cand_tok, void* stream) {
  if (!logits || !lse || !cum || !alive || !cand_score || !cand_beam || !cand_tok) return A3V_ERR_ARG;
  if (G <= 0 || G > 65535 || K < 1 || K > BEAM_MAX || V <= 0 || ld < V || (int64_t)K * V > INT_MAX) return A3V_ERR_ARG;
  if (trans && (!state || n_states <= 0 || n_states > 32767)) return A3V_ERR_ARG;
#define A3V_BEAM_SELECT(N2)                                                                                                              \
  case N2 / 2:                                                                                                                           \
    hipLaunchKernelGGL(beam_select_kernel<N2>, dim3(G), dim3(1024), 0, ST, logits, ld, lse, cum, alive, trans, n_states, state, K, V,    \
                       cand_score, cand_beam, cand_tok);                                                                                 \
    break;
  switch (K) {
    A3V_BEAM_SELECT(2) A3V_BEAM_SELECT(4) A3V_BEAM_SELECT(6) A3V_BEAM_SELECT(8) A3V_BEAM_SELECT(10) A3V_BEAM_SELECT(12)
    A3V_BEAM_SELECT(14) A3V_BEAM_SELECT(16)
  }
#undef A3V_BEAM_SELECT
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_beam_advance(const float* cand_score, const int32_t* cand_beam, const int32_t* cand_tok, int G, int K, int V, int eos,
                                int early_stopping, const float* len_div, int n_div, const int16_t* trans, int n_states,
                                const int32_t* base, const int32_t* limit, int pos_cap, float* cum, uint8_t* alive, int32_t* state,
                                int32_t* glen, uint8_t* done, int32_t* parent, int64_t* next_tok, int32_t* pos, const int64_t* tokens_in,
                                int64_t* tokens_out, int64_t ld_tok, int32_t* pool_n, int32_t* pool_added, float* pool_score,
                                float* pool_cum, int32_t* pool_len, int32_t* pool_seq, int64_t* pool_ids, void* stream) {
  if (!cand_score || !cand_beam || !cand_tok || !len_div || !base || !limit || !cum || !alive || !state || !glen || !done || !parent ||
      !next_tok || !pos || !tokens_in || !tokens_out || !pool_n || !pool_added || !pool_score || !pool_cum || !pool_len || !pool_seq || !pool_ids)
    return A3V_ERR_ARG;
  if (G <= 0 || G > 65535 || K < 1 || K > BEAM_MAX || V <= 0 || n_div < 2 || ld_tok <= 0 || pos_cap <= 0 || tokens_in == tokens_out) return A3V_ERR_ARG;
  if (trans && (n_states <= 0 || n_states > 32767)) return A3V_ERR_ARG;
  AdvanceArgs a;
  a.cand_score = cand_score; a.cand_beam = cand_beam; a.cand_tok = cand_tok;
  a.K = K; a.V = V; a.eos = eos; a.early = early_stopping; a.n_div = n_div; a.n_states = n_states; a.pos_cap = pos_cap;
  a.len_div = len_div; a.trans = trans; a.base = base; a.limit = limit;
  a.cum = cum; a.alive = alive; a.state = state; a.glen = glen; a.done = done; a.parent = parent; a.next_tok = next_tok; a.pos = pos;
  a.tokens_in = tokens_in; a.tokens_out = tokens_out; a.ld_tok = ld_tok;
  a.pool_n = pool_n; a.pool_added = pool_added; a.pool_score = pool_score; a.pool_cum = pool_cum; a.pool_len = pool_len;
  a.pool_seq = pool_seq; a.pool_ids = pool_ids;
  hipLaunchKernelGGL(beam_advance_kernel, dim3(G), dim3(256), 0, ST, a);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_kv_permute_tails(const void* const* k_ptrs, const void* const* vt_ptrs, int n_layers, const int32_t* parent,
                                    const int32_t* tail_lo, const int32_t* pos, int tail_max, int G, int K, int Hkv, int hd, int Smax,
                                    int dtype, void* stream) {
  if (!k_ptrs || !vt_ptrs || !parent || !tail_lo || !pos || n_layers <= 0 || G <= 0 || K < 1 || K > BEAM_MAX || tail_max < 0) return A3V_ERR_ARG;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  if (Hkv <= 0 || Hkv > 65535 || hd <= 0 || hd % 8 || Smax <= 0 || Smax % 8 || (int64_t)n_layers * G > 65535) return A3V_ERR_SHAPE;
  if (tail_max == 0) return A3V_OK;                              // nothing to move: nothing launched
  if (tail_max > Smax) tail_max = Smax;
  const dim3 g((tail_max + 7 + PT_CHUNK - 1) / PT_CHUNK, Hkv, n_layers * G);
  if (dtype == A3V_BF16)
    hipLaunchKernelGGL(kv_permute_tails_kernel<bf16_t>, g, dim3(PT_THREADS), 0, ST, k_ptrs, vt_ptrs, parent, tail_lo, pos, G, K, Hkv, hd, Smax);
  else
    hipLaunchKernelGGL(kv_permute_tails_kernel<float>, g, dim3(PT_THREADS), 0, ST, k_ptrs, vt_ptrs, parent, tail_lo, pos, G, K, Hkv, hd, Smax);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
