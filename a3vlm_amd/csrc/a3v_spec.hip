// Lookup decoding for gfx950: one decode step over Q = D + 1 query positions per cache row -- the row's last emitted token and D
// drafted ones (include/a3vlm_hip.h, "Lookup decoding").  Virtual row m = b * Q + j is query j of cache row b; pos / nq are device
// int32[B].  A query is LIVE when pos[b] >= 0, j < nq[b] and pos[b] + j lies inside the cache (the attention: inside sk_max); every
// other query is idle: it writes nothing into a cache and its outputs are zeros.
//
//  * rope_kv_spans_kernel<T>       : rope_kv_rows_kernel (a3v_ragged.hip) with the position pos[b] + j and cache row b for virtual
//    row m -- the same expressions element for element, so a live virtual row is bit-equal to a3v_rope_kvcache_rows at its position.
//  * attn_verify_rows_kernel<HD,G> : the walk of attn_decode_rows_kernel with G queries of ONE cache row per block: grid
//    (nsplit, H, B * ngroups), eight waves, every eighth 32-key tile of the block's key range per wave, K(t+1) and V^T(t) in flight
//    together, non-temporal loads.  A tile is loaded ONCE and applied to the G queries: G dot products per K row against the q rows
//    kept in LDS, G wave-private score rows, and per query its own key count n_j (mask by select, before any sum), its own (m, l)
//    and its own accumulators.  The walk of a wave ends at the largest n_j of the group; for a query whose keys end earlier the
//    remaining tiles are the identity on its state (mt = -inf: alpha = exp(0) = 1, every p = 0 by select), so its bits do not
//    depend on the queries behind it.  One merge of the eight waves through LDS per query, partials in the layout of the rows kernel
//    over the B * Q virtual rows, and ONE last-arriver counter per (cache row, group, head): the scheme of decode_combine_tail
//    (a3v_common.h: agent-coherent re-store of the block's partials, counter bump, the last block merges) for G outputs at once.
//    An idle query carries (m, l) = (-inf, 0) through all of it and its output is the selected 0, never 0 / 0.
//  * attn_verify_generic_kernel<T> : one wave per (virtual row, head): attn_rows_generic_kernel's walk with sk = pos[b] + j + 1.
//  * lookup_draft_rows_kernel      : prompt-lookup drafts from the row's own tokens (integer work, tests/spec_ref.py).
//  * accept_rows_kernel            : argmax of the Q logits rows of a cache row, then the emissions -- each one the token step of
//    generate_step_rows_kernel at cur[b] -- while the drafts agree (tests/spec_ref.py).
//  * a3v_llama_decode_step_verify  : the fused layer loop of a3v_llama_decode_step (a3v_decode.hip: a3v_decode_fused_layers) over B * Q
//    GEMV rows with the two kernels above as its attention stage (attend_verify below), six launches per layer.
#include "a3v_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(64) void rope_kv_spans_kernel(const T* __restrict__ qkv, int64_t ldqkv, T* __restrict__ q_out, int64_t ldq,
                                                           T* __restrict__ k_cache, T* __restrict__ vt_cache,
                                                           const float* __restrict__ cos_sin, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ nq, int Q, int H, int Hkv, int hd, int Smax) {
  const int slot = blockIdx.x, m = blockIdx.y;
  const int b = m / Q, j = m - b * Q;
  const int p0 = pos[b];
  const int p = p0 + j;
  const int half = hd / 2;
  if (p0 < 0 || j >= nq[b] || p >= Smax) {   // idle query: no cache write; its q row is zeros
    if (slot < H)
      for (int pr = threadIdx.x; pr < half; pr += 64) {
        T* dst = q_out + (int64_t)m * ldq + (int64_t)slot * hd + 2 * pr;
        Cvt<T>::st(dst, 0.f);
        Cvt<T>::st(dst + 1, 0.f);
      }
    return;
  }
  const T* src = qkv + (int64_t)m * ldqkv + (int64_t)slot * hd;
  for (int pr = threadIdx.x; pr < half; pr += 64) {
    const float a = Cvt<T>::ld(src + 2 * pr), bb = Cvt<T>::ld(src + 2 * pr + 1);
    if (slot < H + Hkv) {
      const float co = cos_sin[((int64_t)p * half + pr) * 2], si = cos_sin[((int64_t)p * half + pr) * 2 + 1];
      const float o0 = a * co - bb * si, o1 = a * si + bb * co;
      T* dst = slot < H ? q_out + (int64_t)m * ldq + (int64_t)slot * hd + 2 * pr
                        : k_cache + (((int64_t)b * Hkv + (slot - H)) * Smax + p) * hd + 2 * pr;
      Cvt<T>::st(dst, o0);
      Cvt<T>::st(dst + 1, o1);
    } else {
      T* dst = vt_cache + (((int64_t)b * Hkv + (slot - H - Hkv)) * hd + 2 * pr) * (int64_t)Smax + p;
      Cvt<T>::st(dst, a);
      Cvt<T>::st(dst + Smax, bb);
    }
  }
}

struct VerifyArgs {
  const void* q; const void* k; const void* vt; void* out;
  const int32_t* pos; const int32_t* nq;
  int64_t q_sb, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_sd, o_sb, o_sh;   // q_sb / o_sb: per VIRTUAL row; k_sb / v_sb: per cache row
  int Q, sk_max, H, Hkv;
  float scale;
};

// keys of query j of a row at position p0 with nqb live queries: p0 + j + 1, or 0 for an idle query
__device__ __forceinline__ int verify_keys(int p0, int nqb, int j, int Q, int sk_max) {
  return (p0 >= 0 && j < nqb && j < Q && p0 + j < sk_max) ? p0 + j + 1 : 0;
}

// sums / maxima over the 8 (16) lanes of a DPP half row (row), as the rows kernel
__device__ __forceinline__ float v8_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  return v;
}
__device__ __forceinline__ float v16_sum(float v) { v = v8_sum(v); return v + dpp_f<0x140>(v); }
__device__ __forceinline__ float v4_sum(float v) {          // over a quad
  v += dpp_f<0xB1>(v);
  return v + dpp_f<0x4E>(v);
}
__device__ __forceinline__ float v4_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  return fmaxf(v, dpp_f<0x4E>(v));
}

template <int HD, int G>
__global__ __launch_bounds__(512) void attn_verify_rows_kernel(VerifyArgs p, float* part, int nsplit, int chunk, int ngroups, int* counters) {
  constexpr int LPR = HD / 8;        // lanes per K row (16 B each)
  constexpr int RPW = 64 / LPR;      // K rows per wave-wide load
  constexpr int TK = 32;             // keys per tile: half the rows kernel's, so that 8 sets of accumulators fit beside the tiles
  constexpr int NKL = TK / RPW;      // K loads per tile
  constexpr int NVL = HD / 16;       // V^T loads per tile (16 d rows x 64 B per load)
  __shared__ __attribute__((aligned(16))) float sc_s[8][G][TK];
  __shared__ __attribute__((aligned(16))) float q_s[G][HD];
  __shared__ float comb[8][G][HD + 2];
  __shared__ int last_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y;
  const int b = blockIdx.z / ngroups, g = blockIdx.z - b * ngroups;
  const int j0 = g * G;
  const int p0 = p.pos[b], nqb = p.nq[b];
  const int m0 = b * p.Q + j0;                           // first virtual row of the group
  int cnt[G], cmax = 0;
#pragma unroll
  for (int j = 0; j < G; ++j) { cnt[j] = verify_keys(p0, nqb, j0 + j, p.Q, p.sk_max); cmax = max(cmax, cnt[j]); }
  if (cmax <= 0) {                   // every query of the group idle, the same for every block of it: the counter is not touched
    if (sp == 0)
      for (int i = tid; i < G * HD; i += 512) {
        const int j = i / HD, d = i - j * HD;
        if (j0 + j < p.Q) ((bf16_t*)p.out)[(m0 + j) * p.o_sb + h * p.o_sh + d] = f2bf(0.f);
      }
    return;
  }
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  for (int i = tid; i < G * HD; i += 512) {              // the q rows of the group (an idle query: whatever the row holds, never summed)
    const int j = i / HD, d = i - j * HD;
    q_s[j][d] = j0 + j < p.Q ? (float)((const bf16_t*)p.q)[(m0 + j) * p.q_sb + h * p.q_sh + d] : 0.f;
  }
  __syncthreads();
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh + (int64_t)kv_lo * p.k_ss;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh + kv_lo;
  int nj[G];                          // keys of query j inside this block's range (<= 0: none)
#pragma unroll
  for (int j = 0; j < G; ++j) nj[j] = min(cnt[j], kv_lo + chunk) - kv_lo;
  const int lo = wave * TK, hi = max(min(cmax, kv_lo + chunk) - kv_lo, 0);
  float m[G], l[G], acc[G][NVL];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    m[j] = -INFINITY; l[j] = 0.f;
#pragma unroll
    for (int v = 0; v < NVL; ++v) acc[j][v] = 0.f;
  }
  const int lr = lane / LPR, lc = (lane % LPR) * 8;
  const int dr = lane >> 2, c8 = (lane & 3) * 8;
  if (hi > lo) {
    const int last_vec = (hi - 1) & ~7;
    bf16x8 kk[NKL];
    auto load_k = [&](int t0) {
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        const int r = min(t0 + u * RPW + lr, hi - 1);
        const bf16x8* kp = reinterpret_cast<const bf16x8*>(K + (int64_t)r * p.k_ss + lc);
        kk[u] = __builtin_nontemporal_load(kp);            // the K / V^T stream is read once per step by one block
      }
    };
    load_k(lo);
    for (int t0 = lo; t0 < hi; t0 += 8 * TK) {
      bf16x8 vv[NVL];
      const int kvc = min(t0 + c8, last_vec);              // vectors past the wave's range re-read its last one (masked below)
#pragma unroll
      for (int v = 0; v < NVL; ++v) {
        const bf16x8* vp = reinterpret_cast<const bf16x8*>(VT + (int64_t)(v * 16 + dr) * p.v_sd + kvc);
        vv[v] = __builtin_nontemporal_load(vp);
      }
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const f32x4 qa = *reinterpret_cast<const f32x4*>(&q_s[j][lc]);
        const f32x4 qb = *reinterpret_cast<const f32x4*>(&q_s[j][lc + 4]);
        const float qv[8] = {qa[0], qa[1], qa[2], qa[3], qb[0], qb[1], qb[2], qb[3]};
#pragma unroll
        for (int u = 0; u < NKL; ++u) {
          float a = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) a = fmaf(qv[e], (float)kk[u][e], a);
          a = LPR == 16 ? v16_sum(a) : v8_sum(a);
          // the query's own key count, by select: a key at or beyond it (NaN, a rejected draft, a later draft) never reaches a sum
          if ((lane % LPR) == 0) sc_s[wave][j][u * RPW + lr] = (t0 + u * RPW + lr < nj[j]) ? a * p.scale : -INFINITY;
        }
      }
      if (t0 + 8 * TK < hi) load_k(t0 + 8 * TK);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // wave-private round trip through LDS: no barrier, in-order LDS
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const f32x4 sa = *reinterpret_cast<const f32x4*>(&sc_s[wave][j][c8]);
        const f32x4 sb = *reinterpret_cast<const f32x4*>(&sc_s[wave][j][c8 + 4]);
        const float s8[8] = {sa[0], sa[1], sa[2], sa[3], sb[0], sb[1], sb[2], sb[3]};
        float mt = s8[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) mt = fmaxf(mt, s8[e]);
        mt = v4_max(mt);
        const float mn = fmaxf(m[j], mt);                    // -inf only while the query has had no key yet
        const float alpha = (m[j] == -INFINITY) ? 0.f : __expf(m[j] - mn);
        float pe[8], ps = 0.f;
        const int nvalid = nj[j] - (t0 + c8);                // <= 0 for the vectors past the query's keys
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          pe[e] = e < nvalid ? __expf(s8[e] - mn) : 0.f;
          ps += pe[e];
        }
        l[j] = l[j] * alpha + ps;
#pragma unroll
        for (int v = 0; v < NVL; ++v) {
          float a = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) a = fmaf(pe[e], e < nvalid ? (float)vv[v][e] : 0.f, a);   // the cache tail may hold anything
          acc[j][v] = acc[j][v] * alpha + a;
        }
        m[j] = mn;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the score rows are read before the next tile overwrites them
    }
  }
#pragma unroll
  for (int j = 0; j < G; ++j) {
#pragma unroll
    for (int v = 0; v < NVL; ++v) acc[j][v] = v4_sum(acc[j][v]);
    l[j] = v4_sum(l[j]);
    if ((lane & 3) == 0) {
#pragma unroll
      for (int v = 0; v < NVL; ++v) comb[wave][j][v * 16 + dr] = acc[j][v];
    }
    if (lane == 0) { comb[wave][j][HD] = m[j]; comb[wave][j][HD + 1] = l[j]; }
  }
  __syncthreads();
  for (int i = tid; i < G * HD; i += 512) {
    const int j = i / HD, d = i - j * HD;
    if (j0 + j >= p.Q) continue;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 8; ++w) M = fmaxf(M, comb[w][j][HD]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const float mw = comb[w][j][HD];
      const float sw = (mw == -INFINITY) ? 0.f : __expf(mw - M);
      o += sw * comb[w][j][d];
      L += sw * comb[w][j][HD + 1];
    }
    if (nsplit == 1) {
      ((bf16_t*)p.out)[(m0 + j) * p.o_sb + h * p.o_sh + d] = f2bf(L > 0.f ? o / L : 0.f);   // an idle query: L = 0
    } else {                                                              // an empty range: o = 0, M = -inf, L = 0
      float* po = part + ((int64_t)((m0 + j) * p.H + h) * nsplit + sp) * (HD + 2);
      po[d] = o;
      if (d == 0) { po[HD] = M; po[HD + 1] = L; }
    }
  }
  if (nsplit == 1) return;
  // The last-arriver combine of decode_combine_tail (a3v_common.h) for the G partials of the block: re-store them agent-coherently
  // (the splits of a head may sit on different XCDs), wait for the acknowledgement, bump the (cache row, group, head) counter; the
  // block that arrives last merges the nsplit partials of every query of the group and leaves the counter zero.
  __syncthreads();
  for (int i = tid; i < G * (HD + 2); i += 512) {
    const int j = i / (HD + 2), e = i - j * (HD + 2);
    if (j0 + j >= p.Q) continue;
    float* po = part + ((int64_t)((m0 + j) * p.H + h) * nsplit + sp) * (HD + 2);
    st_agent(po + e, po[e]);
  }
  agent_wait();
  __syncthreads();
  if (tid == 0) {
    int* ctr = counters + (int64_t)blockIdx.z * p.H + h;
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = old == nsplit - 1;
    if (old == nsplit - 1) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last_s) return;
  for (int i = tid; i < G * HD; i += 512) {
    const int j = i / HD, d = i - j * HD;
    if (j0 + j >= p.Q) continue;
    const float* pp = part + (int64_t)((m0 + j) * p.H + h) * nsplit * (HD + 2);
    float o = 0.f, L = 0.f;
    if (nsplit <= 8) {                                  // all loads in flight at once: one memory round trip
      float mv[8], av[8], lv[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float* qq = pp + (s < nsplit ? s : nsplit - 1) * (HD + 2);
        mv[s] = ld_agent_issue(qq + HD);
        av[s] = ld_agent_issue(qq + d);
        lv[s] = ld_agent_issue(qq + HD + 1);
      }
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(mv[0]), "+v"(mv[1]), "+v"(mv[2]), "+v"(mv[3]), "+v"(mv[4]), "+v"(mv[5]), "+v"(mv[6]), "+v"(mv[7])::"memory");
      asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]), "+v"(av[6]), "+v"(av[7]));
      asm volatile("" : "+v"(lv[0]), "+v"(lv[1]), "+v"(lv[2]), "+v"(lv[3]), "+v"(lv[4]), "+v"(lv[5]), "+v"(lv[6]), "+v"(lv[7]));
      float M = -INFINITY;
#pragma unroll
      for (int s = 0; s < 8; ++s) if (s < nsplit) M = fmaxf(M, mv[s]);
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (s < nsplit) {
          const float w = (mv[s] == -INFINITY) ? 0.f : __expf(mv[s] - M);
          o += w * av[s];
          L += w * lv[s];
        }
    } else {
      float M = -INFINITY;
      for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ld_agent(pp + s * (HD + 2) + HD));
      for (int s = 0; s < nsplit; ++s) {
        const float ms = ld_agent(pp + s * (HD + 2) + HD);
        const float a1 = ld_agent(pp + s * (HD + 2) + d);
        const float l1 = ld_agent(pp + s * (HD + 2) + HD + 1);
        const float w = (ms == -INFINITY) ? 0.f : __expf(ms - M);
        o += w * a1;
        L += w * l1;
      }
    }
    ((bf16_t*)p.out)[(m0 + j) * p.o_sb + h * p.o_sh + d] = f2bf(L > 0.f ? o / L : 0.f);
  }
}

// one wave per (head, virtual row): the walk of attn_rows_generic_kernel (a3v_ragged.hip) over pos[b] + j + 1 keys of cache row b
template <typename T>
__global__ __launch_bounds__(64) void attn_verify_generic_kernel(VerifyArgs p, int hd) {
  __shared__ float pbuf[64];
  __shared__ float qs[256];
  const int lane = threadIdx.x;
  const int h = blockIdx.x, mrow = blockIdx.y;
  const int b = mrow / p.Q, j = mrow - b * p.Q;
  const int hk = h / (p.H / p.Hkv);
  const int kv_end = verify_keys(p.pos[b], p.nq[b], j, p.Q, p.sk_max);
  T* O = (T*)p.out + mrow * p.o_sb + h * p.o_sh;
  if (kv_end <= 0) {
    for (int d = lane; d < hd; d += 64) Cvt<T>::st(O + d, 0.f);
    return;
  }
  const T* Q = (const T*)p.q + mrow * p.q_sb + h * p.q_sh;
  const T* K = (const T*)p.k + b * p.k_sb + hk * p.k_sh;
  const T* VT = (const T*)p.vt + b * p.v_sb + hk * p.v_sh;
  for (int d = lane; d < hd; d += 64) qs[d] = Cvt<T>::ld(Q + d);
  __syncthreads();
  float m = -INFINITY, l = 0.f;
  float o[4] = {0.f, 0.f, 0.f, 0.f};   // d = lane + 64*i
  for (int kv0 = 0; kv0 < kv_end; kv0 += 64) {
    const int kv = kv0 + lane;
    float s = -INFINITY;
    if (kv < kv_end) {
      const T* kr = K + (int64_t)kv * p.k_ss;
      float a = 0.f;
      for (int d = 0; d < hd; ++d) a = fmaf(qs[d], Cvt<T>::ld(kr + d), a);
      s = a * p.scale;
    }
    const float mt = wave_max(s);
    const float mn = fmaxf(m, mt);
    const float alpha = __expf(m - mn);   // m = -inf on the first tile -> 0
    const float pv = (kv < kv_end) ? __expf(s - mn) : 0.f;
    l = l * alpha + wave_sum(pv);
    m = mn;
    __syncthreads();
    pbuf[lane] = pv;
    __syncthreads();
    const int cnt = min(64, kv_end - kv0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = lane + 64 * i;
      if (d < hd) {
        const T* vr = VT + (int64_t)d * p.v_sd + kv0;
        float a = o[i] * alpha;
        for (int jj = 0; jj < cnt; ++jj) a = fmaf(pbuf[jj], Cvt<T>::ld(vr + jj), a);
        o[i] = a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < hd) Cvt<T>::st(O + d, o[i] / l);
  }
}

// Prompt-lookup drafts of one cache row per block.  c = tokens[b, 0 .. cur): for n = max_ngram .. 1 the largest i with
// i + n <= cur - 1 and c[i .. i+n) == c[cur-n .. cur); the first n with a match wins and the drafts are c[i+n ..].
__global__ __launch_bounds__(256) void lookup_draft_rows_kernel(const int64_t* __restrict__ tokens, int64_t ld_tok, const int32_t* __restrict__ cur,
                                                                const int32_t* __restrict__ limit, const int32_t* __restrict__ pos,
                                                                const uint8_t* __restrict__ stopped, const int64_t* __restrict__ next_tok,
                                                                int D, int max_ngram, int Smax, int64_t* __restrict__ x,
                                                                int32_t* __restrict__ nq) {
  __shared__ int best_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Q = D + 1;
  const int c = cur[b], p0 = pos[b];
  const bool running = !stopped[b] && p0 >= 0 && c >= 1 && c <= ld_tok;     // block-uniform
  const int64_t* t = tokens + (int64_t)b * ld_tok;
  int at = -1;                                                              // index of the first draft
  if (running) {
    for (int n = min(max_ngram, c - 1); n >= 1 && at < 0; --n) {
      if (tid == 0) best_s = -1;
      __syncthreads();
      int best = -1;
      for (int i = tid; i + n <= c - 1; i += 256) {
        bool hit = true;
        for (int e = 0; e < n && hit; ++e) hit = t[i + e] == t[c - n + e];
        if (hit) best = i;                                                  // ascending i: the thread's latest match
      }
      if (best >= 0) atomicMax(&best_s, best);
      __syncthreads();
      if (best_s >= 0) at = best_s + n;
      __syncthreads();
    }
  }
  if (tid != 0) return;
  int nd = 0;
  if (at >= 0) nd = max(min(min(D, c - at), min(limit[b] - 1 - c, Smax - 1 - p0)), 0);
  x[(int64_t)b * Q] = next_tok[b];
  for (int e = 1; e < Q; ++e) x[(int64_t)b * Q + e] = e <= nd ? t[at + e - 1] : 0;
  nq[b] = 1 + nd;
}

// One block per cache row: argmax (first index on ties, as generate_step_rows_kernel) of the logits rows of its live queries, then
// thread 0 emits t_0, and t_j while j <= nd and t_{j-1} == x[b, j]; every emission is that kernel's token step at cur[b].
__global__ __launch_bounds__(1024) void accept_rows_kernel(const float* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ x,
                                                           const int32_t* __restrict__ nq, int Q, int64_t* __restrict__ tokens, int64_t ld_tok,
                                                           int32_t* __restrict__ cur, const int32_t* __restrict__ limit, int pos_base,
                                                           const int64_t* __restrict__ stop_seq, const int32_t* __restrict__ stop_off,
                                                           int n_stop, uint8_t* __restrict__ stopped, int64_t* __restrict__ stop_pos,
                                                           int64_t* __restrict__ next_tok, int32_t* __restrict__ pos,
                                                           unsigned long long* __restrict__ stats) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  __shared__ int tj[8];
  const int row = blockIdx.x;
  if (stopped[row]) {                  // block-uniform: a stopped row is not touched
    if (threadIdx.x == 0) { next_tok[row] = 0; pos[row] = -1; }
    return;
  }
  const int nd = min(max(nq[row], 1), Q) - 1;
  for (int j = 0; j <= nd; ++j) {
    float best = -INFINITY;
    int idx = 0x7fffffff;
    const float* r = logits + ((int64_t)row * Q + j) * ld;
    auto take = [&](float v, int i) { if (v > best || (v == best && i < idx)) { best = v; idx = i; } };
    const bool vec = ((reinterpret_cast<uintptr_t>(r) & 15) == 0);
    const int V4 = vec ? V / 4 : 0;
    for (int i0 = threadIdx.x; i0 < V4; i0 += 4 * 1024) {
      f32x4 xx[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * 1024;
        xx[q] = i < V4 ? reinterpret_cast<const f32x4*>(r)[i] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) take(xx[q][e], (i0 + q * 1024) * 4 + e);
    }
    for (int i = V4 * 4 + threadIdx.x; i < V; i += 1024) take(r[i], i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    __syncthreads();                   // bv / bi of the previous query are read
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 16; ++w)
        if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
      tj[j] = idx == 0x7fffffff ? 0 : idx;
    }
  }
  if (threadIdx.x != 0) return;
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
  bool st = false;
  int64_t sp = 0, next = 0;
  int emitted = 0;
  for (int j = 0; j <= nd && !st; ++j) {
    if (j > 0 && (int64_t)tj[j - 1] != xr[j]) break;   // a draft the model did not produce ends the run
    if (c >= ld_tok) { st = true; break; }             // (an emission is one token step: nothing writable stops the row)
    next = tj[j];
    trow[c] = next;
    sp = (int64_t)c + 1;
    for (int s = 0; s < n_stop; ++s) {
      const int o = stop_off[s], n = stop_off[s + 1] - o;
      if (c + 1 - n < 0 || st) continue;
      bool hit = true;
      for (int k = 0; k < n && hit; ++k) hit = trow[c + 1 - n + k] == stop_seq[o + k];
      if (hit) { sp = c + 1 - n; st = true; }
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

// queries per block: the power of two that holds all Q of a row (every tile of a row is then loaded once per head); at hd 128 at
// most 4 -- 8 sets of accumulators beside the tiles need more than the 256 registers of a wave at two waves per SIMD (the compiler
// spills 164 bytes per lane) -- so Q = 5..8 run there as two groups of 4 over the grid's z dimension
inline int verify_group(int hd, int Q) {
  const int cap = hd == 128 ? 4 : 8;
  int g = 1;
  while (g < Q && g < cap) g *= 2;
  return g;
}

template <int HD, int G>
void launch_verify(const VerifyArgs& p, float* scratch, int ns, int ch, int B, int* counters, hipStream_t st) {
  const int ngroups = (p.Q + G - 1) / G;
  hipLaunchKernelGGL((attn_verify_rows_kernel<HD, G>), dim3(ns, p.H, B * ngroups), dim3(512), 0, st, p, scratch, ns, ch, ngroups, counters);
}

}  // namespace

extern "C" int a3v_rope_kvcache_spans(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                                      const float* cos_sin, const int32_t* pos, const int32_t* nq, int B, int Q, int H, int Hkv, int hd,
                                      int Smax, int dtype, void* stream) {
  if (!qkv || !q_out || !k_cache || !vt_cache || !cos_sin || !pos || !nq || B <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8 || (int64_t)B * Q > 65535) return A3V_ERR_SHAPE;
  if (hd <= 0 || hd % 8 || hd > 128 || ldqkv % 8 || ldq % 8 || Smax <= 0) return A3V_ERR_SHAPE;
  if (ldqkv < (int64_t)(H + 2 * Hkv) * hd || ldq < (int64_t)H * hd) return A3V_ERR_SHAPE;
  const dim3 g(H + 2 * Hkv, B * Q);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_BF16)
    hipLaunchKernelGGL(rope_kv_spans_kernel<bf16_t>, g, dim3(64), 0, st, (const bf16_t*)qkv, ldqkv, (bf16_t*)q_out, ldq, (bf16_t*)k_cache,
                       (bf16_t*)vt_cache, cos_sin, pos, nq, Q, H, Hkv, hd, Smax);
  else if (dtype == A3V_F32)
    hipLaunchKernelGGL(rope_kv_spans_kernel<float>, g, dim3(64), 0, st, (const float*)qkv, ldqkv, (float*)q_out, ldq, (float*)k_cache,
                       (float*)vt_cache, cos_sin, pos, nq, Q, H, Hkv, hd, Smax);
  else return A3V_ERR_DTYPE;
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_attention_verify_rows_splits(int B, int H, int sk_max) {
  if (B <= 0 || H <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  return ns;
}

extern "C" int64_t a3v_attention_verify_rows_scratch_floats(int B, int Q, int H, int hd, int sk_max) {
  if (B <= 0 || Q <= 0 || H <= 0 || sk_max <= 0) return 0;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  return (int64_t)B * Q * H * ns * (hd + 2);
}

extern "C" int a3v_attention_verify_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* pos, const int32_t* nq,
                                         int sk_max, int B, int Q, int H, int Hkv, int hd, const int64_t* strides, float* scratch,
                                         int* counters, int dtype, void* stream) {
  if (!q || !k || !vt || !out || !pos || !nq || !strides || B <= 0 || H <= 0 || Hkv <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8 || (int64_t)B * Q > 65535) return A3V_ERR_SHAPE;
  if (H % Hkv || hd <= 0 || hd > 256) return A3V_ERR_SHAPE;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  // the caches are [B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] in whatever strides: a V^T row (strides[8]) and a K head (strides[4]) bound sk_max
  if (sk_max > strides[8] || (int64_t)sk_max * strides[5] > strides[4]) return A3V_ERR_SHAPE;
  VerifyArgs p;
  p.q = q; p.k = k; p.vt = vt; p.out = out; p.pos = pos; p.nq = nq;
  p.q_sb = strides[0]; p.q_sh = strides[2];
  p.k_sb = strides[3]; p.k_sh = strides[4]; p.k_ss = strides[5];
  p.v_sb = strides[6]; p.v_sh = strides[7]; p.v_sd = strides[8];
  p.o_sb = strides[9]; p.o_sh = strides[11];
  p.Q = Q; p.sk_max = sk_max; p.H = H; p.Hkv = Hkv;
  p.scale = 1.0f / sqrtf((float)hd);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_F32 || (hd != 64 && hd != 128)) {
    if (dtype == A3V_F32) hipLaunchKernelGGL(attn_verify_generic_kernel<float>, dim3(H, B * Q), dim3(64), 0, st, p, hd);
    else hipLaunchKernelGGL(attn_verify_generic_kernel<bf16_t>, dim3(H, B * Q), dim3(64), 0, st, p, hd);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  if (!scratch || !counters) return A3V_ERR_ARG;
  for (int i = 0; i < 12; ++i)
    if (i != 1 && i != 10 && (strides[i] % 8)) return A3V_ERR_SHAPE;      // 16-B vector access (the Sq strides are not used)
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt)) & 15) return A3V_ERR_SHAPE;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  const int G = verify_group(hd, Q);
  if (hd == 64) {
    if (G == 1) launch_verify<64, 1>(p, scratch, ns, ch, B, counters, st);
    else if (G == 2) launch_verify<64, 2>(p, scratch, ns, ch, B, counters, st);
    else if (G == 4) launch_verify<64, 4>(p, scratch, ns, ch, B, counters, st);
    else launch_verify<64, 8>(p, scratch, ns, ch, B, counters, st);
  } else {
    if (G == 1) launch_verify<128, 1>(p, scratch, ns, ch, B, counters, st);
    else if (G == 2) launch_verify<128, 2>(p, scratch, ns, ch, B, counters, st);
    else launch_verify<128, 4>(p, scratch, ns, ch, B, counters, st);
  }
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_lookup_draft_rows(const int64_t* tokens, int64_t ld_tok, const int32_t* cur, const int32_t* limit, const int32_t* pos,
                                     const uint8_t* stopped, const int64_t* next_tok, int B, int D, int max_ngram, int Smax, int64_t* x,
                                     int32_t* nq, void* stream) {
  if (!tokens || !cur || !limit || !pos || !stopped || !next_tok || !x || !nq || B <= 0 || ld_tok <= 0) return A3V_ERR_ARG;
  if (D < 0 || D > 7 || max_ngram < 1 || Smax <= 0) return A3V_ERR_SHAPE;
  hipLaunchKernelGGL(lookup_draft_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tokens, ld_tok, cur, limit, pos, stopped, next_tok,
                     D, max_ngram, Smax, x, nq);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_accept_rows(const float* logits, int64_t ld, int B, int Q, int V, const int64_t* x, const int32_t* nq, int64_t* tokens,
                               int64_t ld_tok, int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq,
                               const int32_t* stop_off, int n_stop, uint8_t* stopped, int64_t* stop_pos, int64_t* next_tok, int32_t* pos,
                               int64_t* stats, void* stream) {
  if (!logits || !x || !nq || !tokens || !cur || !limit || !stopped || !stop_pos || !next_tok || !pos) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld_tok <= 0 || pos_base < 0 || n_stop < 0 || (n_stop > 0 && (!stop_seq || !stop_off))) return A3V_ERR_ARG;
  if (Q < 1 || Q > 8) return A3V_ERR_SHAPE;
  hipLaunchKernelGGL(accept_rows_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ld, V, x, nq, Q, tokens, ld_tok, cur, limit,
                     pos_base, stop_seq, stop_off, n_stop, stopped, stop_pos, next_tok, pos, (unsigned long long*)stats);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

namespace {
// cache rows per GEMV chunk: everything up to 16 virtual rows, else whole cache rows of Q queries that fit 16 GEMV rows
inline int verify_chunk_rows(int B, int Q) { return B * Q <= 16 ? B : 16 / Q; }
}  // namespace

extern "C" int a3v_llama_decode_step_verify_form(int B, int Q, int dim, int H, int Hkv, int hd, int ffn, int w8) {
  if (B <= 0 || Q < 1 || Q > 8 || B * Q > 32) return 0;
  const int Bc = verify_chunk_rows(B, Q);
  if (B * H * (int)sizeof(int) * ((Q + 3) / 4) > A3V_WS_SSQ - A3V_WS_ATTN_COUNTERS) return 0;
  return a3v_llama_decode_step_rows_form(Bc * Q, dim, H, Hkv, hd, ffn, w8) == 2 ? 2 : 0;
}

namespace {
// what a3v_decode_fused_layers (a3v_decode.hip) runs between the plain-store qkv GEMV and the wo GEMV over the chunk's nbr * Q GEMV
// rows: RoPE + cache write of the rows' spans, then the verify attention -- six launches per layer
struct VerifyStage { const float* cos_sin; const int32_t* pos; const int32_t* nq; int Q, sk_max; };
int attend_verify(const void* ctx, const a3v_decode_chunk& c) {
  const VerifyStage& s = *(const VerifyStage*)ctx;
  const int64_t ldq = c.strides[0];
  const int32_t* pc = s.pos + c.b0;
  const int32_t* nc = s.nq + c.b0;
  bf16_t* kc = (bf16_t*)c.L->k_cache + c.b0 * c.kv_row;
  bf16_t* vc = (bf16_t*)c.L->vt_cache + c.b0 * c.kv_row;
  int rc;
  if ((rc = a3v_rope_kvcache_spans(c.q, ldq, c.q, ldq, kc, vc, s.cos_sin, pc, nc, c.nbr, s.Q, c.H, c.Hkv, c.hd, c.Smax, A3V_BF16, c.stream))) return rc;
  return a3v_attention_verify_rows(c.q, kc, vc, c.att, pc, nc, s.sk_max, c.nbr, s.Q, c.H, c.Hkv, c.hd, c.strides, c.scratch, c.counters, A3V_BF16,
                                   c.stream);
}
}  // namespace

extern "C" int a3v_llama_decode_step_verify(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                                            float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos,
                                            const int32_t* nq, int pos_max, int B, int Q, int dim, int H, int Hkv, int hd, int ffn,
                                            int Smax, float eps, void* stream) {
  if (!layers || n_layers <= 0 || !h || !xn || !qkv || !att || !act || !attn_scratch || !skinny_ws || !cos_sin || !pos || !nq) return A3V_ERR_ARG;
  if (B <= 0 || Q < 1 || Q > 8 || B * Q > 32 || pos_max < 0 || pos_max >= Smax || Smax % 8) return A3V_ERR_SHAPE;
  int rc, w8;
  if ((rc = a3v_decode_layer_table(layers, n_layers, true, &w8))) return rc;
  if (a3v_llama_decode_step_verify_form(B, Q, dim, H, Hkv, hd, ffn, w8) != 2) return A3V_ERR_SHAPE;    // nothing launched
  const VerifyStage ctx{cos_sin, pos, nq, Q, pos_max + Q < Smax ? pos_max + Q : Smax};
  // the rope and attention launches of a chunk see whole cache rows
  const a3v_decode_stage stage{verify_chunk_rows(B, Q), Q, nullptr, nullptr, nullptr, 0, 0, attend_verify, &ctx};
  return a3v_decode_fused_layers(layers, n_layers, w8, h, qkv, att, act, attn_scratch, skinny_ws, B, dim, H, Hkv, hd, ffn, Smax, eps, stage, stream);
}
