// Ragged decode for gfx950: every batch row at its own cache position (include/a3vlm_hip.h, "Ragged decode").  All position arrays
// are device int32[B]; an idle row (negative position, or one outside the cache) writes nothing into a cache and produces zeros.
//
//  * rope_kv_rows_kernel<T>        : rope_kv_small_kernel (a3v_rowops.hip) at S = 1 with the position read per row -- the same
//    expressions element for element, so a row is bit-equal to a3v_rope_kvcache at that position.
//  * attn_decode_rows_kernel<HD>   : the walk of attn_decode_wave_kernel (a3v_attn.hip) restated with the row's own key count: grid
//    (nsplit, H, B), eight waves, every eighth 64-key tile of the block's range per wave, K(t+1) and V^T(t) in flight together,
//    non-temporal loads, masking by select, wave-private online softmax, one merge of the eight waves through LDS, split-KV with
//    the last-arriver combine of a3v_common.h.  The split plan comes from sk_max (host); a block's range holds
//    n = min(sk[b], lo + chunk) - lo keys, an empty range contributes (m, l) = (-inf, 0) and still arrives at the combine.  Split 0
//    of a running row holds at least one key, so the combined l is > 0; an idle row (every block of it sees the same sk[b] <= 0)
//    leaves before the combine with its counter untouched and split 0 writes the zeros.
//  * attn_rows_generic_kernel<T>   : attn_generic_kernel at Sq = 1 with the row's key count (fp32 parity path, odd head dims).
//  * generate_step_rows_kernel     : generate_step_kernel with per-row cur / limit, no text_mask; emits the next id and its position.
//  * a3v_llama_decode_step_rows    : the fused layer loop of a3v_llama_decode_step (a3v_decode.hip: a3v_decode_fused_layers) with those
//    kernels as its attention stage (attend_rows below), six launches per layer.
//  * shared prompt keys (the SH = true instantiations of the two attention kernels, a3v_attention_decode_rows_shared): a row's
//    64-key tiles below its shared length are read from another cache row.  Only the base pointer of a tile differs -- a
//    wave-uniform select of one 64-bit offset -- so the walk, the masks and the merges are the expressions above in their order.
//    Every tile starts at a multiple of 64 in absolute position (chunk is a multiple of 64) and the shared length is one too, so
//    a tile, its clamped K re-reads and its 16-byte V^T vectors lie in one row.  The SH = false instantiations take RowsAttnArgs
//    as before: their code does not change.
//  * kv_copy_span_kernel<T>        : positions [lo, hi) of one cache row into other rows, every layer in one launch.
#include "a3v_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(64) void rope_kv_rows_kernel(const T* __restrict__ qkv, int64_t ldqkv, T* __restrict__ q_out, int64_t ldq,
                                                          T* __restrict__ k_cache, T* __restrict__ vt_cache,
                                                          const float* __restrict__ cos_sin, const int32_t* __restrict__ pos, int H,
                                                          int Hkv, int hd, int Smax) {
  const int slot = blockIdx.x, b = blockIdx.y;
  const int p = pos[b];
  const int half = hd / 2;
  if (p < 0 || p >= Smax) {            // idle row: no cache write; its q row is zeros
    if (slot < H)
      for (int pr = threadIdx.x; pr < half; pr += 64) {
        T* dst = q_out + (int64_t)b * ldq + (int64_t)slot * hd + 2 * pr;
        Cvt<T>::st(dst, 0.f);
        Cvt<T>::st(dst + 1, 0.f);
      }
    return;
  }
  const T* src = qkv + (int64_t)b * ldqkv + (int64_t)slot * hd;
  for (int pr = threadIdx.x; pr < half; pr += 64) {
    const float a = Cvt<T>::ld(src + 2 * pr), bb = Cvt<T>::ld(src + 2 * pr + 1);
    if (slot < H + Hkv) {
      const float co = cos_sin[((int64_t)p * half + pr) * 2], si = cos_sin[((int64_t)p * half + pr) * 2 + 1];
      const float o0 = a * co - bb * si, o1 = a * si + bb * co;
      T* dst = slot < H ? q_out + (int64_t)b * ldq + (int64_t)slot * hd + 2 * pr
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

struct RowsAttnArgs {
  const void* q; const void* k; const void* vt; void* out;
  const int32_t* sk;
  int64_t q_sb, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_sd, o_sb, o_sh;
  int sk_add, sk_max, H, Hkv;        // keys of row b = min(sk[b] + sk_add, sk_max)
  float scale;
};
// + the shared-prefix arrays.  k / vt are the caches of ALL Btot rows; batch index b of the launch is cache row row0 + b, and
// src_row[b] is a cache row (absolute), read as the own row when outside [0, Btot).
struct RowsSharedArgs : RowsAttnArgs {
  const int32_t* src_row; const int32_t* shared;
  int row0, Btot;
};
template <bool SH> struct RowsArgsOf { using type = RowsAttnArgs; };
template <> struct RowsArgsOf<true> { using type = RowsSharedArgs; };

// effective shared length of a row with skb keys: min(shared, skb) rounded down to a multiple of 64; 0 for the own row
__device__ __forceinline__ int shared_len(const RowsSharedArgs& p, int b, int skb, int* src) {
  const int own = p.row0 + b;
  int s = p.src_row[b];
  if (s < 0 || s >= p.Btot) s = own;
  *src = s;
  return s == own ? 0 : max(min(p.shared[b], skb), 0) & ~63;
}

// sums / maxima over the 8 (16) lanes of a DPP half row (row): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ float r8_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  return v;
}
__device__ __forceinline__ float r16_sum(float v) { v = r8_sum(v); return v + dpp_f<0x140>(v); }
__device__ __forceinline__ float r8_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  return v;
}

template <int HD, bool SH>
__global__ __launch_bounds__(512) void attn_decode_rows_kernel(typename RowsArgsOf<SH>::type p, float* part, int nsplit, int chunk,
                                                               int* counters) {
  constexpr int LPR = HD / 8;        // lanes per K row (16 B each)
  constexpr int RPW = 64 / LPR;      // K rows per wave-wide load
  constexpr int NKL = 64 / RPW;      // K loads per 64-key tile
  constexpr int NVL = HD / 8;        // V^T loads per tile (8 d rows x 128 B per load)
  __shared__ __attribute__((aligned(16))) float sc_s[8][64];
  __shared__ float comb[8][HD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int sk0 = p.sk[b];
  const int skb = sk0 >= p.sk_max ? p.sk_max : min(sk0 + p.sk_add, p.sk_max);
  if (skb <= 0) {                    // idle row, the same for every block of the row: none of them touches the counter
    if (sp == 0 && tid < HD) ((bf16_t*)p.out)[b * p.o_sb + h * p.o_sh + tid] = f2bf(0.f);
    return;
  }
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int n = min(skb, kv_lo + chunk) - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * nsplit + sp) * (HD + 2);
  const bf16_t* Q = (const bf16_t*)p.q + b * p.q_sb + h * p.q_sh;
  int64_t row = b, dk = 0, dv = 0;                        // the own cache row; element offsets from it to the source row
  int sh_rel = 0;                                          // tiles of the range that start below it come from the source row
  if constexpr (SH) {
    int src;
    sh_rel = shared_len(p, b, skb, &src) - kv_lo;
    row = p.row0 + b;
    dk = (src - row) * p.k_sb;
    dv = (src - row) * p.v_sb;
  }
  const bf16_t* K = (const bf16_t*)p.k + row * p.k_sb + hk * p.k_sh + (int64_t)kv_lo * p.k_ss;
  const bf16_t* VT = (const bf16_t*)p.vt + row * p.v_sb + hk * p.v_sh + kv_lo;
  const int lo = wave * 64, hi = max(n, 0);
  float m = -INFINITY, l = 0.f, acc[NVL];
#pragma unroll
  for (int j = 0; j < NVL; ++j) acc[j] = 0.f;
  const int lr = lane / LPR, lc = (lane % LPR) * 8;
  const int dr = lane >> 3, c8 = (lane & 7) * 8;
  if (hi > lo) {
    float qv[8];
    load8(Q + lc, qv);
    const int last_vec = (hi - 1) & ~7;
    bf16x8 kk[NKL];
    auto load_k = [&](int t0) {
      const bf16_t* Kt = K;
      if constexpr (SH) Kt = K + (t0 < sh_rel ? dk : 0);    // wave-uniform: t0 is a multiple of 64, the clamped rows stay in the tile
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        const int r = min(t0 + u * RPW + lr, hi - 1);
        const bf16x8* kp = reinterpret_cast<const bf16x8*>(Kt + (int64_t)r * p.k_ss + lc);
        kk[u] = __builtin_nontemporal_load(kp);            // the K / V^T stream is read once per step by one block
      }
    };
    load_k(lo);
    for (int t0 = lo; t0 < hi; t0 += 512) {
      bf16x8 vv[NVL];
      const int kvc = min(t0 + c8, last_vec);              // vectors past the wave's range re-read its last one (masked below)
      const bf16_t* Vt = VT;
      if constexpr (SH) Vt = VT + (t0 < sh_rel ? dv : 0);   // last_vec >= t0: the re-read vector lies in the tile too
#pragma unroll
      for (int j = 0; j < NVL; ++j) {
        const bf16x8* vp = reinterpret_cast<const bf16x8*>(Vt + (int64_t)(j * 8 + dr) * p.v_sd + kvc);
        vv[j] = __builtin_nontemporal_load(vp);
      }
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(qv[e], (float)kk[u][e], a);
        a = LPR == 16 ? r16_sum(a) : r8_sum(a);
        if ((lane % LPR) == 0) sc_s[wave][u * RPW + lr] = (t0 + u * RPW + lr < hi) ? a * p.scale : -INFINITY;
      }
      if (t0 + 512 < hi) load_k(t0 + 512);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // wave-private round trip through LDS: no barrier, in-order LDS
      const f32x4 sa = *reinterpret_cast<const f32x4*>(&sc_s[wave][c8]);
      const f32x4 sb = *reinterpret_cast<const f32x4*>(&sc_s[wave][c8 + 4]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      float s8[8] = {sa[0], sa[1], sa[2], sa[3], sb[0], sb[1], sb[2], sb[3]};
      float mt = s8[0];
#pragma unroll
      for (int e = 1; e < 8; ++e) mt = fmaxf(mt, s8[e]);
      mt = r8_max(mt);
      const float mn = fmaxf(m, mt);                         // finite: the tile holds at least one key of the range
      const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
      float pe[8], ps = 0.f;
      const int nvalid = hi - (t0 + c8);                     // <= 0 for the vectors past the range
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pe[e] = e < nvalid ? __expf(s8[e] - mn) : 0.f;
        ps += pe[e];
      }
      l = l * alpha + ps;
#pragma unroll
      for (int j = 0; j < NVL; ++j) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(pe[e], e < nvalid ? (float)vv[j][e] : 0.f, a);   // the cache tail may hold anything
        acc[j] = acc[j] * alpha + a;
      }
      m = mn;
    }
  }
#pragma unroll
  for (int j = 0; j < NVL; ++j) acc[j] = r8_sum(acc[j]);
  l = r8_sum(l);
  if ((lane & 7) == 0) {
#pragma unroll
    for (int j = 0; j < NVL; ++j) comb[wave][j * 8 + dr] = acc[j];
  }
  if (lane == 0) { comb[wave][HD] = m; comb[wave][HD + 1] = l; }
  __syncthreads();
  if (tid < HD) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 8; ++w) M = fmaxf(M, comb[w][HD]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const float mw = comb[w][HD];
      const float sw = (mw == -INFINITY) ? 0.f : __expf(mw - M);
      o += sw * comb[w][tid];
      L += sw * comb[w][HD + 1];
    }
    if (nsplit == 1) {
      ((bf16_t*)p.out)[b * p.o_sb + h * p.o_sh + tid] = f2bf(o / L);    // skb >= 1: L > 0
    } else {                                                            // an empty range: o = 0, M = -inf, L = 0
      po[tid] = o;
      if (tid == 0) { po[HD] = M; po[HD + 1] = L; }
    }
  }
  if (nsplit == 1) return;
  decode_combine_tail<HD>(p.out, p.o_sb, p.o_sh, p.H, part, po, nsplit, counters, b, h, tid);
}

// one wave per (head, batch): attn_generic_kernel (a3v_attn.hip) at Sq = 1 over the row's own keys; any hd <= 256
template <typename T, bool SH>
__global__ __launch_bounds__(64) void attn_rows_generic_kernel(typename RowsArgsOf<SH>::type p, int hd) {
  __shared__ float pbuf[64];
  __shared__ float qs[256];
  const int lane = threadIdx.x;
  const int h = blockIdx.x, b = blockIdx.y;
  const int hk = h / (p.H / p.Hkv);
  const int sk0 = p.sk[b];
  const int kv_end = sk0 >= p.sk_max ? p.sk_max : min(sk0 + p.sk_add, p.sk_max);
  T* O = (T*)p.out + b * p.o_sb + h * p.o_sh;
  if (kv_end <= 0) {
    for (int d = lane; d < hd; d += 64) Cvt<T>::st(O + d, 0.f);
    return;
  }
  const T* Q = (const T*)p.q + b * p.q_sb + h * p.q_sh;
  int64_t row = b, dk = 0, dv = 0;
  int sh = 0;
  if constexpr (SH) {
    int src;
    sh = shared_len(p, b, kv_end, &src);
    row = p.row0 + b;
    dk = (src - row) * p.k_sb;
    dv = (src - row) * p.v_sb;
  }
  const T* K = (const T*)p.k + row * p.k_sb + hk * p.k_sh;
  const T* VT = (const T*)p.vt + row * p.v_sb + hk * p.v_sh;
  for (int d = lane; d < hd; d += 64) qs[d] = Cvt<T>::ld(Q + d);
  __syncthreads();
  float m = -INFINITY, l = 0.f;
  float o[4] = {0.f, 0.f, 0.f, 0.f};   // d = lane + 64*i
  for (int kv0 = 0; kv0 < kv_end; kv0 += 64) {
    const int kv = kv0 + lane;
    float s = -INFINITY;
    if (kv < kv_end) {
      const T* kr = K + (SH && kv0 < sh ? dk : 0) + (int64_t)kv * p.k_ss;
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
        const T* vr = VT + (SH && kv0 < sh ? dv : 0) + (int64_t)d * p.v_sd + kv0;
        float a = o[i] * alpha;
        for (int j = 0; j < cnt; ++j) a = fmaf(pbuf[j], Cvt<T>::ld(vr + j), a);
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

// One step of generate_many's token bookkeeping for one batch row per block: generate_step_kernel (a3v_rowops.hip) at
// cur_pos = cur[row], without teacher forcing, plus the row's own limit and the (next id, cache position) pair of the next step.
__global__ __launch_bounds__(1024) void generate_step_rows_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ sampled,
                                                                  int V, int64_t* __restrict__ tokens, int64_t ld_tok, int32_t* __restrict__ cur,
                                                                  const int32_t* __restrict__ limit, int pos_base,
                                                                  const int64_t* __restrict__ stop_seq, const int32_t* __restrict__ stop_off,
                                                                  int n_stop, uint8_t* __restrict__ stopped, int64_t* __restrict__ stop_pos,
                                                                  int32_t* __restrict__ live, int64_t* __restrict__ next_tok,
                                                                  int32_t* __restrict__ pos) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  const int row = blockIdx.x;
  if (stopped[row]) {                  // block-uniform: a stopped row is not touched
    if (threadIdx.x == 0) { next_tok[row] = 0; pos[row] = -1; }
    return;
  }
  float best = -INFINITY;
  int idx = 0x7fffffff;
  if (!sampled) {
    const float* r = logits + (int64_t)row * ld;
    auto take = [&](float v, int i) { if (v > best || (v == best && i < idx)) { best = v; idx = i; } };
    const bool vec = ((reinterpret_cast<uintptr_t>(r) & 15) == 0);
    const int V4 = vec ? V / 4 : 0;
    for (int i0 = threadIdx.x; i0 < V4; i0 += 4 * 1024) {
      f32x4 x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * 1024;
        x[q] = i < V4 ? reinterpret_cast<const f32x4*>(r)[i] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) take(x[q][e], (i0 + q * 1024) * 4 + e);
    }
    for (int i = V4 * 4 + threadIdx.x; i < V; i += 1024) take(r[i], i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  int c = cur[row];
  const int lim = limit[row];
  if (c < 0 || c >= lim || c >= ld_tok) {            // nothing writable: the row stops where it is
    stopped[row] = 1;
    if (live) atomicSub(live, 1);
    next_tok[row] = 0;
    pos[row] = -1;
    return;
  }
  int64_t next;
  if (sampled) {
    next = sampled[row];
  } else {
    for (int w = 1; w < 16; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    next = idx == 0x7fffffff ? 0 : idx;
  }
  int64_t* trow = tokens + (int64_t)row * ld_tok;
  trow[c] = next;
  bool st = false;
  int64_t sp = (int64_t)c + 1;
  for (int s = 0; s < n_stop; ++s) {
    const int o = stop_off[s], n = stop_off[s + 1] - o;
    if (c + 1 - n < 0 || st) continue;
    bool hit = true;
    for (int k = 0; k < n && hit; ++k) hit = trow[c + 1 - n + k] == stop_seq[o + k];
    if (hit) { sp = c + 1 - n; st = true; }
  }
  c += 1;
  cur[row] = c;
  if (c >= lim) st = true;                           // the last writable index is written: stop_pos stays c
  if (st && live) atomicSub(live, 1);
  stopped[row] = st ? 1 : 0;
  stop_pos[row] = sp;
  next_tok[row] = st ? 0 : next;
  pos[row] = st ? -1 : pos_base + c - 1;
}

// Positions [lo, hi) (0 < hi - lo < 64) of cache row src into the rows dst[0..n_dst): grid (n_dst, Hkv, layers).  K: one contiguous
// run of (hi - lo) * hd elements per (row, head), 16-byte vectors (hd is a multiple of 8).  V^T: hi - lo elements per d row, one
// thread per d row: elements up to the first 16-byte boundary, vectors, then the elements behind the last whole vector (source
// and destination sit at the same offset of 16-byte aligned rows, so they share the alignment).  Nothing outside the span is written.
template <typename T>
__global__ __launch_bounds__(256) void kv_copy_span_kernel(const void* const* __restrict__ k_ptrs, const void* const* __restrict__ vt_ptrs,
                                                           int src, const int32_t* __restrict__ dst, int B, int lo, int hi, int Hkv, int hd,
                                                           int Smax) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int r = dst[blockIdx.x];
  if (r < 0 || r >= B || r == src) return;             // block-uniform
  const int hk = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
  T* kb = (T*)k_ptrs[layer];
  T* vb = (T*)vt_ptrs[layer];
  const int64_t head = (int64_t)Smax * hd;
  const T* ks = kb + ((int64_t)src * Hkv + hk) * head + (int64_t)lo * hd;
  T* kd = kb + ((int64_t)r * Hkv + hk) * head + (int64_t)lo * hd;
  const int nvec = (hi - lo) * hd / VEC;
  for (int i = tid; i < nvec; i += 256) reinterpret_cast<f32x4*>(kd)[i] = reinterpret_cast<const f32x4*>(ks)[i];
  const int a0 = min(hi, (lo + VEC - 1) / VEC * VEC), a1 = a0 + (hi - a0) / VEC * VEC;
  for (int d = tid; d < hd; d += 256) {
    const T* vs = vb + (((int64_t)src * Hkv + hk) * hd + d) * Smax;
    T* vd = vb + (((int64_t)r * Hkv + hk) * hd + d) * Smax;
    for (int e = lo; e < a0; ++e) vd[e] = vs[e];
    for (int e = a0; e < a1; e += VEC) *reinterpret_cast<f32x4*>(vd + e) = *reinterpret_cast<const f32x4*>(vs + e);
    for (int e = a1; e < hi; ++e) vd[e] = vs[e];
  }
}

// src_row == NULL: the plain kernels on k / vt = the caches of the B rows of the call.  Otherwise the shared-prefix forms: k / vt
// are the caches of all Btot rows and row b of the call is cache row row0 + b.
int attention_rows_impl(const void* q, const void* k, const void* vt, void* out, const int32_t* sk, int sk_add, int sk_max, int B, int H,
                        int Hkv, int hd, const int64_t* strides, float* scratch, int* counters, int dtype, void* stream,
                        const int32_t* src_row = nullptr, const int32_t* shared = nullptr, int row0 = 0, int Btot = 0) {
  if (!q || !k || !vt || !out || !sk || !strides || B <= 0 || H <= 0 || Hkv <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  if (src_row && (!shared || row0 < 0 || Btot < row0 + B)) return A3V_ERR_ARG;
  if (H % Hkv || hd <= 0 || hd > 256) return A3V_ERR_SHAPE;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  // the caches are [B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] in whatever strides: a V^T row (strides[8]) and a K head (strides[4]) bound sk_max
  if (sk_max > strides[8] || (int64_t)sk_max * strides[5] > strides[4]) return A3V_ERR_SHAPE;
  RowsSharedArgs p;
  p.src_row = src_row; p.shared = shared; p.row0 = row0; p.Btot = Btot;
  p.q = q; p.k = k; p.vt = vt; p.out = out; p.sk = sk;
  p.q_sb = strides[0]; p.q_sh = strides[2];
  p.k_sb = strides[3]; p.k_sh = strides[4]; p.k_ss = strides[5];
  p.v_sb = strides[6]; p.v_sh = strides[7]; p.v_sd = strides[8];
  p.o_sb = strides[9]; p.o_sh = strides[11];
  p.sk_add = sk_add; p.sk_max = sk_max; p.H = H; p.Hkv = Hkv;
  p.scale = 1.0f / sqrtf((float)hd);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_F32 || (hd != 64 && hd != 128)) {
    const RowsAttnArgs& pp = p;
    if (src_row) {
      if (dtype == A3V_F32) hipLaunchKernelGGL((attn_rows_generic_kernel<float, true>), dim3(H, B), dim3(64), 0, st, p, hd);
      else hipLaunchKernelGGL((attn_rows_generic_kernel<bf16_t, true>), dim3(H, B), dim3(64), 0, st, p, hd);
    } else if (dtype == A3V_F32) hipLaunchKernelGGL((attn_rows_generic_kernel<float, false>), dim3(H, B), dim3(64), 0, st, pp, hd);
    else hipLaunchKernelGGL((attn_rows_generic_kernel<bf16_t, false>), dim3(H, B), dim3(64), 0, st, pp, hd);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  if (!scratch || !counters) return A3V_ERR_ARG;
  for (int i = 0; i < 12; ++i)
    if (i != 1 && i != 10 && (strides[i] % 8)) return A3V_ERR_SHAPE;      // 16-B vector access (the Sq strides are not used)
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt)) & 15) return A3V_ERR_SHAPE;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  const dim3 grid(ns, H, B);
  const RowsAttnArgs& pp = p;
  if (src_row) {
    if (hd == 128) hipLaunchKernelGGL((attn_decode_rows_kernel<128, true>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
    else hipLaunchKernelGGL((attn_decode_rows_kernel<64, true>), grid, dim3(512), 0, st, p, scratch, ns, ch, counters);
  } else if (hd == 128) hipLaunchKernelGGL((attn_decode_rows_kernel<128, false>), grid, dim3(512), 0, st, pp, scratch, ns, ch, counters);
  else hipLaunchKernelGGL((attn_decode_rows_kernel<64, false>), grid, dim3(512), 0, st, pp, scratch, ns, ch, counters);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

}  // namespace

extern "C" int a3v_rope_kvcache_rows(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                                     const float* cos_sin, const int32_t* pos, int B, int H, int Hkv, int hd, int Smax, int dtype,
                                     void* stream) {
  if (!qkv || !q_out || !k_cache || !vt_cache || !cos_sin || !pos || B <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (hd <= 0 || hd % 8 || hd > 128 || ldqkv % 8 || ldq % 8 || Smax <= 0) return A3V_ERR_SHAPE;
  if (ldqkv < (int64_t)(H + 2 * Hkv) * hd || ldq < (int64_t)H * hd) return A3V_ERR_SHAPE;
  const dim3 g(H + 2 * Hkv, B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_BF16)
    hipLaunchKernelGGL(rope_kv_rows_kernel<bf16_t>, g, dim3(64), 0, st, (const bf16_t*)qkv, ldqkv, (bf16_t*)q_out, ldq, (bf16_t*)k_cache,
                       (bf16_t*)vt_cache, cos_sin, pos, H, Hkv, hd, Smax);
  else if (dtype == A3V_F32)
    hipLaunchKernelGGL(rope_kv_rows_kernel<float>, g, dim3(64), 0, st, (const float*)qkv, ldqkv, (float*)q_out, ldq, (float*)k_cache,
                       (float*)vt_cache, cos_sin, pos, H, Hkv, hd, Smax);
  else return A3V_ERR_DTYPE;
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_attention_decode_rows_splits(int B, int H, int sk_max) {
  if (B <= 0 || H <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  int ns, ch;
  a3v_decode_wave_plan(B, H, sk_max, &ns, &ch);
  return ns;
}

extern "C" int a3v_attention_decode_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* sk, int sk_max, int B,
                                         int H, int Hkv, int hd, const int64_t* strides, float* scratch, int* counters, int dtype,
                                         void* stream) {
  return attention_rows_impl(q, k, vt, out, sk, 0, sk_max, B, H, Hkv, hd, strides, scratch, counters, dtype, stream);
}

extern "C" int a3v_attention_decode_rows_shared(const void* q, const void* k, const void* vt, void* out, const int32_t* sk,
                                                const int32_t* src_row, const int32_t* shared, int sk_max, int B, int H, int Hkv, int hd,
                                                const int64_t* strides, float* scratch, int* counters, int dtype, void* stream) {
  if (!src_row) return attention_rows_impl(q, k, vt, out, sk, 0, sk_max, B, H, Hkv, hd, strides, scratch, counters, dtype, stream);
  return attention_rows_impl(q, k, vt, out, sk, 0, sk_max, B, H, Hkv, hd, strides, scratch, counters, dtype, stream, src_row, shared, 0, B);
}

extern "C" int a3v_kv_copy_span(const void* const* k_ptrs, const void* const* vt_ptrs, int n_layers, int src_row, const int32_t* dst_rows,
                                int n_dst, int B, int lo, int hi, int Hkv, int hd, int Smax, int dtype, void* stream) {
  if (!k_ptrs || !vt_ptrs || n_layers <= 0 || n_dst < 0 || (n_dst > 0 && !dst_rows) || B <= 0 || src_row < 0 || src_row >= B) return A3V_ERR_ARG;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  if (Hkv <= 0 || hd <= 0 || hd % 8 || Smax <= 0 || Smax % 8 || lo < 0 || hi < lo || hi - lo >= 64 || hi > Smax) return A3V_ERR_SHAPE;
  if (n_layers > 65535 || Hkv > 65535) return A3V_ERR_SHAPE;
  if (hi == lo || n_dst == 0) return A3V_OK;             // nothing to copy: nothing launched
  const dim3 g(n_dst, Hkv, n_layers);
  if (dtype == A3V_BF16)
    hipLaunchKernelGGL(kv_copy_span_kernel<bf16_t>, g, dim3(256), 0, (hipStream_t)stream, k_ptrs, vt_ptrs, src_row, dst_rows, B, lo, hi, Hkv, hd, Smax);
  else
    hipLaunchKernelGGL(kv_copy_span_kernel<float>, g, dim3(256), 0, (hipStream_t)stream, k_ptrs, vt_ptrs, src_row, dst_rows, B, lo, hi, Hkv, hd, Smax);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_generate_step_rows(const float* logits, int64_t ld, const int64_t* sampled, int B, int V, int64_t* tokens,
                                      int64_t ld_tok, int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq,
                                      const int32_t* stop_off, int n_stop, uint8_t* stopped, int64_t* stop_pos, int32_t* live,
                                      int64_t* next_tok, int32_t* pos, void* stream) {
  if ((!logits && !sampled) || !tokens || !cur || !limit || !stopped || !stop_pos || !next_tok || !pos) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || ld_tok <= 0 || pos_base < 0 || n_stop < 0 || (n_stop > 0 && (!stop_seq || !stop_off))) return A3V_ERR_ARG;
  hipLaunchKernelGGL(generate_step_rows_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, ld, sampled, V, tokens, ld_tok, cur, limit,
                     pos_base, stop_seq, stop_off, n_stop, stopped, stop_pos, live, next_tok, pos);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_llama_decode_step_rows_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8) {
  return a3v_llama_decode_step_form(B, dim, H, Hkv, hd, ffn, w8) == 2 ? 2 : 0;
}

namespace {
// what a3v_decode_fused_layers (a3v_decode.hip) runs between the plain-store qkv GEMV and the wo GEMV: RoPE + cache write at the
// rows' own positions, then the per-row attention -- six launches per layer
struct RowsStage { const float* cos_sin; const int32_t* pos; const int32_t* src_row; const int32_t* shared; int pos_max, B; };
int attend_rows(const void* ctx, const a3v_decode_chunk& c) {
  const RowsStage& s = *(const RowsStage*)ctx;
  const int64_t ldq = c.strides[0];
  const int32_t* pc = s.pos + c.b0;
  bf16_t* kc = (bf16_t*)c.L->k_cache + c.b0 * c.kv_row;
  bf16_t* vc = (bf16_t*)c.L->vt_cache + c.b0 * c.kv_row;
  int rc;
  if ((rc = a3v_rope_kvcache_rows(c.q, ldq, c.q, ldq, kc, vc, s.cos_sin, pc, c.nbr, c.H, c.Hkv, c.hd, c.Smax, A3V_BF16, c.stream))) return rc;
  if (!s.src_row)
    return attention_rows_impl(c.q, kc, vc, c.att, pc, 1, s.pos_max + 1, c.nbr, c.H, c.Hkv, c.hd, c.strides, c.scratch, c.counters, A3V_BF16,
                               c.stream);
  // src_row[] names rows of the whole cache: its base, and the chunk's first row
  return attention_rows_impl(c.q, c.L->k_cache, c.L->vt_cache, c.att, pc, 1, s.pos_max + 1, c.nbr, c.H, c.Hkv, c.hd, c.strides, c.scratch,
                             c.counters, A3V_BF16, c.stream, s.src_row + c.b0, s.shared + c.b0, c.b0, s.B);
}

int decode_step_rows_impl(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                          float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos, const int32_t* src_row,
                          const int32_t* shared, int pos_max, int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps,
                          void* stream) {
  if (!layers || n_layers <= 0 || !h || !xn || !qkv || !att || !act || !attn_scratch || !skinny_ws || !cos_sin || !pos) return A3V_ERR_ARG;
  if (B <= 0 || B > 32 || pos_max < 0 || pos_max >= Smax || Smax % 8) return A3V_ERR_SHAPE;
  int rc, w8;
  if ((rc = a3v_decode_layer_table(layers, n_layers, true, &w8))) return rc;
  if (a3v_llama_decode_step_rows_form(B, dim, H, Hkv, hd, ffn, w8) != 2) return A3V_ERR_SHAPE;    // nothing launched
  const RowsStage ctx{cos_sin, pos, src_row, shared, pos_max, B};
  const a3v_decode_stage stage{B > 16 ? (B + 1) / 2 : B, 1, nullptr, nullptr, nullptr, 0, 0, attend_rows, &ctx};   // 17..32 rows: two row chunks
  return a3v_decode_fused_layers(layers, n_layers, w8, h, qkv, att, act, attn_scratch, skinny_ws, B, dim, H, Hkv, hd, ffn, Smax, eps, stage, stream);
}
}  // namespace

extern "C" int a3v_llama_decode_step_rows(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                                          float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos, int pos_max,
                                          int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps, void* stream) {
  return decode_step_rows_impl(layers, n_layers, h, xn, qkv, att, act, attn_scratch, skinny_ws, cos_sin, pos, nullptr, nullptr, pos_max, B,
                               dim, H, Hkv, hd, ffn, Smax, eps, stream);
}

extern "C" int a3v_llama_decode_step_rows_shared(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att,
                                                 void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos,
                                                 const int32_t* src_row, const int32_t* shared, int pos_max, int B, int dim, int H, int Hkv,
                                                 int hd, int ffn, int Smax, float eps, void* stream) {
  if (!src_row != !shared) return A3V_ERR_ARG;
  return decode_step_rows_impl(layers, n_layers, h, xn, qkv, att, act, attn_scratch, skinny_ws, cos_sin, pos, src_row, shared, pos_max, B,
                               dim, H, Hkv, hd, ffn, Smax, eps, stream);
}
