// Ragged "extend" prefill for gfx950: causal attention of PACKED query spans over per-row caches, with an optional shared prefix
// that another cache row holds (include/a3vlm_hip.h, "Extend prefill").  Row b brings nq[b] = q_off[b+1] - q_off[b] queries (rows
// q_off[b].. of the packed q / out), its cache holds sk[b] keys after the extend, query j sits at position sk[b] - nq[b] + j.
//
//  * attn_extend_bf16_kernel<HD, SH> : the walk of attn_prefill_bf16_kernel<HD, true> (a3v_attn.hip) restated per row: 128-query
//    tiles counted from the row's first query, 64-key tiles from position 0, the LDS-DMA double buffer, the MFMA order, the lazy
//    rescale and the staged O of that kernel, expression for expression.  Only a tile's base and its bounds differ: Sq / Sk are the
//    row's (device values), and with SH a tile below the row's shared length S_b comes from cache row src_row[b] -- a second buffer
//    descriptor chosen per tile by a wave-uniform select (SGPRs).  A KV tile is 64 keys and starts at a multiple of 64, S_b is a
//    multiple of 64: a tile, its clamped re-reads and its 16-byte vectors lie wholly in one row.  Blocks of query tiles past the
//    row's nq leave at once.
//  * attn_extend_one_kernel<HD, SH> + attn_extend_one_combine_kernel<HD> : rows with ONE query.  a3v_attention sends Sq == 1 to its
//    two-phase decode kernel (attn_decode_bf16_kernel + attn_decode_combine_kernel) under decode_plan(1, H, Sk); these two restate
//    that pair with the plan computed on the device from the row's own key count, so such a row keeps the bits of that entry.
//  * attn_extend_generic_kernel<T, SH> : attn_generic_kernel, one wave per (query, head, row): fp32, and bf16 at other head dims.
//  * rope_kv_extend_kernel<T>        : rope_kv_kernel (a3v_rowops.hip) per row: S = nq[b], start_pos = rope_pos0 = sk[b] - nq[b].
#include "a3v_common.h"
#include <type_traits>

namespace {

struct ExtArgs {
  const void* q; const void* k; const void* vt; void* out;
  const int32_t* q_off; const int32_t* sk; const int32_t* src_row; const int32_t* shared;
  int64_t q_ss, q_sh;           // packed q: row, head
  int64_t k_sb, k_sh, k_ss;     // k strides: cache row, kv-head, seq   (hd contiguous)
  int64_t v_sb, v_sh, v_sd;     // vt strides: cache row, kv-head, d    (seq contiguous)
  int64_t o_ss, o_sh;
  int B, H, Hkv, nq_max, sk_max;
  float scale_log2, scale;
  int lazy_rescale;
};

// The row's query and key counts as every kernel of this file reads them: nq clamped to nq_max, sk to sk_max, and nq to sk (a
// causal span cannot be longer than the keys it ends on).  Idle (nq <= 0 or sk <= 0): both 0.
__device__ __forceinline__ void ext_row(const ExtArgs& p, int b, int* q0, int* nq, int* sk) {
  const int o0 = p.q_off[b], o1 = p.q_off[b + 1];
  int n = min(o1 - o0, p.nq_max), s = min(p.sk[b], p.sk_max);
  n = min(n, s);
  if (n <= 0 || s <= 0 || o0 < 0) { n = 0; s = 0; }
  *q0 = o0; *nq = n; *sk = s;
}
// a3v_attention_decode_rows_shared's rule: S_b = min(shared, sk) rounded down to 64; a src_row outside [0, B) or the own row: 0
__device__ __forceinline__ int ext_shared(const ExtArgs& p, int b, int skb, int* src) {
  int s = p.src_row[b];
  if (s < 0 || s >= p.B) s = b;
  *src = s;
  return s == b ? 0 : max(min(p.shared[b], skb), 0) & ~63;
}

__device__ __forceinline__ void buf_dma16(__amdgpu_buffer_rsrc_t rs, char* lds_dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void xchg32(float x, float& a, float& b) {
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

template <int HD, bool SH>
__global__ __launch_bounds__(256, 2) void attn_extend_bf16_kernel(ExtArgs p) {
  constexpr int KVB = 64;
  constexpr int KROW = HD * 2;
  constexpr int KCH = HD / 8;
  constexpr int K_LOADS = KVB * KCH / 256;
  constexpr int V_LOADS = HD * 8 / 256;
  constexpr int TILEB = KVB * KROW + HD * 128;
  __shared__ __attribute__((aligned(1024))) char lds[2 * TILEB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // block order of the prefill kernel: XCD x takes a contiguous range of (row, head, query tile) triples, heavy tiles first
  const int nqt = (p.nq_max + 127) / 128;
  int vb;
  {
    const int total = gridDim.x, id = blockIdx.x;
    const int xcd = id & 7, q = total >> 3, r = total & 7;
    vb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int head_slot = vb / nqt;
  const int qt = nqt - 1 - (vb - head_slot * nqt);
  const int b = head_slot / p.H, h = head_slot - b * p.H;
  int qbase, Sq, Sk;
  ext_row(p, b, &qbase, &Sq, &Sk);
  // idle rows, tiles past the row's queries, and one-query rows (attn_extend_one_kernel's): block-uniform, before any barrier
  if (Sq <= 1 || qt * 128 >= Sq) return;
  const int hk = h / (p.H / p.Hkv);
  const int q0 = qt * 128 + wave * 32;
  const int off = Sk - Sq;

  const bf16_t* Q = (const bf16_t*)p.q + (int64_t)qbase * p.q_ss + h * p.q_sh;
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh;
  const bf16_t* Ks_ = K;
  const bf16_t* VTs_ = VT;
  int S_b = 0;                                  // keys below it come from the source row (a multiple of 64, <= Sk)
  if constexpr (SH) {
    int src;
    S_b = __builtin_amdgcn_readfirstlane(ext_shared(p, b, Sk, &src));
    src = __builtin_amdgcn_readfirstlane(src);
    Ks_ = (const bf16_t*)p.k + src * p.k_sb + hk * p.k_sh;
    VTs_ = (const bf16_t*)p.vt + src * p.v_sb + hk * p.v_sh;
  }

  const int ql = lane & 31, hh = lane >> 5;
  int qrow = q0 + ql;
  const int qrow_c = qrow < Sq ? qrow : Sq - 1;
  bf16x8 qf[HD / 16];
#pragma unroll
  for (int ks = 0; ks < HD / 16; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8*>(Q + (int64_t)qrow_c * p.q_ss + ks * 16 + hh * 8);

  f32x16 o[HD / 32];
#pragma unroll
  for (int d = 0; d < HD / 32; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int last_q = min(qt * 128 + 127, Sq - 1);
  const int kv_end = min(Sk, last_q + off + 1);
  const int n_tiles = (kv_end + KVB - 1) / KVB;

  u32x4 kreg[K_LOADS], vreg[V_LOADS];
  auto load_tile = [&](int kv0) {               // the ragged last tile (keys past Sk inside it): never a shared one (S_b <= Sk & ~63)
    const bf16_t* Kt = (SH && kv0 < S_b) ? Ks_ : K;
    const bf16_t* Vt = (SH && kv0 < S_b) ? VTs_ : VT;
#pragma unroll
    for (int i = 0; i < K_LOADS; ++i) {
      const int id = tid + i * 256;
      const int row = id / KCH, ch = id % KCH;
      int kr = kv0 + row;
      kr = kr < Sk ? kr : Sk - 1;
      kreg[i] = *reinterpret_cast<const u32x4*>(Kt + (int64_t)kr * p.k_ss + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < V_LOADS; ++i) {
      const int id = tid + i * 256;
      const int d = id >> 3, ch = id & 7;
      const int kv = kv0 + ch * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kv + 8 <= Sk) {
        v = *reinterpret_cast<const u32x4*>(Vt + (int64_t)d * p.v_sd + kv);
      } else if (kv < Sk) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(Vt + (int64_t)d * p.v_sd + kv);
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (kv + j < Sk) ? src[j] : (unsigned short)0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
      }
      vreg[i] = v;
    }
  };
  auto write_tile = [&](char* Ks, char* Vs) {
#pragma unroll
    for (int i = 0; i < K_LOADS; ++i) {
      const int id = tid + i * 256;
      const int row = id / KCH, ch = id % KCH;
      const int sw = (HD == 128) ? (row & 15) : ((row >> 1) & 7);
      *reinterpret_cast<u32x4*>(Ks + row * KROW + ((ch ^ sw) << 4)) = kreg[i];
    }
#pragma unroll
    for (int i = 0; i < V_LOADS; ++i) {
      const int id = tid + i * 256;
      const int d = id >> 3, ch = id & 7;
      *reinterpret_cast<u32x4*>(Vs + d * 128 + ((ch ^ ((d >> 1) & 7)) << 4)) = vreg[i];
    }
  };
  // one descriptor per (row, matrix); a full tile reads [kv0, kv0 + 64) of ONE row, so the source row is a select between two
  // descriptors that lives in SGPRs.  num_records stays the prefill kernel's: the offsets are bounded by kv0 + 64 <= Sk <= Smax.
  const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)K, 0, 0x7fffffff, 0x00020000);
  const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)VT, 0, 0x7fffffff, 0x00020000);
  const auto rsKs = __builtin_amdgcn_make_buffer_rsrc((void*)Ks_, 0, 0x7fffffff, 0x00020000);
  const auto rsVs = __builtin_amdgcn_make_buffer_rsrc((void*)VTs_, 0, 0x7fffffff, 0x00020000);
  unsigned koff[K_LOADS], voff[V_LOADS];
#pragma unroll
  for (int i = 0; i < K_LOADS; ++i) {
    const int id = tid + i * 256;
    const int row = id / KCH, slot = id % KCH;
    const int sw = (HD == 128) ? (row & 15) : ((row >> 1) & 7);
    koff[i] = (unsigned)((row * p.k_ss + (slot ^ sw) * 8) * 2);
  }
#pragma unroll
  for (int i = 0; i < V_LOADS; ++i) {
    const int id = tid + i * 256;
    const int d = id >> 3, slot = id & 7;
    voff[i] = (unsigned)((d * p.v_sd + (slot ^ ((d >> 1) & 7)) * 8) * 2);
  }
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  auto dma_tile = [&](int kv0, char* Ks, char* Vs) {
    const unsigned ks_off = (unsigned)(kv0 * p.k_ss * 2), vs_off = (unsigned)(kv0 * 2);
    if (SH && kv0 < S_b) {                      // wave-uniform (s_cbranch): kv0 and S_b are SGPR values
#pragma unroll
      for (int i = 0; i < K_LOADS; ++i) buf_dma16(rsKs, Ks + (wave_u * 64 + i * 256) * 16, koff[i], ks_off);
#pragma unroll
      for (int i = 0; i < V_LOADS; ++i) buf_dma16(rsVs, Vs + (wave_u * 64 + i * 256) * 16, voff[i], vs_off);
    } else {
#pragma unroll
      for (int i = 0; i < K_LOADS; ++i) buf_dma16(rsK, Ks + (wave_u * 64 + i * 256) * 16, koff[i], ks_off);
#pragma unroll
      for (int i = 0; i < V_LOADS; ++i) buf_dma16(rsV, Vs + (wave_u * 64 + i * 256) * 16, voff[i], vs_off);
    }
  };
  auto full_tile = [&](int t) { return t * KVB + KVB <= Sk; };

  if (n_tiles > 0 && full_tile(0)) dma_tile(0, lds, lds + KVB * KROW);
  const int kfb = ql * KROW + ((hh ^ ((HD == 128) ? (ql & 15) : ((ql >> 1) & 7))) << 4);
  const int vfb = ql * 128 + ((hh ^ ((ql >> 1) & 7)) << 4);
  auto body = [&](int t, auto bufc) {
    constexpr int BUF = decltype(bufc)::value;
    const int kv0 = t * KVB;
    char* Ks = lds + BUF * TILEB;
    char* Vs = Ks + KVB * KROW;
    if (full_tile(t)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    } else {
      load_tile(kv0);
      write_tile(Ks, Vs);
      __syncthreads();
    }
    if (t + 1 < n_tiles && full_tile(t + 1)) dma_tile(kv0 + KVB, lds + (1 - BUF) * TILEB, lds + (1 - BUF) * TILEB + KVB * KROW);
    if (kv0 > q0 + 31 + off) return;
    f32x16 s[2];
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[tb][r] = 0.f;
    constexpr bool FRAG_AHEAD = HD == 128;
    if constexpr (!FRAG_AHEAD) {
#pragma unroll
      for (int ks = 0; ks < HD / 16; ++ks)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + tb * 32 * KROW + (kfb ^ (ks << 5)));
          s[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[tb], 0, 0, 0);
        }
    } else {
      bf16x8 kr[3][2];
#pragma unroll
      for (int pre = 0; pre < 2; ++pre)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) kr[pre][tb] = *reinterpret_cast<const bf16x8*>(Ks + tb * 32 * KROW + (kfb ^ (pre << 5)));
      asm volatile("" ::: "memory");
#pragma unroll
      for (int ks = 0; ks < HD / 16; ++ks) {
        if (ks + 2 < HD / 16) {
#pragma unroll
          for (int tb = 0; tb < 2; ++tb) kr[(ks + 2) % 3][tb] = *reinterpret_cast<const bf16x8*>(Ks + tb * 32 * KROW + (kfb ^ ((ks + 2) << 5)));
          asm volatile("" : "+v"(qf[ks]) :: "memory");
        }
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) s[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr[ks % 3][tb], qf[ks], s[tb], 0, 0, 0);
      }
    }
    const int qlim = qrow + off;
    const bool need_mask = (kv0 + KVB > Sk) || (kv0 + KVB - 1 > q0 + off);
    float mx = -INFINITY;
    if (need_mask) {
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + tb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const bool ok = (kv < Sk) && (kv <= qlim);
          s[tb][r] = ok ? s[tb][r] : -INFINITY;
        }
    }
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[tb][r]);
    { float x0, x1; xchg32(mx, x0, x1); mx = fmaxf(x0, x1); }
    const float m_new = fmaxf(m_run, mx);
    const bool grow = (p.lazy_rescale & 1) ? ((m_new - m_run) * p.scale_log2 > 8.f || m_run == -INFINITY) : true;
    const bool resc = __builtin_amdgcn_ballot_w64(grow && m_new != m_run) != 0;
    const float m_tgt = resc ? m_new : m_run;
    const float m_use = (m_tgt == -INFINITY) ? 0.f : m_tgt;
    float alpha = 1.f;
    if (resc) alpha = __builtin_amdgcn_exp2f((m_run - m_use) * p.scale_log2);
    m_run = m_tgt;
    float lsum = 0.f;
    const float mb = m_use * p.scale_log2;
    bf16x8 pf[2][2];
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[tb][r], p.scale_log2, -mb));
        lsum += pv;
        pf[tb][r >> 3][r & 7] = f2bf(pv);
      }
    l_run = resc ? l_run * alpha + lsum : l_run + lsum;
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 w;
        __builtin_memcpy(&w, &pf[tb][c], 16);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(w[e], w[2 + e], false, false);
          w[e] = sw[0];
          w[2 + e] = sw[1];
        }
        __builtin_memcpy(&pf[tb][c], &w, 16);
      }
    if (resc) {
#pragma unroll
      for (int d = 0; d < HD / 32; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    }
    if constexpr (FRAG_AHEAD) {
      constexpr int ND = HD / 32;
      bf16x8 vr[2][ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) vr[0][d] = *reinterpret_cast<const bf16x8*>(Vs + d * 32 * 128 + (vfb ^ (0 << 4)));
      asm volatile("" ::: "memory");
#pragma unroll
      for (int gI = 0; gI < 4; ++gI) {
        const int tb = gI >> 1, c = gI & 1;
        if (gI + 1 < 4) {
          const int c16n = 4 * ((gI + 1) >> 1) + 2 * ((gI + 1) & 1);
#pragma unroll
          for (int d = 0; d < ND; ++d) vr[(gI + 1) & 1][d] = *reinterpret_cast<const bf16x8*>(Vs + d * 32 * 128 + (vfb ^ (c16n << 4)));
          asm volatile("" : "+v"(pf[tb][c]) :: "memory");
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vr[gI & 1][d], pf[tb][c], o[d], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int d = 0; d < HD / 32; ++d) {
            const int c16 = 4 * tb + 2 * c;
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vs + d * 32 * 128 + (vfb ^ (c16 << 4)));
            o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[tb][c], o[d], 0, 0, 0);
          }
    }
  };
  {
    int t = 0;
    for (; t + 1 < n_tiles; t += 2) {
      body(t, std::integral_constant<int, 0>{});
      body(t + 1, std::integral_constant<int, 1>{});
    }
    if (t < n_tiles) body(t, std::integral_constant<int, 0>{});
  }

  float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  // staged O (the host checked the 16-byte conditions): the wave's 32 x HD tile leaves through an LDS patch as whole rows
  constexpr int ROWB = HD * 2, NPAIR = HD / 8, RPI = 64 / NPAIR;
  __syncthreads();
  char* patch = lds + wave * (32 * ROWB);
  char* wrow = patch + ql * ROWB;
  const int wx = (ql & (NPAIR - 1)) << 1;
#pragma unroll
  for (int d = 0; d < HD / 32; ++d)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = f2bf(o[d][g4 * 4 + e] * inv);
      *reinterpret_cast<bf16x4*>(wrow + (((d * 8 + g4 * 2 + hh) ^ wx) << 3)) = ov;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int pr = lane % NPAIR, rr = lane / NPAIR;
  bf16_t* Ob = (bf16_t*)p.out + (int64_t)qbase * p.o_ss + h * p.o_sh + pr * 8;
  const int qw = qt * 128 + wave * 32;
#pragma unroll
  for (int it = 0; it < 32 / RPI; ++it) {
    const int r = it * RPI + rr;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(patch + r * ROWB + ((pr ^ (r & (NPAIR - 1))) << 4));
    if (qw + r < Sq) *reinterpret_cast<bf16x8*>(Ob + (int64_t)(qw + r) * p.o_ss) = v;
  }
}

// decode_plan (a3v_attn.hip) at B = 1, on the device
__host__ __device__ inline void one_plan(int H, int Sk, int* nsplit, int* chunk) {
  const int want = (768 + H - 1) / H;
  const int maxs = (Sk + 127) / 128;
  int ns = want < maxs ? want : maxs;
  if (ns < 1) ns = 1;
  int ch = (Sk + ns - 1) / ns;
  ch = (ch + 63) & ~63;
  *nsplit = (Sk + ch - 1) / ch;
  *chunk = ch;
}

// One-query rows: attn_decode_bf16_kernel (a3v_attn.hip) for row b at B = 1.  grid (ns_bound, H, B), block 256, dynamic LDS for the
// largest chunk; part[b][h][split] = {o[HD], m, l} with ns_bound slots per (b, h).
template <int HD, bool SH>
__global__ __launch_bounds__(256) void attn_extend_one_kernel(ExtArgs p, float* part, int ns_bound) {
  constexpr int LPR = HD / 8;
  constexpr int RPW = 64 / LPR;
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* sc = reinterpret_cast<float*>(dsm);
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int qbase, Sq, Sk;
  ext_row(p, b, &qbase, &Sq, &Sk);
  if (Sq != 1) return;
  int nsplit, chunk;
  one_plan(p.H, Sk, &nsplit, &chunk);
  if (sp >= nsplit) return;
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int kv_hi = min(Sk, kv_lo + chunk);
  const int n = kv_hi - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * ns_bound + sp) * (HD + 2);
  if (n <= 0) {
    if (tid < HD) po[tid] = 0.f;
    if (tid == 0) { po[HD] = -INFINITY; po[HD + 1] = 0.f; }
    return;
  }
  const bf16_t* Q = (const bf16_t*)p.q + (int64_t)qbase * p.q_ss + h * p.q_sh;
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh;
  int64_t dk = 0, dv = 0;
  int S_b = 0;
  if constexpr (SH) {
    int src;
    S_b = ext_shared(p, b, Sk, &src);
    dk = (src - b) * p.k_sb;
    dv = (src - b) * p.v_sb;
  }
  float qv[8];
  load8(Q + (lane % LPR) * 8, qv);
  constexpr int U = 8;
  const int lr = lane / LPR, lc = (lane % LPR) * 8;
  for (int r0 = wave * RPW * U; r0 < n; r0 += 4 * RPW * U) {
    bf16x8 kk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int r = r0 + u * RPW + lr;
      r = r < n ? r : n - 1;
      const int kv = kv_lo + r;
      const bf16x8* kp = reinterpret_cast<const bf16x8*>(K + (SH && kv < S_b ? dk : 0) + (int64_t)kv * p.k_ss + lc);
      kk[u] = *kp;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = fmaf(qv[e], (float)kk[u][e], acc);
#pragma unroll
      for (int o2 = LPR / 2; o2 > 0; o2 >>= 1) acc += __shfl_xor(acc, o2, 64);
      const int r = r0 + u * RPW + lr;
      if (r < n && (lane % LPR) == 0) sc[r] = acc * p.scale;
    }
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int i = tid; i < n; i += 256) mx = fmaxf(mx, sc[i]);
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float ls = 0.f;
  for (int i = tid; i < n; i += 256) {
    const float e = __expf(sc[i] - mx);
    sc[i] = e;
    ls += e;
  }
  ls = wave_sum(ls);
  __syncthreads();
  if (lane == 0) red[4 + wave] = ls;
  __syncthreads();
  ls = red[4] + red[5] + red[6] + red[7];
  const int n8 = (n + 7) & ~7;
  for (int i = n + tid; i < n8; i += 256) sc[i] = 0.f;
  __syncthreads();
  // 16-byte V^T vectors start at multiples of 8 keys (chunk is a multiple of 64): a vector lies on one side of S_b, and
  // kv_lo + n8 <= Smax because Smax is a multiple of 8 (host check)
  constexpr int DB = 8;
  for (int d0 = wave * (HD / 4); d0 < (wave + 1) * (HD / 4); d0 += DB) {
    float acc[DB];
#pragma unroll
    for (int j = 0; j < DB; ++j) acc[j] = 0.f;
    for (int c = lane * 8; c < n8; c += 64 * 8) {
      bf16x8 vv[DB];
      const int64_t so = (SH && kv_lo + c < S_b) ? dv : 0;
#pragma unroll
      for (int j = 0; j < DB; ++j) {
        const bf16x8* vp = reinterpret_cast<const bf16x8*>(VT + so + (int64_t)(d0 + j) * p.v_sd + kv_lo + c);
        vv[j] = *vp;
      }
      float pv[8];
      const int nvalid = Sk - (kv_lo + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = e < nvalid ? sc[c + e] : 0.f;
#pragma unroll
      for (int j = 0; j < DB; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j] = fmaf(pv[e], e < nvalid ? (float)vv[j][e] : 0.f, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < DB; ++j) {
      const float t = wave_sum(acc[j]);
      if (lane == 0) po[d0 + j] = t;
    }
  }
  if (tid == 0) { po[HD] = mx; po[HD + 1] = ls; }
}

// attn_decode_combine_kernel for the one-query rows: grid (H, B), block HD
template <int HD>
__global__ void attn_extend_one_combine_kernel(ExtArgs p, const float* part, int ns_bound) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int qbase, Sq, Sk;
  ext_row(p, b, &qbase, &Sq, &Sk);
  if (Sq != 1) return;
  int nsplit, chunk;
  one_plan(p.H, Sk, &nsplit, &chunk);
  const float* pp = part + (int64_t)(b * p.H + h) * ns_bound * (HD + 2);
  float m = -INFINITY;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, pp[s * (HD + 2) + HD]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = pp[s * (HD + 2) + HD];
    const float w = (ms == -INFINITY) ? 0.f : __expf(ms - m);
    acc += w * pp[s * (HD + 2) + d];
    l += w * pp[s * (HD + 2) + HD + 1];
  }
  const float v = acc / l;
  ((bf16_t*)p.out)[(int64_t)qbase * p.o_ss + h * p.o_sh + d] = f2bf(v);
}

// attn_generic_kernel (a3v_attn.hip) per row: grid (nq_max, H, B), one wave per (query, head, row); any hd <= 256
template <typename T, bool SH>
__global__ __launch_bounds__(64) void attn_extend_generic_kernel(ExtArgs p, int hd) {
  __shared__ float pbuf[64];
  __shared__ float qs[256];
  const int lane = threadIdx.x;
  const int qi = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int qbase, Sq, Sk;
  ext_row(p, b, &qbase, &Sq, &Sk);
  if (qi >= Sq) return;                       // idle rows too (Sq = 0)
  const int hk = h / (p.H / p.Hkv);
  const T* Q = (const T*)p.q + (int64_t)(qbase + qi) * p.q_ss + h * p.q_sh;
  const T* K = (const T*)p.k + b * p.k_sb + hk * p.k_sh;
  const T* VT = (const T*)p.vt + b * p.v_sb + hk * p.v_sh;
  int64_t dk = 0, dv = 0;
  int sh = 0;
  if constexpr (SH) {
    int src;
    sh = ext_shared(p, b, Sk, &src);
    dk = (src - b) * p.k_sb;
    dv = (src - b) * p.v_sb;
  }
  for (int d = lane; d < hd; d += 64) qs[d] = Cvt<T>::ld(Q + d);
  __syncthreads();
  const int kv_end = min(Sk, qi + (Sk - Sq) + 1);
  float m = -INFINITY, l = 0.f;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
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
    const float alpha = __expf(m - mn);
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
  T* O = (T*)p.out + (int64_t)(qbase + qi) * p.o_ss + h * p.o_sh;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < hd) Cvt<T>::st(O + d, o[i] / l);
  }
}

// rope_kv_kernel (a3v_rowops.hip) per row: grid (ceil(nq_max / 64), H + 2 Hkv, B), block 256 = 64 tokens x one head.  S = the row's
// span, start_pos = rope_pos0 = sk[b] - S, the token rows q_off[b] + s of the packed qkv.  A span that does not fit
// (start < 0 or sk[b] > Smax) or a longer one than nq_max is an idle row: nothing is written.
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_extend_kernel(const T* __restrict__ qkv, int64_t ldqkv, T* __restrict__ q_out, int64_t ldq,
                                                             T* __restrict__ k_cache, T* __restrict__ vt_cache,
                                                             const float* __restrict__ cos_sin, const int32_t* __restrict__ q_off,
                                                             const int32_t* __restrict__ sk, int nq_max, int H, int Hkv, int hd, int Smax) {
  __shared__ T tile[64][128 + 8];
  const int s0 = blockIdx.x * 64, slot = blockIdx.y, b = blockIdx.z;
  const int m0 = q_off[b], S = q_off[b + 1] - m0, skb = sk[b];
  const int start_pos = skb - S;
  if (S <= 0 || S > nq_max || m0 < 0 || start_pos < 0 || skb > Smax || s0 >= S) return;     // block-uniform
  const int tid = threadIdx.x;
  const int cpr = hd / 8;
  const int n_chunks = 64 * cpr;
  const T* src = qkv + (int64_t)m0 * ldqkv + (int64_t)slot * hd;
  if (slot < H + Hkv) {
    const bool is_q = slot < H;
    for (int id = tid; id < n_chunks; id += 256) {
      const int r = id / cpr, c = (id % cpr) * 8;
      const int s = s0 + r;
      if (s >= S) continue;
      float v[8], o[8];
      load8(src + (int64_t)s * ldqkv + c, v);
      const float* cs = cos_sin + ((int64_t)(start_pos + s) * (hd / 2) + c / 2) * 2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float co = cs[2 * e], si = cs[2 * e + 1];
        const float a = v[2 * e], bb = v[2 * e + 1];
        o[2 * e] = a * co - bb * si;
        o[2 * e + 1] = a * si + bb * co;
      }
      if (is_q) {
        store8(q_out + ((int64_t)m0 + s) * ldq + (int64_t)slot * hd + c, o);
      } else {
        const int hk = slot - H;
        store8(k_cache + (((int64_t)b * Hkv + hk) * Smax + start_pos + s) * hd + c, o);
      }
    }
    return;
  }
  const int hk = slot - H - Hkv;
  for (int id = tid; id < n_chunks; id += 256) {
    const int r = id / cpr, c = (id % cpr) * 8;
    const int s = s0 + r;
    float v[8];
    if (s < S) load8(src + (int64_t)s * ldqkv + c, v);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) Cvt<T>::st(&tile[r][c + e], v[e]);
  }
  __syncthreads();
  T* dst = vt_cache + ((int64_t)b * Hkv + hk) * (int64_t)hd * Smax + start_pos + s0;
  const int nvalid = min(64, S - s0);
  const bool aligned = ((start_pos + s0) % 8 == 0) && (Smax % 8 == 0);
  for (int id = tid; id < hd * 8; id += 256) {
    const int d = id >> 3, t0 = (id & 7) * 8;
    if (t0 >= nvalid) continue;
    T* dp = dst + (int64_t)d * Smax + t0;
    if (aligned && t0 + 8 <= nvalid) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = Cvt<T>::ld(&tile[t0 + e][d]);
      store8(dp, o);
    } else {
      for (int e = 0; e < 8 && t0 + e < nvalid; ++e) dp[e] = tile[t0 + e][d];
    }
  }
}

inline int one_bound(int H, int sk_max, int* ch_max) {
  const int want = (768 + H - 1) / H;
  const int maxs = (sk_max + 127) / 128;
  const int ns0 = want < maxs ? want : maxs;       // every row's split count is <= its own min(want, maxs) <= this one
  int ch = (sk_max + want - 1) / want;
  ch = (ch + 63) & ~63;
  *ch_max = ch > 128 ? ch : 128;                   // maxs <= want: ceil(Sk / maxs) <= 128
  return ns0 < 1 ? 1 : ns0;
}

}  // namespace

extern "C" int64_t a3v_attention_extend_rows_scratch_floats(int B, int H, int hd, int sk_max) {
  if (B <= 0 || H <= 0 || hd <= 0 || sk_max <= 0) return 0;
  int ch;
  return (int64_t)B * H * one_bound(H, sk_max, &ch) * (hd + 2);
}

extern "C" int a3v_attention_extend_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* q_off, const int32_t* sk,
                                         const int32_t* src_row, const int32_t* shared, int nq_max, int sk_max, int B, int H, int Hkv,
                                         int hd, const int64_t* strides, float* scratch, int dtype, void* stream) {
  if (!q || !k || !vt || !out || !q_off || !sk || !strides || B <= 0 || H <= 0 || Hkv <= 0 || nq_max <= 0 || sk_max <= 0) return A3V_ERR_ARG;
  if (!src_row != !shared) return A3V_ERR_ARG;
  if (H % Hkv || hd <= 0 || hd > 256) return A3V_ERR_SHAPE;
  if (dtype != A3V_BF16 && dtype != A3V_F32) return A3V_ERR_DTYPE;
  // a V^T row (strides[8]) and a K head (strides[4]) bound sk_max, as in a3v_attention_decode_rows
  if (sk_max > strides[8] || (int64_t)sk_max * strides[5] > strides[4]) return A3V_ERR_SHAPE;
  if (B > 65535 || H > 65535) return A3V_ERR_SHAPE;
  ExtArgs p;
  p.q = q; p.k = k; p.vt = vt; p.out = out; p.q_off = q_off; p.sk = sk; p.src_row = src_row; p.shared = shared;
  p.q_ss = strides[1]; p.q_sh = strides[2];
  p.k_sb = strides[3]; p.k_sh = strides[4]; p.k_ss = strides[5];
  p.v_sb = strides[6]; p.v_sh = strides[7]; p.v_sd = strides[8];
  p.o_ss = strides[10]; p.o_sh = strides[11];
  p.B = B; p.H = H; p.Hkv = Hkv; p.nq_max = nq_max; p.sk_max = sk_max;
  p.scale = 1.0f / sqrtf((float)hd);
  p.scale_log2 = p.scale * 1.4426950408889634f;
  p.lazy_rescale = A3V_ENV_INT("A3V_ATTN_LAZY", 1);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_F32 || (hd != 64 && hd != 128)) {
    const dim3 g(nq_max, H, B);
    if (src_row) {
      if (dtype == A3V_F32) hipLaunchKernelGGL((attn_extend_generic_kernel<float, true>), g, dim3(64), 0, st, p, hd);
      else hipLaunchKernelGGL((attn_extend_generic_kernel<bf16_t, true>), g, dim3(64), 0, st, p, hd);
    } else if (dtype == A3V_F32) hipLaunchKernelGGL((attn_extend_generic_kernel<float, false>), g, dim3(64), 0, st, p, hd);
    else hipLaunchKernelGGL((attn_extend_generic_kernel<bf16_t, false>), g, dim3(64), 0, st, p, hd);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  if (!scratch) return A3V_ERR_ARG;
  for (int i = 0; i < 12; ++i)
    if (i != 0 && i != 9 && (strides[i] % 8)) return A3V_ERR_SHAPE;       // 16-B vector access, staged O (the row strides 0 / 9 are not used)
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt) | reinterpret_cast<uintptr_t>(out)) & 15)
    return A3V_ERR_SHAPE;
  if (nq_max > 1) {
    const int64_t blocks = (int64_t)((nq_max + 127) / 128) * H * B;
    if (blocks > 0x7fffffff) return A3V_ERR_SHAPE;
    const dim3 grid((unsigned)blocks);
    if (src_row) {
      if (hd == 128) hipLaunchKernelGGL((attn_extend_bf16_kernel<128, true>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((attn_extend_bf16_kernel<64, true>), grid, dim3(256), 0, st, p);
    } else if (hd == 128) hipLaunchKernelGGL((attn_extend_bf16_kernel<128, false>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((attn_extend_bf16_kernel<64, false>), grid, dim3(256), 0, st, p);
    A3V_LAUNCH_CHECK();
  }
  // one-query rows (the host cannot see q_off: the pair is always launched; its blocks leave at once for every other row)
  int chm;
  const int nsb = one_bound(H, sk_max, &chm);
  const size_t shm = (size_t)(chm + 8) * sizeof(float);
  if (shm > 48 * 1024) return A3V_ERR_SHAPE;
  const dim3 g1(nsb, H, B);
  if (src_row) {
    if (hd == 128) hipLaunchKernelGGL((attn_extend_one_kernel<128, true>), g1, dim3(256), shm, st, p, scratch, nsb);
    else hipLaunchKernelGGL((attn_extend_one_kernel<64, true>), g1, dim3(256), shm, st, p, scratch, nsb);
  } else if (hd == 128) hipLaunchKernelGGL((attn_extend_one_kernel<128, false>), g1, dim3(256), shm, st, p, scratch, nsb);
  else hipLaunchKernelGGL((attn_extend_one_kernel<64, false>), g1, dim3(256), shm, st, p, scratch, nsb);
  A3V_LAUNCH_CHECK();
  if (hd == 128) hipLaunchKernelGGL(attn_extend_one_combine_kernel<128>, dim3(H, B), dim3(128), 0, st, p, (const float*)scratch, nsb);
  else hipLaunchKernelGGL(attn_extend_one_combine_kernel<64>, dim3(H, B), dim3(64), 0, st, p, (const float*)scratch, nsb);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_rope_kvcache_extend(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                                       const float* cos_sin, const int32_t* q_off, const int32_t* sk, int nq_max, int B, int H, int Hkv,
                                       int hd, int Smax, int dtype, void* stream) {
  if (!qkv || !q_out || !k_cache || !vt_cache || !cos_sin || !q_off || !sk || B <= 0 || H <= 0 || Hkv <= 0 || nq_max <= 0) return A3V_ERR_ARG;
  if (hd <= 0 || hd % 8 || hd > 128 || ldqkv % 8 || ldq % 8 || Smax <= 0 || B > 65535 || H + 2 * Hkv > 65535) return A3V_ERR_SHAPE;
  if (ldqkv < (int64_t)(H + 2 * Hkv) * hd || ldq < (int64_t)H * hd) return A3V_ERR_SHAPE;
  const dim3 g((nq_max + 63) / 64, H + 2 * Hkv, B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3V_BF16)
    hipLaunchKernelGGL(rope_kv_extend_kernel<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)qkv, ldqkv, (bf16_t*)q_out, ldq, (bf16_t*)k_cache,
                       (bf16_t*)vt_cache, cos_sin, q_off, sk, nq_max, H, Hkv, hd, Smax);
  else if (dtype == A3V_F32)
    hipLaunchKernelGGL(rope_kv_extend_kernel<float>, g, dim3(256), 0, st, (const float*)qkv, ldqkv, (float*)q_out, ldq, (float*)k_cache,
                       (float*)vt_cache, cos_sin, q_off, sk, nq_max, H, Hkv, hd, Smax);
  else return A3V_ERR_DTYPE;
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
