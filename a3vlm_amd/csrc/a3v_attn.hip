// Attention for gfx950: softmax(q k^T / sqrt(hd) [+ right-aligned causal]) v.
//
// Layout contract (elements, explicit strides): q/out [b][s][h][hd]; k [b][hkv][s][hd];
// vt = V TRANSPOSED [b][hkv][hd][s].  V^T lets both MFMA products run "transposed":
//     S^T = K . Q^T   (A = K rows from LDS, B = Q rows from registers)
//     O^T = V^T . P^T (A = V^T rows from LDS, B = P straight from the S^T accumulators)
// With v_mfma_f32_32x32x16_bf16 the C/D map is col = lane&31, row = (r&3)+8(r>>2)+4(lane>>5),
// so a lane owns ONE query column of S^T and of O^T: the online softmax (max, exp, sum,
// rescale) is lane-local plus one lane<->lane+32 exchange, and P never leaves registers --
// the 16 accumulator values of a lane are, in register order, exactly the k-elements the
// P^T B-operand wants when V^T rows are read at kv = base + 4*(lane>>5) + {0..3, 8..11}.
//
//  * attn_prefill_bf16_kernel<HD,CAUSAL>: 4 waves x 32 query rows, KV tiles of 64 through
//    LDS (K rows XOR-swizzled for ds_read_b128, V^T rows for ds_read_b64), two waves per SIMD.
//  * attn_decode_bf16_kernel<HD>: Sq == 1, split-KV (flash-decoding), HBM-bound streaming of
//    K rows / V^T rows with 16-byte loads, + combine kernel.
//  * attn_f32_kernel: fp32 parity path (any Sq), one wave per (b, h, q).
#include "a3v_common.h"
#include <type_traits>
#include <cstdlib>

namespace {

struct AttnArgs {
  const void* q; const void* k; const void* vt; void* out;
  int64_t q_sb, q_ss, q_sh;     // q strides: batch, seq, head
  int64_t k_sb, k_sh, k_ss;     // k strides: batch, kv-head, seq   (hd contiguous)
  int64_t v_sb, v_sh, v_sd;     // vt strides: batch, kv-head, d    (seq contiguous)
  int64_t o_sb, o_ss, o_sh;
  int B, Sq, Sk, H, Hkv;
  float scale_log2;             // log2(e) / sqrt(hd)
  float scale;
  float* lse;                   // optional [B,H,Sq] log-sum-exp of the scaled scores (training backward)
  int head_group;               // causal prefill: heads per tile-rank-major group of the block order (1 = head-major)
  int staged_o;                 // prefill: O leaves through an LDS patch as whole rows (0, the decode entry: per-lane row stores)
  int lazy_rescale;             // prefill: the softmax reference only moves when a row's exponent would exceed 2^8 (A3V_ATTN_LAZY=0: every tile)
};

// one 16-B-per-lane LDS-DMA through a buffer descriptor: per-lane byte offset + wave-uniform byte offset (an SGPR)
__device__ __forceinline__ void buf_dma16(__amdgpu_buffer_rsrc_t rs, char* lds_dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}

// own value and the value of lane ^ 32 in (a, b) (lanes < 32) / (b, a) (lanes >= 32).  Asm form: with the same value in both operands
// of __builtin_amdgcn_permlane32_swap hipcc uses ONE of the two results for both (v_max v, v, v in the ISA) and the exchange disappears.
__device__ __forceinline__ void xchg32(float x, float& a, float& b) {
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// The P^T operand is regrouped so that a lane half holds 8 CONSECUTIVE keys (two v_permlane32_swap per 16 keys exchange the
// {4 hh .. 4 hh + 3} quarters between lanes l and l + 32), and the V^T fragment becomes ONE 16-B chunk per lane (ds_read_b128,
// lanes 0-31 chunk c, lanes 32-63 chunk c + 1: the 16 lanes of a read group cover 16 distinct bank slots) instead of two 8-B
// halves of two chunks (ds_read_b64 pairs where rows r and r + 16 of a lane half share their banks: 2-way on every read,
// 1.18e7 conflict cycles per launch against 3.2e6 active LDS cycles in profiles/r01u_pmc_decode_lds.txt).
template <int HD, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_prefill_bf16_kernel(AttnArgs p) {
  constexpr int KVB = 64;
  constexpr int KROW = HD * 2;            // bytes per K row in LDS
  constexpr int KCH = HD / 8;             // 16-B chunks per K row
  constexpr int K_LOADS = KVB * KCH / 256;   // 16-B chunks per thread (4 for HD=128, 2 for 64)
  constexpr int V_LOADS = HD * 8 / 256;      // V^T tile: HD rows x 8 chunks of 16 B
  constexpr int TILEB = KVB * KROW + HD * 128;   // K tile + V^T tile
  __shared__ __attribute__((aligned(1024))) char lds[2 * TILEB];   // double buffered: tile t+1 lands by LDS-DMA while tile t is consumed

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1-D grid, XCD-aware: workgroups go to XCDs round-robin (id & 7), and every query tile of a (batch, head) reads the same
  // K / V^T, so XCD x takes a CONTIGUOUS range of (head, query tile) pairs -- a head's K/V then lives in ONE 4-MB L2 instead
  // of being fetched into all eight.  Within a head the heavy (late) causal tiles go first.
  const int nqt = (p.Sq + 127) / 128;
  int vb;
  {
    const int total = gridDim.x, id = blockIdx.x;
    const int xcd = id & 7, q = total >> 3, r = total & 7;
    vb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  int head_slot = vb / nqt;
  int qt = nqt - 1 - (vb - head_slot * nqt);
  if (CAUSAL && p.head_group > 1) {
    // causal tiles cost 2, 4, ..., 2 nqt KV tiles: with "heavy first" per head the long blocks of the XCD's last heads start late
    // and run alone (a list-scheduling simulation of the 7B prefill: 129 us against 103 for perfect packing).  Groups of
    // `head_group` heads are walked tile-rank-major instead (every head's heaviest tile, then every head's second, ...): the
    // group's K / V (head_group x 0.56 MB at S = 1091) still sits in the XCD's L2 while its tiles run.
    const int G = p.head_group, per = G * nqt;
    const int grp = vb / per, r = vb - grp * per;
    head_slot = grp * G + r % G;
    qt = nqt - 1 - r / G;
  }
  const int b = head_slot / p.H, h = head_slot - b * p.H;
  const int hk = h / (p.H / p.Hkv);
  const int q0 = qt * 128 + wave * 32;
  const int off = p.Sk - p.Sq;                 // right alignment (llama_ens5.py:181-185)

  const bf16_t* Q = (const bf16_t*)p.q + b * p.q_sb + h * p.q_sh;
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh;

  const int ql = lane & 31, hh = lane >> 5;
  int qrow = q0 + ql;
  const int qrow_c = qrow < p.Sq ? qrow : p.Sq - 1;
  // Q fragments (B operand): Q[q][16*ks + 8*hh + e]
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

  // kv range for this block: all q rows of the block
  int kv_end = p.Sk;
  if (CAUSAL) {
    const int last_q = min(qt * 128 + 127, p.Sq - 1);
    kv_end = min(p.Sk, last_q + off + 1);
  }
  const int n_tiles = (kv_end + KVB - 1) / KVB;

  u32x4 kreg[K_LOADS], vreg[V_LOADS];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < K_LOADS; ++i) {
      const int id = tid + i * 256;
      const int row = id / KCH, ch = id % KCH;
      int kr = kv0 + row;
      kr = kr < p.Sk ? kr : p.Sk - 1;
      kreg[i] = *reinterpret_cast<const u32x4*>(K + (int64_t)kr * p.k_ss + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < V_LOADS; ++i) {
      const int id = tid + i * 256;
      const int d = id >> 3, ch = id & 7;
      const int kv = kv0 + ch * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kv + 8 <= p.Sk) {
        v = *reinterpret_cast<const u32x4*>(VT + (int64_t)d * p.v_sd + kv);
      } else if (kv < p.Sk) {   // ragged tail: zero the columns >= Sk (0 * garbage must stay 0)
        const unsigned short* src = reinterpret_cast<const unsigned short*>(VT + (int64_t)d * p.v_sd + kv);
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (kv + j < p.Sk) ? src[j] : (unsigned short)0;
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
  // LDS-DMA form of load_tile + write_tile for tiles whose 64 keys all exist (kv0 + 64 <= Sk): the chunk permutation is
  // applied on the per-lane SOURCE offset (DMA destinations are lane-linear), no VGPRs are held while the tile is in flight.
  // Buffer-descriptor form: the per-lane byte offsets are loop constants, the tile's position is one scalar offset per
  // instruction -- issuing a tile costs 8 VMEM instructions and no address VALU (the flat-address form spent ~500 cycles per tile).
  const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)K, 0, 0x7fffffff, 0x00020000);
  const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)VT, 0, 0x7fffffff, 0x00020000);
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
#pragma unroll
    for (int i = 0; i < K_LOADS; ++i)
      buf_dma16(rsK, Ks + (wave_u * 64 + i * 256) * 16, koff[i], ks_off);
#pragma unroll
    for (int i = 0; i < V_LOADS; ++i)
      buf_dma16(rsV, Vs + (wave_u * 64 + i * 256) * 16, voff[i], vs_off);
  };
  auto full_tile = [&](int t) { return t * KVB + KVB <= p.Sk; };

  // Software pipeline with ONE barrier per tile: at the top of iteration t every wave waits for its own share of tile t's DMA
  // and meets the others -- which also proves that all of them finished iteration t-1, so the buffer tile t+1 goes to (the one
  // iteration t-1 read) is free and its DMA is issued right after the barrier, a full tile of compute ahead of its use.
  // A ragged last tile (keys past Sk inside it) takes the register path, which zero-fills the missing V^T columns.
#ifdef AP_STAMP
  unsigned long long* stamps = (vb == AP_STAMP && tid == 0) ? reinterpret_cast<unsigned long long*>(p.lse) : nullptr;
#define AP_ST(t, k) do { if (stamps && (t) < 64) stamps[(t) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define AP_ST(t, k) do {} while (0)
#endif
  if (n_tiles > 0 && full_tile(0)) dma_tile(0, lds, lds + KVB * KROW);
  // Per-lane fragment bases: the K chunk swizzle looks at row bits 0-3 (HD 128) / 1-3 (HD 64) and the V^T one at bits 1-3, which the
  // block offsets (32 tb rows of K, 32 d rows of V^T) leave alone, and (2 ks | hh) ^ sw == (2 ks) ^ (hh ^ sw): every fragment
  // address is tile + block offset + (base ^ constant).  The loop is unrolled by two so that the tile buffer is a compile-time
  // constant too: the whole address becomes one v_xor + an instruction offset (the per-fragment row / swizzle / buffer arithmetic
  // was ~125 of the ~330 VALU instructions of a tile).
  const int kfb = ql * KROW + ((hh ^ ((HD == 128) ? (ql & 15) : ((ql >> 1) & 7))) << 4);
  const int vfb = ql * 128 + ((hh ^ ((ql >> 1) & 7)) << 4);
  auto body = [&](int t, auto bufc) {
    constexpr int BUF = decltype(bufc)::value;
    AP_ST(t, 0);
    const int kv0 = t * KVB;
    char* Ks = lds + BUF * TILEB;
    char* Vs = Ks + KVB * KROW;
    if (full_tile(t)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      AP_ST(t, 6);
      __syncthreads();
    } else {                          // this tile's buffer was last read in iteration t-2, which the barrier of t-1 closed
      load_tile(kv0);
      write_tile(Ks, Vs);
      __syncthreads();
    }
    AP_ST(t, 5);
    if (t + 1 < n_tiles && full_tile(t + 1)) dma_tile(kv0 + KVB, lds + (1 - BUF) * TILEB, lds + (1 - BUF) * TILEB + KVB * KROW);
    AP_ST(t, 1);
    // causal: a tile whose first key lies past this wave's LAST query row contributes nothing to the wave (the block walks the
    // tiles its last wave needs); the wave only keeps the block's barrier / DMA cadence and leaves the SIMD to its partner
    if (CAUSAL && kv0 > q0 + 31 + off) return;
    // ---- S^T = K . Q^T : two 32-row kv blocks ----
    f32x16 s[2];
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[tb][r] = 0.f;
    // the two key blocks' accumulation chains alternate (back-to-back MFMAs on ONE accumulator issue at ~72 cycles, not 32)
    constexpr bool FRAG_AHEAD = HD == 128;      // hd 64 (the ViT) measured 15 % slower with the reads ahead: 34.5-36.0 against 29.8-30.6 us
    if constexpr (!FRAG_AHEAD) {
#pragma unroll
      for (int ks = 0; ks < HD / 16; ++ks)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + tb * 32 * KROW + (kfb ^ (ks << 5)));
          s[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[tb], 0, 0, 0);
        }
    } else {
      // fragment reads TWO k-steps (4 MFMAs, >= 128 cycles) ahead of their MFMAs: hipcc reuses one register pair and issues every read
      // right in front of its consumer (ds_read, s_waitcnt lgkmcnt, v_mfma: the LDS latency of every pair is exposed)
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
          asm volatile("" : "+v"(qf[ks]) :: "memory");      // the k-step's MFMAs (they read qf[ks]) stay BEHIND the reads issued above
        }
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) s[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr[ks % 3][tb], qf[ks], s[tb], 0, 0, 0);
      }
    }
    AP_ST(t, 2);
    // ---- mask + online softmax (lane owns query column ql; kv = 32tb + (r&3)+8(r>>2)+4hh) ----
    const int qlim = CAUSAL ? (qrow + off) : 0x7fffffff;
    // interior tiles (every key of the tile visible to every query row of this wave) skip the 32 compare/selects
    const bool need_mask = (kv0 + KVB > p.Sk) || (CAUSAL && kv0 + KVB - 1 > q0 + off);
    float mx = -INFINITY;
    if (need_mask) {
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + tb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const bool ok = (kv < p.Sk) && (kv <= qlim);
          s[tb][r] = ok ? s[tb][r] : -INFINITY;
        }
    }
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[tb][r]);
    // lane <-> lane + 32 by v_permlane32_swap (VALU) instead of __shfl_xor (ds_bpermute_b32: an LDS-pipe round trip + lgkmcnt(0) in the
    // max -> reference -> exponentials chain of every tile); asm form, see xchg32
    if (p.lazy_rescale & 2) mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // (A3V_ATTN_LAZY=3: the ds_bpermute form, A/B runs)
    else { float x0, x1; xchg32(mx, x0, x1); mx = fmaxf(x0, x1); }
    const float m_new = fmaxf(m_run, mx);
    // Lazy rescale: m_run is the REFERENCE the exponentials are taken against, not necessarily the running maximum.  It only moves
    // when some row of the wave would otherwise see exp2 arguments above +LAZY (2^8: P <= 256 in bf16, the sums in fp32) -- after the
    // first tiles of a row that is rare, and the 64 multiplies of the O rescale + the l update (a quarter of the tile's VALU work,
    // which is what bounds this kernel) are skipped by a wave-uniform branch.  O / l and the LSE are unchanged in exact arithmetic.
    const bool grow = (p.lazy_rescale & 1) ? ((m_new - m_run) * p.scale_log2 > 8.f || m_run == -INFINITY) : true;
    const bool resc = __builtin_amdgcn_ballot_w64(grow && m_new != m_run) != 0;
    // rows past Sq (clamped duplicates) and fully-masked tiles keep m finite once any tile was seen
    const float m_tgt = resc ? m_new : m_run;
    const float m_use = (m_tgt == -INFINITY) ? 0.f : m_tgt;
    // raw v_exp_f32 (the arguments are <= 0 [<= LAZY] and results below the denormal range flush to 0, which is what a probability
    // that small should do; exp2f() wraps every call in a range fix-up: +4 VALU per element)
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
        __builtin_memcpy(&w, &pf[tb][c], 16);           // dwords: keys 16c + 4hh + {0,1 | 2,3} and 16c + 8 + 4hh + {0,1 | 2,3}
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(w[e], w[2 + e], false, false);
          w[e] = sw[0];                                 // lanes < 32: own first quarter   | lanes >= 32: partner's third quarter
          w[2 + e] = sw[1];                             // lanes < 32: partner's 2nd quarter | lanes >= 32: own fourth quarter
        }
        __builtin_memcpy(&pf[tb][c], &w, 16);           // lanes < 32: keys 16c + 0..7, lanes >= 32: keys 16c + 8..15
      }
    if (resc) {
#pragma unroll
      for (int d = 0; d < HD / 32; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    }
    AP_ST(t, 3);
    // ---- O^T += V^T . P^T ----
    if constexpr (FRAG_AHEAD) {
      // the four V^T fragments of the next (key block, 16-key chunk) group are read while the current group's four MFMAs run
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
          asm volatile("" : "+v"(pf[tb][c]) :: "memory");   // the group's MFMAs (they read pf[tb][c]) stay BEHIND the reads issued above
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
          for (int d = 0; d < HD / 32; ++d) {   // (the d blocks' chains interleaved, see the QK product)
            const int c16 = 4 * tb + 2 * c;     // lane half hh takes the WHOLE 16-B chunk c16 + hh (8 consecutive keys)
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vs + d * 32 * 128 + (vfb ^ (c16 << 4)));
            o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[tb][c], o[d], 0, 0, 0);
          }
    }
    AP_ST(t, 4);
  };
  {
    int t = 0;
    for (; t + 1 < n_tiles; t += 2) {
      body(t, std::integral_constant<int, 0>{});
      body(t + 1, std::integral_constant<int, 1>{});
    }
    if (t < n_tiles) body(t, std::integral_constant<int, 0>{});
  }

#ifdef AP_STAMP
  if (stamps) return;
#endif
  // ---- normalise and store O[q][d], d = 32*db + 8*g + 4*hh + {0..3} ----
  float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
#ifndef AP_STAMP
  if (p.lse && qrow < p.Sq && hh == 0)
#else
  if (false)
#endif
    p.lse[((int64_t)b * p.H + h) * p.Sq + qrow] = m_run * p.scale + __logf(l_tot);
  if (p.staged_o && !(p.o_ss & 7) && !(p.o_sh & 7) && !(p.o_sb & 7) && !(reinterpret_cast<uintptr_t>(p.out) & 15)) {
    // The lane owns one query row: stored directly, an instruction writes 16 bytes into each of 32 rows (partial lines, ~6 B/clk/CU:
    // tools/ubench/stores.hip).  The wave's 32 x HD tile goes through a private LDS patch (the K / V^T buffers are free after one
    // more barrier) and leaves as whole rows, 16 bytes per lane.  8-byte slot s of row r sits at slot s ^ ((r & (HD/8 - 1)) << 1).
    constexpr int ROWB = HD * 2, NPAIR = HD / 8, RPI = 64 / NPAIR;          // row bytes, 16-byte pairs per row, rows per store instruction
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
    bf16_t* Ob = (bf16_t*)p.out + b * p.o_sb + h * p.o_sh + pr * 8;
    const int qw = qt * 128 + wave * 32;
#pragma unroll
    for (int it = 0; it < 32 / RPI; ++it) {
      const int r = it * RPI + rr;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(patch + r * ROWB + ((pr ^ (r & (NPAIR - 1))) << 4));
      if (qw + r < p.Sq) *reinterpret_cast<bf16x8*>(Ob + (int64_t)(qw + r) * p.o_ss) = v;
    }
    return;
  }
  if (qrow < p.Sq) {
    bf16_t* O = (bf16_t*)p.out + b * p.o_sb + (int64_t)qrow * p.o_ss + h * p.o_sh;
#pragma unroll
    for (int d = 0; d < HD / 32; ++d)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = f2bf(o[d][g4 * 4 + e] * inv);
        *reinterpret_cast<bf16x4*>(O + d * 32 + g4 * 8 + hh * 4) = ov;
      }
  }
}

// ------------------------------------------------------------------------------------
// Decode (Sq == 1): grid (nsplit, H, B); block 256.  part[b][h][split] = {o[HD], m, l}
// ------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_bf16_kernel(AttnArgs p, float* part, int nsplit, int chunk) {
  constexpr int LPR = HD / 8;            // lanes per K row (16-B each)
  constexpr int RPW = 64 / LPR;          // K rows per wave-load
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* sc = reinterpret_cast<float*>(dsm);       // chunk scores / probabilities
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int kv_hi = min(p.Sk, kv_lo + chunk);
  const int n = kv_hi - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * nsplit + sp) * (HD + 2);
  if (n <= 0) {          // cannot happen with decode_plan's splits (every split owns >= 1 key); kept for safety
    if (tid < HD) po[tid] = 0.f;
    if (tid == 0) { po[HD] = -INFINITY; po[HD + 1] = 0.f; }
    return;
  }
  const bf16_t* Q = (const bf16_t*)p.q + b * p.q_sb + h * p.q_sh;
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh;
  // phase 1: scores.  lane -> (row-in-group, 8 d's); U independent row groups in flight per wave
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
      const bf16x8* kp = reinterpret_cast<const bf16x8*>(K + (int64_t)(kv_lo + r) * p.k_ss + lc);
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
    // P is rounded to bf16 before P.V in the prefill kernel and in bf16 SDPA; keep fp32 sum
    sc[i] = e;
    ls += e;
  }
  ls = wave_sum(ls);
  __syncthreads();
  if (lane == 0) red[4 + wave] = ls;
  __syncthreads();
  ls = red[4] + red[5] + red[6] + red[7];
  // zero-pad the probabilities to a multiple of 8 for the vector loop
  const int n8 = (n + 7) & ~7;
  for (int i = n + tid; i < n8; i += 256) sc[i] = 0.f;
  __syncthreads();

  // phase 2: o[d] = sum_kv p[kv] * VT[d][kv].  wave -> HD/4 consecutive d rows, 8 rows (8 x 16 B per lane) in
  // flight per batch, lanes -> 8-kv chunks of the row; one shuffle reduction per row at the end of a batch.
  // Loads are unconditional 16-B vectors (kv_lo + n8 <= Skmax: the cache row is allocated to a multiple of 64);
  // columns >= Sk are masked on the VALUES after the load (a select on the load itself would serialise them).
  constexpr int DB = 8;
  for (int d0 = wave * (HD / 4); d0 < (wave + 1) * (HD / 4); d0 += DB) {
    float acc[DB];
#pragma unroll
    for (int j = 0; j < DB; ++j) acc[j] = 0.f;
    for (int c = lane * 8; c < n8; c += 64 * 8) {
      bf16x8 vv[DB];
#pragma unroll
      for (int j = 0; j < DB; ++j) {
        const bf16x8* vp = reinterpret_cast<const bf16x8*>(VT + (int64_t)(d0 + j) * p.v_sd + kv_lo + c);
        vv[j] = *vp;
      }
      float pv[8];
      const int nvalid = p.Sk - (kv_lo + c);          // >= 8 except in the last chunk
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

// Sums over the 16 (8) lanes of a DPP row (half row) with four (three) v_add_f32_dpp: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror.  (__shfl_xor compiles to ds_bpermute_b32: an LDS-pipe round trip per step.)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)));
}
__device__ __forceinline__ float row8_sum(float v) { return dpp_add<0x141>(dpp_add<0x4E>(dpp_add<0xB1>(v))); }
__device__ __forceinline__ float row16_sum(float v) { return dpp_add<0x140>(row8_sum(v)); }
__device__ __forceinline__ float row8_max(float v) { return dpp_max<0x141>(dpp_max<0x4E>(dpp_max<0xB1>(v))); }

// ------------------------------------------------------------------------------------
// Decode, wave-streaming form (round 2): grid (nsplit, H, B), block 512 = 8 waves; nsplit = 1 when B*H alone fills the CUs.
// The first form streams K, synchronises the block for the softmax, then streams V^T: every block of the chip changes phase
// together and ~17 of its 37 us at context 1100 did not scale with the bytes (tools/attn_decode_bench.py).  Here each WAVE owns
// every eighth 64-key tile: the tile's K rows (16 KB) AND its V^T columns (128 B of each of the HD rows, 16 KB) are in flight
// together (32 x 16 B per lane), the next tile's K rows are requested before this tile's softmax, scores -> wave-private online softmax -> P.V
// without leaving the wave; the eight waves merge (m, l, o) once through LDS.  No block-wide phase change, and with one block
// per (batch, head) no cross-block hand-off either.
// ------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(512) void attn_decode_wave_kernel(AttnArgs p, float* part, int nsplit, int chunk, int* counters) {
  constexpr int LPR = HD / 8;        // lanes per K row (16 B each)
  constexpr int RPW = 64 / LPR;      // K rows per wave-wide load
  constexpr int NKL = 64 / RPW;      // K loads per 64-key tile
  constexpr int NVL = HD / 8;        // V^T loads per tile (8 d rows x 128 B per load)
  __shared__ __attribute__((aligned(16))) float sc_s[8][64];
  __shared__ float comb[8][HD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int hk = h / (p.H / p.Hkv);
  const int kv_lo = sp * chunk;
  const int n = min(p.Sk, kv_lo + chunk) - kv_lo;
  float* po = part + ((int64_t)(b * p.H + h) * nsplit + sp) * (HD + 2);
  const bf16_t* Q = (const bf16_t*)p.q + b * p.q_sb + h * p.q_sh;
  const bf16_t* K = (const bf16_t*)p.k + b * p.k_sb + hk * p.k_sh + (int64_t)kv_lo * p.k_ss;
  const bf16_t* VT = (const bf16_t*)p.vt + b * p.v_sb + hk * p.v_sh + kv_lo;
  // 64-key tiles of the block's n keys go round-robin to the eight waves: every V^T request is a whole, aligned 128-byte line
  // (contiguous eighths of the keys start at multiples of 8 keys: Sk = 1110 put every wave 32 B into a line, 43 us against 30)
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
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        const int r = min(t0 + u * RPW + lr, hi - 1);
        const bf16x8* kp = reinterpret_cast<const bf16x8*>(K + (int64_t)r * p.k_ss + lc);
        kk[u] = __builtin_nontemporal_load(kp);            // non-temporal: the K / V^T stream is read once per step by one block
      }
    };
    load_k(lo);
    // software pipeline: V^T(t) is requested before the scores of tile t are computed, K(t+1) before its softmax / P.V -- the
    // memory system always has 16-32 KB per wave outstanding (without it every wave of the chip asks for its 32 KB at the same
    // moment, computes while HBM idles, and asks again: 40 us instead of the 33 of the two-phase form)
    for (int t0 = lo; t0 < hi; t0 += 512) {
      bf16x8 vv[NVL];
      const int kvc = min(t0 + c8, last_vec);              // vectors past the wave's range re-read its last one (masked below)
#pragma unroll
      for (int j = 0; j < NVL; ++j) {
        const bf16x8* vp = reinterpret_cast<const bf16x8*>(VT + (int64_t)(j * 8 + dr) * p.v_sd + kvc);
        vv[j] = __builtin_nontemporal_load(vp);
      }
#pragma unroll
      for (int u = 0; u < NKL; ++u) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(qv[e], (float)kk[u][e], a);
        a = LPR == 16 ? row16_sum(a) : row8_sum(a);
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
      mt = row8_max(mt);
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
  for (int j = 0; j < NVL; ++j) {
    acc[j] = row8_sum(acc[j]);
  }
  l = row8_sum(l);
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
    if (nsplit == 1 && counters) {
      ((bf16_t*)p.out)[b * p.o_sb + h * p.o_sh + tid] = f2bf(o / L);
    } else {
      po[tid] = o;
      if (tid == 0) { po[HD] = M; po[HD + 1] = L; }
    }
  }
  if (!counters || nsplit == 1) return;
  decode_combine_tail<HD>(p.out, p.o_sb, p.o_sh, p.H, part, po, nsplit, counters, b, h, tid);
}

template <int HD>
__global__ void attn_decode_combine_kernel(const float* part, void* out, int64_t o_sb, int64_t o_sh,
                                           int H, int nsplit, int dtype) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const float* pp = part + (int64_t)(b * H + h) * nsplit * (HD + 2);
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
  if (dtype == A3V_BF16) ((bf16_t*)out)[b * o_sb + h * o_sh + d] = f2bf(v);
  else ((float*)out)[b * o_sb + h * o_sh + d] = v;
}

// ------------------------------------------------------------------------------------
// Generic attention (fp32 parity path; also bf16 with head dims the MFMA kernels do not
// cover): one wave per (q row, head, batch); any hd <= 256, any Sq.  fp32 math throughout.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void attn_generic_kernel(AttnArgs p, int hd, int causal) {
  __shared__ float pbuf[64];
  __shared__ float qs[256];
  const int lane = threadIdx.x;
  const int qi = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int hk = h / (p.H / p.Hkv);
  const T* Q = (const T*)p.q + b * p.q_sb + (int64_t)qi * p.q_ss + h * p.q_sh;
  const T* K = (const T*)p.k + b * p.k_sb + hk * p.k_sh;
  const T* VT = (const T*)p.vt + b * p.v_sb + hk * p.v_sh;
  for (int d = lane; d < hd; d += 64) qs[d] = Cvt<T>::ld(Q + d);
  __syncthreads();
  const int kv_end = causal ? min(p.Sk, qi + (p.Sk - p.Sq) + 1) : p.Sk;
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
        for (int j = 0; j < cnt; ++j) a = fmaf(pbuf[j], Cvt<T>::ld(vr + j), a);
        o[i] = a;
      }
    }
  }
  T* O = (T*)p.out + b * p.o_sb + (int64_t)qi * p.o_ss + h * p.o_sh;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < hd) Cvt<T>::st(O + d, o[i] / l);
  }
  if (p.lse && lane == 0) p.lse[((int64_t)b * p.H + h) * p.Sq + qi] = m + __logf(l);
}

inline void decode_plan(int B, int H, int Sk, int* nsplit, int* chunk) {
  // ~768 blocks: at B*H = 256 three splits of the context beat four by 5-8 % for 600..1500 keys (larger chunks fill the 64 lanes of
  // the V^T scan and the K scan's 128-row passes)
  constexpr int A3V_DECODE_BLOCKS = 768;
  int want = (A3V_DECODE_BLOCKS + B * H - 1) / (B * H);
  int maxs = (Sk + 127) / 128;
  int ns = want < maxs ? want : maxs;
  if (ns < 1) ns = 1;
  int ch = (Sk + ns - 1) / ns;
  ch = (ch + 63) & ~63;
  ns = (Sk + ch - 1) / ch;
  *nsplit = ns;
  *chunk = ch;
}

}  // namespace

// The split plan of every wave-streaming decode attention (attn_decode_wave_kernel here, the fp8-KV, per-row and verify kernels of
// a3v_kv8 / a3v_ragged / a3v_spec.hip): one block per (batch, head) when that alone covers the CUs, else the fewest splits that do --
// never more than the two-phase plan, which a3v_attention_scratch_floats sizes the scratch for -- on chunks of whole 64-key tiles.
// (decode_plan returns ns >= 1 for Sk >= 1, so ns2 >= 1 without a clamp of its own.)
void a3v_decode_wave_plan(int B, int H, int Sk, int* nsplit, int* chunk) {
  int ns, ch;
  decode_plan(B, H, Sk, &ns, &ch);
  int ns2 = (256 + B * H - 1) / (B * H);
  if (ns2 > ns) ns2 = ns;
  int ch2 = (Sk + ns2 - 1) / ns2;
  ch2 = (ch2 + 63) & ~63;
  *nsplit = (Sk + ch2 - 1) / ch2;
  *chunk = ch2;
}

extern "C" int64_t a3v_attention_scratch_floats(int B, int H, int hd, int Sk) {
  int ns, ch;
  decode_plan(B, H, Sk, &ns, &ch);
  return (int64_t)B * H * ns * (hd + 2);
}

static int attention_impl(const void* q, const void* k, const void* vt, void* out, int B, int Sq, int Sk,
                          int H, int Hkv, int hd, const int64_t* strides, int causal, float* scratch,
                          float* lse, int dtype, void* stream) {
  if (!q || !k || !vt || !out || !strides || B <= 0 || Sq <= 0 || Sk <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (H % Hkv) return A3V_ERR_SHAPE;
  if (causal && Sk < Sq) return A3V_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  AttnArgs p;
  p.q = q; p.k = k; p.vt = vt; p.out = out;
  p.q_sb = strides[0]; p.q_ss = strides[1]; p.q_sh = strides[2];
  p.k_sb = strides[3]; p.k_sh = strides[4]; p.k_ss = strides[5];
  p.v_sb = strides[6]; p.v_sh = strides[7]; p.v_sd = strides[8];
  p.o_sb = strides[9]; p.o_ss = strides[10]; p.o_sh = strides[11];
  p.B = B; p.Sq = Sq; p.Sk = Sk; p.H = H; p.Hkv = Hkv;
  p.scale = 1.0f / sqrtf((float)hd);
  p.scale_log2 = p.scale * 1.4426950408889634f;
  p.lse = lse;
  p.head_group = 1;
  p.staged_o = 1;
  p.lazy_rescale = A3V_ENV_INT("A3V_ATTN_LAZY", 1);     // bit 0: lazy rescale; bit 1: ds_bpermute form of the row-maximum exchange (A/B)
  if (lse && Sq == 1 && dtype == A3V_BF16 && (hd == 64 || hd == 128)) return A3V_ERR_ARG;  // decode kernel has no LSE output
  if (dtype == A3V_F32) {
    if (hd > 256) return A3V_ERR_SHAPE;
    hipLaunchKernelGGL(attn_generic_kernel<float>, dim3(Sq, H, B), dim3(64), 0, st, p, hd, causal);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  if (dtype != A3V_BF16) return A3V_ERR_DTYPE;
  if (hd != 128 && hd != 64) {   // bf16 with an uncommon head dim: generic (slow, correct) kernel
    if (hd > 256) return A3V_ERR_SHAPE;
    hipLaunchKernelGGL(attn_generic_kernel<bf16_t>, dim3(Sq, H, B), dim3(64), 0, st, p, hd, causal);
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  for (int i = 0; i < 12; ++i)
    if (i != 2 && i != 4 && i != 11 && (strides[i] % 8)) return A3V_ERR_SHAPE;  // 16-B vector access
  if ((strides[2] % 8) || (strides[4] % 8) || (strides[11] % 4)) return A3V_ERR_SHAPE;
  if (Sq == 1) {
    if (!scratch) return A3V_ERR_ARG;
    int ns, ch;
    decode_plan(B, H, Sk, &ns, &ch);
    const size_t shm = (size_t)(ch + 8) * sizeof(float);
    const bool we = A3V_ENV_INT("A3V_ATTN_DECODE_WAVE_STANDALONE", 0) == 1;     // tuning runs (tools/attn_decode_bench.py): the wave-streaming form here too
    if (we && dtype == A3V_BF16) {
      int ns2, ch2;
      a3v_decode_wave_plan(B, H, Sk, &ns2, &ch2);
      if (hd == 128) {
        hipLaunchKernelGGL((attn_decode_wave_kernel<128>), dim3(ns2, H, B), dim3(512), 0, st, p, scratch, ns2, ch2, (int*)nullptr);
        hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(H, B), dim3(128), 0, st, scratch, out, p.o_sb, p.o_sh, H, ns2, dtype);
      } else {
        hipLaunchKernelGGL((attn_decode_wave_kernel<64>), dim3(ns2, H, B), dim3(512), 0, st, p, scratch, ns2, ch2, (int*)nullptr);
        hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(H, B), dim3(64), 0, st, scratch, out, p.o_sb, p.o_sh, H, ns2, dtype);
      }
      A3V_LAUNCH_CHECK();
      return A3V_OK;
    }
    if (hd == 128) {
      hipLaunchKernelGGL(attn_decode_bf16_kernel<128>, dim3(ns, H, B), dim3(256), shm, st, p, scratch, ns, ch);
      A3V_LAUNCH_CHECK();
      hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(H, B), dim3(128), 0, st, scratch, out, p.o_sb, p.o_sh, H, ns, dtype);
    } else {
      hipLaunchKernelGGL(attn_decode_bf16_kernel<64>, dim3(ns, H, B), dim3(256), shm, st, p, scratch, ns, ch);
      A3V_LAUNCH_CHECK();
      hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(H, B), dim3(64), 0, st, scratch, out, p.o_sb, p.o_sh, H, ns, dtype);
    }
    A3V_LAUNCH_CHECK();
    return A3V_OK;
  }
  dim3 grid(((Sq + 127) / 128) * H * B);
  if (causal && (grid.x & 7) == 0 && ((B * H) & 7) == 0) {
    // default: the largest power of two (<= 16) whose K + V^T fit ~9 MB (measured best: 16 heads at S = 1091, 8 at S ~ 2000 --
    // twice the 4-MB L2, the Infinity Cache absorbs the rest; tools/ab_attn_order.py): 160.8 -> 142.3 us at S = 1091
    const int ge = A3V_ENV_INT("A3V_ATTN_HEAD_GROUP", 0);      // > 0: forces the group size (A/B runs)
    int want = 16;
    while (want > 1 && (int64_t)want * Sk * hd * 4 > (9 << 20)) want >>= 1;
    if (ge > 0) want = ge;
    int G = want < 1 ? 1 : want;
    while (G > 1 && ((B * H) / 8) % G) G >>= 1;            // groups must not straddle an XCD's range of heads
    p.head_group = G;
  }
  if (hd == 128) {
    if (causal) hipLaunchKernelGGL((attn_prefill_bf16_kernel<128, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((attn_prefill_bf16_kernel<128, false>), grid, dim3(256), 0, st, p);
  } else {
    if (causal) hipLaunchKernelGGL((attn_prefill_bf16_kernel<64, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((attn_prefill_bf16_kernel<64, false>), grid, dim3(256), 0, st, p);
  }
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_attention(const void* q, const void* k, const void* vt, void* out, int B, int Sq, int Sk,
                             int H, int Hkv, int hd, const int64_t* strides, int causal, float* scratch,
                             int dtype, void* stream) {
  return attention_impl(q, k, vt, out, B, Sq, Sk, H, Hkv, hd, strides, causal, scratch, nullptr, dtype, stream);
}

extern "C" int a3v_attention_lse(const void* q, const void* k, const void* vt, void* out, float* lse, int B, int Sq,
                                 int Sk, int H, int Hkv, int hd, const int64_t* strides, int causal, int dtype,
                                 void* stream) {
  if (!lse) return A3V_ERR_ARG;
  return attention_impl(q, k, vt, out, B, Sq, Sk, H, Hkv, hd, strides, causal, nullptr, lse, dtype, stream);
}

// Decode attention with the split combine folded into the same launch (see attn_decode_wave_kernel); `counters` are
// B*H zero-initialised ints that the kernel leaves zero.  bf16, hd in {64, 128}.
int a3v_attention_decode_fused(const void* q, const void* k, const void* vt, void* out, int B, int Sk, int H, int Hkv, int hd,
                               const int64_t* strides, float* scratch, int* counters, void* stream) {
  if (!q || !k || !vt || !out || !strides || !scratch || !counters || B <= 0 || Sk <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (H % Hkv || (hd != 64 && hd != 128)) return A3V_ERR_SHAPE;
  AttnArgs p;
  p.q = q; p.k = k; p.vt = vt; p.out = out;
  p.q_sb = strides[0]; p.q_ss = strides[1]; p.q_sh = strides[2];
  p.k_sb = strides[3]; p.k_sh = strides[4]; p.k_ss = strides[5];
  p.v_sb = strides[6]; p.v_sh = strides[7]; p.v_sd = strides[8];
  p.o_sb = strides[9]; p.o_ss = strides[10]; p.o_sh = strides[11];
  p.B = B; p.Sq = 1; p.Sk = Sk; p.H = H; p.Hkv = Hkv;
  p.scale = 1.0f / sqrtf((float)hd);
  p.scale_log2 = p.scale * 1.4426950408889634f;
  p.lse = nullptr;
  p.head_group = 1;
  p.staged_o = 0;
  int ns2, ch2;
  a3v_decode_wave_plan(B, H, Sk, &ns2, &ch2);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ns2, H, B);
  if (hd == 128) hipLaunchKernelGGL(attn_decode_wave_kernel<128>, grid, dim3(512), 0, st, p, scratch, ns2, ch2, counters);
  else hipLaunchKernelGGL(attn_decode_wave_kernel<64>, grid, dim3(512), 0, st, p, scratch, ns2, ch2, counters);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

// The split plan as the library computes it, for callers that place key counts at its edges (tests/decode_attn_ref.py):
// wave != 0: a3v_decode_wave_plan (every wave-streaming entry); wave == 0: the two-phase plan of a3v_attention at Sq = 1.
extern "C" int a3v_attention_decode_plan(int B, int H, int Sk, int wave, int* nsplit, int* chunk) {
  if (!nsplit || !chunk || B <= 0 || H <= 0 || Sk <= 0) return A3V_ERR_ARG;
  if (wave) a3v_decode_wave_plan(B, H, Sk, nsplit, chunk);
  else decode_plan(B, H, Sk, nsplit, chunk);
  return A3V_OK;
}

// a3v_attention_decode_fused behind the checks of the other bf16 decode entries (16-byte vector access: strides and bases)
extern "C" int a3v_attention_decode_fused_bf16(const void* q, const void* k, const void* vt, void* out, int B, int Sk, int H, int Hkv,
                                               int hd, const int64_t* strides, float* scratch, int* counters, void* stream) {
  if (!q || !k || !vt || !out || !strides || !scratch || !counters || B <= 0 || Sk <= 0 || H <= 0 || Hkv <= 0) return A3V_ERR_ARG;
  if (H % Hkv || (hd != 64 && hd != 128)) return A3V_ERR_SHAPE;
  for (int i = 0; i < 12; ++i)
    if (i != 1 && i != 10 && (strides[i] % 8)) return A3V_ERR_SHAPE;      // the Sq strides are not used
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt)) & 15) return A3V_ERR_SHAPE;
  if (Sk > strides[8] || (int64_t)Sk * strides[5] > strides[4]) return A3V_ERR_SHAPE;    // a V^T row and a K head bound Sk
  return a3v_attention_decode_fused(q, k, vt, out, B, Sk, H, Hkv, hd, strides, scratch, counters, stream);
}
