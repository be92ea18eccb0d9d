// Shared device helpers for the gfx950 kernels (wave64, MFMA, bf16 <-> f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3vlm_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define A3V_WAVE 64

// ---- A3V_* environment switches (A/B runs, tuning scripts and equality tests; the defaults are the product path and none of
// them selects a CPU path).  A switch is read ONCE per call site and cached: no launch calls getenv in steady state.  A process
// that flips a switch after the first launch calls a3v_reload_env() (C-ABI; a3vlm_amd.lib.env(...) does it) to have them re-read.
int a3v_env_generation();
#include <stdlib.h>
#define A3V_ENV_INT(name, dflt)                                                        \
  ([]() -> int {                                                                       \
    static int gen_ = -1, v_ = 0;                                                      \
    const int g_ = a3v_env_generation();                                               \
    if (gen_ != g_) { const char* e_ = getenv(name); v_ = e_ ? atoi(e_) : (dflt); gen_ = g_; } \
    return v_;                                                                         \
  }())

__device__ __forceinline__ float bf2f(bf16_t v) { return (float)v; }
__device__ __forceinline__ bf16_t f2bf(float v) { return (bf16_t)v; }  // RNE (v_cvt_pk_bf16_f32)
// d(gate), d(up) of act = silu(gate) * up for one element (a3v_swiglu_bwd and the A3V_EPI_SWIGLU_BWD GEMM epilogue share this
// expression so that the fused and the un-fused path round identically)
__device__ __forceinline__ void swiglu_bwd_pair(float g, float u, float da, float& dg, float& du) {
  const float sig = 1.f / (1.f + __expf(-g));
  dg = da * u * (sig * (1.f + g * (1.f - sig)));
  du = da * (g * sig);
}
// x * sigmoid(x) with v_rcp_f32 (1 ulp) instead of the IEEE division sequence: the SwiGLU epilogues of the GEMMs and of the decode GEMVs
__device__ __forceinline__ float silu(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
// round-trip: the value a bf16 store of v would hold
__device__ __forceinline__ float rbf(float v) { return (float)((bf16_t)v); }

// bitsandbytes' NF4 code book (16 entries, 0 at index 7): one table for the quantiser, the dequantisers and the LoRA merge over an NF4 base
__device__ __forceinline__ float nf4_value(int i) {
  constexpr float t[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
                           -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
                           0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f,
                           1.0f};
  return t[i];
}

// One element of the AdamW update (torch.optim.AdamW, decoupled weight decay; the host scalars are derived in a3v_adamw_scaled):
//   p *= 1 - lr*wd;  m += (1-b1)(g - m);  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// adamw_kernel (a3v_train.hip, fp32 moments) and adamw8_kernel (a3v_adam8.hip, e4m3 moments) share these statements, so both are
// contracted into the same fma sequence and the 8-bit step equals dequantise -> a3v_adamw_scaled -> quantise bit for bit.
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, float decay, float b1, float b2, float step_size,
                                             float inv_bc2_sqrt, float eps) {
  p *= decay;
  m += (1.f - b1) * (g - m);
  v = b2 * v + (1.f - b2) * g * g;
  p -= step_size * m / (sqrtf(v) * inv_bc2_sqrt + eps);
}

// The clip coefficient that makes an AdamW step a no-op: NaN or sign bit set (negative, and -0.0 with them: the sign is the flag)
__device__ __forceinline__ bool adamw_skip(float gs) { return !(gs >= 0.f) || (__float_as_uint(gs) >> 31); }

template <typename T> struct Cvt;
template <> struct Cvt<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
  static __device__ __forceinline__ float rnd(float v) { return v; }
};
template <> struct Cvt<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return (float)*p; }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = (bf16_t)v; }
  static __device__ __forceinline__ float rnd(float v) { return rbf(v); }
};

// 8 contiguous elements <-> 8 floats
__device__ __forceinline__ void load8(const bf16_t* p, float* o) {
  bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
}
__device__ __forceinline__ void load8(const float* p, float* o) {
  f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}
// non-temporal forms for streams that are touched once (NT is a compile-time flag of the calling kernel)
template <bool NT>
__device__ __forceinline__ void load8_s(const bf16_t* p, float* o) {
  const bf16x8 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p)) : *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
}
template <bool NT>
__device__ __forceinline__ void load8_s(const float* p, float* o) {
  const f32x4 a = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)) : *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4)) : *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}
template <bool NT>
__device__ __forceinline__ void store8_s(bf16_t* p, const float* v) {
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (bf16_t)v[i];
  if (NT) __builtin_nontemporal_store(o, reinterpret_cast<bf16x8*>(p)); else *reinterpret_cast<bf16x8*>(p) = o;
}
template <bool NT>
__device__ __forceinline__ void store8_s(float* p, const float* v) {
  f32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[4 + i]; }
  if (NT) { __builtin_nontemporal_store(a, reinterpret_cast<f32x4*>(p)); __builtin_nontemporal_store(b, reinterpret_cast<f32x4*>(p + 4)); }
  else { *reinterpret_cast<f32x4*>(p) = a; *reinterpret_cast<f32x4*>(p + 4) = b; }
}
__device__ __forceinline__ void store8(bf16_t* p, const float* v) {
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (bf16_t)v[i];
  *reinterpret_cast<bf16x8*>(p) = o;
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  f32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[4 + i]; }
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}

// Wave-wide butterfly reductions WITHOUT the LDS pipe (round 4).  __shfl_xor compiles to ds_bpermute_b32: six LDS round trips of ~100+
// cycles each per reduction, in front of every row's second pass and in the prologue of every decode GEMV.  The same butterfly
// (partner lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 in this order -- the same pairs, hence the same bits as the __shfl_xor form) on the VALU:
//   ^ 32 / ^ 16 : v_permlane32_swap / v_permlane16_swap (asm: with one value in both operands of the builtins hipcc keeps ONE of the
//                 two results for both and the exchange disappears);
//   ^ 8  / ^ 4  : DPP row_ror:8 / row_ror:4 (after the ^ 8 level the lanes i and i ^ 8 of a row hold the same value, so lane i + 4
//                 mod 16 holds what lane i ^ 4 holds);   ^ 2 / ^ 1 : DPP quad_perm [2,3,0,1] / [1,0,3,2].
__device__ __forceinline__ void lane_xchg32(float x, float& a, float& b) {
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void lane_xchg16(float x, float& a, float& b) {
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
#ifdef A3V_WAVE_SHFL      // A/B builds: the __shfl_xor (ds_bpermute) forms of rounds 1-3
#define wave_sum wave_sum_shfl
#define wave_max wave_max_shfl
#else
__device__ __forceinline__ float wave_sum(float v) {
  float a, b;
  lane_xchg32(v, a, b); v = a + b;
  lane_xchg16(v, a, b); v = a + b;
  v += dpp_f<0x128>(v);
  v += dpp_f<0x124>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0xB1>(v);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  float a, b;
  lane_xchg32(v, a, b); v = fmaxf(a, b);
  lane_xchg16(v, a, b); v = fmaxf(a, b);
  v = fmaxf(v, dpp_f<0x128>(v));
  v = fmaxf(v, dpp_f<0x124>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0xB1>(v));
  return v;
}
#endif
// (the LDS-pipe forms, kept for the equality test of the two: a3v_probe_wave_reduce)
__device__ __forceinline__ float wave_sum_shfl(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max_shfl(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide sum for blockDim.x = NT (multiple of 64); red: NT/64 floats of LDS
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if (NT == 64) return v;
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t += red[i];
  return t;
}

// Opt a kernel into more than 64 KiB of dynamic LDS ONCE PER DEVICE (the attribute is per device; a process-wide "done" flag left a
// second GPU of the process without it: launch failure).  `done`: a per-call-site table [A3V_MAX_DEV][slots]; the set is idempotent, so
// two host threads racing through the flag at worst both make the call.  Returns the hipError_t of the set (0 = fine).
constexpr int A3V_MAX_DEV = 16;
template <int SLOTS>
inline int a3v_dyn_lds_once(bool (&done)[A3V_MAX_DEV][SLOTS], int slot, const void* kern, int bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= A3V_MAX_DEV) dev = 0, done[0][slot] = false;
  if (done[dev][slot]) return 0;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return (int)e;
  done[dev][slot] = true;
  return 0;
}

#define A3V_LAUNCH_CHECK()                         \
  do {                                             \
    hipError_t e_ = hipGetLastError();             \
    if (e_ != hipSuccess) return (int)e_;          \
  } while (0)

// Agent-coherent (sc0 sc1) scalar accesses for in-kernel hand-offs between workgroups that may sit on different XCDs
// (L2 is per XCD): the store is written through, the load bypasses stale lines; no cache-wide write-back / invalidate.
// ld_agent_issue only ISSUES the load: the caller must `s_waitcnt vmcnt(0)` (agent_wait) before using the value.
__device__ __forceinline__ void st_agent(float* p, float v) { asm volatile("global_store_dword %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ float ld_agent_issue(const float* p) {
  float v;
  asm volatile("global_load_dword %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void agent_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ float ld_agent(const float* p) {          // issue + wait (the value is tied to the wait)
  float v = ld_agent_issue(p);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)::"memory");
  return v;
}

// Fused combine of the wave-streaming decode kernels (a3v_attn.hip, a3v_kv8.hip; all threads of the block call it; `po` = this block's partial, already written with plain stores)
template <int HD>
__device__ __forceinline__ void decode_combine_tail(void* out, int64_t o_sb, int64_t o_sh, int H, float* part, float* po, int nsplit, int* counters, int b, int h, int tid) {
  // Fused combine (decode step): the block that arrives last at the (batch, head) counter merges the nsplit partials.
  // The splits of a head may run on different XCDs (private L2s), so the hand-off uses agent-coherent accesses: this
  // block re-writes its HD+2 partial values with sc0 sc1 stores (write-through), waits for the acknowledgement, bumps
  // the counter; the last block reads all partials with sc0 sc1 loads.  (An agent-scope fence instead = L2 write-back
  // + invalidate per wave: measured 5x slower on the GEMV that uses the same scheme.)
  __shared__ int last_s;
  __syncthreads();                                    // po[] of this block is complete (plain stores, same CU)
  if (tid < HD + 2) st_agent(po + tid, po[tid]);      // L1 is write-through: the value read back is this block's own
  agent_wait();
  __syncthreads();
  if (tid == 0) {
    int* ctr = counters + b * H + h;
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = old == nsplit - 1;
    if (old == nsplit - 1) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last_s || tid >= HD) return;
  const float* pp = part + (int64_t)(b * H + h) * nsplit * (HD + 2);
  float acc = 0.f, l = 0.f;
  if (nsplit <= 8) {                                  // all loads in flight at once: one memory round trip
    float mv[8], av[8], lv[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float* q = pp + (s < nsplit ? s : nsplit - 1) * (HD + 2);
      mv[s] = ld_agent_issue(q + HD);
      av[s] = ld_agent_issue(q + tid);
      lv[s] = ld_agent_issue(q + HD + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(mv[0]), "+v"(mv[1]), "+v"(mv[2]), "+v"(mv[3]), "+v"(mv[4]), "+v"(mv[5]), "+v"(mv[6]), "+v"(mv[7])::"memory");
    asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]), "+v"(av[6]), "+v"(av[7]));
    asm volatile("" : "+v"(lv[0]), "+v"(lv[1]), "+v"(lv[2]), "+v"(lv[3]), "+v"(lv[4]), "+v"(lv[5]), "+v"(lv[6]), "+v"(lv[7]));
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < 8; ++s) if (s < nsplit) m = fmaxf(m, mv[s]);
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (s < nsplit) {
        const float w = (mv[s] == -INFINITY) ? 0.f : __expf(mv[s] - m);
        acc += w * av[s];
        l += w * lv[s];
      }
  } else {
    float m = -INFINITY;
    for (int s = 0; s < nsplit; ++s) m = fmaxf(m, ld_agent(pp + s * (HD + 2) + HD));
    for (int s = 0; s < nsplit; ++s) {
      const float ms = ld_agent(pp + s * (HD + 2) + HD);
      const float a1 = ld_agent(pp + s * (HD + 2) + tid);
      const float l1 = ld_agent(pp + s * (HD + 2) + HD + 1);
      const float w = (ms == -INFINITY) ? 0.f : __expf(ms - m);
      acc += w * a1;
      l += w * l1;
    }
  }
  ((bf16_t*)out)[b * o_sb + h * o_sh + tid] = f2bf(acc / l);
}

// Layout of the decode workspace (a3v_gemm_skinny `partial` / a3v_llama_decode_step `skinny_ws`): zero-filled once by the
// caller; every kernel leaves the counter areas zero.
//   [0, 16 KB)      GEMV split-K arrival counters (one per 16-row tile, N <= 65536)
//   [16 KB, 32 KB)  decode-attention arrival counters (one per (batch, head))
//   [32 KB, 64 KB)  per-tile sums of squares of the residual rows (RMSNorm fused into the consuming GEMV): dim / 16 tiles x 16 rows x 4 B,
//                   i.e. dim <= 8192 (round 4: was 16 KB = dim <= 4096, which kept the 13B geometry, dim 5120, out of the fused decode step)
//   [64 KB, ...)    split-K partial accumulators
constexpr int A3V_WS_ATTN_COUNTERS = 16384;
constexpr int A3V_WS_SSQ = 32768;
constexpr int A3V_WS_PARTIALS = 65536;
// (a3v_gemv_fused, the decode step's GEMV building block, is declared with its contract in include/a3vlm_hip.h)
bool a3v_gemv_supported(int M, int N, int K, int epilogue, int w8);
// compute units of the current device rounded down to whole XCD rounds (a3v_gemm.hip; 256 without a device): the GEMM and GEMV planners' `cus`
int a3v_cu_count();
int a3v_attention_decode_fused(const void* q, const void* k, const void* vt, void* out, int B, int Sk, int H, int Hkv, int hd,
                               const int64_t* strides, float* scratch, int* counters, void* stream);
// the split plan of every wave-streaming decode attention (a3v_attn.hip): the launches and the exported *_splits / *_scratch_floats
void a3v_decode_wave_plan(int B, int H, int Sk, int* nsplit, int* chunk);

// ---- The fused decode step's one layer loop (a3v_decode.hip), shared by a3v_llama_decode_step[_kv8 | _rows | _rows_shared | _verify].
// An entry checks its own arguments, calls a3v_decode_layer_table, takes its _form decision, and hands a3v_decode_fused_layers a
// stage: the rows of a chunk, whether the qkv GEMV carries the RoPE + cache epilogue, and the launches between it and the wo GEMV.
struct a3v_decode_chunk {            // one (row chunk, layer), as the loop hands it to the stage's attend()
  const a3v_llama_layer* L;
  int layer, b0, nbr;                // layer index; first cache row of the chunk and its cache rows
  bf16_t* q; bf16_t* att;            // the chunk's GEMV rows of the qkv buffer (row stride (H + 2 Hkv) hd) and of the attention output
  int H, Hkv, hd, Smax;
  int64_t kv_row;                    // elements per cache row of a bf16 K / V^T cache: the chunk's rows start at b0 * kv_row
  const int64_t* strides;            // [12] of q / caches / att at this geometry, as a3v_attention takes them
  float* scratch; int* counters; void* stream;
};
struct a3v_decode_stage {
  int Bc, Q;                         // cache rows per chunk and queries per cache row: a chunk is nbr * Q <= 16 GEMV rows
  // The qkv GEMV's RoPE + cache epilogue (cos_sin == NULL: plain store, the stage rotates and writes the cache itself): the table
  // row of the position, the cache pair [B, Hkv, Smax, hd] / [B, Hkv, hd, Smax] (NULL: the layer's own), its Smax and the position.
  const float* cos_sin; void* k; void* vt; int Smax, pos;
  int (*attend)(const void* ctx, const a3v_decode_chunk& c);   // every launch between the qkv GEMV and the wo GEMV
  const void* ctx;
};
// every layer in one weight format, images with their scales, norm weights, and (need_kv) the bf16 caches: A3V_OK and
// *w8 = 0 bf16 / 1 fp8 images / 2 NF4 images, else A3V_ERR_ARG
int a3v_decode_layer_table(const a3v_llama_layer* layers, int n_layers, bool need_kv, int* w8);
// the loop; the caller has decided the fused form for (stage.Bc * stage.Q rows, w8).  Nothing here refuses before the first launch.
int a3v_decode_fused_layers(const a3v_llama_layer* layers, int n_layers, int w8, void* h, void* qkv, void* att, void* act, float* attn_scratch,
                            void* skinny_ws, int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps,
                            const a3v_decode_stage& stage, void* stream);
// internal (a3v_train.hip): bf16 transposes of n_out x n_in matrices [R, C] -> [C, Rpad] in one launch
int a3v_transpose_2level(const bf16_t* src, int64_t ld_src, int64_t bs_in, int64_t bs_out, bf16_t* dst, int64_t ld_dst, int64_t bsd_in,
                         int64_t bsd_out, int R, int C, int Rpad, int n_in, int n_out, void* stream);

// ---------------------------------------------------------------- mass selection of the device samplers
// (a3v_rowops.hip: a3v_sample_top_p, where the algorithm is described; a3v_sampler.hip: a3v_sample_top_k_p.  One block = one row.)
struct TopPSel { unsigned key; float above; int rank; int id; };

// CACHE 1 (true): e_i is read from the LDS copy ec[V]; 0 (false): recomputed from the row.  2 (a3v_sampler.hip above the cache's
// size): recomputed where the token's bit in the keep bitmap (`ec` reinterpreted, bit i of 32-bit word i / 32) is set, else the
// negative value every pass skips.  The first two forms are a3v_sample_top_p's, unchanged.
template <int CACHE>
__device__ __forceinline__ float topp_e(const float* __restrict__ r, const float* __restrict__ ec, int i, float T, float xm) {
  if constexpr (CACHE == 1) return ec[i];
  else if constexpr (CACHE == 2) return ((reinterpret_cast<const unsigned*>(ec)[i >> 5] >> (i & 31)) & 1u) ? expf(r[i] / T - xm) : -1.f;
  else return expf(r[i] / T - xm);
}

// shared scratch of the selection (one block = one row)
struct TopPShared {
  float hist[16][256];        // per-wave mass histograms of the current digit
  float bin[256];
  float bin_top[256];         // the first digit's merged histogram: the same for both selections of a row (taken once)
  unsigned long long ball[64][16];   // tie ballots per (iteration, wave) of the last pass
  int wcnt[64][16];
  float red[16];
  unsigned ured[2][16];
  unsigned sel_key; float sel_above; int sel_bin; int found;
  int tie_n;
};

// target in units of Z.  want_id: also locate the token (selection 2); else only (key, above, rank) are needed (selection 1).
// kmin / levels / lsh: keys are ranked as (bits(e) - kmin) << lsh -- the left shift puts the range's top bit on the top bit of the
// first of `levels` 8-bit digits (0 levels: every element has the same value), so the first histogram already spreads over 128+ bins.
template <int CACHE>
__device__ void topp_select(const float* __restrict__ r, const float* __restrict__ ec, int V, float T, float xm, unsigned kmin, int levels, int lsh,
                            float target, bool want_id, bool reuse_top, TopPShared& sh, TopPSel& out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned prefix = 0;
  float above = 0.f;
  bool all_kept = false;
  for (int level = levels - 1; level >= 0; --level) {
    const int shift = level * 8;
    if (level == levels - 1 && reuse_top) {               // selection 2: the first digit's histogram of selection 1
      if (tid < 256) sh.bin[tid] = sh.bin_top[tid];
      if (tid == 0) sh.found = -1;
      __syncthreads();
    } else {
    for (int b = tid; b < 16 * 256; b += 1024) (&sh.hist[0][0])[b] = 0.f;
    __syncthreads();
    // four elements per trip: the reads (LDS or expf) of a trip are in flight together; the adds keep the element order of the plain loop
    for (int i0 = tid; i0 < V; i0 += 4096) {
      float e4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * 1024;
        e4[q] = i < V ? topp_e<CACHE>(r, ec, i, T, xm) : -1.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned k = (__float_as_uint(e4[q]) - kmin) << lsh;
        if (e4[q] >= 0.f && (level == levels - 1 || (k >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&sh.hist[wave][(k >> shift) & 255], e4[q]);
      }
    }
    __syncthreads();
    if (tid < 256) {
      float m = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) m += sh.hist[w][tid];
      sh.bin[tid] = m;
      if (level == levels - 1) sh.bin_top[tid] = m;
    }
    if (tid == 0) sh.found = -1;
    __syncthreads();
    }
    if (wave == 0) {
      // lane l owns bins 4 l .. 4 l + 3; suffix sums from bin 255 down
      float b4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) b4[q] = sh.bin[lane * 4 + q];
      const float own = (b4[0] + b4[1]) + (b4[2] + b4[3]);
      float suf = own;                                   // inclusive suffix over lanes >= l
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float v = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += v;
      }
      const float nxt = __shfl_down(suf, 1, 64);
      float excl = above + (lane < 63 ? nxt : 0.f);      // mass of everything ranked before bin 4 l + 3
      int hi = -1, lo = 0x7fffffff;                      // highest bin whose inclusive mass passes the target / lowest non-empty bin
      float hi_excl = 0.f, lo_excl = 0.f;
#pragma unroll
      for (int q = 3; q >= 0; --q) {
        const float incl = excl + b4[q];
        if (b4[q] > 0.f) {
          if (hi < 0 && incl > target) { hi = lane * 4 + q; hi_excl = excl; }
          lo = lane * 4 + q; lo_excl = excl;
        }
        excl = incl;
      }
      int best_hi = hi, best_lo = lo;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        best_hi = max(best_hi, __shfl_xor(best_hi, o, 64));
        best_lo = min(best_lo, __shfl_xor(best_lo, o, 64));
      }
      // no bin passes: at the top level the target is beyond the total mass (cut: nothing is cut; draw: clamp onto the last
      // token); below it, the sub-bins' sum fell an ulp short of their parent's -- take the last non-empty one
      const bool clamp_lo = best_hi < 0 && (level < levels - 1 || want_id) && best_lo != 0x7fffffff;
      if (best_hi >= 0 && best_hi == hi) { sh.found = hi; sh.sel_above = hi_excl; }
      if (clamp_lo && best_lo == lo) { sh.found = lo; sh.sel_above = lo_excl; }
    }
    __syncthreads();
    if (sh.found < 0) { all_kept = true; break; }        // target >= total mass: nothing is cut (top_p >= 1)
    prefix |= (unsigned)sh.found << shift;
    above = sh.sel_above;
    __syncthreads();
  }
  if (all_kept) { out.key = 0u; out.above = -1.f; out.rank = 0; out.id = -1; return; }
  const unsigned key = (prefix >> lsh) + kmin;           // (levels == 0: every element equals the smallest key)
  const float ek = __uint_as_float(key);
  // ties on the selected value: rank inside them by token index
  int rank = ek > 0.f ? (int)floorf((target - above) / ek) : 0;
  if (rank < 0) rank = 0;
  out.key = key; out.above = above; out.rank = rank; out.id = -1;
  const int iters = (V + 1023) / 1024;
  for (int k = 0; k < iters; ++k) {
    const int i = k * 1024 + tid;
    const bool tie = i < V && __float_as_uint(topp_e<CACHE>(r, ec, i, T, xm)) == key;
    const unsigned long long bl = __ballot(tie);
    if (lane == 0) { sh.ball[k][wave] = bl; sh.wcnt[k][wave] = __popcll(bl); }
  }
  __syncthreads();
  // (k, w) slots in token order = flat index t = k * 16 + w; thread t holds slot t's count: total and the slot the rank falls into by a
  // block-wide scan over the <= 1024 slots (was: one thread walking 512 LDS words twice, ~10 us per selection)
  {
    const int c = tid < iters * 16 ? (&sh.wcnt[0][0])[tid] : 0;
    int incl = c;                                        // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) sh.ured[0][wave] = (unsigned)incl;
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int t = (int)sh.ured[0][w];
      if (w < wave) base += t;
      n += t;
    }
    if (rank >= n) rank = n - 1;                         // float division landed past the last tied element
    if (tid == 0) { sh.tie_n = rank; sh.sel_bin = -1; }
    __syncthreads();
    const int before = base + incl - c;                  // ties in earlier slots
    if (want_id && c > 0 && rank >= before && rank < before + c) {
      unsigned long long bl = (&sh.ball[0][0])[tid];
      for (int q = 0; q < rank - before; ++q) bl &= bl - 1;   // drop the lowest set bits
      sh.sel_bin = (tid >> 4) * 1024 + (tid & 15) * 64 + __ffsll((long long)bl) - 1;
    }
  }
  __syncthreads();
  out.rank = sh.tie_n;
  out.id = sh.sel_bin;
  __syncthreads();
}
