// One greedy-decode step of the Llama decoder stack (seqlen == 1, llama_ens5.py:490-531 with
// mask == None) issued from ONE host call: every kernel of every layer is enqueued back to back on
// the caller's stream, so the per-kernel host cost is a C++ launch (~2-3 us) instead of a Python
// ctypes round trip -- at batch 8 the step is HBM-bound on the GPU only if the host keeps up.
//
// Fused form (dim, ffn, H*hd multiples of 128; hd in {64, 128}): FIVE launches per layer instead of ten --
//   qkv GEMV  [RMSNorm prologue | RoPE + KV-cache epilogue]      (was rmsnorm, GEMV, rope)
//   attention [split-KV, combine folded in by the last-arriving block]   (was attention, combine)
//   wo GEMV   [+residual, emits per-tile sums of squares of the new h]
//   w1|w3 GEMV [RMSNorm prologue from those sums | SwiGLU]       (was rmsnorm, GEMV)
//   w2 GEMV   [+residual, sums of squares for the next layer's prologue]
// The small kernels were ~5-7 us each of pure launch + latency: 24 of ~146 us per 7B layer.
#include "a3v_common.h"

namespace {
// sums of squares of the rows of h [B, dim] in the producer layout ([dim/16][16]) for the first layer's prologue
__global__ __launch_bounds__(256) void rows_ssq_kernel(const bf16_t* __restrict__ h, int64_t ld, int B, int dim, float* __restrict__ ssq) {
  const int t = blockIdx.x * 256 + threadIdx.x;         // (tile, m)
  const int tile = t >> 4, m = t & 15;
  if (tile * 16 >= dim) return;
  float s = 0.f;
  if (m < B) {
    const bf16_t* r = h + (int64_t)m * ld + tile * 16;
#pragma unroll
    for (int e = 0; e < 16; ++e) { const float x = (float)r[e]; s = fmaf(x, x, s); }
  }
  ssq[t] = s;
}
}  // namespace

// Which form a3v_llama_decode_step takes for a geometry, decided BEFORE anything is launched: 2 = the fused five-launch form, 1 = the
// per-kernel form (<= 16 rows, bf16 weights), 0 = not taken (A3V_ERR_SHAPE up front; the host runs its general path on untouched state).
static int decode_step_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8) {
  if (B <= 0 || B > 32) return 0;
  const int64_t ldq = (int64_t)(H + 2 * Hkv) * hd;
  const int Bc = B > 16 ? (B + 1) / 2 : B;
  const bool fused = (hd == 64 || hd == 128) && dim % 16 == 0 && dim / 16 * 16 * 4 <= A3V_WS_PARTIALS - A3V_WS_SSQ &&
                     a3v_gemv_supported(Bc, (int)ldq, dim, 0, w8) && a3v_gemv_supported(Bc, dim, H * hd, A3V_EPI_RESIDUAL, w8) &&
                     a3v_gemv_supported(Bc, 2 * ffn, dim, A3V_EPI_SWIGLU, w8) && a3v_gemv_supported(Bc, dim, ffn, A3V_EPI_RESIDUAL, w8) &&
                     ldq % 16 == 0 && (2 * ffn) % 32 == 0 && Bc * H * (int)sizeof(int) <= A3V_WS_SSQ - A3V_WS_ATTN_COUNTERS;
  if (fused) return 2;
  return (w8 || B > 16) ? 0 : 1;
}
extern "C" int a3v_llama_decode_step_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8) { return decode_step_form(B, dim, H, Hkv, hd, ffn, w8); }

// q rows of the qkv buffer, the [B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] caches and the attention output, as a3v_attention takes them
struct StepStrides {
  int64_t s[12];
  StepStrides(int64_t ldq, int H, int Hkv, int hd, int Smax)
      : s{ldq, ldq, hd,
          (int64_t)Hkv * Smax * hd, (int64_t)Smax * hd, hd,
          (int64_t)Hkv * hd * Smax, (int64_t)hd * Smax, Smax,
          (int64_t)H * hd, (int64_t)H * hd, hd} {}
};

// Layer-table check of every step entry: all four matrices of every layer in the format of layer 0's wqkv (fp8 and NF4 fields
// together are an error), images with their scales, the norm weights, and the bf16 caches where the entry reads them.
int a3v_decode_layer_table(const a3v_llama_layer* layers, int n_layers, bool need_kv, int* w8_out) {
  const int w8 = layers[0].wqkv_q != nullptr ? 1 : layers[0].wqkv_n4 != nullptr ? 2 : 0;
  for (int i = 0; i < n_layers; ++i) {
    const a3v_llama_layer& L = layers[i];
    const int q8 = (L.wqkv_q != nullptr) + (L.wo_q != nullptr) + (L.w13_q != nullptr) + (L.w2_q != nullptr);
    const int n4 = (L.wqkv_n4 != nullptr) + (L.wo_n4 != nullptr) + (L.w13_n4 != nullptr) + (L.w2_n4 != nullptr);
    if (q8 != (w8 == 1 ? 4 : 0) || (w8 == 1 && (!L.wqkv_s || !L.wo_s || !L.w13_s || !L.w2_s))) return A3V_ERR_ARG;   // all four or none
    if (n4 != (w8 == 2 ? 4 : 0) || (w8 == 2 && (!L.wqkv_n4s || !L.wo_n4s || !L.w13_n4s || !L.w2_n4s))) return A3V_ERR_ARG;
    if (!L.attn_norm_w || !L.ffn_norm_w || (need_kv && (!L.k_cache || !L.vt_cache))) return A3V_ERR_ARG;
  }
  *w8_out = w8;
  return A3V_OK;
}

// The fused layer loop of every step entry (a3v_common.h: what a stage supplies).  The GEMV kernels take up to 16 activation rows.
// Cache rows are independent through the whole stack (each has its own KV cache rows), so more rows run as row chunks through the
// same fused launches: the weights are streamed once per chunk (a 32-row batch costs two 16-row steps, i.e. the 16-row tok/s),
// every buffer is addressed at its row offset.
int a3v_decode_fused_layers(const a3v_llama_layer* layers, int n_layers, int w8, void* h, void* qkv, void* att, void* act, float* attn_scratch,
                            void* skinny_ws, int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps,
                            const a3v_decode_stage& stage, void* stream) {
  const int64_t ldq = (int64_t)(H + 2 * Hkv) * hd;
  const StepStrides strides(ldq, H, Hkv, hd, Smax);
  float* ssq = (float*)((char*)skinny_ws + A3V_WS_SSQ);
  int* actr = (int*)((char*)skinny_ws + A3V_WS_ATTN_COUNTERS);
  const bool q4 = w8 == 2;
  const int dv = q4 ? 2 : 1;                             // row stride divisor: elements of bf16, bytes of fp8 / NF4
  const bool rope = stage.cos_sin != nullptr;
  const int64_t rope_row = (int64_t)Hkv * stage.Smax * hd;   // elements per row of the cache pair the epilogue writes
  int rc;
  for (int b0 = 0; b0 < B; b0 += stage.Bc) {
    const int nbr = B - b0 < stage.Bc ? B - b0 : stage.Bc;   // cache rows of the chunk
    const int nb = nbr * stage.Q;                            // its GEMV rows
    const int64_t r0 = (int64_t)b0 * stage.Q;
    bf16_t* hc = (bf16_t*)h + r0 * dim;
    bf16_t* qc = (bf16_t*)qkv + r0 * ldq;
    bf16_t* ac = (bf16_t*)att + r0 * H * hd;
    bf16_t* fc = (bf16_t*)act + r0 * ffn;
    hipLaunchKernelGGL(rows_ssq_kernel, dim3((dim / 16 * 16 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)hc, (int64_t)dim, nb, dim, ssq);
    A3V_LAUNCH_CHECK();
    for (int i = 0; i < n_layers; ++i) {
      const a3v_llama_layer& L = layers[i];
      // per matrix: weight image and scales
      const void* wqkv = q4 ? L.wqkv_n4 : w8 ? L.wqkv_q : L.wqkv;
      const void* wo = q4 ? L.wo_n4 : w8 ? L.wo_q : L.wo;
      const void* w13 = q4 ? L.w13_n4 : w8 ? L.w13_q : L.w13;
      const void* w2 = q4 ? L.w2_n4 : w8 ? L.w2_q : L.w2;
      const float* sqkv = q4 ? L.wqkv_n4s : L.wqkv_s;
      const float* so = q4 ? L.wo_n4s : L.wo_s;
      const float* s13 = q4 ? L.w13_n4s : L.w13_s;
      const float* s2 = q4 ? L.w2_n4s : L.w2_s;
      bf16_t* kc = rope ? (bf16_t*)(stage.k ? stage.k : L.k_cache) + b0 * rope_row : nullptr;
      bf16_t* vc = rope ? (bf16_t*)(stage.vt ? stage.vt : L.vt_cache) + b0 * rope_row : nullptr;
      if ((rc = a3v_gemv_fused(hc, dim, wqkv, dim / dv, sqkv, q4, qc, ldq, nb, (int)ldq, dim, nullptr, 0, 0, L.attn_norm_w, ssq, eps, nullptr,
                               rope, stage.cos_sin, kc, vc, H, Hkv, hd, rope ? stage.Smax : Smax, rope ? stage.pos : 0, skinny_ws, stream))) return rc;
      const a3v_decode_chunk c{&L, i, b0, nbr, qc, ac, H, Hkv, hd, Smax, (int64_t)Hkv * Smax * hd, strides.s, attn_scratch, actr, stream};
      if ((rc = stage.attend(stage.ctx, c))) return rc;
      // (Smax and the position of a GEMV record are read by the RoPE epilogue alone)
      if ((rc = a3v_gemv_fused(ac, (int64_t)H * hd, wo, (int64_t)H * hd / dv, so, q4, hc, dim, nb, dim, H * hd, hc, dim, A3V_EPI_RESIDUAL,
                               nullptr, nullptr, eps, ssq, 0, nullptr, nullptr, nullptr, H, Hkv, hd, Smax, 0, skinny_ws, stream))) return rc;
      if ((rc = a3v_gemv_fused(hc, dim, w13, dim / dv, s13, q4, fc, ffn, nb, 2 * ffn, dim, nullptr, 0, A3V_EPI_SWIGLU, L.ffn_norm_w, ssq,
                               eps, nullptr, 0, nullptr, nullptr, nullptr, H, Hkv, hd, Smax, 0, skinny_ws, stream))) return rc;
      if ((rc = a3v_gemv_fused(fc, ffn, w2, ffn / dv, s2, q4, hc, dim, nb, dim, ffn, hc, dim, A3V_EPI_RESIDUAL, nullptr, nullptr, eps, ssq,
                               0, nullptr, nullptr, nullptr, H, Hkv, hd, Smax, 0, skinny_ws, stream))) return rc;
    }
  }
  return A3V_OK;
}

namespace {
// a3v_llama_decode_step: the qkv GEMV's epilogue has written position `pos` of the layer's caches; attention over pos + 1 keys
int attend_plain(const void* ctx, const a3v_decode_chunk& c) {
  const int pos = *(const int*)ctx;
  return a3v_attention_decode_fused(c.q, (bf16_t*)c.L->k_cache + c.b0 * c.kv_row, (bf16_t*)c.L->vt_cache + c.b0 * c.kv_row, c.att, c.nbr, pos + 1,
                                    c.H, c.Hkv, c.hd, c.strides, c.scratch, c.counters, c.stream);
}

// a3v_llama_decode_step_kv8: the epilogue has written the new position into the staging pair as a cache of Smax = 1 at position 0; one
// more launch quantises it into the fp8 cache at `pos` and the attention reads the fp8 cache -- SIX launches per layer.  The S = 1
// quantisation is not folded into a neighbour: the GEMV's epilogue is a3v_gemv.hip's, and inside the attention launch the blocks of
// the heads that share a kv-head would have to wait for the one that writes the row they all read back.
struct Kv8Stage { const a3v_kv8_layer* kv8; void* stage_k; void* stage_vt; int pos; };
int attend_kv8(const void* ctx, const a3v_decode_chunk& c) {
  const Kv8Stage& s = *(const Kv8Stage*)ctx;
  const a3v_kv8_layer& Q8 = s.kv8[c.layer];
  const bf16_t* kc = (const bf16_t*)s.stage_k + (int64_t)c.b0 * c.Hkv * c.hd;
  const bf16_t* vc = (const bf16_t*)s.stage_vt + (int64_t)c.b0 * c.Hkv * c.hd;
  uint8_t* kq = (uint8_t*)Q8.k_q + c.b0 * c.kv_row;
  uint8_t* vq = (uint8_t*)Q8.vt_q + c.b0 * c.kv_row;
  float* ksc = Q8.k_scale + (int64_t)c.b0 * c.Hkv * c.Smax;
  float* vsc = Q8.v_scale + (int64_t)c.b0 * c.Hkv * c.Smax;
  int rc;
  if ((rc = a3v_kv_quantize_fp8(kc, vc, 1, 0, kq, vq, ksc, vsc, c.nbr, c.Hkv, c.hd, 1, c.Smax, s.pos, c.stream))) return rc;
  return a3v_attention_decode_fp8kv(c.q, c.strides[0], kq, vq, ksc, vsc, c.att, (int64_t)c.H * c.hd, c.nbr, s.pos + 1, c.H, c.Hkv, c.hd, c.Smax,
                                    c.scratch, c.counters, c.stream);
}
}  // namespace

// The step behind a3v_llama_decode_step (kv8 == NULL: bf16 KV caches of `layers`) and a3v_llama_decode_step_kv8 (fp8 caches of `kv8`,
// fused form only).
static int decode_step_impl(const a3v_llama_layer* layers, const a3v_kv8_layer* kv8, int n_layers, void* h, void* xn, void* qkv, void* att,
                            void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, void* stage_k, void* stage_vt, int B,
                            int dim, int H, int Hkv, int hd, int ffn, int Smax, int pos, float eps, void* stream) {
  if (!layers || n_layers <= 0 || !h || !xn || !qkv || !att || !act || !attn_scratch || !skinny_ws || !cos_sin) return A3V_ERR_ARG;
  if (B <= 0 || B > 32 || pos < 0 || pos >= Smax) return A3V_ERR_SHAPE;   // the plugin contract's max_batch_size = 32 (meta.py:34-52)
  int rc, w8;
  if ((rc = a3v_decode_layer_table(layers, n_layers, kv8 == nullptr, &w8))) return rc;   // (the kv8 step does not read the bf16 caches)
  const int form = decode_step_form(B, dim, H, Hkv, hd, ffn, w8);
  if (!form) return A3V_ERR_SHAPE;                 // fp8 / NF4 images and 17..32 rows exist only in the fused form (the host takes its general path)
  const int Bc = B > 16 ? (B + 1) / 2 : B;         // 17..32 rows: two row chunks
  if (kv8) {
    if (form != 2 || Smax % 64) return A3V_ERR_SHAPE;
    if (!stage_k || !stage_vt) return A3V_ERR_ARG;
    for (int i = 0; i < n_layers; ++i)
      if (!kv8[i].k_q || !kv8[i].vt_q || !kv8[i].k_scale || !kv8[i].v_scale) return A3V_ERR_ARG;
    // (the epilogue has ONE position for angle and cache row: row `pos` of the table is handed in as row 0)
    const Kv8Stage ctx{kv8, stage_k, stage_vt, pos};
    const a3v_decode_stage stage{Bc, 1, cos_sin + (int64_t)pos * hd, stage_k, stage_vt, 1, 0, attend_kv8, &ctx};
    return a3v_decode_fused_layers(layers, n_layers, w8, h, qkv, att, act, attn_scratch, skinny_ws, B, dim, H, Hkv, hd, ffn, Smax, eps, stage, stream);
  }
  if (form == 2) {
    const a3v_decode_stage stage{Bc, 1, cos_sin, nullptr, nullptr, Smax, pos, attend_plain, &pos};
    return a3v_decode_fused_layers(layers, n_layers, w8, h, qkv, att, act, attn_scratch, skinny_ws, B, dim, H, Hkv, hd, ffn, Smax, eps, stage, stream);
  }
  const int64_t ldq = (int64_t)(H + 2 * Hkv) * hd;
  const StepStrides strides(ldq, H, Hkv, hd, Smax);
  for (int i = 0; i < n_layers; ++i) {
    const a3v_llama_layer& L = layers[i];
    if ((rc = a3v_rmsnorm(h, dim, L.attn_norm_w, xn, dim, B, dim, eps, A3V_BF16, A3V_BF16, A3V_BF16, stream))) return rc;
    if ((rc = a3v_gemm_skinny(xn, dim, L.wqkv, dim, qkv, ldq, B, (int)ldq, dim, nullptr, 0, 0, skinny_ws, stream))) return rc;
    if ((rc = a3v_rope_kvcache(qkv, ldq, qkv, ldq, L.k_cache, L.vt_cache, cos_sin, B, 1, H, Hkv, hd, Smax, pos, pos, A3V_BF16, stream))) return rc;
    if ((rc = a3v_attention(qkv, L.k_cache, L.vt_cache, att, B, 1, pos + 1, H, Hkv, hd, strides.s, 0, attn_scratch, A3V_BF16, stream))) return rc;
    if ((rc = a3v_gemm_skinny(att, (int64_t)H * hd, L.wo, (int64_t)H * hd, h, dim, B, dim, H * hd, h, dim, A3V_EPI_RESIDUAL, skinny_ws, stream))) return rc;
    if ((rc = a3v_rmsnorm(h, dim, L.ffn_norm_w, xn, dim, B, dim, eps, A3V_BF16, A3V_BF16, A3V_BF16, stream))) return rc;
    if ((rc = a3v_gemm_skinny(xn, dim, L.w13, dim, act, ffn, B, 2 * ffn, dim, nullptr, 0, A3V_EPI_SWIGLU, skinny_ws, stream))) return rc;
    if ((rc = a3v_gemm_skinny(act, ffn, L.w2, ffn, h, dim, B, dim, ffn, h, dim, A3V_EPI_RESIDUAL, skinny_ws, stream))) return rc;
  }
  return A3V_OK;
}

extern "C" int a3v_llama_decode_step(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att,
                                     void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, int B, int dim, int H, int Hkv,
                                     int hd, int ffn, int Smax, int pos, float eps, void* stream) {
  return decode_step_impl(layers, nullptr, n_layers, h, xn, qkv, att, act, attn_scratch, skinny_ws, cos_sin, nullptr, nullptr, B, dim, H, Hkv,
                          hd, ffn, Smax, pos, eps, stream);
}

extern "C" int a3v_llama_decode_step_kv8(const a3v_llama_layer* layers, const a3v_kv8_layer* kv8, int n_layers, void* h, void* xn, void* qkv,
                                         void* att, void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, void* stage_k,
                                         void* stage_vt, int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, int pos, float eps,
                                         void* stream) {
  if (!kv8) return A3V_ERR_ARG;
  return decode_step_impl(layers, kv8, n_layers, h, xn, qkv, att, act, attn_scratch, skinny_ws, cos_sin, stage_k, stage_vt, B, dim, H, Hkv, hd,
                          ffn, Smax, pos, eps, stream);
}
