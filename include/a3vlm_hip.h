/*
 * a3vlm_hip.h -- C ABI of liba3vlm_hip.so: the MI355X (gfx950 / CDNA4) kernels of the
 * A3VLM multimodal hot path (ViT patch-embed + encoder -> projector -> Llama decoder
 * -> LM head / CE / greedy decode; opt-in: NF4 / fp8 weights, fp8 KV cache, ragged decode with one cache position per batch row).
 *
 * The reference (changhaonan/A3VLM) is pure Python on PyTorch and has no FFI of its
 * own: its "native" layer is whatever ATen/cuBLAS/flash-attn kernel each torch call
 * reaches.  Each entry point below therefore cites the
 * reference call site (path:line under model/accessory/) whose arithmetic it
 * replaces.  The reference-side binding is a ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless noted.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are
 *    enqueued asynchronously on it and never synchronise.
 *  - never allocates; scratch is passed in by the caller.
 *  - re-entrant from any host thread.  The only process-wide state is (i) the table of scratch registrations of
 *    a3v_gemm_set_workspace_for (mutex-protected, keyed by device and stream: two streams never share split-K planes) and (ii) the
 *    cached values of the A3V_* environment switches (A/B runs only; a3v_reload_env re-reads them).  No kernel result depends on
 *    state left by an earlier call on another stream.
 *  - return value: 0 on success, a hipError_t (>0) from the launch, or a negative
 *    A3V_ERR_* for argument errors.  The Python host raises RuntimeError on != 0.
 *  - dtype codes: A3V_BF16 activations/weights are bfloat16 with fp32 accumulation
 *    (the throughput path); A3V_F32 is the fp32 parity path (same op order).
 *  - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef A3VLM_HIP_H
#define A3VLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { A3V_BF16 = 0, A3V_F32 = 1 };

enum {
  A3V_OK = 0,
  A3V_ERR_SHAPE = -1,   /* unsupported size / alignment */
  A3V_ERR_DTYPE = -2,
  A3V_ERR_ARG = -3
};

/* GEMM epilogue flags (bit-or) */
enum {
  A3V_EPI_NONE = 0,
  A3V_EPI_BIAS = 1,        /* + bias[n]                                             */
  A3V_EPI_GELU = 2,        /* erf GELU   (open_clip mlp)          */
  A3V_EPI_QUICKGELU = 4,   /* x*sigmoid(1.702x) (open_clip 'openai' pretrained cfg)  */
  A3V_EPI_RESIDUAL = 8,    /* out = residual + y  (LLM/llama_ens5.py:238,241)        */
  A3V_EPI_SWIGLU = 16,     /* W rows interleaved [w1 blk16 | w3 blk16]: out[:, N/2] =
                              silu(x w1^T) * (x w3^T)   (LLM/llama_ens5.py:213-217)   */
  A3V_EPI_OUT_F32 = 32,    /* store fp32 (logits .float(), LLM/llama_ens5.py:531)     */
  A3V_EPI_RES_F32 = 64,    /* residual stream (and output) kept in fp32 (training
                              under autocast: engine_finetune.py:44-50)               */
  A3V_EPI_SWIGLU_BWD = 128, /* the GEMM's [M, N] product is d(act) of the SwiGLU (the input gradient of w2, llama_ens5.py:213-217
                               backward): `residual` = gu [M, 2N] bf16 (gate columns 0..N-1, up columns N..2N-1, as the forward's
                               un-fused w1|w3 output keeps them), C [M, >= 2N] bf16 receives d(gate) in columns 0..N-1 and d(up)
                               in N..2N-1 -- a3v_swiglu_bwd applied to the bf16-rounded product, bit for bit, without the
                               d(act) round trip through HBM.  bf16 only; N % 8 == 0.                                   */
  A3V_EPI_TILE_128 = 1 << 16,  /* force the 128x128 tile kernel (tuning / tests)       */
  A3V_EPI_TILE_256 = 1 << 17,  /* force the 256x256 tile kernel (tuning / tests)       */
  A3V_EPI_TILE_256PP = 1 << 18,/* force the 256x256 ping-pong kernel (tuning / tests)  */
  /* 1 << 19: retired (was a tuning switch): A3V_ERR_ARG                              */
  A3V_EPI_TILE_192PP = 1 << 23  /* force the ring kernel's 192 x 256 tile form (round 5; tuning / tests) */
};

int a3v_version(void);

/* A3V_* environment switches (A/B runs, tuning scripts, equality tests) are read once per call site and
 * cached: a process that changes one after its first launch calls this to have them re-read.  Returns the new generation.
 * (No reference counterpart: the reference has no native code.) */
int a3v_reload_env(void);
/* C[M,N] = epilogue(A[M,K] @ W[N,K]^T).  Replaces every F.linear on the path:
 * wq/wk/wv/wo (LLM/llama_ens5.py:63-90,112,169), w1/w2/w3 (:202-217), output (:267-269,
 * 486,530), visual_proj[0] (:330-333), the open_clip in_proj/out_proj/c_fc/c_proj, and
 * conv1 as an im2col GEMM (:354).  bf16: K % 64 == 0, lda/ldw % 8 == 0, N % 4 == 0.
 * With A3V_EPI_SWIGLU, N counts the interleaved rows (2*ffn) and C has N/2 columns. */
int a3v_gemm_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                int M, int N, int K, const void* bias, const void* residual, int64_t ldr,
                int epilogue, int dtype, void* stream);

/* Prefill qkv projection with the rotary embedding and the KV-cache write in the GEMM epilogue (LLM/llama_ens5.py:155-176:
 * xq, xk, xv = wq(x), wk(x), wv(x); apply_rotary_emb; cache_k/cache_v[:bsz, start_pos:start_pos+seqlen] = xk/xv) --
 * a3v_gemm_nt on the fused [(H+2Hkv)*hd, K] weight followed by a3v_rope_kvcache, value for value (the accumulator is rounded
 * to the bf16 activation before the rotation), minus one HBM round trip of the [B*S, (H+2Hkv)*hd] activation.
 * A [B*S, K] bf16; q_out [B*S, ldq] receives the rotated q in columns 0..H*hd; caches as a3v_rope_kvcache; hd 64 or 128.
 * v_rows (optional, [B*S, ldv]): v also stored token-major, the layout the attention backward reads (training forward).
 * delta (optional, bf16 [B*S, ldd]): an additive term of the projection -- the LoRA branch lora_b(lora_a(x)) of model/peft.py:89-95
 * -- added to the bf16 linear output (and rounded, as the reference does) before the rotation; may alias v_rows' buffer. */
int a3v_gemm_qkv_rope(const void* A, int64_t lda, const void* W, int64_t ldw, int K, void* q_out, int64_t ldq,
                      void* k_cache, void* vt_cache, void* v_rows, int64_t ldv, const void* delta, int64_t ldd,
                      const float* cos_sin, int B, int S, int H, int Hkv, int hd, int Smax, int start_pos, int rope_pos0,
                      void* stream);

/* fp8 (OCP e4m3fn) W8A8 prefill GEMM (BASELINE config 5 "quantised inference"; the reference's quantised path is bitsandbytes
 * NF4/INT8, util/quant.py:95-163, so there is no reference oracle: parity is stated against the exact product of the
 * dequantised operands): C = epilogue((Aq . Wq^T) * sa[m] * sw[n]) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales.
 * Aq [M, K] / Wq [N, K] fp8 bytes (lda, ldw % 16 == 0, K % 128 == 0), sa [M] / sw [N] fp32 per-row scales; C bf16 (or fp32 with
 * OUT_F32 / RES_F32); epilogues BIAS / GELU / QUICKGELU / RESIDUAL / SWIGLU / OUT_F32 / RES_F32 as a3v_gemm_nt. */
int a3v_gemm_nt_fp8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, void* C,
                    int64_t ldc, int M, int N, int K, const void* bias, const void* residual, int64_t ldr, int epilogue,
                    void* stream);
/* a3v_gemm_qkv_rope with fp8 operands. */
int a3v_gemm_qkv_rope_fp8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, int K,
                          void* q_out, int64_t ldq, void* k_cache, void* vt_cache, const float* cos_sin, int B, int S,
                          int H, int Hkv, int hd, int Smax, int start_pos, int rope_pos0, void* stream);
/* Dynamic per-row activation quantisation for a3v_gemm_nt_fp8: scales[r] = max|y[r,:]| / 448, q[r,k] = fp8(y[r,k] / scales[r]),
 * y = x (bf16 rows) or, with norm_w != NULL, the bf16 RMSNorm of x (model/components.py:39,52-53) without writing it out.
 * dim % 8 == 0, dim <= 16384. */
int a3v_quantize_rows_fp8(const void* x, int64_t ldx, const void* norm_w, float eps, void* q, int64_t ldq, float* scales,
                          int rows, int dim, int x_dtype, void* stream);
/* The column-scaled row quantiser of the fp8 frozen base (no reference counterpart, as above): the input gradient of a
 * base linear whose weight is Wq[n,k] * sw[n] is dX = (dY * sw) . Wq, so the row scales of W are folded into dY before it is
 * quantised: y[r,c] = fl32(x[r,c] * cs[c]), scales[r] = max|y[r,:]| / 448, q[r,c] = fp8(y[r,c] / scales[r]) with the rounding and the
 * all-zero-row rule of a3v_quantize_rows_fp8.  x [rows, cols] bf16 or fp32 (x_dtype), cs [cols] fp32; q gets cols_pad >= cols bytes
 * per row, ZERO beyond cols (cols_pad % 128 == 0 makes q the A operand of a3v_gemm_nt_fp8 over a zero-padded W^T without a padded
 * copy of x).  cols % 8 == 0, cols_pad % 16 == 0, cols_pad <= 32768, ldx % 8 == 0, ldq % 16 == 0, ldq >= cols_pad; x, cs, q 16-byte
 * aligned.  Anything else: A3V_ERR_*, nothing written. */
int a3v_quantize_rows_fp8_cs(const void* x, int64_t ldx, const float* cs, void* q, int64_t ldq, float* scales, int rows, int cols,
                             int cols_pad, int x_dtype, void* stream);
/* The training form of a3v_gemm_qkv_rope_fp8: the same fp8 product ((Aq . Wq^T) * sa[m] * sw[n]) with the epilogue contract of
 * a3v_gemm_qkv_rope -- the scaled accumulator is rounded to bf16, + delta (optional, bf16 [B*S, ldd]: the LoRA branch) is rounded,
 * then the rotation, the cache writes and v_rows (optional, [B*S, ldv]: v token-major for the attention backward); delta may alias
 * v_rows' buffer.  Value for value a3v_gemm_nt_fp8, the bf16 add of delta, a3v_rope_kvcache and the token-major copy of v. */
int a3v_gemm_qkv_rope_fp8_train(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, int K,
                                void* q_out, int64_t ldq, void* k_cache, void* vt_cache, void* v_rows, int64_t ldv,
                                const void* delta, int64_t ldd, const float* cos_sin, int B, int S, int H, int Hkv, int hd, int Smax,
                                int start_pos, int rope_pos0, void* stream);

/* "TN" GEMM: C[M,N] = epilogue(At^T . Wt) with At [K, M] and Wt [K, N] (the contracted index is the ROW index of both
 * operands): the weight gradient dW = dY^T . X on the token-major activations autograd holds (engine_finetune.py:55-57
 * loss.backward()), without transposing either.  lda, ldw % 8 == 0, M % 8 == 0; epilogues NONE / RESIDUAL / RES_F32 / OUT_F32. */
int a3v_gemm_tn(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N,
                int K, const void* residual, int64_t ldr, int epilogue, void* stream);

/* a3v_gemm_tn with an fp32 output kind (A3V_EPI_OUT_F32 / A3V_EPI_RES_F32: the weight gradients) that also leaves the sum of
 * squares of the values it stored, as a3v_gemm_tn_sumsq_slots(M, N) partial sums in `sumsq` (the caller zeroes the buffer once per
 * step; slots of tiles outside C are not written).  The global-norm clip (reference util/clip_grad.py:59-210) then needs no pass
 * over these gradients at all. */
int64_t a3v_gemm_tn_sumsq_slots(int M, int N);
int a3v_gemm_tn_sumsq(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                      const void* residual, int64_t ldr, int epilogue, float* sumsq, int64_t sumsq_cap, void* stream);

/* "NN" GEMM: C[M,N] = epilogue(A . Wt), A [M, K] and Wt [K, N] both row-major (the contracted index is Wt's ROW index): the
 * input gradient dX = dY . W of F.linear (autograd of LLM/llama_ens5.py:112,169,214-217) on the weight image the forward pass
 * uses -- no transposed copy of W.  K % 64 == 0, N % 8 == 0; epilogues NONE / RESIDUAL / RES_F32 / OUT_F32. */
int a3v_gemm_nn(const void* A, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                const void* residual, int64_t ldr, int epilogue, void* stream);

/* Split-K form of a3v_gemm_tn for adapter-sized outputs (the LoRA weight gradients, model/peft.py:40-64 under autograd):
 * partial [S][M][N] raw fp32 planes, to be summed by a3v_splitk_reduce. */
int a3v_gemm_tn_splitk(const void* At, int64_t lda, const void* Wt, int64_t ldw, float* partial, int M, int N, int K,
                       int S, void* stream);

/* Optional: register a scratch buffer (device memory, >= 32 MiB recommended; NULL unregisters) that a3v_gemm_nt / _nn / _tn /
 * _nt_fp8 may use for the split-K planes of their hybrid tile dispatch (the few-hundred-row tail, few-tile problems).  The library
 * itself never allocates.  Registrations are keyed by (current device, stream): GEMM calls issued on `stream` use that buffer and no
 * other, so two streams (a second model, an optimizer stream, a second device of one process) never share planes.  The buffer must
 * outlive every later GEMM call on that stream. */
int a3v_gemm_set_workspace_for(void* stream, void* ptr, int64_t bytes);
/* Legacy form for callers that do not name a stream: the buffer is bound to the FIRST (device, stream) whose GEMM call uses it; calls
 * on any other stream without a registration of their own get no scratch (plain launches), never this buffer. */
int a3v_gemm_set_workspace(void* ptr, int64_t bytes);

/* Which kernels a3v_gemm_nt / _qkv_rope (A3V_GEMM_NT), a3v_gemm_nt_fp8 / _qkv_rope_fp8 (A3V_GEMM_NT_FP8), a3v_gemm_tn / _tn_sumsq
 * (A3V_GEMM_TN) and a3v_gemm_nn (A3V_GEMM_NN) launch for a problem, on what grid: the plan those entry points execute, computed by the
 * same host code from values alone (no device, no pointer; the A3V_* switches apply).  `epilogue` / `dtype` as passed to the entry
 * point (dtype is read by A3V_GEMM_NT only); rope: the fused-qkv form; bias_aligned: the bias pointer is 8-byte aligned; sumsq: the
 * _tn_sumsq form; workspace_bytes: the registered workspace of the stream (0 = none); cus: the device's compute units (256 on MI355X).
 * Writes up to A3V_GEMM_MAX_STEPS steps of A3V_GEMM_STEP_INTS values each into `steps` -- kernel (A3V_GEMM_K_*), grid x, grid y,
 * block size, xmap, first row of C, rows of C, K-slices -- in launch order and returns their number, or A3V_ERR_*.  Shapes that the
 * entry point itself refuses are not checked here. */
enum { A3V_GEMM_NT = 0, A3V_GEMM_NT_FP8 = 1, A3V_GEMM_TN = 2, A3V_GEMM_NN = 3 };
enum { A3V_GEMM_MAX_STEPS = 3, A3V_GEMM_STEP_INTS = 8 };
enum {                          /* one value per kernel instantiation the dispatch launches */
  A3V_GEMM_K_NT_128 = 0,        /* gemm_nt_bf16_kernel<128, 128, 2, 2>                      */
  A3V_GEMM_K_NT_256,            /* gemm_nt_bf16_kernel<256, 256, 2, 4>                      */
  A3V_GEMM_K_RING,              /* gemm_nt_bf16_ring_kernel<COMMON>                         */
  A3V_GEMM_K_RING_PRE,          /* ...<COMMON | PRE> (bias / GELU forms)                    */
  A3V_GEMM_K_RING_ROPE,         /* ...<ROPE> (fused qkv)                                    */
  A3V_GEMM_K_RING_192,          /* ...<COMMON, 192>                                         */
  A3V_GEMM_K_RING_PRE_192,      /* ...<COMMON | PRE, 192>                                   */
  A3V_GEMM_K_RING_F8,           /* ...<COMMON, 256, fp8>                                    */
  A3V_GEMM_K_RING_ROPE_F8,      /* ...<ROPE, 256, fp8>                                      */
  A3V_GEMM_K_RING_192_F8,       /* ...<COMMON, 192, fp8>                                    */
  A3V_GEMM_K_FP8_PP,            /* gemm_nt_fp8_pp_kernel (two-stage)                        */
  A3V_GEMM_K_TN,                /* gemm_tn_bf16_pp_kernel<false>                            */
  A3V_GEMM_K_NN,                /* gemm_tn_bf16_pp_kernel<true>                             */
  A3V_GEMM_K_F32,               /* gemm_nt_f32_kernel                                       */
  A3V_GEMM_K_REDUCE,            /* splitk_epilogue_kernel                                   */
  A3V_GEMM_K_COUNT
};
int a3v_gemm_plan(int family, int M, int N, int K, int64_t lda, int64_t ldw, int epilogue, int dtype, int rope,
                  int bias_aligned, int sumsq, int64_t workspace_bytes, int cus, int32_t* steps);

/* Split-K form for skinny products with a long K (the LoRA adapter GEMMs of model/peft.py:84-99 and their gradients:
 * N or M = 64, K = 4096 ... 22016): slice s of S writes the fp32 plane partial[s][M][N]; a3v_splitk_reduce sums the
 * planes in order, optionally accumulates into `out` (fp32 gradients) and rounds once to out_dtype.
 * N <= 64, M >= 512: the streamed operand A goes through a multi-stage LDS ring (k-tiles stay in flight across the block barrier) as
 * 256-row blocks when S * ceil(M / 256) fills between half and all of the CUs -- one resident block per CU, the caller picks S for that
 * (S = CUs / ceil(M / 256)) -- else as 64-row blocks; every form writes the same planes bit for bit. */
int a3v_gemm_nt_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, float* partial, int M, int N,
                       int K, int S, void* stream);
int a3v_splitk_reduce(const float* partial, int S, int M, int N, void* out, int64_t ldo, int out_dtype,
                      int accumulate, void* stream);

/* Skinny-M (decode) form of the same contract, M <= 16: streams W once from HBM (one launch).
 * `partial` is a workspace of a3v_gemm_skinny_ws_bytes(M, N, K) bytes: the first 16384 bytes are
 * split-K arrival counters that the caller zero-fills ONCE; every call leaves them zero.  The
 * workspace must not be shared by calls that can run concurrently (different streams).
 * a3v_gemm_skinny_split reports the split-K factor used.  Epilogues: NONE, RESIDUAL, SWIGLU, OUT_F32. */
int a3v_gemm_skinny_split(int M, int N, int K);
int64_t a3v_gemm_skinny_ws_bytes(int M, int N, int K);
/* Which kernel a3v_gemm_skinny / _fp8 / _nf4 and the decode step's fused GEMVs launch for a problem, on what grid: the plan those
 * entry points execute, computed by the same host code from values alone (no device, no pointer; A3V_GEMV_KQ applies).  epilogue as
 * passed to the entry point; format: the weight image; prologue / rope / ssq: the decode step's fused forms (RMSNorm on the way in,
 * RoPE + KV-cache write, sums of squares on the way out); inblock_ok: A is 16-byte aligned with lda % 8 == 0 and so are the norm
 * weights, if any; cus: the device's compute units (256 on MI355X).  Writes A3V_GEMV_PLAN_INTS values into `plan` -- kernel, activation
 * rows of the template form (8 / 16), prologue, format, grid x, block size, dynamic LDS bytes, K slices across blocks (what
 * a3v_gemm_skinny_split reports), 128-k blocks of K, 64-row groups of W, 128-k blocks of A per slice, K slices as launched (inside the
 * block for A3V_GEMV_K_KQ), k per wave of the direct kernels -- and returns the kernel (A3V_GEMV_K_*), A3V_ERR_SHAPE where no kernel
 * can run the problem, or A3V_ERR_ARG.  The direct kernels exist for a3v_gemm_skinny alone: the other entry points answer
 * A3V_ERR_SHAPE where this names one.  Shapes that the entry point itself refuses are not checked here. */
enum { A3V_GEMV_BF16 = 0, A3V_GEMV_FP8 = 1, A3V_GEMV_NF4 = 2 };
enum { A3V_GEMV_PLAN_INTS = 13 };
enum {
  A3V_GEMV_K_DMA = 0,           /* gemv_dma_bf16_kernel<arows, prologue, fp8, nf4>: K slices across blocks   */
  A3V_GEMV_K_KQ,                /* gemv_kq_bf16_kernel<prologue>: K slices inside the block                  */
  A3V_GEMV_K_DIRECT1,           /* gemm_skinny1_bf16_kernel<1>: direct-to-VGPR                               */
  A3V_GEMV_K_DIRECT2,           /* gemm_skinny1_bf16_kernel<2>: the same on gate / up row pairs (SwiGLU)     */
  A3V_GEMV_K_COUNT
};
int a3v_gemv_plan(int M, int N, int K, int epilogue, int format, int prologue, int rope, int ssq, int inblock_ok, int cus,
                  int32_t* plan);
/* Weight-only fp8 form (BASELINE config 5): Wq [N,K] OCP e4m3fn bytes (row stride ldw in BYTES,
 * % 16 == 0), wscale [N] fp32 per-row dequantisation scales; C = epilogue((A . float(Wq)^T) * wscale), K % 256 == 0.
 * The reference's quantised path is CUDA-only bitsandbytes NF4 (util/quant.py:95-163): there is NO reference oracle for
 * fp8 -- parity is stated against the bf16 kernel on the dequantised weights. */
int a3v_gemm_skinny_fp8(const void* A, int64_t lda, const void* Wq, int64_t ldw, const float* wscale, void* C,
                        int64_t ldc, int M, int N, int K, const void* residual, int64_t ldr, int epilogue,
                        void* workspace, void* stream);
/* NF4 weight-only inference (the reference's quantised mode: bitsandbytes Linear4bit nf4, blocksize 64, compress_statistics=True,
 * util/quant.py:95-163, applied by MetaModel.from_pretrained(quant=True), meta.py:197-219).  Format, per original module W [N, K]
 * bf16 (contiguous rows, K % 64 == 0):
 *   blocks of 64 consecutive elements of the flattened matrix; absmax_b = max|w| (fp32); code q = argmin_i |w * (1/absmax_b) - NF4[i]|
 *   (correctly rounded fp32 reciprocal, then a product; first minimum on ties) over bitsandbytes' 16-entry NF4 table; two codes per
 *   byte, the earlier element in the HIGH nibble; an all-zero block gets code 7 and scale 0;
 *   double quantisation: offset = mean(absmax) over the module, absmax - offset quantised in groups of 256 consecutive blocks to
 *   the nearest entry of bitsandbytes' signed 8-bit dynamic map with absmax2_g = max|absmax - offset|;
 *   effective scale s_b = map[qa_b] * absmax2_g + offset in fp32 (two roundings, as dequantize_4bit rebuilds absmax), stored per block;
 *   dequantised weight Wd = bf16(NF4[q] * s_b).
 * a3v_quantize_nf4: W -> q [N, K/2] uint8 + scales [N, K/64] fp32; ws = a3v_quantize_nf4_ws_bytes(N, K) bytes of caller workspace
 * (16-B aligned; after the call ws[0] holds the module offset as a float).  Allocates nothing. */
int64_t a3v_quantize_nf4_ws_bytes(int N, int K);
int a3v_quantize_nf4(const void* W, int N, int K, void* q, float* scales, float* ws, void* stream);
/* Wd [N, K] bf16 (row stride ldd elements, ldd % 8 == 0) = bf16(NF4[q] * s_b): the multi-token forward of an NF4 model runs the bf16
 * GEMMs on it (bit-identical to the bf16 model holding Wd). */
int a3v_dequantize_nf4(const void* q, const float* scales, void* Wd, int64_t ldd, int N, int K, void* stream);
/* The same values in either orientation from ONE read of the codes and scales (the QLoRA training step: the per-layer GEMM images of
 * an NF4 base).  Wd [N, K] at row stride ldd and / or Wt [K, N] = Wd^T at row stride ldt (elements); either may be NULL, both NULL is
 * A3V_ERR_ARG.  Wd is bit-equal to a3v_dequantize_nf4.  ONLY the N x K / K x N windows are written: the destinations are windows of
 * larger images (ldd > K, ldt > N) whose tail columns hold adapter blocks.  K % 64 == 0, ldd % 8 == 0, ldt % 8 == 0, q / Wd / Wt 16-B
 * aligned (A3V_ERR_SHAPE before any launch otherwise); N is arbitrary. */
int a3v_dequantize_nf4_images(const void* q, const float* scales, int N, int K, void* Wd, int64_t ldd, void* Wt, int64_t ldt, void* stream);
/* LoRA merge: the adapters of one linear folded into its base matrix, W' = W + lora_b . lora_a (no alpha / rank scaling, as the
 * adapter forward y = W x + lora_b(lora_a(x))).
 *   out[n,k] = round_to_dtype( fp32(base[n,k]) + sum_r fp32(B[n,r]) * fp32(A[r,k]) )
 * The sum over r is accumulated in fp32 (ascending r in 32-wide MFMA steps; the order does not depend on the base format), the base is
 * added in fp32 and the result is rounded ONCE (not bf16(acc) + base as the residual epilogue of a3v_gemm_nt rounds: a merged weight is
 * written once and read forever).  Base: either W [N, K] (row stride ldw elements) or, with W NULL, the NF4 image (q [N, K/2],
 * scales [N, K/64]) of a3v_quantize_nf4, for which base[n,k] is Wd = bf16(NF4[q] * s_b) exactly as a3v_dequantize_nf4 writes it: a
 * merge over an NF4 base is bit-equal to a merge over a bf16 base that holds Wd.
 * dtype A3V_BF16: B [N, R], A [R, K], out [N, K] and a non-NULL W are bf16; the product runs on MFMA.  dtype A3V_F32 (parity path):
 * fp32 storage, plain FMA, no NF4 base (A3V_ERR_ARG).  out == W (in place) is allowed and is the normal use; any other overlap of out
 * with an input is undefined.  Only the N x K window of out is written (ldo > K: the columns beyond K are untouched).
 * Limits (A3V_ERR_SHAPE before any launch; a NULL B / A / out, both or neither of W / q, or q without scales: A3V_ERR_ARG):
 * R % 8 == 0 and 8 <= R <= 256; K % 8 == 0 (K % 64 == 0 for an NF4 base); ldw, ldo >= K, lda >= K, ldb >= R, all multiples of 8
 * elements; every pointer 16-B aligned; N arbitrary (<= 65535 * 128 rows).  Allocates nothing. */
int a3v_lora_merge(const void* W, int64_t ldw, const void* q, const float* scales, const void* B, int64_t ldb, const void* A, int64_t lda,
                   void* out, int64_t ldo, int N, int K, int R, int dtype, void* stream);
/* Weight-only NF4 decode GEMV, M <= 16, K % 256 == 0: q [N, K/2] (row stride ldw BYTES), scales [N, K/64]; workspace and epilogues
 * (NONE, RESIDUAL, SWIGLU, OUT_F32) as a3v_gemm_skinny; SWIGLU needs K >= 512 (A3V_ERR_SHAPE otherwise, as the fp8 form).  The codes enter the MFMA as bf16 and each 64-k block sum is scaled by s_b in
 * fp32, so results differ from the bf16 GEMV on Wd by rounding only. */
int a3v_gemm_skinny_nf4(const void* A, int64_t lda, const void* Wq, int64_t ldw, const float* scales, void* C, int64_t ldc,
                        int M, int N, int K, const void* residual, int64_t ldr, int epilogue, void* workspace, void* stream);
int a3v_gemm_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                    int M, int N, int K, const void* residual, int64_t ldr, int epilogue,
                    void* partial, void* stream);
/* The decode step's building block: the GEMV a3v_llama_decode_step calls four times per layer, i.e. a3v_gemm_skinny (wscale NULL),
 * a3v_gemm_skinny_fp8 (wscale [N], n4 == 0) or a3v_gemm_skinny_nf4 (wscale = block scales [N, K/64], n4 != 0) with up to three fused forms:
 *   norm_w != NULL  RMSNorm prologue.  A holds the un-normalised rows x; ssq_in [K/16][16] fp32 holds, for every 16-column tile t and row
 *                   m, a partial sum of squares (a producer's ssq_out; all 16 columns are read).  rinv[m] = rsqrtf(sum_t ssq_in[t][m] / K
 *                   + eps) and the GEMV runs on a' = bf16(bf16(x * rinv) * norm_w): the rounding of a3v_rmsnorm on bf16 rows.
 *   rope != 0       RoPE + KV-cache epilogue.  Rows n of W are [H q heads | Hkv k heads | Hkv v heads] x hd.  With v = bf16(acc), every
 *                   pair (v0, v1) = (v[2i], v[2i+1]) of a q or k head becomes bf16(v0 c - v1 s), bf16(v0 s + v1 c), (c, s) =
 *                   cos_sin[pos][i] (fp32 [positions][hd/2][2]); q goes to C[m, n] (only the first H hd columns of C are written), k to
 *                   k_cache[m, h, pos, :] of a bf16 [M, Hkv, Smax, hd] cache, v unrotated to vt_cache[m, h, :, pos] of [M, Hkv, hd, Smax].
 *                   `residual` and `epilogue` are ignored by this form.
 *   ssq_out != NULL sum-of-squares side output (with the plain bf16 or the RESIDUAL epilogue): ssq_out[n/16][m] = the sum over the 16
 *                   columns of the tile of the squares of the bf16 values stored to C, for all 16 m (0 for m >= M): the next GEMV's ssq_in.
 * C may alias `residual` (each element is read, then written by the same lane).  ws: as a3v_gemm_skinny's `partial`.
 * Needs M <= 16, K % 128 == 0 (fp8 / NF4: % 256), N % 16 == 0, N <= 65536 and a non-NULL ws (A3V_ERR_SHAPE otherwise; also where only the
 * direct-to-VGPR kernel could run the problem: more than 150 KiB of LDS, SWIGLU without a K split -- the fused forms have no fallback);
 * NF4 without scales or with K % 256, and rope with hd % 16 != 0 or without cos_sin / k_cache / vt_cache: A3V_ERR_ARG.  Beyond that
 * it checks neither strides nor epilogue bits: lda % 8, ldw % 8 (fp8 / NF4: bytes, % 16), ldc % 4, ldr % 4, 16-byte aligned A, W,
 * scales and norm_w, and an epilogue of RESIDUAL, SWIGLU (N % 32 == 0) or OUT_F32 alone are the caller's to guarantee. */
int a3v_gemv_fused(const void* A, int64_t lda, const void* W, int64_t ldw, const float* wscale, int n4, void* C, int64_t ldc, int M, int N,
                   int K, const void* residual, int64_t ldr, int epilogue, const void* norm_w, const float* ssq_in, float eps,
                   float* ssq_out, int rope, const float* cos_sin, void* k_cache, void* vt_cache, int H, int Hkv, int hd,
                   int Smax, int pos, void* ws, void* stream);

/* ---- MXFP4 weights (OCP Microscaling v1.0: the 4-bit format CDNA4's scaled MFMA decodes in hardware; opt-in beside NF4) ----
 * Weights W [N, K] bf16, K % 128 == 0, in blocks of 32 consecutive k of one row:
 *   codes  q [N, K/2] bytes, row stride ldq BYTES (% 16 == 0), element 2j in the LOW nibble of byte j;
 *   scales s [N, K/32] uint8 (contiguous rows), e8m0, value 2^(s - 127).
 *   Block: E = floor(log2(max|w|)) - 2 clamped to [-127, 127], s = E + 127; an all-zero block gets s = 127 and codes 0; 0xFF is never
 *   written.  Element: w / 2^E (exact) rounded to the nearest e2m1 value, ties to the even code, saturating at +-6.  e2m1 grid: codes
 *   0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 the sign; -0 is written as +0.  4.25 bits per weight.
 *   Dequantised weight Wd = e2m1(q) * 2^(s - 127), exact in bf16.
 * Activations (inside the GEMV only): MXFP8 by the same rule with OCP e4m3fn elements: E = floor(log2(max|a|)) - 8 over 32 consecutive
 *   k of one row, a / 2^E rounded to nearest even, saturating at +-448; zero block: byte 127, codes 0.  Block-local: no row reduction,
 *   so a K slice of a split plan quantises exactly as the whole row would.
 * a3v_quantize_mxfp4: one launch, one pass over W (row stride ldw elements, % 8 == 0).  a3v_dequantize_mxfp4: out [N, K] bf16 (row
 * stride ldo elements, % 8 == 0) = Wd.  w, q, out 16-B aligned.  A3V_ERR_ARG (NULL pointer) / A3V_ERR_SHAPE before any launch. */
int a3v_quantize_mxfp4(const void* w, int64_t ldw, void* q, int64_t ldq, void* s, int N, int K, void* stream);
int a3v_dequantize_mxfp4(const void* q, int64_t ldq, const void* s, void* out, int64_t ldo, int N, int K, void* stream);
/* MXFP4 decode GEMV, M <= 16, N % 16 == 0 (<= 65536), K % 128 == 0 (<= 16384), A bf16 [M, K] (row stride lda elements, % 8 == 0):
 *   C = epilogue( sum_blocks 2^(ea + ew) * sum_32 a_q * w_q )
 * a_q / ea: the MXFP8 codes and block exponents of A as stated above, computed by the kernel as it stages A; w_q / ew: the image.  Both
 * block scales are handed to v_mfma_scale_f32_16x16x128_f8f6f4 as its scale operands; accumulation is fp32 (within a slice in MFMA
 * order, the K slices of a split plan summed in slice order: bit-identical from run to run).  Epilogues as a3v_gemm_skinny with its
 * rounding sequence: NONE bf16(acc); RESIDUAL bf16(bf16(acc) + residual); SWIGLU (N counts the 16-row-interleaved w1|w3 rows, N % 32
 * == 0, C has N/2 columns) bf16(bf16(silu(bf16(gate))) * bf16(up)); OUT_F32 stores float(bf16(acc)) (the LM head; with RESIDUAL the
 * fp32 sum).  workspace: a3v_gemm_skinny_mxfp4_ws_bytes(M, N, K) bytes laid out as a3v_gemm_skinny's (the first 16384 bytes are arrival
 * counters zero-filled ONCE by the caller and left zero; the two entry points may share one workspace).  A, q, C, workspace 16-B
 * aligned, s 4-B, residual 8-B; ldc, ldr % 4 == 0.
 * a3v_mx4_gemv_plan: the plan the entry point executes, from values alone (no device, no pointer; cus: compute units, 256 on
 * MI355X).  Writes A3V_MX4_PLAN_INTS values -- grid x, block size, K slices across blocks, W rows per block, dynamic LDS bytes, 512-k
 * units of K, 64-row groups of W, units of A staged per block -- and returns A3V_OK, or A3V_ERR_SHAPE for what cannot run (the entry
 * point answers the same before any launch), or A3V_ERR_ARG (NULL plan). */
enum { A3V_MX4_PLAN_INTS = 8 };
int a3v_mx4_gemv_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan);
int64_t a3v_gemm_skinny_mxfp4_ws_bytes(int M, int N, int K);
int a3v_gemm_skinny_mxfp4(const void* A, int64_t lda, const void* q, int64_t ldq, const void* s, void* C, int64_t ldc, int M, int N,
                          int K, const void* residual, int64_t ldr, int epilogue, void* workspace, void* stream);
/* W4A8 GEMM on the same images, for any M (prefill, and decode steps of more than 32 rows): the activation rows are quantised ONCE per
 * product by a3v_quantize_rows_mxfp8 and a3v_gemm_nt_mxfp4 hands the e8m0 block scales of both operands to the scaled MFMA.
 * a3v_quantize_rows_mxfp8: x [rows, K] bf16 (row stride ldx elements, % 8 == 0, >= K; x and norm_w 16-B aligned) -> codes q [rows, K]
 *   e4m3fn bytes (row stride ldq BYTES, % 8 == 0, >= K; q 8-B aligned) and block exponents e [rows, K/32] e8m0 bytes (contiguous rows),
 *   exactly the "Activations" rule above: E = floor(log2(max|a|)) - 8 per 32 k clamped to [-127, 127], byte E + 127, a / 2^E rounded to
 *   nearest even, saturating at +-448; zero block: byte 127, codes 0.  norm_w != NULL: the rows quantised are the bf16 RMSNorm of x
 *   (weight norm_w [K] bf16, eps) without writing it: bit-equal to a3v_rmsnorm (bf16 in, weight and out; K <= 8192 there) followed by the
 *   plain form.
 *   K % 128 == 0, K <= 16384; one launch, one block per row.
 * a3v_gemm_nt_mxfp4: C = epilogue( sum_blocks 2^(ea + ew) * sum_32 a_q * w_q ), Aq [M, K] / ea [M, K/32] as written by the quantiser
 *   (lda BYTES, % 16 == 0; Aq 16-B aligned), q / s an image as above, the 16-row interleaved w1|w3 rows of SWIGLU included (no second copy
 *   of an image).  Any M >= 1, N % 16 == 0 (SWIGLU: % 32) and <= 65536, K % 128 == 0 and <= 16384.  Epilogues NONE / RESIDUAL / SWIGLU /
 *   OUT_F32 with the rounding sequences stated for a3v_gemm_skinny_mxfp4 (residual may be C); no RoPE form: qkv is stored plainly and
 *   a3v_rope_kvcache follows.  Accumulation is fp32, every accumulator sums its 128-k MFMA steps in k order: the summation order depends
 *   on (M, N, K, epilogue) alone, a call is bit-identical from run to run; there is no split-K form and no workspace.  C 8-B aligned
 *   (OUT_F32: 16-B), residual 8-B; ldc, ldr % 4 == 0.
 * a3v_mx4_gemm_plan: the plan the entry point executes, from values alone (no device, no pointer; cus: compute units, 256 on MI355X --
 *   today's plan does not depend on it).  Writes A3V_MX4_GEMM_PLAN_INTS values -- tile rows (16, 32, 64 or 128: the smallest that holds M,
 *   so up to 128 rows the image is streamed once), tile columns (rows of W per block: 64, SWIGLU 128), K stage in k (512), grid x (row
 *   tiles x column tiles, the row tiles of a column tile adjacent), block size, LDS bytes (0: operands go from global memory / L2 to
 *   registers), K slices (1), K stages per slice (ceil(K / 512); the K % 512 remainder runs in steps of 128 k).
 * All three: A3V_ERR_ARG (NULL pointer; RESIDUAL without residual) / A3V_ERR_SHAPE (anything the entry cannot run) before any launch. */
enum { A3V_MX4_GEMM_PLAN_INTS = 8 };
int a3v_quantize_rows_mxfp8(const void* x, int64_t ldx, const void* norm_w, float eps, void* q, int64_t ldq, void* e, int rows, int K,
                            void* stream);
int a3v_mx4_gemm_plan(int M, int N, int K, int epilogue, int cus, int32_t* plan);
int a3v_gemm_nt_mxfp4(const void* Aq, int64_t lda, const void* ea, const void* q, int64_t ldq, const void* s, void* C, int64_t ldc, int M,
                      int N, int K, const void* residual, int64_t ldr, int epilogue, void* stream);

/* y = rmsnorm(x) * w  with the reference's rounding order (model/components.py:39,52-53):
 * fp32 normalise -> cast to x's dtype -> multiply by weight.  x_dtype may be A3V_F32 with
 * y bf16 (training under autocast: fp32 residual stream feeding bf16 GEMMs). */
int a3v_rmsnorm(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int rows, int dim,
                float eps, int x_dtype, int w_dtype, int y_dtype, void* stream);

/* The same over the rows of a list: y[i] = rmsnorm(x[row_idx[i]]) * w for i < rows (int32 indices, every one inside x): the rows
 * are gathered by the pass that normalises them. */
int a3v_rmsnorm_rows(const void* x, int64_t ldx, const int32_t* row_idx, const void* w, void* y, int64_t ldy,
                     int rows, int dim, float eps, int x_dtype, int w_dtype, int y_dtype, void* stream);

/* y[row_map ? row_map[r] : r] = layernorm(x[r]) * w + b   (torch.nn.LayerNorm, eps 1e-5):
 * open_clip ln_pre/ln_1/ln_2/ln_post and the projector LayerNorm (LLM/llama_ens5.py:325-333,
 * 363,370).  row_map (int32, device) lets the projector write straight into the
 * [BOS | image tokens | text] sequence buffer (:471-479). */
int a3v_layernorm(const void* x, int64_t ldx, const void* w, const void* b, void* y, int64_t ldy,
                  const int32_t* row_map, int rows, int dim, float eps, int x_dtype, int p_dtype,
                  int y_dtype, void* stream);

/* RoPE on q,k (interleaved pairs, fp32 math, LLM/llama_ens5.py:118 + restated llama.py) and
 * KV-cache write (:124-129) from a fused qkv activation [B*S, (H+2*Hkv)*hd]:
 *   q_out [B*S, ldq]            rotated q (may alias qkv: in-place, ldq = ldqkv)
 *   k_cache[B,Hkv,Smax,hd]      rotated k at positions start_pos..start_pos+S-1
 *   vt_cache[B,Hkv,hd,Smax]     v TRANSPOSED (this library's cache layout: the attention
 *                               kernels consume V^T tiles with no in-loop transpose)
 * cos_sin: fp32 table [n_pos, hd/2, 2]; row = rope_pos0 + s. */
int a3v_rope_kvcache(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache,
                     void* vt_cache, const float* cos_sin, int B, int S, int H, int Hkv, int hd,
                     int Smax, int start_pos, int rope_pos0, int dtype, void* stream);

/* v [N, L, H*hd] (row stride ldv, e.g. the v third of nn.MultiheadAttention's packed
 * in_proj output) -> vt [N, H, hd, Lpad] zero padded: the V^T operand of a3v_attention. */
int a3v_vt_pack(const void* v, int64_t ldv, void* vt, int N, int L, int H, int hd, int Lpad,
                int dtype, void* stream);

/* softmax(q k^T / sqrt(hd) [+ right-aligned causal mask]) v, flash style, fp32 softmax.
 * Replaces F.scaled_dot_product_attention / flash_attn_func (LLM/llama_ens5.py:142-167,
 * mask :181-185) and nn.MultiheadAttention's core (open_clip resblocks).
 * strides (ELEMENTS, host array of 12): q {batch, seq, head}, k {batch, kv-head, seq},
 * vt {batch, kv-head, d}, out {batch, seq, head}; hd is contiguous in q/k/out and seq is
 * contiguous in vt.  bf16: hd in {64,128}, strides multiples of 8.  Sq == 1 selects the
 * split-KV decode kernel (`scratch`: fp32, a3v_attention_scratch_floats() entries; may be
 * NULL when Sq > 1).  causal requires Sk >= Sq (queries are the LAST Sq positions). */
int64_t a3v_attention_scratch_floats(int B, int H, int hd, int Sk);
int a3v_attention(const void* q, const void* k, const void* vt, void* out, int B, int Sq, int Sk,
                  int H, int Hkv, int hd, const int64_t* strides, int causal, float* scratch,
                  int dtype, void* stream);
/* a3v_attention_decode_plan: the split of Sk keys the decode entries use at (B, H): nsplit key ranges of `chunk` keys (a multiple
 * of 64; the last range holds the rest).  wave != 0: the plan of every wave-streaming entry (decode_fused, decode_rows,
 * decode_fp8kv, verify_rows at sk_max); wave == 0: the two-phase plan of a3v_attention at Sq = 1, which also sizes the scratch.
 * a3v_attention_decode_fused_bf16: the decode attention of a3v_llama_decode_step as an entry of its own: bf16, hd in {64, 128},
 * strides as a3v_attention at Sq = 1, 16-byte aligned q / k / vt, scratch of a3v_attention_scratch_floats(B, H, hd, Sk) floats,
 * counters: B*H zero-initialised ints, left zero (the split partials are merged inside the launch). */
int a3v_attention_decode_plan(int B, int H, int Sk, int wave, int* nsplit, int* chunk);
int a3v_attention_decode_fused_bf16(const void* q, const void* k, const void* vt, void* out, int B, int Sk, int H, int Hkv, int hd,
                                    const int64_t* strides, float* scratch, int* counters, void* stream);

/* h[b, s, :] for the sequence [BOS | image words | text]: rows s==0 and s>W come from the
 * embedding table (tok_embeddings, LLM/llama_ens5.py:464,495), rows 1..W are left untouched
 * (written by a3v_layernorm(row_map) / a3v_fill_rows).  tokens int64 [B,T]. */
int a3v_embed_assemble(const int64_t* tokens, int64_t ld_tok, const void* table, void* h, int B,
                       int T, int W, int dim, int vocab, int table_dtype, int h_dtype, void* stream);

/* dst[row_idx[i], :] = src[0, :]  (start_img / end_img tags, LLM/llama_ens5.py:472-474) */
int a3v_fill_rows(const void* src, void* dst, int64_t ldd, const int32_t* row_idx, int n_rows,
                  int dim, int src_dtype, int dst_dtype, void* stream);

/* im2col for the k=s=P, bias-free patch-embed conv (LLM/llama_ens5.py:354): img [N,3,Hi,Wi]
 * -> cols [N*g*g, Kpad] with k = c*P*P + py*P + px (conv1.weight.view(width,-1) order),
 * zero padded to Kpad. */
int a3v_patch_im2col(const void* img, void* cols, int N, int Hi, int Wi, int P, int Kpad,
                     int in_dtype, int out_dtype, void* stream);

/* LLM/llama_ens5.py:383-385: img [B,3,2c,2c] -> out [5B,3,c,c] = [fp16 bicubic 2x downsample
 * of the whole image ; top-left ; top-right ; bottom-left ; bottom-right]. */
int a3v_split_views(const void* img, void* out, int B, int crop, int in_dtype, int out_dtype,
                    void* stream);

/* x[n, 0, :] = cls + pos[0]; x[n, 1+t, :] = patch[n*T+t, :] + pos[1+t]  (:358-362) */
int a3v_vit_embed(const void* patch, const void* cls, const void* pos, void* x, int N, int T,
                  int width, int dtype, void* stream);

/* Image preprocessing of the input contract on the device (data/transform.py:13-68: PadToSquare with the CLIP-mean fill ->
 * Resize(bicubic) -> ToTensor -> Normalize): src = one decoded RGB image, uint8 [H][W][3]; it sits at (pad_x, pad_y) inside a
 * side x side square filled with fill_rgb; the square is resized to out_size x out_size with Pillow's 8-bit two-pass resampling
 * (the reference transform runs torchvision on PIL images, i.e. Pillow's ImagingResample): kx / ky = the fixed-point (2^22)
 * coefficient rows of the horizontal / vertical pass, ksize_* ints per output sample, bx / by = (first input index, tap count)
 * per output sample -- tables computed on the host from (side, out_size) exactly as Resample.c does (a3vlm_amd/data/transform.py).
 * tmp: uint8 scratch [side][out_size][3].  dst: [3][out_size][out_size] in dst_dtype, ((v / 255) - mean[c]) / std[c] with fp32
 * arithmetic.  Host-side scalars (fill_rgb, mean, std) are HOST pointers; everything else is device memory.  Bit-identical to
 * the PIL path (tests/test_gpu_preprocess.py). */
int a3v_preprocess_image(const uint8_t* src, int H, int W, int side, int pad_x, int pad_y, const int* fill_rgb,
                         const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y,
                         int out_size, uint8_t* tmp, void* dst, int dst_dtype, const float* mean, const float* std, void* stream);

/* The same transform for a BATCH of decoded images (the loaders of eval_affordance_v2.py:109-180 and main_finetune.py's dataset
 * build: workers decode to uint8 HWC, the device does the rest), two launches per 16 images.  Each image carries the tables of ITS
 * padded side (coeffs / bounds of a3vlm_amd/data/transform.py:pillow_bicubic_coeffs, used for both passes: the square is resized
 * to a square).  `images` is a HOST array of n descriptors whose pointers are DEVICE pointers.  tmp: uint8 scratch, tmp_stride bytes
 * per image (>= side x out_size x 3); dst: [n][3][out_size][out_size] in dst_dtype, dst_stride ELEMENTS per image.  Same arithmetic,
 * bit for bit, as a3v_preprocess_image. */
typedef struct {
  const uint8_t* src;        /* [H][W][3] */
  const int32_t* coeffs;     /* [out_size][ksize] */
  const int32_t* bounds;     /* [out_size][2] */
  int H, W, side, pad_x, pad_y, ksize;
} a3v_image_desc;
int a3v_preprocess_batch(const a3v_image_desc* images, int n, const int* fill_rgb, int out_size, uint8_t* tmp, int64_t tmp_stride,
                         void* dst, int64_t dst_stride, int dst_dtype, const float* mean, const float* std, void* stream);

/* One step of the token bookkeeping of MetaModel.generate (model/meta.py:456-477), one launch for the whole batch: greedy argmax of
 * logits [B, V] (fp32, row stride ld) -- or, when `sampled` is non-NULL, the externally sampled ids of the top-p branch (:457-459) --
 * then, per row: teacher forcing of prompt positions (text_mask[row, cur_pos], :463-465), tokens[row, cur_pos] = next,
 * stop_pos / stopped update and the multi-token stop-sequence match (:468-475; stop_seq = all sequences concatenated, stop_off =
 * n_stop + 1 offsets, tried in order).  text_mask / stopped are one byte per element (torch.bool).  `live` (optional): device
 * counter of rows still running, decremented when a row stops -- the host reads that one word every k steps instead of
 * `stopped.all()` every step (:476).  Values are bit-identical to the reference's torch ops (integer work). */
int a3v_generate_step(const float* logits, int64_t ld, const int64_t* sampled, int B, int V, int64_t* tokens, int64_t ld_tok,
                      const uint8_t* text_mask, int64_t ld_mask, int cur_pos, const int64_t* stop_seq, const int32_t* stop_off,
                      int n_stop, uint8_t* stopped, int64_t* stop_pos, int32_t* live, void* stream);

/* The sampled branch of MetaModel.generate (model/meta.py:456-459) with sample_top_p (model/meta.py:568-583) on the device, one
 * launch for the batch and no full-vocabulary sort: probs = softmax(logits / temperature); a token is kept iff the probability
 * mass ranked before it (value descending, index ascending on ties) is <= top_p; out[b] = the kept token the inverse CDF of the
 * renormalised nucleus reaches at u[b] (u[b] uniform in [0, 1), supplied by the caller's generator: torch.multinomial's own
 * random stream is not part of the contract).  logits fp32 [B, V] (V <= 65536), temperature > 0, top_p > 0 (>= 1 keeps all). */
int a3v_sample_top_p(const float* logits, int64_t ld, int B, int V, float temperature, float top_p, const float* u,
                     int64_t* out, void* stream);

/* a3v_sample_top_p with two more filters, in HF's order: temperature, top-k, top-p, min-p.  No reference counterpart (opt-in).
 * z = one row of fp32 logits (with a repetition penalty: the row a3v_logits_prepare wrote), T = temperature > 0,
 * x_i = z_i / T, xm = max x, e_i = expf(x_i - xm) -- the expressions of a3v_sample_top_p.
 *   1. top-k   top_k = 0 or >= V: off.  t = the top_k-th largest value of z counting duplicates; K = {i : z_i >= t}, decided on the
 *              logits' own bits (nothing rounds; every token tied at t is kept, as HF's TopKLogitsWarper does).  Outside K: mass 0.
 *   2. top-p   a3v_sample_top_p's rule on K: rank K by e descending, token index ascending; kept iff the mass ranked before the
 *              token is <= top_p * Z_K, Z_K = sum of e over K.
 *   3. min-p   0 <= min_p <= 1, 0: off.  kept iff e_i >= min_p; e_max is exactly 1, so this is p_i >= min_p * p_max under either
 *              renormalisation above, and the arg-max always survives.
 *   4. draw    the inverse CDF over the kept tokens in ranked order at u * M, M = the kept mass, u clamped into [0, 1).
 * Inside K the top-p set and the min-p set are prefixes of one ranking: the final set is the shorter one.  A row without a finite
 * logit gives id 0.  With top_k = 0 and min_p = 0 the ids are a3v_sample_top_p's, bit for bit.
 * Returns A3V_ERR_ARG for top_k < 0 or min_p outside [0, 1] (and a3v_sample_top_p's argument errors), A3V_ERR_SHAPE as
 * a3v_sample_top_p; nothing is launched on an error. */
int a3v_sample_top_k_p(const float* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p, float min_p,
                       const float* u, int64_t* out, void* stream);

/* torch.argmax(logits, -1) with first-index tie break (model/meta.py:460).  fp32 [B,V]. */
int a3v_argmax(const float* logits, int64_t ld, int64_t* out, int B, int V, void* stream);

/* CrossEntropyLoss(ignore_index=0) pieces (model/meta.py:67,256-262): per-row loss (fp32)
 * and, if dlogits != NULL, d(mean loss)/dlogits scaled by grad_scale / n_valid where
 * n_valid is read from n_valid_dev (device int32, produced by a3v_count_valid).
 * logits bf16 or f32 [rows, V]; labels int64 (already shifted). */
int a3v_count_valid(const int64_t* labels, int rows, int32_t* n_valid_dev, void* stream);
int a3v_cross_entropy(const void* logits, int64_t ld, const int64_t* labels, float* row_loss,
                      void* dlogits, int64_t ldd, const int32_t* n_valid_dev, float grad_scale,
                      int rows, int V, int dtype, void* stream);

/* One decode step (seqlen == 1) of the whole decoder stack from a single host call: per layer
 * RMSNorm -> fused QKV (skinny GEMM) -> RoPE + KV-cache write at `pos` -> split-KV attention over
 * pos+1 keys -> WO (+residual) -> RMSNorm -> W1|W3 SwiGLU -> W2 (+residual)  (LLM/llama_ens5.py:
 * 220-249, 490-531).  h [B,dim] bf16 is updated in place; xn/qkv/att/act are caller workspaces of
 * [B,dim], [B,(H+2Hkv)hd], [B,H*hd], [B,ffn]; attn_scratch as for a3v_attention at Sk = Smax;
 * skinny_ws as for a3v_gemm_skinny, sized for the largest of the four linears. */
typedef struct a3v_llama_layer {
  const void* attn_norm_w;
  const void* wqkv;     /* [wq;wk;wv] rows */
  const void* wo;
  const void* ffn_norm_w;
  const void* w13;      /* w1/w3 interleaved in 16-row blocks */
  const void* w2;
  void* k_cache;        /* [B,Hkv,Smax,hd] */
  void* vt_cache;       /* [B,Hkv,hd,Smax] */
  /* optional weight-only fp8 (OCP e4m3fn) images of the four matrices, same row order as the bf16 images, with one fp32
   * scale per row (a3v_gemm_skinny_fp8); all NULL = bf16.  Used only by the fused step form (dims % 256 == 0). */
  const void* wqkv_q; const float* wqkv_s;
  const void* wo_q;   const float* wo_s;
  const void* w13_q;  const float* w13_s;
  const void* w2_q;   const float* w2_s;
  /* optional NF4 images of the four matrices (a3v_quantize_nf4 per original module, rows permuted as the bf16 images: nibbles
   * [N, K/2], block scales [N, K/64]); all NULL = not NF4.  Setting fp8 and NF4 fields together returns A3V_ERR_ARG.  Fused step
   * form only (a3v_llama_decode_step_form with w8 = 2). */
  const void* wqkv_n4; const float* wqkv_n4s;
  const void* wo_n4;   const float* wo_n4s;
  const void* w13_n4;  const float* w13_n4s;
  const void* w2_n4;   const float* w2_n4s;
} a3v_llama_layer;
int a3v_llama_decode_step(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv,
                          void* att, void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, int B,
                          int dim, int H, int Hkv, int hd, int ffn, int Smax, int pos, float eps,
                          void* stream);
/* Which form a3v_llama_decode_step takes for a geometry, decided before anything is launched: 2 = the fused five-launch form,
 * 1 = the per-kernel form (<= 16 rows, bf16 weights), 0 = not taken (the call returns A3V_ERR_SHAPE with every buffer untouched and
 * the host runs the general kernels: llama_ens5.py:490-531 has no batch limit below max_batch_size). */
int a3v_llama_decode_step_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8);   /* w8: 0 bf16, 1 fp8, 2 NF4 images */

/* ---------------------------------------------------------------------------------------
 * fp8 KV cache (opt-in; no reference counterpart: the reference's cache is bf16, LLM/llama_ens5.py:171-176).  Format:
 *   k_q  [B,Hkv,Smax,hd] and vt_q [B,Hkv,hd,Smax]: OCP e4m3fn bytes in the layouts of the bf16 caches, Smax % 64 == 0;
 *   k_scale, v_scale [B,Hkv,Smax] fp32: one scale per (batch, kv-head, position) for K and one for V;
 *   over the hd values x of one head at one position (K: after RoPE), as a3v_quantize_rows_fp8 / oracle.quant_fp8:
 *   scale = max(max|x|, 1e-12) / 448, q = e4m3(x / scale) (round to nearest even, saturating); a zero row stays finite;
 *   the dequantised value is float(q) * scale.
 * hd must be 64 or 128: anything else is A3V_ERR_SHAPE before any launch.  Every cache / scale pointer 16-B aligned.
 *
 * a3v_kv_quantize_fp8: positions src_pos .. src_pos+S-1 of a bf16 K / V^T pair (k_src [B,Hkv,Smax_src,hd], vt_src
 * [B,Hkv,hd,Smax_src]) -> positions dst_pos .. dst_pos+S-1 of the fp8 caches and their scales, one launch for S = 1 (decode,
 * Smax_src = 1) as for a prefill.  Nothing outside the S positions is written.
 * a3v_kv_dequantize_fp8: positions 0 .. n-1 -> the same positions of a bf16 pair (k_dst [B,Hkv,Smax_dst,hd], vt_dst
 * [B,Hkv,hd,Smax_dst]), each value bf16(float(q) * scale); nothing else is written. */
int a3v_kv_quantize_fp8(const void* k_src, const void* vt_src, int Smax_src, int src_pos, void* k_q, void* vt_q, float* k_scale,
                        float* v_scale, int B, int Hkv, int hd, int S, int Smax, int dst_pos, void* stream);
int a3v_kv_dequantize_fp8(const void* k_q, const void* vt_q, const float* k_scale, const float* v_scale, int Smax, void* k_dst,
                          void* vt_dst, int Smax_dst, int B, int Hkv, int hd, int n, void* stream);
/* Decode attention (one query row per batch row) over an fp8 cache: out[b, h*hd ..] = softmax((q . kq) k_scale softmax_scale) .
 * (vq v_scale) over keys 0 .. Sk-1, every factor applied in fp32.  q bf16 [B, ldq] (head h at column h*hd), out bf16 [B, ldo].
 * Cache positions >= Sk and their scales may hold anything (NaN codes, inf).  scratch: a3v_attention_scratch_floats(B, H, hd, Sk)
 * floats.  counters: NULL = the split partials are merged by a second launch; else B*H zero-initialised ints (left zero) and the
 * last-arriving block of a (batch, head) merges them in the same launch -- both forms give the same bits.
 * a3v_attention_decode_fp8kv_splits: the number of key ranges a (batch, head) is split into (> 1: partials are merged). */
int a3v_attention_decode_fp8kv(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                               const float* v_scale, void* out, int64_t ldo, int B, int Sk, int H, int Hkv, int hd, int Smax,
                               float* scratch, int* counters, void* stream);
int a3v_attention_decode_fp8kv_splits(int B, int H, int Sk);
/* a3v_llama_decode_step over an fp8 KV cache: the same arguments (the k_cache / vt_cache fields of `layers` are not read) plus one
 * a3v_kv8_layer per layer and ONE bf16 staging pair stage_k [B,Hkv,1,hd] / stage_vt [B,Hkv,hd,1] shared by all layers.  Fused
 * form only (a3v_llama_decode_step_form == 2, else A3V_ERR_SHAPE with nothing touched), SIX launches per layer: the qkv GEMV
 * writes the rotated k / v of the new position into the staging pair, a3v_kv_quantize_fp8 (S = 1) moves it to `pos`,
 * a3v_attention_decode_fp8kv reads pos + 1 keys -- the new one from the fp8 cache like every other -- then wo, w1|w3, w2. */
typedef struct a3v_kv8_layer {
  void* k_q;          /* [B,Hkv,Smax,hd] e4m3 */
  void* vt_q;         /* [B,Hkv,hd,Smax] e4m3 */
  float* k_scale;     /* [B,Hkv,Smax] */
  float* v_scale;     /* [B,Hkv,Smax] */
} a3v_kv8_layer;
int a3v_llama_decode_step_kv8(const a3v_llama_layer* layers, const a3v_kv8_layer* kv8, int n_layers, void* h, void* xn, void* qkv,
                              void* att, void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin, void* stage_k,
                              void* stage_vt, int B, int dim, int H, int Hkv, int hd, int ffn, int Smax, int pos, float eps,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Ragged decode (opt-in; no reference counterpart: model/meta.py:413-485 keeps every batch row at one cache position).  Each
 * batch row decodes at its own position; every position array is a DEVICE int32[B].  An idle row (a negative position, or one
 * outside the cache) writes nothing into any cache and its outputs are zeros, never NaN.  These entries take the bf16 KV cache
 * (the fp8 one: "fp8 KV cache on the ragged decode path" below).
 *
 * a3v_rope_kvcache_rows: a3v_rope_kvcache at S = 1 with start_pos = rope_pos0 = pos[b] per row, one launch, bf16 and fp32, the
 * per-element arithmetic of that entry (a row is bit-equal to the uniform call at its position).  pos[b] outside [0, Smax) is an
 * idle row (bounded by the kernel: the host cannot see a device array): its q_out row is zeros.
 * a3v_attention_decode_rows: decode attention over sk[b] keys for row b, 0 < sk[b] <= sk_max <= Smax (strides as a3v_attention
 * with Sq = 1; sk[b] above sk_max is read as sk_max); sk[b] <= 0: the row's output is zeros.  bf16 at hd 64 / 128: the
 * wave-streaming kernel of a3v_attention_decode_fused with the split plan of that entry at Sk = sk_max (counters: B*H
 * zero-initialised ints, left zero; key ranges beyond sk[b] contribute nothing).  fp32 (any hd <= 256; also bf16 at other head
 * dims): one wave per (batch, head), counters unused.  scratch: a3v_attention_scratch_floats(B, H, hd, sk_max) floats.
 * a3v_attention_decode_rows_splits: the number of key ranges of that plan.
 * a3v_generate_step_rows: a3v_generate_step with per-row state and no text_mask (a refilled row was prefilled with its whole
 * prompt).  cur[b] (in/out): the index of tokens[b] this step writes; limit[b]: one past the last writable index; pos_base: the
 * image words in the cache.  A row with stopped[b] set on entry is not touched.  Otherwise: next = argmax (or sampled[b]);
 * tokens[b, cur] = next; stop_pos / stopped / live as a3v_generate_step at cur_pos = cur[b]; cur[b] += 1; cur[b] == limit[b] stops
 * the row (stop_pos stays cur[b]).  Outputs: next_tok[b] (int64) = the id to embed next and pos[b] = pos_base + cur[b] - 1, its
 * cache position, for a row that still runs; 0 and -1 for a row that is stopped on entry or stops in this step.  A cur[b]
 * outside [0, min(limit[b], ld_tok)) stops the row without a write.  Integer work: bit-identical to tests/ragged_ref.py.
 * a3v_llama_decode_step_rows: a3v_llama_decode_step with row b at cache position pos[b] (idle rows: pos[b] < 0), pos_max = the
 * largest of them (host value, 0 <= pos_max < Smax).  Fused form only (a3v_llama_decode_step_rows_form == 2: bf16, fp8 or NF4
 * weight images, 17..32 rows as two chunks; else the form query says 0, the call returns A3V_ERR_SHAPE with nothing touched and
 * the host runs kernel by kernel).  SIX launches per layer: the qkv GEMV with the RMSNorm prologue and a plain store,
 * a3v_rope_kvcache_rows on the qkv buffer in place, a3v_attention_decode_rows over pos[b] + 1 keys (sk_max = pos_max + 1; the kernel
 * adds the one to pos[b] itself, there is no second array), wo, w1|w3, w2.  The GEMV's RoPE epilogue has one position for
 * angle and cache row, so it is not used: q and k are rounded to bf16 once more than in a3v_llama_decode_step (GEMV store, then
 * the rotation's store).  The step therefore equals the per-kernel sequence bit for bit, not the uniform fused step. */
int a3v_rope_kvcache_rows(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                          const float* cos_sin, const int32_t* pos, int B, int H, int Hkv, int hd, int Smax, int dtype, void* stream);
int a3v_attention_decode_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* sk, int sk_max, int B, int H,
                              int Hkv, int hd, const int64_t* strides, float* scratch, int* counters, int dtype, void* stream);
int a3v_attention_decode_rows_splits(int B, int H, int sk_max);
int a3v_generate_step_rows(const float* logits, int64_t ld, const int64_t* sampled, int B, int V, int64_t* tokens, int64_t ld_tok,
                           int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq, const int32_t* stop_off,
                           int n_stop, uint8_t* stopped, int64_t* stop_pos, int32_t* live, int64_t* next_tok, int32_t* pos,
                           void* stream);
int a3v_llama_decode_step_rows(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                               float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos, int pos_max, int B,
                               int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps, void* stream);
int a3v_llama_decode_step_rows_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8);

/* Shared prompt keys (opt-in; parallel sampling: n answers of one prompt decode over ONE stored copy of its keys).  Two more
 * DEVICE int32[B] arrays sit beside sk / pos:
 *   src_row[b]  the cache row that holds row b's shared keys.  A value outside [0, B) is read as b (bounded by the kernel: the
 *               host cannot see a device array).  One level only: the source row's own src_row is never followed.
 *   shared[b]   row b's keys at positions < S_b are read from row src_row[b] of the same K / V^T caches, every other key from its
 *               own row, where S_b = min(shared[b], sk[b]) rounded DOWN to a multiple of 64 (a shared[b] that is no multiple of
 *               64 acts as the multiple below it; one above the row's key count is clamped first, so the keys between the last
 *               64 boundary below sk[b] and sk[b] are the row's own).  shared[b] <= 0 or src_row[b] == b: exactly the plain row.
 * Why 64: the split plan rounds a key range to 64 keys, so every 64-key tile of the walk starts at a multiple of 64 in absolute
 * position and lies wholly in one row; the 16-byte V^T vectors and the clamped re-reads at a range's end never straddle two rows.
 * Positions below S_b of row b's own cache are never read (they may hold anything).  Idle rows (sk[b] <= 0): zeros, as before.
 *
 * a3v_attention_decode_rows_shared: a3v_attention_decode_rows plus the two arrays: the same three forms (bf16 wave-streaming at hd
 * 64 / 128; one wave per (batch, head) for fp32 and for bf16 at other head dims), the same split plan at sk_max, walk, masks,
 * (m, l) merges and combine -- only the base pointer of a tile differs.  BIT-EQUALITY CONTRACT: the output equals
 * a3v_attention_decode_rows on caches in which positions [0, S_b) of row src_row[b] were copied into row b, bit for bit; counters
 * are left zero.  k / vt must hold all B rows (src_row indexes them).  src_row == NULL: the call IS a3v_attention_decode_rows.
 * a3v_kv_copy_span: positions [lo, hi), 0 <= hi - lo < 64, of cache row src_row into the rows dst_rows[0..n_dst) (DEVICE int32;
 * entries outside [0, B) or equal to src_row are skipped) of EVERY layer in one launch: k_ptrs / vt_ptrs are DEVICE arrays of
 * n_layers base pointers of [B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] caches (16-byte aligned, contiguous; hd and Smax multiples of 8),
 * bf16 or fp32.  K rows by 16-byte vectors; V^T runs of hi - lo elements per d row, vector stores where aligned and element by
 * element at the edges.  Nothing outside the span is written.  hi == lo or n_dst == 0 launches nothing.  (A sibling needs
 * [P & ~63, P) of its leader's prompt of P positions in its own row: the part of the prompt behind the last 64 boundary.)
 * a3v_llama_decode_step_rows_shared: a3v_llama_decode_step_rows with the two arrays handed to the attention launch: six launches
 * per layer, the same form query and the same two-chunk rule for 17..32 rows.  src_row[] holds absolute rows of the whole cache:
 * the attention of the chunk that starts at row b0 gets the un-offset cache base, the slices src_row + b0 / shared + b0 / pos + b0
 * and the row offset b0 (batch index b of the launch is cache row b0 + b; src_row is bounded by [0, B) of the whole call), so a
 * sibling in the second chunk may read a leader in the first.  The step writes the new key of row b at pos[b] of its OWN row, so
 * shared[b] <= pos[b] is the caller's to keep (share_prefix hands out P & ~63 <= P <= pos[b]).  Both arrays NULL: a3v_llama_decode_step_rows; one NULL: an error.
 * a3v_llama_decode_step_rows keeps its signature and its bits. */
int a3v_attention_decode_rows_shared(const void* q, const void* k, const void* vt, void* out, const int32_t* sk,
                                     const int32_t* src_row, const int32_t* shared, int sk_max, int B, int H, int Hkv, int hd,
                                     const int64_t* strides, float* scratch, int* counters, int dtype, void* stream);
int a3v_kv_copy_span(const void* const* k_ptrs, const void* const* vt_ptrs, int n_layers, int src_row, const int32_t* dst_rows,
                     int n_dst, int B, int lo, int hi, int Hkv, int hd, int Smax, int dtype, void* stream);
int a3v_llama_decode_step_rows_shared(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                                      float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos,
                                      const int32_t* src_row, const int32_t* shared, int pos_max, int B, int dim, int H, int Hkv,
                                      int hd, int ffn, int Smax, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * Extend prefill (opt-in; a3v_extend.hip; no reference counterpart).  The forward of a row's own SUFFIX tokens over keys that are
 * already cached -- in the row itself or, below a shared length, in another row ("Shared prompt keys" above).  The queries of all
 * rows are PACKED: row b brings nq[b] = q_off[b+1] - q_off[b] of them, rows q_off[b] .. q_off[b+1]-1 of q / out [M, H*hd]
 * (q_off: DEVICE int32[B+1], non-decreasing, within [0, M]; the host cannot see it).  sk[b] (DEVICE int32[B]) is the row's key
 * count AFTER the extend: query j of row b sits at cache position sk[b] - nq[b] + j and sees the keys [0, that position].
 * These entries take the bf16 / fp32 KV cache; no prefill attention reads fp8 keys.
 *
 * a3v_attention_extend_rows: causal attention of the packed queries.  k [B,Hkv,Smax,hd] / vt [B,Hkv,hd,Smax] and the 12 strides
 * as a3v_attention_decode_rows takes them (strides[1] / [2]: q row / head, [10] / [11]: out row / head, [0] and [9] unused; a V^T
 * row and a K head bound sk_max).  src_row / shared: the two arrays of a3v_attention_decode_rows_shared with exactly their
 * meaning and bounding (S_b = min(shared[b], sk[b]) rounded down to 64; a src_row outside [0, B) reads as b; one level only; k / vt
 * hold all B rows).  Both NULL: the plain form.  One NULL: A3V_ERR_ARG.  nq_max / sk_max (host) size the grid.
 * Rows: nq[b] <= 0 or sk[b] <= 0 is an IDLE row: it reads nothing and its out rows are NOT written (they are not zeroed either).
 * nq[b] above nq_max is read as nq_max (the row's first nq_max packed queries), sk[b] above sk_max as sk_max, and a span longer
 * than its keys as the keys: bounded by the kernels, nothing is read outside q_off's rows or a cache row.
 * Forms.  bf16 at hd 64 / 128: the walk of a3v_attention's causal prefill kernel per row -- 128-query tiles from the row's first
 * query, 64-key tiles from position 0, the same LDS-DMA double buffer, MFMA order, lazy rescale and staged O; a key tile starts at
 * a multiple of 64 and S_b is one, so a tile lies wholly in src_row[b]'s cache or wholly in the row's own (the source is a
 * wave-uniform choice between two buffer descriptors).  A row with ONE query takes a3v_attention's Sq == 1 route instead (its
 * two-phase decode kernel and combine under the split plan of B = 1, computed per row on the device): two further launches whose
 * blocks leave at once for every other row.  scratch: a3v_attention_extend_rows_scratch_floats(B, H, hd, sk_max) floats (bf16 at
 * hd 64 / 128 only; q, k, vt, out 16-byte aligned, strides multiples of 8).  fp32 (any hd <= 256; also bf16 at other head dims):
 * one wave per (query, head, row), a3v_attention's generic kernel; scratch unused.
 * BIT-EQUALITY CONTRACT: (a) plain form: row b's out rows equal a3v_attention(B = 1, Sq = nq[b], Sk = sk[b], causal = 1) on that
 * row's slice of q and the caches; (b) shared form: equals the plain form on caches into which positions [0, S_b) of row
 * src_row[b] were copied; (c) src_row == NULL is the plain call; (d) an idle row leaves its out rows untouched.
 * a3v_rope_kvcache_extend: rotates the packed q in place (q_out may be qkv) and writes k / v^T of row b at positions
 * sk[b]-nq[b] .. sk[b]-1 of its OWN cache row ([B,Hkv,Smax,hd] / [B,Hkv,hd,Smax] contiguous): per element a3v_rope_kvcache(B = 1,
 * S = nq[b], start_pos = rope_pos0 = sk[b] - nq[b]) on the row's slice, bit for bit, one launch.  (a3v_rope_kvcache_spans keeps its
 * contract: at most 8 positions per row in a [B*Q] layout.)  A row with nq[b] <= 0, nq[b] > nq_max, sk[b] < nq[b] or sk[b] > Smax
 * is idle: nothing of it is written, neither q_out rows nor cache.  Nothing outside the spans is written. */
int64_t a3v_attention_extend_rows_scratch_floats(int B, int H, int hd, int sk_max);
int a3v_attention_extend_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* q_off, const int32_t* sk,
                              const int32_t* src_row, const int32_t* shared, int nq_max, int sk_max, int B, int H, int Hkv, int hd,
                              const int64_t* strides, float* scratch, int dtype, void* stream);
int a3v_rope_kvcache_extend(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                            const float* cos_sin, const int32_t* q_off, const int32_t* sk, int nq_max, int B, int H, int Hkv, int hd,
                            int Smax, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * fp8 KV cache on the ragged decode path (opt-in; a3v_kv8_rows.hip).  The arrays are those of "fp8 KV cache" above (k_q, vt_q,
 * k_scale, v_scale of one layer; Smax % 64 == 0; every pointer 16-B aligned), the position arrays those of "Ragged decode" (DEVICE
 * int32[B]; an idle row writes nothing into any cache array and its outputs are zeros, never NaN).  bf16 model, hd 64 or 128:
 * anything else is A3V_ERR_SHAPE before any launch.
 *
 * a3v_rope_kvquant_rows: the per-row RoPE and the quantising cache write in ONE launch.  qkv [B, ldqkv] bf16 as the plain-store qkv
 * GEMV leaves it (q heads, k heads, v heads).  For a running row (0 <= pos[b] < Smax): q is rotated at pos[b] into q_out (may be
 * qkv: in place) with a3v_rope_kvcache_rows' arithmetic; k is rotated and rounded to bf16; that bf16 k row and the bf16 v row are
 * quantised per kv-head with a3v_kv_quantize_fp8's arithmetic (scale = max(amax, 1e-12) / 448, a true division, e4m3 round to
 * nearest even, saturating) and written at position pos[b] of the row's own cache: hd K bytes, hd single V^T bytes (one per d row,
 * column pos[b]) and the two scales.  BIT CONTRACT: q_out, the codes and the scales equal a3v_rope_kvcache_rows into a bf16 cache
 * followed by a3v_kv_quantize_fp8 (S = 1) of that position.  Nothing outside position pos[b] of row b is written.  An idle row
 * (pos[b] < 0 or >= Smax, bounded in the kernel) writes nothing to any cache array and its q_out row is zeros.
 *
 * a3v_attention_decode_rows_fp8kv: a3v_attention_decode_fp8kv over sk[b] keys for row b, 0 < sk[b] <= sk_max <= Smax (sk[b] above
 * sk_max is read as sk_max; sk[b] <= 0: the row's output is zeros).  The walk, the fp32 products score = (q . kq) k_scale
 * softmax_scale and p v_scale, and the masks by select are that entry's; the split plan is a3v_attention_decode_plan's at
 * Sk = sk_max, a key range beyond sk[b] contributes (m, l) = (-inf, 0) and still arrives at the combine.  counters: B*H
 * zero-initialised ints, required, left zero.  scratch: a3v_attention_scratch_floats(B, H, hd, sk_max) floats.  CONTRACTS: (a) with
 * one key range a row is bit-equal to a3v_attention_decode_fp8kv at Sk = sk[b]; (b) with every row at sk_max the launch is bit-equal
 * to the uniform one.  a3v_attention_decode_rows_fp8kv_splits: the number of key ranges of that plan.
 * a3v_attention_decode_rows_fp8kv_shared: plus src_row / shared of "Shared prompt keys" (the same rule: S_b = min(shared[b], sk[b])
 * rounded down to 64, src_row outside [0, B) read as b, one level only).  Below S_b all FOUR streams of row b -- K bytes, V^T
 * bytes, k_scale and v_scale -- come from row src_row[b]; a tile starts at a multiple of 64 and a 16-B V^T load is 16 keys, so
 * nothing straddles two rows.  (c) The output equals the plain entry on caches into which bytes AND scales of [0, S_b) of row
 * src_row[b] were copied into row b, bit for bit; positions below S_b of row b's own arrays are never read.  (d) src_row == NULL:
 * the call IS the plain one.
 *
 * a3v_kv8_copy_span: a3v_kv_copy_span for the fp8 cache: positions [lo, hi), 0 <= hi - lo < 64, of cache row src_row into the rows
 * dst_rows[0..n_dst) (DEVICE int32; entries outside [0, B) or equal to src_row are skipped) of EVERY layer in one launch -- K bytes,
 * V^T byte runs and both scale runs.  k_ptrs / vt_ptrs / ks_ptrs / vs_ptrs: DEVICE arrays of n_layers base pointers.  Vector stores
 * where aligned, elements at the edges; nothing outside the span is written.  hi == lo or n_dst == 0 launches nothing.
 *
 * a3v_llama_decode_step_rows_kv8: a3v_llama_decode_step_rows[_shared] over the fp8 caches of `kv8` (the k_cache / vt_cache fields
 * of `layers` are not read).  src_row / shared: both or neither.  Fused form only (a3v_llama_decode_step_rows_kv8_form == 2: bf16,
 * fp8 or NF4 weight images; else the query says 0, the call returns A3V_ERR_SHAPE with nothing touched and the host runs kernel by
 * kernel).  SIX launches per layer: the qkv GEMV with the RMSNorm prologue and a plain store, a3v_rope_kvquant_rows on the qkv buffer
 * in place, the fp8 rows attention over pos[b] + 1 keys (sk_max = pos_max + 1; the kernel adds the one itself), wo, w1|w3, w2.
 * 17..32 rows run as two chunks; the attention of the chunk at row b0 gets the un-offset bases of all four arrays, the slices at b0
 * and the row offset, so a sibling in the second chunk may read a leader in the first.  The step equals the per-kernel sequence of
 * the entries above bit for bit.  Everything the stage's launches would refuse (H % Hkv, the alignment of qkv and of the four arrays
 * of every layer) is refused by the entry itself, before its first launch.  As in a3v_llama_decode_step_rows, the idle row of the
 * step is pos[b] < 0: a pos[b] >= Smax (which pos_max < Smax excludes for a caller that keeps pos_max honest) is idle for the write
 * but is read by the attention as sk_max keys, so that row's output is not zeros; it is the caller's to keep pos[b] <= pos_max. */
int a3v_rope_kvquant_rows(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_q, void* vt_q, float* k_scale,
                          float* v_scale, const float* cos_sin, const int32_t* pos, int B, int H, int Hkv, int hd, int Smax,
                          void* stream);
int a3v_attention_decode_rows_fp8kv(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                                    const float* v_scale, void* out, int64_t ldo, const int32_t* sk, int sk_max, int B, int H,
                                    int Hkv, int hd, int Smax, float* scratch, int* counters, void* stream);
int a3v_attention_decode_rows_fp8kv_shared(const void* q, int64_t ldq, const void* k_q, const void* vt_q, const float* k_scale,
                                           const float* v_scale, void* out, int64_t ldo, const int32_t* sk, const int32_t* src_row,
                                           const int32_t* shared, int sk_max, int B, int H, int Hkv, int hd, int Smax,
                                           float* scratch, int* counters, void* stream);
int a3v_attention_decode_rows_fp8kv_splits(int B, int H, int sk_max);
int a3v_kv8_copy_span(const void* const* k_ptrs, const void* const* vt_ptrs, const void* const* ks_ptrs, const void* const* vs_ptrs,
                      int n_layers, int src_row, const int32_t* dst_rows, int n_dst, int B, int lo, int hi, int Hkv, int hd,
                      int Smax, void* stream);
int a3v_llama_decode_step_rows_kv8(const a3v_llama_layer* layers, const a3v_kv8_layer* kv8, int n_layers, void* h, void* xn,
                                   void* qkv, void* att, void* act, float* attn_scratch, void* skinny_ws, const float* cos_sin,
                                   const int32_t* pos, const int32_t* src_row, const int32_t* shared, int pos_max, int B, int dim,
                                   int H, int Hkv, int hd, int ffn, int Smax, float eps, void* stream);
int a3v_llama_decode_step_rows_kv8_form(int B, int dim, int H, int Hkv, int hd, int ffn, int w8);

/* ---------------------------------------------------------------------------------------
 * Lookup decoding (opt-in; a3v_spec.hip; no reference counterpart).  One decode step feeds Q = D + 1 query positions per cache row,
 * 1 <= Q <= 8: the row's last emitted token and up to D drafted ones, and keeps the longest prefix of the drafts that the model
 * itself produces (greedy: the answer is the plain loop's).  B cache rows, B * Q <= 32 GEMV rows.  VIRTUAL ROW m = b * Q + j is
 * query j of cache row b: activations (qkv, att, logits) are [B * Q, ...], caches are [B, ...].  pos[b] (the cache position of
 * query 0; negative: idle row) and nq[b] (live queries of the row, 1 <= nq[b] <= Q: one for the last emitted token plus its
 * drafts) are DEVICE int32[B].  Query j of row b is LIVE when pos[b] >= 0, j < nq[b] and pos[b] + j < Smax (attention: < sk_max);
 * any other query is idle: it writes nothing into a cache and its outputs are zeros, never NaN.  bf16 KV cache only.
 * INVARIANT: a step writes the keys of positions pos[b] .. pos[b] + nq[b] - 1.  When only e of them are kept (a3v_accept_rows), the
 * next step starts at pos[b] + e: the keys behind it are never read (every query masks at its own count) and are overwritten.
 *
 * a3v_rope_kvcache_spans: qkv [B*Q, ldqkv]; virtual row m is rotated with the angle of position pos[b] + j, and its K row / V^T
 * column are written at that position of cache row b; an idle query writes nothing and gets a zero q row (bounded by the kernel).
 * bf16 and fp32.  Per live virtual row bit-equal to a3v_rope_kvcache_rows at that position.
 * a3v_attention_verify_rows: query j of row b attends to keys [0, pos[b] + j + 1) of cache row b (the causal mask among the drafts
 * is the key count).  strides as a3v_attention with Sq = 1, where the batch strides of q and out ([0], [9]) step VIRTUAL rows and
 * those of k and vt ([3], [6]) cache rows.  sk_max >= the largest key count (host value, pos_max + Q clamped to Smax); a query whose
 * position is >= sk_max is idle.  bf16 at hd 64 / 128: one block per (cache row, group of queries, head, key range); the group is
 * the power of two >= Q, at most 8 (hd 64) or 4 (hd 128: Q = 5..8 run as two groups of 4); every 32-key K tile and V^T tile of the
 * range is loaded once (non-temporal) and applied to all queries of the group, each with its own key-count mask by select, its own
 * (m, l) and its own output; split plan of a3v_attention_decode_rows at (B, H, sk_max); partials merged by the last-arriving block.
 * A key at or beyond a query's count (NaN, a rejected draft of an earlier step, the key of a later draft) never reaches its sums;
 * a query's output bits do not depend on whether later queries of its row are live.  scratch:
 * a3v_attention_verify_rows_scratch_floats(B, Q, H, hd, sk_max) floats; counters: 2 * B * H zero-initialised ints, left zero.
 * fp32, and bf16 at other head dims <= 256: one wave per (virtual row, head), bit-equal per live query to
 * a3v_attention_decode_rows in its one-wave form with sk = pos[b] + j + 1; scratch / counters unused.
 * a3v_attention_verify_rows_splits: the number of key ranges of the plan.
 * a3v_lookup_draft_rows (integer work, bit-identical to tests/spec_ref.py): prompt lookup.  For a running row (stopped[b] == 0,
 * pos[b] >= 0, 1 <= cur[b] <= ld_tok) with c = tokens[b, 0 .. cur[b]): for n = min(max_ngram, cur - 1) down to 1, the LARGEST i
 * with i + n <= cur - 1 and c[i .. i+n) == c[cur-n .. cur); the first n with a match wins, the drafts are c[i+n ..] and
 * nd = max(0, min(D, cur - (i+n), limit[b] - 1 - cur[b], Smax - 1 - pos[b])).  No match, or a row that is not running: nd = 0.
 * x [B, Q] int64 (Q = D + 1): x[b, 0] = next_tok[b], x[b, 1 .. nd] = the drafts, the rest 0; nq[b] = 1 + nd.  0 <= D <= 7.
 * a3v_accept_rows (integer work on the argmax, bit-identical to tests/spec_ref.py; greedy only): logits fp32 [B*Q, V] (row stride
 * ld).  A row with stopped[b] set is not touched (next_tok 0, pos -1).  Otherwise nd = clamp(nq[b], 1, Q) - 1, t_j = argmax of
 * virtual row (b, j), first index on ties (as a3v_generate_step_rows); the row emits t_0, then t_j while j <= nd and
 * t_{j-1} == x[b, j].  Every emission is exactly one token step of a3v_generate_step_rows at cur[b] with sampled = t_j (the token
 * write, stop sequences, cur += 1, the limit); a stop ends the row's emissions.  Outputs as that entry's: next_tok[b] = the last
 * emitted id and pos[b] = pos_base + cur[b] - 1 for a row that still runs, 0 and -1 for one that stopped.  stats (may be NULL):
 * DEVICE int64[2]; every row that emits adds nd to stats[0] (drafted) and emissions - 1 to stats[1] (accepted).
 * a3v_llama_decode_step_verify: a3v_llama_decode_step_rows over the B * Q virtual rows with a3v_rope_kvcache_spans and
 * a3v_attention_verify_rows (sk_max = min(pos_max + Q, Smax)) in place of the rows kernels: six launches per layer.  Up to 16
 * virtual rows run as one chunk; above that the step runs in chunks of floor(16 / Q) whole cache rows, so the rope and attention
 * launches of a chunk see whole cache rows (two chunks for B * Q = 32 at Q = 2, 4, 8).  attn_scratch:
 * a3v_attention_verify_rows_scratch_floats of the largest chunk.  Fused form only (a3v_llama_decode_step_verify_form == 2: the GEMV
 * forms of a3v_llama_decode_step_rows_form at a chunk's row count -- bf16, fp8 or NF4 images; else the query says 0, the call
 * returns A3V_ERR_SHAPE with nothing touched and the host runs kernel by kernel).  Bit-equal to the per-kernel sequence of public
 * entries over the same chunks. */
int a3v_rope_kvcache_spans(const void* qkv, int64_t ldqkv, void* q_out, int64_t ldq, void* k_cache, void* vt_cache,
                           const float* cos_sin, const int32_t* pos, const int32_t* nq, int B, int Q, int H, int Hkv, int hd, int Smax,
                           int dtype, void* stream);
int a3v_attention_verify_rows(const void* q, const void* k, const void* vt, void* out, const int32_t* pos, const int32_t* nq,
                              int sk_max, int B, int Q, int H, int Hkv, int hd, const int64_t* strides, float* scratch, int* counters,
                              int dtype, void* stream);
int a3v_attention_verify_rows_splits(int B, int H, int sk_max);
int64_t a3v_attention_verify_rows_scratch_floats(int B, int Q, int H, int hd, int sk_max);
int a3v_lookup_draft_rows(const int64_t* tokens, int64_t ld_tok, const int32_t* cur, const int32_t* limit, const int32_t* pos,
                          const uint8_t* stopped, const int64_t* next_tok, int B, int D, int max_ngram, int Smax, int64_t* x,
                          int32_t* nq, void* stream);
int a3v_accept_rows(const float* logits, int64_t ld, int B, int Q, int V, const int64_t* x, const int32_t* nq, int64_t* tokens,
                    int64_t ld_tok, int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq, const int32_t* stop_off,
                    int n_stop, uint8_t* stopped, int64_t* stop_pos, int64_t* next_tok, int32_t* pos, int64_t* stats, void* stream);
int a3v_llama_decode_step_verify_form(int B, int Q, int dim, int H, int Hkv, int hd, int ffn, int w8);
int a3v_llama_decode_step_verify(const a3v_llama_layer* layers, int n_layers, void* h, void* xn, void* qkv, void* att, void* act,
                                 float* attn_scratch, void* skinny_ws, const float* cos_sin, const int32_t* pos, const int32_t* nq,
                                 int pos_max, int B, int Q, int dim, int H, int Hkv, int hd, int ffn, int Smax, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * Generation controls (opt-in; a3v_genctl.hip): a log-probability per generated token and the HF repetition penalty, on the
 * device inside the step.  No existing entry changes; with the options off none of these is launched.
 *
 * Seen set: one bitmap per cache row, uint32 [R, words_per_row], words_per_row >= ceil(V / 32) (the row stride in words).  Token
 *   t is bit t & 31 of word t >> 5.  It holds the row's prompt TEXT tokens and every token generated so far (the scope of HF's
 *   RepetitionPenaltyLogitsProcessor: the whole input_ids); image words are not tokens and are never in it.  Ids outside [0, V)
 *   are ignored, never written.
 * Penalty p > 0 over the raw fp32 logits z of a row:  z'[t] = z[t] / p if t is seen and z[t] > 0;  z[t] * p if t is seen and
 *   z[t] <= 0;  z[t] otherwise.  The division is a true fp32 division (not a reciprocal multiply): the bits are torch's.  It is
 *   applied BEFORE temperature and top-p (HF order: processors, then warpers): the sampler / the step kernel read z'.  Greedy is
 *   the first-index argmax of z'.  NaN and +-inf pass through the same two expressions.
 * Log-prob: lp = z[tok] - logsumexp(z) on the RAW logits at temperature 1 -- the model's own probability, whatever penalty,
 *   temperature and nucleus chose the token.  fp32, max-subtracted.  One value per generated token.  The sequence score is the
 *   sum of lp over the kept tokens of an answer (up to, not including, the stop position, as the text is cut), taken on the
 *   host in fp64 from the device array, read back once.
 *   Reduction order of logsumexp (one 1024-thread block per row, ONE pass): thread t owns the 4-element vectors t, t + 1024, ...
 *   of the row in ascending order, then element 4 (V / 4) + t of the tail (a row whose address -- or whose out row's -- is not
 *   16-byte aligned: single elements t, t + 1024, ...).  Per vector, with the running pair (m, s) of the thread:
 *   M = max(m, x0..x3); s = s * exp(m - M) + (((e0 + e1) + e2) + e3), e_j = exp(x_j - M); m = M.  Per wave: M_w = max of m;
 *   s *= exp(m - M_w); S_w = butterfly sum of s (lanes ^32, ^16, ^8, ^4, ^2, ^1).  Block: M = max of the 16 M_w;
 *   S = sum over w = 0..15 in order of S_w * exp(M_w - M); lse = M + log(S).  exp / log are expf / logf (<= 1 ulp), an infinite
 *   maximum is replaced by 0 as the exponent offset (no inf - inf), an empty partial sum stays 0.  The bound that follows from
 *   this shape is written out in tests/genctl_ref.py (lse_bound).
 *
 * a3v_seen_mark: seen[b] |= bits of tokens[b, 0 .. min(lens[b], ld_tok)) for every row in one launch (vector atomicOr);
 *   lens[b] <= 0 leaves the row alone.  The prompt marking.
 * a3v_seen_clear_rows: zero the first n_words (<= words_per_row) words of the bitmap rows rows[0 .. n_rows) (device int32; an entry
 *   outside [0, R) is skipped).
 * a3v_logits_prepare: logits fp32 [B, V] (row stride ld), never written.  seen != NULL: out [B, V] (row stride ld_out, must not
 *   alias logits) = the penalised rows; seen == NULL: out is not touched.  lse != NULL: lse[b] = logsumexp of the RAW row; NULL:
 *   not computed.  One of the two must be asked for.  Any V.
 * a3v_generate_record: runs AFTER a3v_generate_step / a3v_generate_step_rows has written the chosen id.  Per row b:
 *   column c = col (cur == NULL: the uniform step, col = the cur_pos of a3v_generate_step), or c = cur[b] - 1 (ragged:
 *   generate_step_rows_kernel writes tokens[b, cur[b]] and THEN advances cur[b], so after it the id sits one column back).
 *   generated index g = c - prompt_len[b] (prompt_len != NULL), else idx.  id = tokens[b, c];
 *   logprob[b, g] = logits[b, id] - lse[b] (one fp32 subtraction; logprob [B, n_lp], row stride ld_lp, may be NULL; g >= n_lp is not written);
 *   bit id of seen[b] is set (seen may be NULL).  Nothing is written and nothing is marked for a row with stopped_before[b] set
 *   (the snapshot of `stopped` taken before the step; NULL: no row is skipped for it), with c outside [0, ld_tok) (an idle
 *   ragged row), with g < 0 (a teacher-forced prompt position of a3v_generate_step: marked up front, never scored) or with an
 *   id outside [0, V).  The ragged step kernel can also stop a row WITHOUT a write (cur[b] outside its range); such a row must be
 *   passed as stopped_before by the caller -- generate_many never makes one (a prompt with nothing to write gets no row).
 * ------------------------------------------------------------------------------------- */
int a3v_seen_mark(const int64_t* tokens, int64_t ld_tok, const int32_t* lens, uint32_t* seen, int64_t words_per_row, int B, int V,
                  void* stream);
int a3v_seen_clear_rows(uint32_t* seen, const int32_t* rows, int n_rows, int64_t words_per_row, int64_t n_words, int R, void* stream);
int a3v_logits_prepare(const float* logits, int64_t ld, const uint32_t* seen, int64_t words_per_row, float penalty, float* out,
                       int64_t ld_out, float* lse, int B, int V, void* stream);
int a3v_generate_record(const float* logits, int64_t ld, const float* lse, const int64_t* tokens, int64_t ld_tok, int col,
                        const int32_t* cur, const uint8_t* stopped_before, uint32_t* seen, int64_t words_per_row, float* logprob,
                        int64_t ld_lp, int n_lp, int idx, const int32_t* prompt_len, int B, int V, void* stream);

/* ---------------------------------------------------------------------------------------
 * Constrained decoding (opt-in; a3v_constrain.hip): every step's choice is restricted to the tokens that can still lead to a full
 * match of a regular expression.  No existing entry changes; without a constraint none of these is launched.
 *
 * Token automaton (built on the host, model/constrain.py): trans int16 [n_states, V], row-major, 1 <= n_states <= 32767.
 *   trans[s, v] = the state after token v from state s, or -1 when v is not allowed in s (its text leaves the language, it
 *   contributes no text, or it is the end-of-sequence id in a state that does not accept).  The end-of-sequence id leads from an
 *   accepting state to a last state DONE in which only that id is allowed.  The host refuses an automaton with a reachable state
 *   that allows no token, so a masked row always keeps at least one finite entry.
 * State: device int32 [B], one per cache row.  A value outside [0, n_states) marks an UNCONSTRAINED row: the mask leaves its logits
 *   alone and the advance leaves its state alone.  The kernels bound the state themselves (the host never reads it).
 * Step order: a3v_logits_prepare (repetition penalty) -> a3v_constrain_logits -> sampler / argmax -> the token write of
 *   a3v_generate_step / a3v_generate_step_rows -> a3v_generate_record on the RAW logits -> a3v_constrain_advance.  The scores stay
 *   the unconstrained model's log-probabilities.
 *
 * a3v_constrain_logits: logits / out fp32 [B, V] (row strides ld >= V, ld_out >= V, any value: rows need not be 16-byte aligned);
 *   out == logits with ld_out == ld is the in-place form, any other overlap is undefined.  Row b with 0 <= state[b] < n_states:
 *   out[b, v] = logits[b, v] where trans[state[b], v] >= 0 -- the input's bit pattern, NaN payloads included -- and -inf elsewhere.
 *   Any other state[b]: the row is copied unchanged.  Columns [V, ld_out) are never written.  Any V >= 1; one launch.
 *   The -inf entries are safe for every consumer: a3v_argmax and the step kernels start from -inf with a first-index tie break, so a
 *   finite entry always wins; a3v_sample_top_p / a3v_sample_top_k_p give such a token the mass expf(-inf) = 0 exactly, and their
 *   selection only ever lands on a bin of positive mass (a3v_common.h, topp_select); top-k ranks -inf below every finite value and
 *   min-p > 0 removes a zero mass.
 * a3v_constrain_advance: runs AFTER the step kernel has written the chosen id (and after a3v_generate_record, which it does not
 *   depend on).  Column c = col (cur == NULL: the uniform step), or cur[b] - 1 (the rows form, after a3v_generate_step_rows has
 *   advanced cur).  Nothing changes for a row with stopped_before[b] set (may be NULL), with c outside [0, ld_tok), with
 *   c < first[b] (first: device int32 [B], the index of the row's first generated token: below it the column holds a teacher-forced
 *   prompt token of generate), with a state outside [0, n_states) or with an id outside [0, V).  Otherwise
 *   state[b] = trans[state[b], tokens[b, c]].  Integer work: bit-identical to the restatement in tests/constrain_ref.py.
 * Both return A3V_ERR_ARG for a NULL array, B <= 0, V <= 0, n_states outside [1, 32767], a stride below V, ld_tok <= 0 or (uniform
 *   form) col outside [0, ld_tok); nothing is launched on an error.
 * ------------------------------------------------------------------------------------- */
int a3v_constrain_logits(const float* logits, int64_t ld, const int16_t* trans, int V, int n_states, const int32_t* state, float* out,
                         int64_t ld_out, int B, void* stream);
int a3v_constrain_advance(const int64_t* tokens, int64_t ld_tok, int col, const int32_t* cur, const int32_t* first,
                          const uint8_t* stopped_before, const int16_t* trans, int V, int n_states, int32_t* state, int B, void* stream);

/* ---------------------------------------------------------------------------------------
 * Lookup decoding: sample and match (opt-in; a3v_spec_ctl.hip; generate_many(lookup=D, lookup_verify="choice")).  Lookup decoding
 * under temperature / top-k / top-p / min-p, the repetition penalty, log-probs and a constraint.  No existing entry changes: the
 * verify step, a3v_accept_rows, the samplers and a3v_argmax are called as they are.
 *
 * Rule: the plain loop draws generated token g of an answer with one fixed uniform number, from the row's prepared logits (penalty,
 *   then the constraint mask, then the sampler's filters).  For query j of a row (virtual row m = b * Q + j) the logits are prepared
 *   exactly as the plain loop would prepare them if drafts x[b, 1..j] had been emitted, the draw uses the uniform of generated index
 *   g + j, and draft j + 1 is accepted if and only if the draw equals it.  The emitted tokens are the plain loop's for the same
 *   uniforms (at temperature 0: the first-index argmax of the prepared row), so no rejection sampling is needed.
 * Step order: a3v_lookup_draft_rows -> a3v_llama_decode_step_verify -> a3v_verify_prepare -> a3v_sample_top_p / a3v_sample_top_k_p /
 *   a3v_argmax over the B * Q rows of `out` -> a3v_accept_rows_chosen.
 *
 * a3v_verify_prepare: logits fp32 [B*Q, V] (row stride ld >= V), never written; out fp32 [B*Q, V] (row stride ld_out >= V; out ==
 *   logits is refused, any other overlap is undefined); x int64 [B, Q], nq / pos device int32 [B] as in the verify step.  Query j
 *   of row b is LIVE when pos[b] >= 0 and j < clamp(nq[b], 1, Q).  For a live query, in this order:
 *   1. seen set = seen[b] (the bitmap of "Generation controls", uint32 [B, words_per_row], one row per CACHE row) united with
 *      x[b, 1..j]; x[b, 0] is already in the bitmap (the step that emitted it marked it).  The drafts are compared per element, no
 *      [B*Q, words] bitmap exists; a draft id outside [0, V) is ignored.  seen == NULL: no penalty.
 *   2. penalty: a3v_logits_prepare's two expressions on the raw value, a true fp32 division.
 *   3. constraint state: s_0 = state[b], s_k = trans[s_{k-1}, x[b, k]] for k = 1..j.  s_0 outside [0, n_states): the row is
 *      unconstrained for every j.  If the walk meets -1 (or a state >= n_states), or a draft id outside [0, V), the query is DEAD:
 *      its out row is all -inf.  A dead query is never examined by a3v_accept_rows_chosen: from s_{k-1} the token x[b, k] is masked
 *      in the out row of query k - 1, so it lies below every finite entry for the argmax and has mass expf(-inf) = 0 for the
 *      samplers, whose selection only lands on a bin of positive mass (see a3v_constrain_logits above); the choice of query k - 1
 *      therefore differs from x[b, k] and the chain of acceptances breaks before query k.  trans == NULL: no mask.
 *   4. mask: a3v_constrain_logits's select in state s_j on the penalised value; a kept value keeps its bit pattern.
 *   5. lse[m] (lse != NULL) = logsumexp of the RAW row in the reduction order fixed above for a3v_logits_prepare (1024-thread
 *      block, one pass): bit-equal to that entry's lse on the same logits row with an out row on the same 16-byte phase (both rows
 *      on a 16-byte boundary: the vector walk, and then also its lse-only form; otherwise the element walk).  Dead queries included.
 *   An idle query gets an out row of zeros and lse 0; its logits row is not read.  Any V >= 1; out rows off the 16-byte boundary
 *   take the element form.  One launch, B * Q blocks of 1024 threads, 16-byte loads and stores, 8-byte loads of the int16 row.
 *   A3V_ERR_ARG: a NULL array among logits / x / nq / pos / out, out == logits, B <= 0, V <= 0, a stride below V, seen with
 *   penalty <= 0 or words_per_row < ceil(V / 32), trans without state or n_states outside [1, 32767].  A3V_ERR_SHAPE: Q outside 1..8.
 * a3v_accept_rows_chosen: a3v_accept_rows with t_j = chosen[b * Q + j] (int64 [B*Q]: the samplers' or a3v_argmax's output over the
 *   rows of `out`) -- the emission rule, the token write, stop sequences, cur, limit, next_tok, pos and stats are that entry's.  For
 *   every emission, the one that stops the row included, with id at column c and generated index g = c - prompt_len[b] >= 0 and
 *   0 <= id < V (a3v_generate_record's and a3v_constrain_advance's guards; prompt_len is also the `first` of the latter):
 *   logprob[b, g] = logits[m, id] - lse[m], one fp32 subtraction on the RAW logits of the query m that produced it (g >= n_lp is not
 *   written); bit id of seen[b] is set; state[b] = trans[state[b], id] when state[b] is in [0, n_states).  logprob, seen and state
 *   are each optional (NULL); with any of them prompt_len and V are required.  A row with stopped[b] set is not touched.  With all
 *   three NULL and chosen the argmax of the logits, every output equals a3v_accept_rows's bit for bit.  Integer work apart from the
 *   one subtraction: bit-identical to tests/spec_ctl_ref.py.
 * a3v_verify_uniforms: u[b * Q + j] = uni[clamp(row_base[b] + (cur[b] - prompt_len[b]) + j, 0, n_uni - 1)]: the plain loop's uniform
 *   of the generated index each query would emit at (row_base: device int64 [B], the index of the row's answer in uni).
 * ------------------------------------------------------------------------------------- */
int a3v_verify_prepare(const float* logits, int64_t ld, int B, int Q, int V, const int64_t* x, const int32_t* nq, const int32_t* pos,
                       const uint32_t* seen, int64_t words_per_row, float penalty, const int16_t* trans, int n_states,
                       const int32_t* state, float* lse, float* out, int64_t ld_out, void* stream);
int a3v_accept_rows_chosen(const int64_t* chosen, int B, int Q, const int64_t* x, const int32_t* nq, int64_t* tokens, int64_t ld_tok,
                           int32_t* cur, const int32_t* limit, int pos_base, const int64_t* stop_seq, const int32_t* stop_off,
                           int n_stop, uint8_t* stopped, int64_t* stop_pos, int64_t* next_tok, int32_t* pos, int64_t* stats,
                           const float* logits, int64_t ld, int V, const float* lse, float* logprob, int64_t ld_lp, int n_lp,
                           const int32_t* prompt_len, uint32_t* seen, int64_t words_per_row, const int16_t* trans, int n_states,
                           int32_t* state, void* stream);
int a3v_verify_uniforms(const float* uni, int64_t n_uni, const int64_t* row_base, const int32_t* cur, const int32_t* prompt_len, int B,
                        int Q, float* u, void* stream);

/* ---------------------------------------------------------------------------------------
 * Beam search (opt-in; a3v_beam.hip; no reference counterpart; tests/beam_ref.py restates select and advance, bit for bit).
 * Groups of K = num_beams consecutive cache rows, 1 <= K <= 8: group g of G owns rows [g K, g K + K), R = G K.  Everything per row
 * and per group lives on the DEVICE; no entry reads anything back.
 *   per row:   cum[R] fp32 (sum of raw log-probs), alive[R] uint8, state[R] int32 (the automaton state of a3v_constrain_*; a value
 *              outside [0, n_states) = unconstrained), token rows [R, ld_tok] int64 (the GENERATED ids only), parent[R] / pos[R]
 *              int32, next_tok[R] int64.
 *   per group: glen[G] (ids generated so far), limit[G] (ids it may generate), base[G] (cache position of generated id 0: image
 *              words + prompt length), done[G] uint8, and a pool of at most K finished hypotheses: pool_n[G], pool_added[G] (entries
 *              ever accepted: the source of pool_seq), pool_score / pool_cum [G, K] fp32, pool_len / pool_seq [G, K] int32,
 *              pool_ids [G, K, ld_tok] int64 (without the EOS id).  Pool slots are in no order: the host sorts by (score
 *              descending, seq ascending).
 * a3v_beam_select: one 1024-thread block per group.  Candidate (beam b, token v) of a row with alive != 0 is allowed when trans is
 *   NULL, or the row's state is outside [0, n_states), or trans[state, v] >= 0; its score is s = cum[b] + (z[b, v] - lse[b]): two fp32
 *   operations in that order on the RAW logits [R, V] (row stride ld >= V; rows of any alignment: 16-byte loads of a 16-byte
 *   aligned row, single elements otherwise -- a3v_logits_prepare's rule).  s == -inf or NaN is never taken.  Output: the best 2K
 *   candidates of the group, by s descending, then flat index b V + v ascending, into cand_score / cand_beam / cand_tok [G, 2K];
 *   unfilled slots hold (-inf, -1, -1).  The result depends only on that order, not on the reduction shape.  K V < 2^31.
 * a3v_beam_advance: one block per group; a group with done != 0 is not touched.  With L = glen[g] and the effective limit
 *   lim = min(limit[g], ld_tok, n_div - 1, pos_cap - base[g]) (base < 0: 0): L >= lim ends the group at once.  Otherwise the 2K
 *   candidates are walked in rank order; a slot with a score of -inf / NaN, a beam outside [0, K) or a token outside [0, V) is
 *   skipped.  An EOS candidate at rank < K enters the pool with score s / len_div[L] (a true fp32 division; len_div[j] =
 *   fp32(max(j, 1) ** length_penalty), a host table of n_div entries), sum s, length L and the parent's token row; at rank >= K it
 *   is dropped.  A full pool keeps the best K, a tie keeps the earlier entry.  Any other candidate becomes the next live beam
 *   j = 0, 1, .. until K are taken: row g K + j gets parent = g K + b (absolute row), next_tok, cum = s, alive = 1, state' =
 *   trans[state[parent], tok] (an unconstrained parent: its state), pos = base + L (the cache position of the token to embed),
 *   token row = the parent's L ids plus the token (read from tokens_in, written to tokens_out: the caller swaps the two every step).
 *   The rows behind the takers are dead: parent = itself, next_tok = 0, cum = -inf, alive = 0, pos = -1.  glen = L + 1.  The group
 *   is then DONE when no beam is alive; or glen reached lim (first every live beam enters the pool at its sum over len_div[glen],
 *   in beam order); or the pool is full and early_stopping != 0; or the pool is full and cum[beam 0] / len_div[glen] <= the worst
 *   pool score.  A done group's rows get parent = itself, next_tok = 0, alive = 0, pos = -1 and done = 1.
 * a3v_kv_permute_tails: for every row r whose parent[r] != r (a parent outside r's group is read as r), the positions
 *   [tail_lo[r], pos[r]) (clamped to [0, Smax)) of cache row parent[r] replace the same positions of row r, in K [B,Hkv,Smax,hd] and
 *   V^T [B,Hkv,hd,Smax] of EVERY layer in one launch (k_ptrs / vt_ptrs as a3v_kv_copy_span; bf16 or fp32; hd and Smax multiples of
 *   8).  All rows read the values from before the call: a thread owns one 16-byte offset for all K rows of a group, reads the K
 *   vectors, passes the barrier and writes every row from its parent's copy, so several rows may name one parent and a parent may
 *   itself be overwritten.  tail_max (host value) sizes the grid: it must be >= max(pos) - min(tail_lo) over the MOVED rows of
 *   every group (the longest span when all rows of a group share one span, as beam search has it); positions of a group behind
 *   min(tail_lo) + tail_max are not moved.  16-byte
 *   stores; V^T vectors that straddle an edge of the span element by element.  Nothing outside the spans is written.  tail_max == 0
 *   launches nothing. */
int a3v_beam_select(const float* logits, int64_t ld, const float* lse, const float* cum, const uint8_t* alive, const int16_t* trans,
                    int n_states, const int32_t* state, int G, int K, int V, float* cand_score, int32_t* cand_beam, int32_t* cand_tok,
                    void* stream);
int a3v_beam_advance(const float* cand_score, const int32_t* cand_beam, const int32_t* cand_tok, int G, int K, int V, int eos,
                     int early_stopping, const float* len_div, int n_div, const int16_t* trans, int n_states, const int32_t* base,
                     const int32_t* limit, int pos_cap, float* cum, uint8_t* alive, int32_t* state, int32_t* glen, uint8_t* done,
                     int32_t* parent, int64_t* next_tok, int32_t* pos, const int64_t* tokens_in, int64_t* tokens_out, int64_t ld_tok,
                     int32_t* pool_n, int32_t* pool_added, float* pool_score, float* pool_cum, int32_t* pool_len, int32_t* pool_seq,
                     int64_t* pool_ids, void* stream);
int a3v_kv_permute_tails(const void* const* k_ptrs, const void* const* vt_ptrs, int n_layers, const int32_t* parent,
                         const int32_t* tail_lo, const int32_t* pos, int tail_max, int G, int K, int Hkv, int hd, int Smax, int dtype,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * Training (backward) entry points. Reference: autograd through the same modules under
 * autocast(bf16) with fp32 master weights (engine_finetune.py:44-68, main_finetune.py:212-217).
 * Convention: activations and their grads use `act_dtype` (bf16 / f32 parity); the residual
 * stream h, master weights and weight grads are fp32.  GEMM-shaped backward work goes through
 * a3v_gemm_nt on transposed images built with a3v_transpose.
 * ------------------------------------------------------------------------------------- */

/* a3v_attention + per-row log-sum-exp lse [B,H,Sq] (fp32) kept for the backward pass. */
int a3v_attention_lse(const void* q, const void* k, const void* vt, void* out, float* lse, int B,
                      int Sq, int Sk, int H, int Hkv, int hd, const int64_t* strides, int causal,
                      int dtype, void* stream);

/* dst[b][c][r] = src[b][r][c] for r < R (zero for R <= r < Rpad); leading dims / batch strides
 * in elements.  Builds W^T for dgrad and X^T / dY^T for wgrad. */
int a3v_transpose(const void* src, int64_t ld_src, int64_t bs_src, void* dst, int64_t ld_dst,
                  int64_t bs_dst, int R, int C, int Rpad, int batch, int dtype, void* stream);

/* backward of a3v_rmsnorm with fp32 x, w: dh += d/dx ; dw += d/dw (may be NULL). dy in act_dtype.
 * dw_scratch (may be NULL): a3v_rmsnorm_bwd_scratch_floats(rows, dim) floats; with it the per-block weight-gradient
 * partials are written as rows and column-summed by a second small kernel instead of ~rows/8 x dim atomics on dw. */
int64_t a3v_rmsnorm_bwd_scratch_floats(int rows, int dim);
int a3v_rmsnorm_bwd(const float* x, int64_t ldx, const float* w, const void* dy, int64_t lddy,
                    float* dh, int64_t lddh, float* dw, float* dw_scratch, int rows, int dim, float eps,
                    int act_dtype, void* stream);
/* The same, and the updated dh also as bf16 (dh_bf16 [rows][ld_bf16]): the operand of the weight / input gradient GEMMs that
 * follow (autograd casts the fp32 stream gradient for the autocast linears, engine_finetune.py:49) without a pass of its own. */
int a3v_rmsnorm_bwd_cast(const float* x, int64_t ldx, const float* w, const void* dy, int64_t lddy,
                         float* dh, int64_t lddh, float* dw, float* dw_scratch, int rows, int dim, float eps,
                         int act_dtype, void* dh_bf16, int64_t ld_bf16, void* stream);

/* bf16 residual stream: under FSDP MixedPrecision(param_dtype = bf16) + autocast (main_finetune.py:241-263, engine_finetune.py:44-50)
 * the reference's embeddings, block outputs and hence the residual stream AND ITS GRADIENT are bf16 tensors; these forms take the
 * stream (x) and the accumulated stream gradient (dh, read-modify-write, rounded to bf16 as autograd rounds it at the residual add) in
 * bf16, with fp32 arithmetic inside.  dy bf16.  Same formulas as a3v_rmsnorm_bwd / a3v_layernorm_bwd / a3v_embed_bwd. */
int a3v_rmsnorm_bwd_bf16(const void* x, int64_t ldx, const float* w, const void* dy, int64_t lddy, void* dh, int64_t lddh,
                         float* dw, float* dw_scratch, int rows, int dim, float eps, void* stream);
int a3v_layernorm_bwd_bf16(const void* x, int64_t ldx, const float* w, const void* dy, int64_t lddy, const int32_t* row_map,
                           void* dx, int64_t lddx, float* dw, float* db, int rows, int dim, float eps, void* stream);
/* a3v_rmsnorm_bwd_bf16 over the rows of a list without repeats: dy row i (compact, i < rows) belongs to x row row_idx[i], and the input
 * gradient is accumulated into dh row row_idx[i]; dw and its scratch as above. */
int a3v_rmsnorm_bwd_rows_bf16(const void* x, int64_t ldx, const int32_t* row_idx, const float* w, const void* dy, int64_t lddy,
                              void* dh, int64_t lddh, float* dw, float* dw_scratch, int rows, int dim, float eps, void* stream);
/* Either of the two (row_idx NULL: every row) WITHOUT the column sum: the weight gradient stays as ceil(rows / 8) partial rows of dim
 * floats in `parts` (a3v_rmsnorm_bwd_scratch_floats(rows, dim) floats, 16-byte aligned), for an A3V_FINISH_COLSUM job of
 * a3v_grad_finish_multi.  A3V_ERR_SHAPE where the kernel with partial rows does not apply (dim or a row stride no multiple of 4). */
int a3v_rmsnorm_bwd_parts_bf16(const void* x, int64_t ldx, const int32_t* row_idx, const float* w, const void* dy, int64_t lddy,
                               void* dh, int64_t lddh, float* parts, int rows, int dim, float eps, void* stream);

/* The rows the loss reads (CrossEntropyLoss(ignore_index=0), model/meta.py:67,256-262): for the shifted labels [B, T] (int64), the
 * ascending list of positions b T + t with a non-zero label -- as rows b S + W + t of the decoder stream [B, S = W + T] in
 * stream_rows and as rows b T + t of the head in head_rows (int32, room for B T entries each), the labels themselves in labels_out
 * (int64, may be NULL) and the length of the list in count_dev.  One launch, one block; the order never depends on timing. */
int a3v_label_rows(const int64_t* labels, int B, int T, int W, int S, int32_t* stream_rows, int32_t* head_rows,
                   int64_t* labels_out, int32_t* count_dev, void* stream);
/* dst[i, :] = src[row_idx[i], :], i < n (bf16 / fp32; 16-byte pieces: cols, both leading dimensions and both pointers multiples of
 * 16 bytes).  An index outside [0, src_rows) reads nothing and gives a zero row. */
int a3v_gather_rows(const void* src, int64_t ld_src, int src_rows, const int32_t* row_idx, int n, void* dst, int64_t ld_dst,
                    int cols, int dtype, void* stream);
/* dst[row_idx[i], :] = src[i, :] for an ASCENDING list without repeats, and every other row of dst[0 .. dst_rows) = 0, written by the
 * same launch (nothing of dst's old content survives in the first `cols` columns).  Same alignment rules. */
int a3v_scatter_rows(const void* src, int64_t ld_src, const int32_t* row_idx, int n, void* dst, int64_t ld_dst, int dst_rows,
                     int cols, int dtype, void* stream);
int a3v_embed_bwd_bf16(const int64_t* tokens, int64_t ld_tok, const void* dh, float* dtable, int B, int T, int W, int dim,
                       int vocab, void* stream);

/* backward of a3v_layernorm (x in act_dtype, fp32 w; dy fp32 rows gathered through row_map):
 * dx (act_dtype), dw += , db += . */
int a3v_layernorm_bwd(const void* x, int64_t ldx, const float* w, const float* dy, int64_t lddy,
                      const int32_t* row_map, void* dx, int64_t lddx, float* dw, float* db, int rows,
                      int dim, float eps, int act_dtype, void* stream);

/* SwiGLU on gu [rows, 2F] (the un-fused form of A3V_EPI_SWIGLU, kept for the backward pass):
 * interleaved = 1: 16-column blocks [gate|up] (inference weight image); 0: [all gates | all ups]
 * (training image = cat(w1, w3), whose fp32 grad buffer splits into w1.grad / w3.grad views).
 * act = silu(g)*u ; dgu from dact. */
int a3v_swiglu_fwd(const void* gu, int64_t ldg, void* act, int64_t lda, int rows, int F,
                   int interleaved, int dtype, void* stream);
int a3v_swiglu_bwd(const void* gu, int64_t ldg, const void* dact, int64_t lda, void* dgu,
                   int64_t lddg, int rows, int F, int interleaved, int dtype, void* stream);

/* inverse RoPE on dq [B,S,H,hd], dk [B,Hkv,S,hd]; dv [B,Hkv,S,hd] copied; packed into
 * dqkv [B*S, (H+2Hkv)*hd] (the gradient of the fused QKV activation). */
int a3v_rope_bwd_pack(const void* dq, const void* dk, const void* dv, void* dqkv, int64_t ld,
                      const float* cos_sin, int B, int S, int H, int Hkv, int hd, int rope_pos0,
                      int dtype, void* stream);

/* backward of causal / full self-attention (Sq == Sk == S).  q,out,dout,dq [B,S,H,hd]; k,dk,dv
 * [B,Hkv,S,hd]; k rows [b][hk][s] at k + b*k_sb + hk*k_sh + s*hd; v rows addressed by element
 * strides (batch, seq, kv-head); lse [B,H,S]; D: fp32 scratch [B,S,H]. */
int a3v_attention_bwd(const void* q, const void* k, int64_t k_sb, int64_t k_sh, const void* v,
                      int64_t v_sb, int64_t v_ss, int64_t v_sh, const void* out, const void* dout,
                      const float* lse, float* D, void* dq, void* dk, void* dv, void* workspace,
                      int B, int S, int H, int Hkv, int hd, int causal, int dtype, void* stream);
/* a3v_attention_bwd + a3v_rope_bwd_pack in one pass (bf16, hd 64 / 128): the gradient of the fused qkv activation
 * dqkv [B*S, ld_qkv] = [dq | dk | dv] with the q / k parts rotated back by -theta (autograd of apply_rotary_emb and of the
 * xq / xk / xv views, LLM/llama_ens5.py:112-118); no dq / dk / dv buffers.  out [B*S, ld_out] (token stride ld_out >= H*hd, 16-B
 * aligned), dout contiguous.  D: scratch [B, S, H] floats. */
int a3v_attention_bwd_packed(const void* q, const void* k, int64_t k_sb, int64_t k_sh, const void* v, int64_t v_sb,
                             int64_t v_ss, int64_t v_sh, const void* out, int64_t ld_out, const void* dout, const float* lse, float* D,
                             void* dqkv, int64_t ld_qkv, const float* cos_sin, int rope_pos0, int B, int S, int H, int Hkv,
                             int hd, int causal, int dtype, void* stream);
/* bytes of `workspace` for the bf16 MFMA path: a non-NULL workspace selects it (NULL = the generic, slow kernels).  The MFMA
 * kernels no longer keep transposed K / Q / dO images there (transpose reads on the row tiles), so this is a token 256 bytes. */
int64_t a3v_attention_bwd_workspace_bytes(int B, int S, int H, int Hkv, int hd);
int a3v_attention_bwd_mfma(const void* q, const void* k, int64_t k_sb, int64_t k_sh, const void* v,
                           int64_t v_sb, int64_t v_ss, int64_t v_sh, const void* dout, const float* lse,
                           const float* D, void* dq, void* dk, void* dv, void* workspace, int B, int S,
                           int H, int Hkv, int hd, int causal, void* stream);

/* dst = (dst_dtype) src, 2-D with leading dimensions (fp32 grad stream -> bf16 GEMM operand). */
/* dst[r, c] += src[r, c] (fp32 or bf16, cols % 4 == 0): accumulates the diagonal blocks of the fused LoRA gradient GEMMs
 * into lora_a.weight.grad / lora_b.weight.grad (model/peft.py adapters) and performs the block's residual add
 * `h + out` (LLM/llama_ens5.py:238,241) when the adapter sum must be rounded before it (peft.py:95). */
int a3v_add2d(void* dst, int64_t ld_dst, const void* src, int64_t ld_src, int rows, int cols, int dtype, void* stream);
int a3v_cast(const void* src, int64_t ld_src, int src_dtype, void* dst, int64_t ld_dst, int dst_dtype,
             int rows, int cols, void* stream);

/* d_table[token] += dh[row] over the text rows of [BOS | W image words | text] (fp32). */
int a3v_embed_bwd(const int64_t* tokens, int64_t ld_tok, const float* dh, float* dtable, int B, int T,
                  int W, int dim, int vocab, void* stream);

/* out[c] += sum_i src[row_idx ? row_idx[i] : i][c]  (bias grads, start_img / end_img grads). */
int a3v_rows_sum(const void* src, int64_t ld, const int32_t* row_idx, int n_rows, int dim, float* out,
                 int dtype, void* stream);

/* One AdamW step on one fp32 parameter tensor (torch.optim.AdamW semantics, decoupled weight decay; the reference optimizer of
 * main_finetune.py:138 with engine_finetune.py:63 optimizer.step()): step = 1-based update count of this parameter.  All four
 * arrays 16-B aligned.  bf16_image (optional): also store the updated parameter rounded to bf16 (the next step's GEMM operand). */
int a3v_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
              float eps, float weight_decay, int64_t step, void* bf16_image, void* stream);

/* a3v_adamw with the gradient multiplied by *grad_scale (a DEVICE fp32 scalar, NULL = 1) as it is read: the clip of
 * NativeScalerWithGradNormCount.__call__ (util/misc.py:302-315) / clip_grad_norm (util/clip_grad.py:187-193: coef =
 * max_norm / (norm + 1e-6) clamped to 1, every gradient multiplied by it) folded into the optimizer pass -- same values as
 * grad.mul_(coef) followed by a3v_adamw, without the extra read + write of every gradient and without a host read of the norm. */
/* A NEGATIVE (sign bit set: -0.0 included) or NaN *grad_scale makes the call a no-op: the trainer folds "loss and gradient norm of this step are finite" into
 * the coefficient on the device, so a bad step never reaches the fp32 masters, the moments or the bf16 weight images (the
 * reference stops before backward on a non-finite loss, engine_finetune.py:56-58; here the host reads the flag later). */
int a3v_adamw_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int64_t step, void* bf16_image, const float* grad_scale, void* stream);

/* Adapter weight gradients of a fused LoRA group (model/peft.py:58-159: lora_b of the n_mods <= 4 linears that share an input):
 * gbt = t^T . dy, fp32 [>= n_mods*r, N] with row stride ld, holds the group's dB^T; module j owns rows j*r..(j+1)*r of columns
 * row0[j]..row0[j]+nj[j]; dst[j] (fp32 [nj[j], r], contiguous: the parameter's gradient) += that block transposed.  dst / row0 / nj
 * are HOST arrays (dst[j] device pointers). */
int a3v_lora_gb_scatter(const float* gbt, int64_t ld, int r, int n_mods, float* const* dst, const int* row0, const int* nj, void* stream);

/* The adapter weight gradients as a streaming kernel: partial[s][R][N] = T[k in slice s][0..R)^T . X[k in slice s][0..N), S token
 * slices (raw fp32 planes, summed / rounded / accumulated by a3v_splitk_reduce exactly like those of a3v_gemm_tn_splitk).  T: bf16
 * [Kt][ldt] with R <= 64 valid columns (the padded rank of a fused adapter group; the kernel always loads 64 columns per row, so
 * ldt >= 64 and the row's first 64 elements must be readable), X: bf16 [Kt][ldx].  dB^T = t^T . dy and dA = dt^T . x of
 * model/peft.py:58-159 (autograd's gradients of lora_b / lora_a, engine_finetune.py:55-57).  Small blocks (64 x 128 tile, 48 KiB of
 * LDS: three per CU) so that the stream of X has several stages in flight per CU. */
int a3v_gemm_tn_strip(const void* T, int64_t ldt, const void* X, int64_t ldx, float* partial, int R, int N, int Kt, int S, void* stream);

/* a3v_adamw_scaled for a [rows, cols] matrix (rows, cols multiples of 64) that ALSO keeps the transposed bf16 image current:
 * bf16_image_t points at element [0][first row of this parameter] of W^T [cols][ldt] (ldt >= rows, multiple of 4; 8-B aligned), the
 * operand of the full fine-tune's input-gradient GEMMs on the NT kernel (loss.backward() through F.linear, engine_finetune.py:55-57;
 * optimizer.step(), :63).  bf16_image (optional) as in a3v_adamw.  Arithmetic identical to a3v_adamw_scaled. */
int a3v_adamw_scaled_t(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int rows, int cols, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int64_t step, void* bf16_image, void* bf16_image_t, int64_t ldt,
                       const float* grad_scale, void* stream);

/* The same update for MANY small tensors of one torch param group in ONE launch (a LoRA step: ~520 adapter / norm tensors; was one
 * launch per tensor plus one a3v_lora_refresh per adapter).  `table` is a DEVICE array of n_tensors descriptors (built once by the
 * host, a3vlm_amd/optim.py); every pointer 16-byte aligned, fp32 contiguous p / g / m / v of n elements viewed as [n / cols, cols].
 * The bf16 value of updated element (i, j) is also stored to d1[i*s1r + j*s1c] and d2[i*s2r + j*s2c] when those are non-NULL
 * (element strides): a same-shape image (s1r = cols, s1c = 1), or an adapter's rows / columns inside the fused group images and
 * their transposes (model/peft.py:40-64 parameters; reference optimizer: main_finetune.py:138).  max_n = the largest n.
 * Arithmetic identical to a3v_adamw_scaled. */
typedef struct {
  float* p; const float* g; float* m; float* v;
  int64_t n, cols;
  void* d1; int64_t s1r, s1c;
  void* d2; int64_t s2r, s2c;
} a3v_adamw_tensor;
int a3v_adamw_multi(const a3v_adamw_tensor* table, int n_tensors, int64_t max_n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, const float* grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * 8-bit AdamW moments (opt-in; no reference counterpart: the reference's optimizer is torch.optim.AdamW with fp32 state,
 * main_finetune.py:138; the idea is bitsandbytes' 8-bit optimizers, here with the project's fp8 convention of
 * a3v_quantize_rows_fp8 / the fp8 KV cache instead of a dynamic code book).  Format:
 *   a parameter tensor of n elements, n % 256 == 0, is viewed flat as n / 256 blocks of 256 consecutive elements;
 *   exp_avg m:    m_q uint8[n] (OCP e4m3fn codes) and m_scale float[n / 256]; per block scale = max(max|m|, 1e-30) / 448,
 *                 q = e4m3(m / scale) with a true division, round to nearest even, saturating; stored value float(q) * scale;
 *   exp_avg_sq v: what is stored is r = sqrtf(v), as r_q / r_scale by the same rule; stored value v^ = (float(q) * scale)^2.  The
 *                 square root halves the exponent range one block scale has to span: e4m3 reaches from 448 down to 2^-9, a ratio of
 *                 2^17.8 in |g| inside one block;
 *   for r only:   a NON-ZERO r whose quotient rounds to code 0 is stored as code 0x01 (value 2^-9 * scale), so that an element that
 *                 has seen a gradient never gets the denominator 0 + eps; m may round to zero;
 *   an all-zero block stays finite: codes 0, scale 1e-30 / 448.
 * The floor of the scale is 1e-30, not the KV cache's 1e-12: moments of small gradients are legitimately far below 1e-12 (a floor
 * of 1e-12 would store every block of a layer whose gradients are ~1e-8 as zeros).  Below r ~ 1e-19 the square v^ underflows in
 * fp32 whatever the code: such elements are, as in the fp32 optimizer, indistinguishable from zero.
 * NaN / inf are NOT kept: the block maximum and the saturating clamp are fmaxf / fminf, which drop a NaN operand, so a NaN or inf that
 * reaches a moment (a non-finite gradient with grad_scale NULL) is stored as finite codes (+-448 or 0) and a finite scale -- the fp32
 * state would stay visibly NaN.  The parameter still turns NaN in that step; the trainer's device-side guard (a negative grad_scale)
 * keeps such a step from being applied at all.
 *
 * Argument checks, before any launch: a NULL required pointer, n <= 0 (step < 1): A3V_ERR_ARG; n % 256 != 0 or any pointer not 16-B
 * aligned (scales and grad_scale: 4-B): A3V_ERR_SHAPE.
 * a3v_adam8_quantize: (m, m_q, m_scale) and (v, r_q, r_scale); either triple may be NULL as a whole (that moment is skipped).
 * a3v_adam8_dequantize: the element-wise inverse, m[i] = float(m_q[i]) * m_scale[i / 256], v[i] = (float(r_q[i]) * r_scale[i / 256])^2
 * (every product rounded to fp32); either triple may be NULL. */
int a3v_adam8_quantize(const float* m, const float* v, uint8_t* m_q, float* m_scale, uint8_t* r_q, float* r_scale, int64_t n,
                       void* stream);
int a3v_adam8_dequantize(const uint8_t* m_q, const float* m_scale, const uint8_t* r_q, const float* r_scale, float* m, float* v,
                         int64_t n, void* stream);
/* a3v_adamw_scaled on 8-bit moments: bit for bit the sequence a3v_adam8_dequantize -> a3v_adamw_scaled -> a3v_adam8_quantize on the
 * parameter, the optional bf16 image, the codes and the scales, in ONE pass that reads and writes every byte once (18.06 B per
 * parameter with the image, against 30).  grad_scale as in a3v_adamw_scaled: a negative or NaN *grad_scale is a no-op on the
 * parameter, the codes, the scales and the image. */
int a3v_adamw8_scaled(float* param, const float* grad, uint8_t* m_q, float* m_scale, uint8_t* r_q, float* r_scale, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t step, void* bf16_image, const float* grad_scale,
                      void* stream);

/* Every fp32 gradient partial of a LoRA backward finished in ONE launch (was one a3v_splitk_reduce per adapter strip, one
 * a3v_lora_gb_scatter per fused group and one column-sum launch per RMSNorm: ~450 launches of 1 - 17 MB per 7B step).  `table` is a
 * DEVICE array of n_jobs descriptors (every field 8 bytes; built once by the host, a3vlm_amd/grad_finish.py), each one of
 *   A3V_FINISH_PLANES   dst[0][r * ldo + c] (+)= rbf(sum_s src[s][r][c]), S planes [R][N]: what a3v_splitk_reduce does into fp32;
 *   A3V_FINISH_SCATTER  dst[j][n * r + c] += rbf(sum_s src[s][j * r + c][row0[j] + n]), n < nj[j], j < n_mods <= 4: that reduce
 *                       followed by a3v_lora_gb_scatter (only the diagonal blocks of the planes are read);
 *   A3V_FINISH_COLSUM   dst[0][c] += sum_r src[r][c], R partial rows of N columns, summed in 16 row chunks with one atomic per column
 *                       and chunk: the column sum behind a3v_rmsnorm_bwd's partial rows.
 * Planes are summed in ascending s; results equal those of the kernels named, element for element.  Every pointer 16-byte aligned;
 * N, ldo, r, row0[j], nj[j] multiples of 4; r <= 64.  unit0 = the running sum of the units of the jobs before this one, a job having
 * ceil(R * (N / 4) / 256) / sum_j ceil(nj[j] / 64) / 16 * ceil(N / 1024) units; total_units = the sum over all jobs.  The grid is
 * max_blocks blocks (0: four per compute unit), never more than total_units, striding over the units. */
enum { A3V_FINISH_PLANES = 0, A3V_FINISH_SCATTER = 1, A3V_FINISH_COLSUM = 2 };
typedef struct {
  int64_t kind;
  const float* src;
  int64_t S, R, N;
  int64_t ldo, accumulate;
  int64_t r, n_mods;
  float* dst[4];
  int64_t row0[4], nj[4];
  int64_t unit0;
} a3v_finish_job;
int a3v_grad_finish_multi(const a3v_finish_job* table, int n_jobs, int64_t total_units, int max_blocks, void* stream);

/* dst[i] = (dst_dtype)(src[i] * scale), n contiguous elements, both 16-B aligned: the wire-dtype conversions of the DP gradient
 * reducer (fp32 bucket -> bf16 wire bucket pre-scaled by 1/world, and back) -- FSDP's reduce_dtype = bf16 averaging
 * (main_finetune.py:251-255) without separate scale / cast / copy passes over the gradient buffer. */
int a3v_scale_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, float scale, void* stream);

/* The exchange step of data-parallel fine-tuning for a host that owns an RCCL communicator itself (the
 * reference reaches NCCL through FSDP's gradient reduction, main_finetune.py:241-263, reduce_dtype :251-255; the Python host of this
 * repository goes through torch.distributed, a3vlm_amd/dp.py).  `grad`: one bucket (n fp32 elements, 16-byte aligned) of the flat
 * gradient buffer, reduced IN PLACE over the ranks of `comm` (an ncclComm_t) on `stream`: average != 0 -> ncclAvg (FSDP's
 * gradient average), else ncclSum.  `wire_bf16` (optional, n bf16 elements): the bucket crosses the wire in bf16 -- one fused cast
 * in, all-reduce of the bf16 buffer, one widening cast back.  Skipping the call on accumulation micro-steps (util/misc.py:311-313)
 * is the caller's decision.  RCCL is not linked into the library: ncclAllReduce is resolved at run time from the librccl already
 * in the process (PyTorch-ROCm's), A3V_RCCL_LIB, or the loader path; A3V_ERR_ARG when none is found. */
int a3v_grad_bucket_allreduce(void* comm, float* grad, int64_t n, void* wire_bf16, int average, void* stream);

/* ZeRO-1 through the same boundary (round 4; the reference trains configs[3] under FSDP SHARD_GRAD_OP, main_finetune.py:241-263:
 * gradients and AdamW state sharded over DP; the Python host drives these two collectives through torch.distributed,
 * a3vlm_amd/zero1.py).  a3v_grad_bucket_reduce_scatter: `grad` = a bucket's sharded span, world * n_per_rank fp32 elements (world =
 * ncclCommCount(comm)); rank r receives the average (or sum) of elements [r n_per_rank, (r + 1) n_per_rank) in `shard` (fp32).
 * wire_bf16 (world * n_per_rank bf16) + wire_shard_bf16 (n_per_rank bf16), both or neither: the span crosses the wire in bf16.
 * a3v_param_shard_all_gather: every rank's updated bf16 parameter slice (n_per_rank elements) gathered into the flat bf16 parameter
 * buffer (world * n_per_rank elements; in place when shard_bf16 = flat_bf16 + rank * n_per_rank).  a3v_rccl_comm_count: the
 * communicator's size (-1 without RCCL).  Same run-time RCCL resolution as a3v_grad_bucket_allreduce. */
int a3v_grad_bucket_reduce_scatter(void* comm, const float* grad, int64_t n_per_rank, float* shard, void* wire_bf16, void* wire_shard_bf16,
                                   int average, void* stream);
int a3v_param_shard_all_gather(void* comm, const void* shard_bf16, void* flat_bf16, int64_t n_per_rank, void* stream);
int a3v_rccl_comm_count(void* comm);
int a3v_rccl_available(void);

/* Partial sums of squares of an fp32 range: out[0 .. A3V_SUMSQ_SLOTS) (every slot written).  The global-norm gradient clip
 * (reference util/clip_grad.py:59-210) = sqrt(sum of the partials of all gradient buckets); called per bucket on a side stream
 * while the backward still runs.  x 16-byte aligned. */
#define A3V_SUMSQ_SLOTS 1024
int a3v_sumsq_partials(const float* x, int64_t n, float* out, void* stream);

/* Re-write one adapter's rows / columns of a fused LoRA group's bf16 images from its fp32 parameters (model/peft.py:40-64
 * lora_a [r, in], lora_b [nj, r]): A[col0+i, :] and At[:, col0+i] from lora_a, B[row0+n, col0+i] and Bt[col0+i, row0+n] from lora_b. */
int a3v_lora_refresh(const float* lora_a, const float* lora_b, int r, int in_f, int nj, void* A, int64_t lda, void* At, int64_t ldat,
                     void* B, int64_t ldb, void* Bt, int64_t ldbt, int col0, int row0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3VLM_HIP_H */
