// Constrained decoding on the device (include/a3vlm_hip.h, "Constrained decoding"): the token automaton of model/constrain.py is an
// int16 table trans[n_states, V]; every cache row carries one int32 state.  Opt-in: nothing here runs unless MetaModel.generate /
// generate_many are called with constraint=...
//  * constrain_logits_kernel  : out[b, v] = trans[state[b], v] >= 0 ? logits[b, v] : -inf -- a pure stream of 4 + 2 + 4 bytes per
//                               element.  Values move as 32-bit integers (an allowed slot keeps its bits, NaN payloads included).
//                               A row whose state is outside [0, n_states) is copied unchanged (in place: not touched at all).
//                               Block (x, b) owns the 2048 elements x * 2048 .. of row b behind the row's scalar head: 16-byte
//                               loads of the logits, 8-byte loads of the int16 row, 16-byte stores, two vectors in flight per thread.
//  * constrain_advance_kernel : after the step kernel has written the chosen id: state[b] = trans[state[b], id].  One thread per row.
#include "a3v_common.h"

namespace {

constexpr unsigned NEG_INF_BITS = 0xff800000u;
constexpr int CL_THREADS = 256, CL_VECS = 2, CL_CHUNK = CL_THREADS * CL_VECS * 4;      // elements per block

typedef __attribute__((ext_vector_type(4))) short i16x4;

// No __restrict__ on logits / out: the in-place form (out == logits) is part of the contract; every element is read and written by
// the same thread, the read first.
__global__ __launch_bounds__(CL_THREADS) void constrain_logits_kernel(const uint32_t* logits, int64_t ld, const int16_t* __restrict__ trans,
                                                                      int V, int n_states, const int32_t* __restrict__ state,
                                                                      uint32_t* out, int64_t ld_out) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const uint32_t* r = logits + (int64_t)b * ld;
  uint32_t* o = out + (int64_t)b * ld_out;
  const int s = state[b];
  const bool masked = s >= 0 && s < n_states;                  // the kernel bounds the state: the host cannot see it
  if (!masked && r == o) return;                               // an unconstrained row, in place: nothing to do
  const int16_t* t = trans + (masked ? (int64_t)s * V : 0);
  // Vector body: elements head .. head + 4 nv of the row, where r + head is 16-byte aligned.  It needs the out row on the same
  // phase; the int16 row is read as 8-byte vectors when t + head is 8-byte aligned, else as four scalars.
  int head = (int)((16 - (reinterpret_cast<uintptr_t>(r) & 15)) & 15) >> 2;
  if (head > V) head = V;
  const bool vec = ((reinterpret_cast<uintptr_t>(o + head) & 15) == 0) && ((reinterpret_cast<uintptr_t>(r + head) & 15) == 0);
  const int nv = vec ? (V - head) / 4 : 0;
  if (!vec) head = 0;
  const bool tvec = (reinterpret_cast<uintptr_t>(t + head) & 7) == 0;
  const u32x4* r4 = reinterpret_cast<const u32x4*>(r + head);
  u32x4* o4 = reinterpret_cast<u32x4*>(o + head);
  const int i0 = blockIdx.x * (CL_THREADS * CL_VECS) + tid;    // vector index; the block's vectors are i0 + q * 256
  u32x4 x[CL_VECS];
  i16x4 m[CL_VECS];
#pragma unroll
  for (int q = 0; q < CL_VECS; ++q) {
    const int i = i0 + q * CL_THREADS;
    if (i >= nv) break;
    x[q] = r4[i];
    if (masked) {
      if (tvec) {
        m[q] = reinterpret_cast<const i16x4*>(t + head)[i];
      } else {
        const int16_t* te = t + head + 4 * (int64_t)i;
        m[q] = i16x4{te[0], te[1], te[2], te[3]};
      }
    }
  }
#pragma unroll
  for (int q = 0; q < CL_VECS; ++q) {
    const int i = i0 + q * CL_THREADS;
    if (i >= nv) break;
    u32x4 y = x[q];
    if (masked) {
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = m[q][e] >= 0 ? x[q][e] : NEG_INF_BITS;
    }
    o4[i] = y;
  }
  // scalar head (block 0) and tail (the whole row when there is no vector body): grid-strided over the row's blocks
  if (blockIdx.x == 0 && tid < head) o[tid] = (!masked || t[tid] >= 0) ? r[tid] : NEG_INF_BITS;
  for (int i = head + 4 * nv + blockIdx.x * CL_THREADS + tid; i < V; i += gridDim.x * CL_THREADS)
    o[i] = (!masked || t[i] >= 0) ? r[i] : NEG_INF_BITS;
}

// Column convention of generate_record_kernel (a3v_genctl.hip): uniform step (cur == NULL): column `col`; ragged: cur[b] - 1, and the
// caller hands in the snapshot of `stopped` taken BEFORE the step for the rows the step kernel did not touch.
__global__ __launch_bounds__(64) void constrain_advance_kernel(const int64_t* __restrict__ tokens, int64_t ld_tok, int col,
                                                               const int32_t* __restrict__ cur, const int32_t* __restrict__ first,
                                                               const uint8_t* __restrict__ stopped_before,
                                                               const int16_t* __restrict__ trans, int V, int n_states,
                                                               int32_t* __restrict__ state, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (stopped_before && stopped_before[b]) return;
  const int64_t c = cur ? (int64_t)cur[b] - 1 : (int64_t)col;
  if (c < 0 || c >= ld_tok) return;                            // idle ragged row, or nothing written yet
  if (c < (int64_t)first[b]) return;                           // a teacher-forced prompt token: the automaton has not started
  const int s = state[b];
  if (s < 0 || s >= n_states) return;                          // an unconstrained row stays one
  const int64_t id = tokens[(int64_t)b * ld_tok + c];
  if (id < 0 || id >= V) return;
  state[b] = (int32_t)trans[(int64_t)s * V + id];
}

}  // namespace

#define ST (hipStream_t)stream

extern "C" int a3v_constrain_logits(const float* logits, int64_t ld, const int16_t* trans, int V, int n_states, const int32_t* state,
                                    float* out, int64_t ld_out, int B, void* stream) {
  if (!logits || !trans || !state || !out) return A3V_ERR_ARG;
  if (B <= 0 || B > 65535 || V <= 0 || n_states <= 0 || n_states > 32767 || ld < V || ld_out < V) return A3V_ERR_ARG;
  if (out == logits && ld_out != ld) return A3V_ERR_ARG;       // in place means the same rows
  const unsigned gx = (unsigned)(((int64_t)V + CL_CHUNK - 1) / CL_CHUNK);
  hipLaunchKernelGGL(constrain_logits_kernel, dim3(gx, B), dim3(CL_THREADS), 0, ST, reinterpret_cast<const uint32_t*>(logits), ld, trans, V,
                     n_states, state, reinterpret_cast<uint32_t*>(out), ld_out);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}

extern "C" int a3v_constrain_advance(const int64_t* tokens, int64_t ld_tok, int col, const int32_t* cur, const int32_t* first,
                                     const uint8_t* stopped_before, const int16_t* trans, int V, int n_states, int32_t* state, int B,
                                     void* stream) {
  if (!tokens || !first || !trans || !state) return A3V_ERR_ARG;
  if (B <= 0 || V <= 0 || n_states <= 0 || n_states > 32767 || ld_tok <= 0 || (!cur && (col < 0 || col >= ld_tok))) return A3V_ERR_ARG;
  hipLaunchKernelGGL(constrain_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, ST, tokens, ld_tok, col, cur, first, stopped_before, trans, V,
                     n_states, state, B);
  A3V_LAUNCH_CHECK();
  return A3V_OK;
}
