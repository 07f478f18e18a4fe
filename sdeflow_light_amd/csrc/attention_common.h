// attention_common.h — the phases of the attention kernels, one function each: integer decodes and two shuffle pairs, no
// floating-point sum is reordered by them.  attention_kernels.hip (sampler) runs on all of them, attention_train_kernels.hip on
// the head addressing; its two main kernels keep their own lines for the rest on a measurement (see the note there).
#pragma once
#include "common.h"

// attn_head: (sample, head) pair pr at C channels per head.  LD / LA: qkv / att row strides; qcol / acol: the pair's first
// qkv / att column.  MH = false is the single-head build: pr is the sample, strides compile-time 3C / C, columns 0.
struct AttnHead { int LD, LA, smp, hd, qcol, acol; };
template <bool MH, int C>
__device__ __forceinline__ AttnHead attn_head(int pr, int nh) {
  const int smp = MH ? pr / nh : pr, hd = MH ? pr - smp * nh : 0;
  return AttnHead{MH ? 3 * C * nh : 3 * C, MH ? C * nh : C, smp, hd, 3 * C * hd, C * hd};
}
// attn_mh_row: the same addressing for kernels indexed by row (pair pr, position t) at a run-time channel count: offset of
// the row's first column in a [sample][T][nh W] tensor with heads W wide (W = C for att, 3C for qkv)
__device__ __forceinline__ size_t attn_mh_row(int64_t pr, int64_t t, int T, int W, int nh) {
  const int64_t smp = pr / nh, hd = pr - smp * nh;
  return ((size_t)smp * T + t) * W * nh + (size_t)W * hd;
}

// attn_slot: float4 slot i (index idx) of thread tid when NT threads stage a [rows][C] tile with coalesced 16-byte accesses:
// its row and the float4 c4 inside the row.  A tile of fewer than NT slots tests idx.
struct AttnSlot { int idx, row, c4; };
template <int C, int NT>
__device__ __forceinline__ AttnSlot attn_slot(int tid, int i) {
  const int idx = tid + NT * i, row = idx / (C / 4);
  return AttnSlot{idx, row, idx - row * (C / 4)};
}

// quad_max / quad_sum: a query's value over the four key groups (lane quarters) of the transposed online softmax
__device__ __forceinline__ float quad_max(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float quad_sum(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }

// more than 64 KB of dynamic LDS has to be allowed per kernel, once per process: `static const int once = attn_allow_lds(..)`
template <class K>
static int attn_allow_lds(K* kernel, size_t bytes) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
