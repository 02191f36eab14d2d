// CPU stand-in for the HIP environment of csrc/png_decode.hip (tools/png_decode_standin.py): tools/png_standin/common.h (a
// std::thread per lane, barriers as barriers, LDS as shared statics) plus what the reader's kernels use on top of it: wave
// shuffles and votes as an exchange array between two barriers, readfirstlane as the identity (the lanes of the stand-in
// are threads, each computes the uniform values itself), the workgroup fence as nothing (a barrier follows every one).
// Found as "common.h" by a COPY of png_decode.hip placed next to it.
#pragma once
#include "standin_base.h"
static int g_xchg[64];
static inline int __shfl_xor(int v, int o, int) {
  g_xchg[threadIdx.x] = v;
  __syncthreads();
  int r = g_xchg[threadIdx.x ^ o];
  __syncthreads();
  return r;
}
static inline int __shfl_up(int v, int d, int) {
  g_xchg[threadIdx.x] = v;
  __syncthreads();
  int r = g_xchg[(int)threadIdx.x >= d ? threadIdx.x - d : threadIdx.x];
  __syncthreads();
  return r;
}
static inline int __any(int p) { return __ballot(p != 0) != 0; }
static inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
static inline void __threadfence_block() {}
