// CPU stand-in for the HIP environment of csrc/png.hip (tools/png_standin.py): a std::thread per lane, one workgroup at a
// time, barriers as barriers, LDS as shared statics, atomics as atomics, a ballot as two barriers around a predicate array.
// Found as "common.h" by a COPY of png.hip placed next to it; include/ must be on the include path.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <pthread.h>
#include <thread>
#include <vector>
#include <cstdlib>
#include "rcdm.h"
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
struct dim3 { int x, y, z; dim3(int a = 1, int b = 1, int c = 1) : x(a), y(b), z(c) {} };
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static pthread_barrier_t g_bar;
static int g_nthreads;
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
template <class T> static inline T atomicAdd(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class T> static inline T atomicOr(T* p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) {
  uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
static inline uint32_t __brev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline int __clz(uint32_t v) { return v ? __builtin_clz(v) : 32; }
static inline int __ffs(uint32_t v) { return __builtin_ffs((int)v); }
template <class T> static inline T __shfl_xor(T v, int) { abort(); return v; }
static uint8_t g_pred[4096];
static inline unsigned long long __ballot(bool e) {   // every thread of the workgroup calls it the same number of times
  g_pred[threadIdx.x] = e;
  __syncthreads();
  unsigned long long r = 0;
  const int w0 = threadIdx.x & ~63;
  for (int l = 0; l < 64 && w0 + l < g_nthreads; ++l) r |= (unsigned long long)g_pred[w0 + l] << l;
  __syncthreads();
  return r;
}
static inline int rcdm_check_launch() { return 0; }
template <class K, class... A> static void launch(K k, dim3 grid, dim3 block, A... a) {
  g_nthreads = block.x;
  pthread_barrier_init(&g_bar, nullptr, block.x);
  for (int by = 0; by < grid.y; ++by)
    for (int bx = 0; bx < grid.x; ++bx) {
      std::vector<std::thread> th;
      for (int t = 0; t < block.x; ++t) th.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(bx, by); k(a...); });
      for (auto& t : th) t.join();
    }
  pthread_barrier_destroy(&g_bar);
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) launch(k, grid, block, __VA_ARGS__)
