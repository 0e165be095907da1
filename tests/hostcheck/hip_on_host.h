// tests/hostcheck/hip_on_host.h -- TEST INFRASTRUCTURE ONLY.
//
// What the kernel headers use of the HIP language, for one thread at a time: the host checks include this in front of the kernel
// headers of the product and run every thread of a grid one after the other (an atomic is then a plain read and write).
// __device__ and __forceinline__ come from dsa_common.h.
#pragma once

#include <cstdint>

struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct Dim3 { uint32_t x = 1, y = 1, z = 1; };
static Dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __launch_bounds__(x)
#define __shared__ static
static inline uint32_t atomicCAS(uint32_t *p, uint32_t cmp, uint32_t val) { const uint32_t old = *p; if (old == cmp) *p = val; return old; }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { const unsigned long long old = *p; *p = old + v; return old; }
static inline uint32_t atomicMin(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v < old) *p = v; return old; }
static inline uint32_t atomicMax(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v > old) *p = v; return old; }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old | v; return old; }

// every thread of a (gx, gy) grid of `block` threads; backwards: blocks and threads in descending order, so that other threads win
// what the kernels race for
template <class K, class... A>
static void launch(K kernel, uint32_t gx, uint32_t gy, uint32_t block, bool backwards, A... args) {
  gridDim.x = gx; gridDim.y = gy; blockDim.x = block;
  for (uint32_t by = 0; by < gy; ++by)
    for (uint32_t b = 0; b < gx; ++b)
      for (uint32_t t = 0; t < block; ++t) {
        blockIdx.x = backwards ? gx - 1 - b : b; blockIdx.y = backwards ? gy - 1 - by : by; threadIdx.x = backwards ? block - 1 - t : t;
        kernel(args...);
      }
}
template <class K, class... A>
static void launch(K kernel, uint32_t gx, uint32_t gy, uint32_t block, A... args) { launch(kernel, gx, gy, block, false, args...); }
