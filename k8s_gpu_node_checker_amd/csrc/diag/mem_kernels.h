// The HBM stream kernels and the memtest.
#pragma once

#include <cstdint>

#include "../common/hip_host.h"

namespace {

// ---------------------------------------------------------------- HBM streams
// Forms picked by the sweeps in tools/hbm_explore.hip on MI355X (profiles/hbm_explore_mi355x.json):
// one 16-byte element per thread and a grid over the whole buffer (no grid-stride loop), nontemporal
// loads/stores for copy and read, plain stores for write: copy 6.59, read 6.97, write 6.87 TB/s,
// vs 5.29 / 6.78 / 5.16 for the best persistent form (8-deep unrolled, 32 blocks of 256 per CU).
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) copy_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

__global__ void __launch_bounds__(256) read_kernel(const f32x4* __restrict__ src, size_t n, float* sink) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) {
    const f32x4 v = __builtin_nontemporal_load(src + i);
    if (v[0] + v[3] == 1234.5678f) *sink = v[1];  // keeps the load alive, practically never stores
  }
}

__global__ void __launch_bounds__(256) write_kernel(f32x4* __restrict__ dst, size_t n, float v) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) dst[i] = f32x4{v, v, v, v};
}

// The bytes the stream rates are computed from, checked outside the timed loops: every 16-byte element of `p` must
// hold `v` in all four lanes; one atomic per wrong element, as mt_verify_kernel.
__global__ void __launch_bounds__(256) stream_verify_kernel(const f32x4* __restrict__ p, size_t n, float v,
                                                            unsigned long long* errors) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    const f32x4 x = p[i];
    if (x[0] != v || x[1] != v || x[2] != v || x[3] != v) atomicAdd(errors, 1ULL);
  }
}

// ---------------------------------------------------------------- memtest
__device__ __forceinline__ uint4 pattern(size_t i, uint64_t seed, bool invert) {
  uint4 v;
  v.x = mix32(4 * i + seed);
  v.y = mix32(4 * i + 1 + seed);
  v.z = mix32(4 * i + 2 + seed);
  v.w = mix32(4 * i + 3 + seed);
  if (invert) {
    v.x = ~v.x;
    v.y = ~v.y;
    v.z = ~v.z;
    v.w = ~v.w;
  }
  return v;
}

__global__ void __launch_bounds__(256) mt_write_kernel(uint4* p, size_t n, uint64_t seed, int invert) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride)
    p[i] = pattern(i, seed, invert != 0);
}

__global__ void __launch_bounds__(256) mt_verify_kernel(const uint4* p, size_t n, uint64_t seed, int invert,
                                                        unsigned long long* errors, unsigned long long* first_bad) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    const uint4 v = p[i];
    const uint4 e = pattern(i, seed, invert != 0);
    if (v.x != e.x || v.y != e.y || v.z != e.z || v.w != e.w) {
      atomicAdd(errors, 1ULL);
      atomicMin(first_bad, static_cast<unsigned long long>(i));
    }
  }
}

}  // namespace
