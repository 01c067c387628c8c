// The per-XCD readers: each XCD's L2 and each XCD's path to HBM, and the fill they verify.
#pragma once

#include <cstdint>

#include "burn_kernels.h"  // wave_slot(): the per-CU map is the burn-ins'
#include "types.h"

namespace {

// ---------------------------------------------------------------------------
// L2 test: each XCD has its own 4 MiB L2.  Every workgroup finds its XCD (XCC_ID) and streams that XCD's
// private slice of the buffer (smaller than the L2) `passes` times, checking every word; after the
// untimed first launch the slice is L2-resident, so the timed launch measures each XCD's L2 read
// bandwidth.  Per-CU map as the burn-in's (waves, wrong words, wave time): an XCD whose L2 has lost
// ways or runs slow falls behind the others; a corrupting path is located to the CU that read it.
__global__ void __launch_bounds__(256) l2_read_kernel(const uint4* __restrict__ buf, uint32_t slice_vec, int passes,
                                                      uint32_t seed, unsigned long long* errors,
                                                      unsigned long long* cu_map) {
  const long long t0 = wall_clock64();
  const unsigned slot = wave_slot();
  const uint32_t base = (slot >> 7) * slice_vec;  // this XCD's slice
  unsigned int bad = 0;
  auto check = [&](const uint4& v, uint32_t i) {
    const uint32_t w = 4u * (base + i);
    return (v.x != (w ^ seed)) + (v.y != ((w + 1u) ^ seed)) + (v.z != ((w + 2u) ^ seed)) + (v.w != ((w + 3u) ^ seed));
  };
  // L2 hits still take hundreds of ns: 8 independent 16-byte loads per lane are issued before any is
  // consumed, so enough bytes are in flight per CU to reach the L2's bandwidth rather than its latency
  constexpr uint32_t U = 8;
  const uint32_t stride = blockDim.x, full = slice_vec - slice_vec % (U * stride);
  for (int p = 0; p < passes; ++p) {
    for (uint32_t i = threadIdx.x; i < full; i += U * stride) {
      uint4 v[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) v[k] = buf[base + i + k * stride];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) bad += check(v[k], i + k * stride);
    }
    for (uint32_t i = full + threadIdx.x; i < slice_vec; i += stride) bad += check(buf[base + i], i);
  }
  unsigned long long wave_bad = bad;
  for (int off = 32; off > 0; off >>= 1) wave_bad += __shfl_down(wave_bad, off, 64);
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* row = cu_map + 3 * slot;
    atomicAdd(row, 1ULL);
    if (wave_bad) {
      atomicAdd(row + 1, wave_bad);
      atomicAdd(errors, wave_bad);
    }
    atomicAdd(row + 2, dt);
  }
}

// ---------------------------------------------------------------------------
// HBM per XCD: each XCD streams its own slice of a buffer far larger than the L2s and the 256 MiB MALL,
// so every byte comes from HBM through that XCD's path to memory.  The XCD's workgroups share its slice
// through a per-XCD chunk counter (found by XCC_ID, so the mapping of workgroups to XCDs does not matter);
// every word is checked.  All XCDs get the same bytes: on a healthy chip they finish together, and an XCD
// whose fabric path to the memory stacks runs slow falls behind the others (per-CU map as the burn-in's).
// Work queue exit: the counter only grows, so every workgroup leaves once it passes nchunks * passes.
constexpr uint32_t HBM_XCD_CHUNK_VEC = 8192;  // 128 KiB per grab
// only_xcd >= 0: the other XCDs' workgroups leave at once, so that XCD streams alone (its own path's rate,
// without the others contending for the memory stacks).
__global__ void __launch_bounds__(256) hbm_xcd_kernel(const uint4* __restrict__ buf, uint32_t slice_vec, int passes,
                                                      uint32_t seed, int only_xcd, unsigned int* next,
                                                      unsigned long long* errors, unsigned long long* cu_map) {
  __shared__ uint32_t s_chunk;
  const long long t0 = wall_clock64();
  const unsigned slot = wave_slot();
  const unsigned xcd = slot >> 7;
  if (only_xcd >= 0 && static_cast<int>(xcd) != only_xcd) return;
  const uint32_t nchunks = slice_vec / HBM_XCD_CHUNK_VEC;
  const uint32_t total = nchunks * static_cast<uint32_t>(passes);
  unsigned int bad = 0;
  constexpr uint32_t U = 8;
  constexpr uint32_t STEP = U * 256;
  static_assert(HBM_XCD_CHUNK_VEC % STEP == 0, "chunk is a whole number of 8-deep block steps");
  for (;;) {
    if (threadIdx.x == 0) s_chunk = atomicAdd(next + xcd, 1u);
    __syncthreads();
    const uint32_t c = s_chunk;
    __syncthreads();  // everyone has read it before thread 0 overwrites it
    if (c >= total) break;
    const uint32_t base = xcd * slice_vec + (c % nchunks) * HBM_XCD_CHUNK_VEC;
    for (uint32_t i = threadIdx.x; i < HBM_XCD_CHUNK_VEC; i += STEP) {
      u32x4 v[U];
      const u32x4* src = reinterpret_cast<const u32x4*>(buf) + base + i;
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) v[k] = __builtin_nontemporal_load(src + k * 256);
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t w = 4u * (base + i + k * 256);
        bad += (v[k].x != (w ^ seed)) + (v[k].y != ((w + 1u) ^ seed)) + (v[k].z != ((w + 2u) ^ seed)) +
               (v[k].w != ((w + 3u) ^ seed));
      }
    }
  }
  unsigned long long wave_bad = bad;
  for (int off = 32; off > 0; off >>= 1) wave_bad += __shfl_down(wave_bad, off, 64);
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* row = cu_map + 3 * slot;
    atomicAdd(row, 1ULL);
    if (wave_bad) {
      atomicAdd(row + 1, wave_bad);
      atomicAdd(errors, wave_bad);
    }
    atomicAdd(row + 2, dt);
  }
}

__global__ void __launch_bounds__(256) l2_fill_kernel(uint4* buf, uint32_t n_vec, uint32_t seed) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += gridDim.x * blockDim.x) {
    const uint32_t w = 4u * i;
    buf[i] = uint4{w ^ seed, (w + 1u) ^ seed, (w + 2u) ^ seed, (w + 3u) ^ seed};
  }
}

}  // namespace
