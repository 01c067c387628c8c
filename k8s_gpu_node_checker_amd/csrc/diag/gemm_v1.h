// GEMM v1: 128x128x64 tiles, 4 waves, register-staged; v4's tail (gemm_v4.h) runs the same K loop.
#pragma once

#include "gemm_common.h"

namespace {

__device__ __forceinline__ void gemm_gload(u32x4 (&ra)[LOADS_PER_THREAD], u32x4 (&rb)[LOADS_PER_THREAD],
                                           const u32x4* __restrict__ Ablk, const u32x4* __restrict__ Bblk,
                                           const int (&g_off)[LOADS_PER_THREAD], int kt) {
#pragma unroll
  for (int i = 0; i < LOADS_PER_THREAD; ++i) {
    ra[i] = Ablk[g_off[i] + kt * CHUNKS_PER_ROW];
    rb[i] = Bblk[g_off[i] + kt * CHUNKS_PER_ROW];
  }
}

__device__ __forceinline__ void gemm_lstore(u32x4 (&buf)[2][TILE_CHUNKS], const u32x4 (&ra)[LOADS_PER_THREAD],
                                            const u32x4 (&rb)[LOADS_PER_THREAD], const int (&l_off)[LOADS_PER_THREAD]) {
#pragma unroll
  for (int i = 0; i < LOADS_PER_THREAD; ++i) {
    buf[0][l_off[i]] = ra[i];
    buf[1][l_off[i]] = rb[i];
  }
}

// One BK=64 step: 2 x (4 A-fragments, 4 B-fragments, 16 MFMA 16x16x32).
__device__ __forceinline__ void gemm_compute(floatx4 (&acc)[4][4], const u32x4 (&buf)[2][TILE_CHUNKS], int wr, int wc,
                                             int frow, int fq) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = __builtin_bit_cast(bf16x8, buf[0][swz(wr * 64 + m * 16 + frow, fq + 4 * s)]);
#pragma unroll
    for (int n = 0; n < 4; ++n) bfr[n] = __builtin_bit_cast(bf16x8, buf[1][swz(wc * 64 + n * 16 + frow, fq + 4 * s)]);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m][n], 0, 0, 0);
  }
}

__global__ void __launch_bounds__(THREADS, 2)
gemm_bf16_kernel(const u32x4* __restrict__ A, const u32x4* __restrict__ Bt, float* __restrict__ C, int M, int N,
                 int K) {
  __shared__ u32x4 lds[2][2][TILE_CHUNKS];  // [buffer][A|B][chunk]  = 64 KiB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int tiles_m = M / BM, tiles_n = N / BN, nwg = tiles_m * tiles_n;
  const auto [tm, tn] = tile_of(xcd_remap(blockIdx.x, nwg), tiles_m, tiles_n, 8);

  const int kchunks = K / 8;  // 16-byte chunks per row of A / Bt
  const u32x4* Ablk = A + static_cast<size_t>(tm) * BM * kchunks;
  const u32x4* Bblk = Bt + static_cast<size_t>(tn) * BN * kchunks;

  u32x4 ra[LOADS_PER_THREAD], rb[LOADS_PER_THREAD];
  // per-thread chunk coordinates are loop invariant
  int g_off[LOADS_PER_THREAD], l_off[LOADS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < LOADS_PER_THREAD; ++i) {
    const int ch = tid + i * THREADS;
    const int r = ch / CHUNKS_PER_ROW, c = ch % CHUNKS_PER_ROW;
    g_off[i] = r * kchunks + c;
    l_off[i] = swz(r, c);
  }
  floatx4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int KT = K / BK;
  const int frow = lane & 15, fq = lane >> 4;
  gemm_gload(ra, rb, Ablk, Bblk, g_off, 0);
  gemm_lstore(lds[0], ra, rb, l_off);
  __syncthreads();
  // two K-steps per trip so the LDS buffer index is a compile-time constant
  for (int kt = 0; kt < KT; kt += 2) {
    const bool more1 = kt + 1 < KT;
    if (more1) gemm_gload(ra, rb, Ablk, Bblk, g_off, kt + 1);
    gemm_compute(acc, lds[0], wr, wc, frow, fq);
    if (more1) gemm_lstore(lds[1], ra, rb, l_off);
    __syncthreads();
    if (!more1) break;
    const bool more2 = kt + 2 < KT;
    if (more2) gemm_gload(ra, rb, Ablk, Bblk, g_off, kt + 2);
    gemm_compute(acc, lds[1], wr, wc, frow, fq);
    if (more2) gemm_lstore(lds[0], ra, rb, l_off);
    __syncthreads();
  }
  store_acc_f32(C, N, tm * BM + wr * 64, tn * BN + wc * 64, frow, fq, acc);
}

}  // namespace
