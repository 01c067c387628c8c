// GEMM v2: 256x256x64 tiles, 8 waves, LDS-DMA staging, one barrier per K-tile.
#pragma once

#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------
// gemm v2: 256x256x64 block tile, 8 waves (2 M x 4 N, 128x64 each), operands
// streamed global -> LDS by LDS-DMA (global_load_lds_dwordx4: no VGPR staging,
// 8 per thread per stage), two LDS stages of 64 KiB (1 block per CU), the same
// XOR swizzle as v1 applied on the *global source* address because an LDS-DMA
// wave instruction writes 1 KiB lane-linearly (8 rows of 128 B).
constexpr int V2_BM = 256, V2_BN = 256, V2_THREADS = 512;
constexpr int V2_ROWS_PER_WAVE = 32;                   // rows of each operand one wave fills per stage
constexpr int V2_STAGE_BYTES = 2 * V2_BM * BK * 2;     // A + B, bf16 = 64 KiB

typedef __attribute__((address_space(3))) void lds_void_t;

template <bool FP8 = false>
__device__ __forceinline__ void v2_fill(unsigned char* lds_stage, const __bf16* __restrict__ A,
                                        const __bf16* __restrict__ Bt, int K, int kt, int wid, int lane) {
  // lane -> (row within an 8-row group, physical chunk); logical chunk = phys ^ swizzle(row)
  const int rsub = lane >> 3, phys = lane & 7;
#pragma unroll
  for (int op = 0; op < 2; ++op) {
    const __bf16* src = op == 0 ? A : Bt;
#pragma unroll
    for (int j = 0; j < V2_ROWS_PER_WAVE / 8; ++j) {
      const int row = wid * V2_ROWS_PER_WAVE + j * 8 + rsub;
      const int c = phys ^ swz_row_xor(row, FP8);
      const __bf16* g = src + static_cast<size_t>(row) * K + kt * BK + c * 8;
      unsigned char* l = lds_stage + op * (V2_BM * BK * 2) + (wid * V2_ROWS_PER_WAVE + j * 8) * (BK * 2);
      __builtin_amdgcn_global_load_lds(g, (lds_void_t*)l, 16, 0, 0);
    }
  }
}

__device__ __forceinline__ void v2_compute(floatx4 (&acc)[8][4], const u32x4* __restrict__ a_img,
                                           const u32x4* __restrict__ b_img, int wr, int wc, int frow, int fq) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 bfr[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) bfr[n] = __builtin_bit_cast(bf16x8, b_img[swz(wc * 64 + n * 16 + frow, fq + 4 * s)]);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const bf16x8 af = __builtin_bit_cast(bf16x8, a_img[swz(wr * 128 + m * 16 + frow, fq + 4 * s)]);
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[n], acc[m][n], 0, 0, 0);
    }
  }
}

__global__ void __launch_bounds__(V2_THREADS, 1)
gemm_bf16_v2_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, float* __restrict__ C, int M, int N,
                    int K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // 2 stages x 64 KiB (dynamic)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;
  const int tiles_m = M / V2_BM, tiles_n = N / V2_BN, nwg = tiles_m * tiles_n;
  const auto [tm, tn] = tile_of(xcd_remap(blockIdx.x, nwg), tiles_m, tiles_n, 4);
  const __bf16* Ab = A + static_cast<size_t>(tm) * V2_BM * K;
  const __bf16* Bb = Bt + static_cast<size_t>(tn) * V2_BN * K;

  floatx4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int KT = K / BK;
  const int frow = lane & 15, fq = lane >> 4;
  v2_fill(smem, Ab, Bb, K, 0, wid, lane);
  __builtin_amdgcn_s_waitcnt(0x3f70);  // vmcnt(0) (gfx9 encoding: vmcnt[3:0]=0, vmcnt[15:14]=0)
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    unsigned char* cur = smem + (kt & 1) * V2_STAGE_BYTES;
    if (kt + 1 < KT) v2_fill(smem + ((kt + 1) & 1) * V2_STAGE_BYTES, Ab, Bb, K, kt + 1, wid, lane);
    v2_compute(acc, reinterpret_cast<const u32x4*>(cur), reinterpret_cast<const u32x4*>(cur + V2_BM * BK * 2), wr, wc,
               frow, fq);
    __builtin_amdgcn_s_waitcnt(0x3f70);  // this wave's LDS-DMA for stage kt+1 has landed
    __syncthreads();                     // ... and everyone's; stage kt is free for kt+2
  }
  store_acc_f32(C, N, tm * V2_BM + wr * 128, tn * V2_BN + wc * 64, frow, fq, acc);
}

}  // namespace
