// What the GEMM kernels share: the 128x128x64 tile constants, the LDS swizzles and the fp32 epilogue.
#pragma once

#include <cstdint>
#include "gemm_epilogue.h"
#include "tile_order.h"
#include "types.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int THREADS = 256;
constexpr int CHUNKS_PER_ROW = BK / 8;                 // 16-byte chunks per 64-wide bf16 row
constexpr int TILE_CHUNKS = BM * CHUNKS_PER_ROW;       // 1024 chunks per operand tile
constexpr int LOADS_PER_THREAD = TILE_CHUNKS / THREADS;  // 4

// LDS image: [row][8 chunks of 16 B], chunk c of row r stored at c ^ ((r >> 1) & 7).
// For the 16x16x32 fragment read (lane l: row l&15, chunk (l>>4)+4s) this puts
// every ds_read_b128 lane group on 16 distinct 16-byte slots (all 64 banks).
__device__ __forceinline__ int swz(int r, int c) { return r * CHUNKS_PER_ROW + (c ^ ((r >> 1) & 7)); }

// The fp8 16x16x128 fragment (lane l: row l&15, 32 bytes = chunks 2(l>>4), 2(l>>4)+1) needs another
// XOR: f8(r) = 3*r[3] ^ 4*r[1] puts each ds_read_b128 lane group of both chunk reads on 16 distinct
// 16-byte slots (searched exhaustively over GF(2)-linear swizzles; it is conflict-free for the bf16
// fragment pattern too).
__device__ __forceinline__ int swz_row_xor(int r, bool fp8) {
  return fp8 ? ((((r >> 3) & 1) * 3) ^ (((r >> 1) & 1) << 2)) : ((r >> 1) & 7);
}
__device__ __forceinline__ int swz8(int r, int c) { return r * CHUNKS_PER_ROW + (c ^ swz_row_xor(r, true)); }

// The direct fp32 epilogue of a wave's MF x 4 blocks of 16x16, straight from the accumulators.
// C/D layout of 16x16x32: col = lane & 15, row = (lane >> 4) * 4 + reg
template <int MF>
__device__ __forceinline__ void store_acc_f32(float* __restrict__ C, int N, int row0, int col0, int frow, int fq,
                                              const floatx4 (&acc)[MF][4]) {
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        C[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * N + col0 + n * 16 + frow] = acc[m][n][j];
}

}  // namespace
