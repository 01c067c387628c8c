// The bf16 / fp8 / fp4 MFMA GEMM kernels, v1 to v4 and the v4 tail, with their staging helpers.
#pragma once

#include <cstdint>

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

  // XCD-aware, grouped tile order: consecutive blocks land on different XCDs
  // (round-robin dispatch), so regroup ids so one XCD walks a compact 2D patch.
  const int tiles_m = M / BM, tiles_n = N / BN;
  const int nwg = tiles_m * tiles_n;
  int bid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  }
  constexpr int GROUP_M = 8;
  const int group = bid / (GROUP_M * tiles_n);
  const int first_m = group * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % (GROUP_M * tiles_n)) % gsize;
  const int tn = (bid % (GROUP_M * tiles_n)) / gsize;

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
  // C/D layout of 16x16x32: col = lane & 15, row = (lane >> 4) * 4 + reg
  const int row0 = tm * BM + wr * 64, col0 = tn * BN + wc * 64;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        C[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * N + col0 + n * 16 + frow] = acc[m][n][j];
}

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
  int bid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  }
  constexpr int GROUP_M = 4;
  const int group = bid / (GROUP_M * tiles_n);
  const int first_m = group * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % (GROUP_M * tiles_n)) % gsize;
  const int tn = (bid % (GROUP_M * tiles_n)) / gsize;
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
  const int row0 = tm * V2_BM + wr * 128, col0 = tn * V2_BN + wc * 64;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        C[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * N + col0 + n * 16 + frow] = acc[m][n][j];
}

// ---------------------------------------------------------------------------
// gemm v3: the v2 tile and LDS image on a staggered 4-phase schedule (tools/gemm_lab.hip "v5";
// +5-7 % over v2 at 4096^3/8192^3 on MI355X, profiles/gemm_lab_*.jsonl).
// Waves 0-3 and 4-7 form two groups (one wave of each per SIMD); group 1 runs one s_barrier behind
// group 0, so on every SIMD one wave's MFMA slot covers the other's load slot and barrier wait.
// Each K-tile is 4 phases, one 64x32 quadrant of the wave's 128x64 output each (16 MFMA):
//   load slot: this quadrant's ds_reads (+ LDS-DMA restaging) -> s_barrier -> lgkmcnt(0) ->
//   MFMA slot -> s_barrier.
// Quadrant order (m0,n0) (m0,n1) (m1,n1) (m1,n0): phase 0 reads A(m0)+B(n0), phase 1 B(n1), phase 2
// A(m1), phase 3 reuses B(n0) from registers.  A stage is restaged region by region (16 KiB each):
// R0 = A rows of m0, R1 = B rows of n0, R2 = B rows of n1, R3 = A rows of m1.  Reads retire after
// the barrier that closes their load slot, so a region read in phase p is free two phases later:
// R0 of tile t+2 goes out in phase 2 of tile t, R1 and R2 in phase 3, and R3 of tile t+1 (other
// buffer, last read in phase 2 of tile t-1) in phase 1 (V3_PHASE: which phase carries which piece
// is worth 4-9 %).  Tile t+1 is retired at phase 3 of tile t with a counted vmcnt(6) (tile t+2's
// R0-R2 may stay in flight); raw s_barrier only -- __syncthreads() would drain the in-flight
// LDS-DMA with vmcnt(0).
#define STG_BARRIER()                  \
  do {                                 \
    __builtin_amdgcn_sched_barrier(0); \
    __builtin_amdgcn_s_barrier();      \
    __builtin_amdgcn_sched_barrier(0); \
  } while (0)

// One 16 KiB region of a stage: 16 LDS-DMA wave-instructions of 8 rows, 2 per wave.
template <bool FP8>
__device__ __forceinline__ void stg_region(unsigned char* lds_stage, const __bf16* __restrict__ A,
                                           const __bf16* __restrict__ Bt, int K, int kt, int region, int i, int wid,
                                           int lane) {
  const int rsub = lane >> 3, phys = lane & 7;
  const int g = wid * 2 + i;
  const bool is_a = region == 0 || region == 3;
  const int row0 = is_a ? (g >> 3) * 128 + (region == 0 ? 0 : 64) + (g & 7) * 8
                        : (g >> 2) * 64 + (region == 1 ? 0 : 32) + (g & 3) * 8;
  const int row = row0 + rsub;
  const int c = phys ^ swz_row_xor(row, FP8);
  const __bf16* gp = (is_a ? A : Bt) + static_cast<size_t>(row) * K + kt * BK + c * 8;
  unsigned char* l = lds_stage + (is_a ? 0 : V2_BM * BK * 2) + row0 * (BK * 2);
  __builtin_amdgcn_global_load_lds(gp, (lds_void_t*)l, 16, 0, 0);
}

// The same region through the buffer path (`buffer_load_dwordx4 ... lds`): the tile's A and B slabs
// are two scalar buffer resources, the per-lane byte offset is loop-invariant and the K-tile moves
// only the scalar soffset, so no 64-bit per-lane address math is redone per K-tile.
struct StgBuf {
  __amdgpu_buffer_rsrc_t a, b;
};

__device__ __forceinline__ StgBuf stg_buf(const __bf16* A, const __bf16* Bt, int K) {
  // CDNA raw-buffer dword3 (32-bit data format, no swizzle); num_records = one 256-row slab
  const int bytes = V2_BM * K * 2;
  return StgBuf{__builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A), static_cast<short>(0), bytes, 0x00020000),
                __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(Bt), static_cast<short>(0), bytes, 0x00020000)};
}

template <bool FP8>
__device__ __forceinline__ void stg_region_buf(unsigned char* lds_stage, const StgBuf& rs, int K, int kt, int region,
                                               int i, int wid, int lane) {
  const int rsub = lane >> 3, phys = lane & 7;
  const int g = wid * 2 + i;
  const bool is_a = region == 0 || region == 3;
  const int row0 = is_a ? (g >> 3) * 128 + (region == 0 ? 0 : 64) + (g & 7) * 8
                        : (g >> 2) * 64 + (region == 1 ? 0 : 32) + (g & 3) * 8;
  const int row = row0 + rsub;
  const int c = phys ^ swz_row_xor(row, FP8);
  const int voff = (row * K + c * 8) * 2;
  unsigned char* l = lds_stage + (is_a ? 0 : V2_BM * BK * 2) + row0 * (BK * 2);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(is_a ? rs.a : rs.b, (lds_void_t*)l, 16, voff, kt * BK * 2, 0, 0);
}

template <bool FP8>
__device__ __forceinline__ void v2_fill_buf(unsigned char* lds_stage, const StgBuf& rs, int K, int kt, int wid,
                                            int lane) {
  const int rsub = lane >> 3, phys = lane & 7;
#pragma unroll
  for (int op = 0; op < 2; ++op) {
#pragma unroll
    for (int j = 0; j < V2_ROWS_PER_WAVE / 8; ++j) {
      const int row = wid * V2_ROWS_PER_WAVE + j * 8 + rsub;
      const int c = phys ^ swz_row_xor(row, FP8);
      unsigned char* l = lds_stage + op * (V2_BM * BK * 2) + (wid * V2_ROWS_PER_WAVE + j * 8) * (BK * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(op == 0 ? rs.a : rs.b, (lds_void_t*)l, 16, (row * K + c * 8) * 2,
                                               kt * BK * 2, 0, 0);
    }
  }
}

__device__ __forceinline__ void stg_mfma(floatx4 (&acc)[8][4], const bf16x8 (&af)[4][2], const bf16x8 (&bf)[2][2],
                                         int m0, int n0) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
        acc[m0 + m][n0 + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][s], bf[n][s], acc[m0 + m][n0 + n], 0, 0, 0);
  // MFMAs are not memory operations, so IR passes may sink them past the next s_barrier into the
  // other group's slot; an empty volatile asm that reads and writes each result pins them here.
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[m0 + m][n0 + n]));
}

// MX-fp8 (E4M3, unit E8M0 scales): one v_mfma_scale_f32_16x16x128_f8f6f4 covers the K-tile's 128 bytes.
__device__ __forceinline__ void stg_mfma(floatx4 (&acc)[8][4], const i32x8 (&af)[4], const i32x8 (&bf)[2], int m0,
                                         int n0) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      acc[m0 + m][n0 + n] =
          __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bf[n], acc[m0 + m][n0 + n], 0, 0, 0, 127, 0, 127);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[m0 + m][n0 + n]));
}

// The same K-tile on the unscaled instruction (zero scale operands select v_mfma_f32_16x16x128_f8f6f4): with unit
// scales the two compute the same products, so the knob only changes which matrix-core path runs.
__device__ __forceinline__ void stg_mfma_unscaled(floatx4 (&acc)[8][4], const i32x8 (&af)[4], const i32x8 (&bf)[2],
                                                  int m0, int n0) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      acc[m0 + m][n0 + n] =
          __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bf[n], acc[m0 + m][n0 + n], 0, 0, 0, 0, 0, 0);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[m0 + m][n0 + n]));
}

// Fragment of one 16-row block: bf16 = two K=32 steps (chunks fq, fq+4); fp8 = the lane's 32
// contiguous bytes of K (chunks 2fq, 2fq+1; lane layout measured by tools/mfma_lab.hip).
__device__ __forceinline__ void stg_load(bf16x8 (&f)[2], const u32x4* img, int row, int fq) {
  f[0] = __builtin_bit_cast(bf16x8, img[swz(row, fq)]);
  f[1] = __builtin_bit_cast(bf16x8, img[swz(row, fq + 4)]);
}
__device__ __forceinline__ void stg_load(i32x8& f, const u32x4* img, int row, int fq) {
  const u32x4 lo = img[swz8(row, 2 * fq)], hi = img[swz8(row, 2 * fq + 1)];
  f = i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
            static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
}

// MX-fp4 (E2M1): a 16-byte chunk is 32 values = one lane's share of a 16x16x128 MFMA, so the fp4
// fragments are read exactly like the bf16 ones (chunks fq, fq + 4) and feed two MFMAs per K-tile.
__device__ __forceinline__ void stg_load(u32x4 (&f)[2], const u32x4* img, int row, int fq) {
  f[0] = img[swz(row, fq)];
  f[1] = img[swz(row, fq + 4)];
}

__device__ __forceinline__ void stg_mfma(floatx4 (&acc)[8][4], const u32x4 (&af)[4][2], const u32x4 (&bf)[2][2],
                                         int m0, int n0) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const u32x4 a = af[m][s], b = bf[n][s];
        const i32x8 a8 = {static_cast<int>(a.x), static_cast<int>(a.y), static_cast<int>(a.z), static_cast<int>(a.w),
                          0, 0, 0, 0};
        const i32x8 b8 = {static_cast<int>(b.x), static_cast<int>(b.y), static_cast<int>(b.z), static_cast<int>(b.w),
                          0, 0, 0, 0};
        acc[m0 + m][n0 + n] =
            __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc[m0 + m][n0 + n], 4, 4, 0, 127, 0, 127);
      }
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[m0 + m][n0 + n]));
}

template <int DT>
struct StgFrags {
  bf16x8 a[4][2], b0[2][2], b1[2][2];
};
template <>
struct StgFrags<DT_FP8> {
  i32x8 a[4], b0[2], b1[2];
};
template <>
struct StgFrags<DT_FP8U> {
  i32x8 a[4], b0[2], b1[2];
};

// One phase's MFMAs for the kernel's data type.
template <int DT, typename FA, typename FB>
__device__ __forceinline__ void phase_mfma(floatx4 (&acc)[8][4], const FA& af, const FB& bf, int m0, int n0) {
  if constexpr (DT == DT_FP8U) stg_mfma_unscaled(acc, af, bf, m0, n0);
  else stg_mfma(acc, af, bf, m0, n0);
}
template <>
struct StgFrags<DT_FP4> {
  u32x4 a[4][2], b0[2][2], b1[2][2];
};

// v3 restaging orders (region r = 0: A rows of m0, 1: B rows of n0, 2: B rows of n1, 3: A rows of m1).
// V3_PHASE[s][r]: the phase of a K-tile whose load slot issues region r, for tile kt+2 into this buffer (R0/R1
// are free from phase 2 on, R2 from phase 3) or, R3, tile kt+1 into the other one (free since tile kt-1).
// Phase 3 retires tile kt+1 with vmcnt(6): tile kt+2's R0-R2 (2 pieces each) may stay in flight.
//   0: R3@0, R0 R1@2, R2@3 -> LDS-DMA pieces per phase 2/0/4/2 (round-2/3 kernel)
//   1: R3@1, R0@2, R1 R2@3 -> 0/2/2/4: no DMA issue beside phase 0's 12 fragment reads, 2 beside phase 2's 8
// An LDS-DMA piece costs 60-185 issue cycles depending on what else its slot does, and a load slot that outruns
// the other group's 256-cycle MFMA slot stalls both: schedule 1 is 4-9 % faster on MI355X (bf16 and MX-fp8,
// 4096^3 / 8192^3, tools/gemm_schedule_ab.py -> profiles/gemm_schedule_ab_mi355x.jsonl; orders 2/2/2/2,
// 0/4/2/2, 0/2/0/6 and DMA between the MFMAs of phase 3 measured in between or below it).
__device__ constexpr int V3_PHASE[2][4] = {{2, 2, 3, 0}, {2, 3, 3, 1}};

// In-kernel stamps of the v3 schedule (a diagnostic build only: -DDIAG_GEMM_STAMPS, tools/gemm_stamps.py).
// Lane 0 of wave 0 (group 0) and wave 4 (group 1) of the first 8 workgroups record s_memtime at four points
// of each phase of the middle K-tile -- load slot start, MFMA slot start, MFMA issue done, slot end -- into a
// buffer of their own that nothing else reads.  The production build compiles the macro to nothing.
#ifdef DIAG_GEMM_STAMPS
__device__ unsigned long long g_gemm_stamps[8][2][4][4];
#define V3_STAMP(p, q)                                                                                   \
  do {                                                                                                 \
    if (kt == KT / 2 && blockIdx.x < 8 && lane == 0 && (wid == 0 || wid == 4))                          \
      g_gemm_stamps[blockIdx.x][wid >> 2][p][q] = __builtin_amdgcn_s_memtime();                         \
  } while (0)
#else
#define V3_STAMP(p, q) \
  do {                 \
  } while (0)
#endif

// DT_BF16: bf16 A[M][K] . Bt[N][K]^T.  DT_FP8 / DT_FP4: MX operands (E4M3 bytes / packed E2M1 pairs,
// unit scales) passed as K = row bytes / 2 "bf16 columns", so the byte-identical LDS-DMA staging is
// shared (a 64-column bf16 K-tile is a 128-byte fp8 or fp4 K-tile); only the swizzle (fp8), the
// fragment reads and the MFMA differ.
// OUT_F32: C is fp32 [M][N].  OUT_BF16_CK (with EPI_LDS): C is bf16 [M][N] -- the output hipBLASLt writes, half
// the bytes -- and csum[M / 128][N] receives every column's sum over each wave row's 128 rows, formed in fp64
// from the fp32 accumulators before the rounding, so the whole-output check (gemm_checksum) needs no second
// pass over C and keeps the accumulators' precision.
template <int DT, bool EPI_LDS = false, bool BUF = false, int SCHED = 1, int OUT = OUT_F32,
          bool PRIO_G1 = DT == DT_BF16 || DT == DT_FP8U>
__global__ void __launch_bounds__(V2_THREADS, 1)
gemm_v3_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, void* __restrict__ Cv,
               double* __restrict__ csum, int M, int N, int K) {
  static_assert(OUT == OUT_F32 || EPI_LDS, "the bf16 output goes through the LDS-staged epilogue");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;
  const int tiles_m = M / V2_BM, tiles_n = N / V2_BN, nwg = tiles_m * tiles_n;
  int bid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  }
  constexpr int GROUP_M = 4;
  const int group = bid / (GROUP_M * tiles_n);
  const int first_m = group * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % (GROUP_M * tiles_n)) % gsize;
  const int tn = (bid % (GROUP_M * tiles_n)) / gsize;
  const __bf16* Ab = A + static_cast<size_t>(tm) * V2_BM * K;
  const __bf16* Bb = Bt + static_cast<size_t>(tn) * V2_BN * K;

  floatx4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int KT = K / BK;
  const int frow = lane & 15, fq = lane >> 4;

  constexpr bool FP8 = DT == DT_FP8 || DT == DT_FP8U;
  const StgBuf rs = stg_buf(Ab, Bb, K);
  auto region = [&](unsigned char* stage, int kt_, int r, int i) {
    if constexpr (BUF) stg_region_buf<FP8>(stage, rs, K, kt_, r, i, wid, lane);
    else stg_region<FP8>(stage, Ab, Bb, K, kt_, r, i, wid, lane);
  };
  auto fill = [&](unsigned char* stage, int kt_) {
    if constexpr (BUF) v2_fill_buf<FP8>(stage, rs, K, kt_, wid, lane);
    else v2_fill<FP8>(stage, Ab, Bb, K, kt_, wid, lane);
  };
  fill(smem, 0);
  if (KT > 1) {
    fill(smem + V2_STAGE_BYTES, 1);
    __builtin_amdgcn_s_waitcnt(0x3f78);  // vmcnt(8): tile 0 landed, tile 1 may be in flight
  } else {
    __builtin_amdgcn_s_waitcnt(0x3f70);  // vmcnt(0)
  }
  STG_BARRIER();
  if (wr == 1) STG_BARRIER();  // the stagger
  // bf16 and fp8 (unscaled MFMA): the second wave group (waves 4-7, one barrier behind) issues at raised priority
  // for the whole loop, so on each SIMD its load slot is not starved behind the other group's MFMA stream (bf16
  // +2-3 % at 4096^3 and 8192^3, profiles/gemm_schedule_ab_mi355x.jsonl; fp8 unscaled +0.7-1.1 %,
  // profiles/gemm_fp8_prio_ab_mi355x.jsonl; neutral-to-negative for the scaled MX form); per-slot priority flips
  // measured below it
  if constexpr (PRIO_G1) {
    if (wr == 1) __builtin_amdgcn_s_setprio(1);
  }

  StgFrags<DT> f;
  for (int kt = 0; kt < KT; ++kt) {
    unsigned char* cur = smem + (kt & 1) * V2_STAGE_BYTES;
    unsigned char* nxt = smem + ((kt + 1) & 1) * V2_STAGE_BYTES;
    const u32x4* a_img = reinterpret_cast<const u32x4*>(cur);
    const u32x4* b_img = reinterpret_cast<const u32x4*>(cur + V2_BM * BK * 2);
    const bool pre = kt + 2 < KT;
    // the phase's restaging (V3_PHASE): R0-R2 of tile kt+2 into this buffer, R3 of tile kt+1 into the other
    // (tile 1 came whole with the prologue)
    auto restage = [&](int phase) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (V3_PHASE[SCHED][r] != phase) continue;
        if (r == 3 ? (kt >= 1 && kt + 1 < KT) : pre) {
          region(r == 3 ? nxt : cur, kt + (r == 3 ? 1 : 2), r, 0);
          region(r == 3 ? nxt : cur, kt + (r == 3 ? 1 : 2), r, 1);
        }
      }
    };
    // phase 0: A(m0), B(n0)
    V3_STAMP(0, 0);
    restage(0);
#pragma unroll
    for (int n = 0; n < 2; ++n) stg_load(f.b0[n], b_img, wc * 64 + n * 16 + frow, fq);
#pragma unroll
    for (int m = 0; m < 4; ++m) stg_load(f.a[m], a_img, wr * 128 + m * 16 + frow, fq);
    STG_BARRIER();
    V3_STAMP(0, 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    phase_mfma<DT>(acc, f.a, f.b0, 0, 0);
    V3_STAMP(0, 2);
    STG_BARRIER();
    V3_STAMP(0, 3);
    // phase 1: B(n1)
    V3_STAMP(1, 0);
    restage(1);
#pragma unroll
    for (int n = 0; n < 2; ++n) stg_load(f.b1[n], b_img, wc * 64 + (n + 2) * 16 + frow, fq);
    STG_BARRIER();
    V3_STAMP(1, 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    phase_mfma<DT>(acc, f.a, f.b1, 0, 2);
    V3_STAMP(1, 2);
    STG_BARRIER();
    V3_STAMP(1, 3);
    // phase 2: A(m1)
    V3_STAMP(2, 0);
    restage(2);
#pragma unroll
    for (int m = 0; m < 4; ++m) stg_load(f.a[m], a_img, wr * 128 + (m + 4) * 16 + frow, fq);
    STG_BARRIER();
    V3_STAMP(2, 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    phase_mfma<DT>(acc, f.a, f.b1, 4, 2);
    V3_STAMP(2, 2);
    STG_BARRIER();
    V3_STAMP(2, 3);
    // phase 3: no LDS reads; retire tile kt+1 (tile kt+2's pieces may stay in flight)
    V3_STAMP(3, 0);
    restage(3);
    if (pre) {
      __builtin_amdgcn_s_waitcnt(0x3f76);  // vmcnt(6)
    } else {
      __builtin_amdgcn_s_waitcnt(0x3f70);  // vmcnt(0)
    }
    STG_BARRIER();
    V3_STAMP(3, 1);
    phase_mfma<DT>(acc, f.a, f.b0, 4, 0);
    V3_STAMP(3, 2);
    STG_BARRIER();
    V3_STAMP(3, 3);
  }
  if (wr == 0) STG_BARRIER();  // balance the stagger
  const int row0 = tm * V2_BM + wr * 128, col0 = tn * V2_BN + wc * 64;
  float* __restrict__ C = static_cast<float*>(Cv);
  if constexpr (OUT == OUT_BF16_CK) {
    // column sums over this wave's 128 rows: 32 per lane (rows m * 16 + fq * 4 + j), then over the 4 lanes
    // (fq) that hold the same column
    double s[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      s[n] = 0.0;
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[n] += static_cast<double>(acc[m][n][j]);
      s[n] += __shfl_xor(s[n], 16);
      s[n] += __shfl_xor(s[n], 32);
    }
    if (fq == 0) {
#pragma unroll
      for (int n = 0; n < 4; ++n) csum[static_cast<size_t>(row0 / 128) * N + col0 + n * 16 + frow] = s[n];
    }
    // C through the wave's LDS patch as in the fp32 epilogue, leaving as 8 bf16 (16 bytes) per lane: one
    // store instruction covers 8 rows x 128 contiguous bytes
    constexpr int LD = 64 + 4;
    __builtin_amdgcn_s_barrier();
    float* patch = reinterpret_cast<float*>(smem) + wid * (16 * LD);
    __bf16* __restrict__ Cb = static_cast<__bf16*>(Cv);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int r = q * 8 + (lane >> 3), c8 = (lane & 7) * 8;
        const floatx4 lo = *reinterpret_cast<const floatx4*>(patch + r * LD + c8);
        const floatx4 hi = *reinterpret_cast<const floatx4*>(patch + r * LD + c8 + 4);
        const floatx8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<bf16x8*>(Cb + static_cast<size_t>(row0 + m * 16 + r) * N + col0 + c8) =
            __builtin_convertvector(v, bf16x8);
      }
    }
  } else if constexpr (EPI_LDS) {
    // Each 16x64 fp32 slice goes through the wave's own LDS patch (no DMA is in flight and every
    // fragment read retired before the last barrier), then leaves as 16-byte row pieces: one store
    // instruction covers 4 rows x 256 contiguous bytes instead of 4 rows x 64.
    constexpr int LD = 64 + 4;
    __builtin_amdgcn_s_barrier();
    float* patch = reinterpret_cast<float*>(smem) + wid * (16 * LD);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = q * 4 + (lane >> 4), c4 = (lane & 15) * 4;
        const floatx4 v = *reinterpret_cast<const floatx4*>(patch + r * LD + c4);
#ifdef DIAG_GEMM_NO_STORE  // lab build (tools/gemm_stamps.py --no-store): everything but the C write itself
        if (N > (1 << 30))
#endif
        *reinterpret_cast<floatx4*>(C + static_cast<size_t>(row0 + m * 16 + r) * N + col0 + c4) = v;
      }
    }
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          C[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * N + col0 + n * 16 + frow] = acc[m][n][j];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// v4 (bf16): hipBLASLt's gfx950 structure -- 256 threads, a 256x256x64 tile, each wave 128x128 (256 accumulator
// AGPRs), 2 LDS stages -- with the loop's instruction order written out.  Every MFMA, fragment ds_read and LDS-DMA
// of the loop is an `asm volatile` statement, so hipcc keeps their interleave and allocates the accumulators to
// AGPRs ("+a") and the fragments to VGPRs once; the lgkmcnt / vmcnt waits are explicit.  Compiler-ordered
// four-wave versions (rounds 2-3) lost to v3 on accumulator shuffling between AGPRs and VGPRs; this one beats it
// (tools/gemm_w4a_lab.hip sweeps the schedule knobs, profiles/gemm_w4a_lab_mi355x.jsonl).
//
// Per K-tile kt (stage s = kt & 1; F0 = k-step 0 fragments of tile kt, already in registers):
//   half 1: 64 MFMA on F0; one ds_read of F1 (tile kt, k-step 1, stage s) after every RS-th of the first 16 * RS;
//           after MFMA X_AT lgkmcnt(0) + s_barrier X (every wave is done with stage s); D1 LDS-DMA pieces of tile
//           kt+2 into stage s spread over the rest
//   half 2: 64 MFMA on F1; after MFMA Y_AT vmcnt(D1) (tile kt+1, issued one K-tile ago, landed) + s_barrier Y;
//           ds_read F0' (tile kt+1, k-step 0, stage s^1) one per R2 MFMAs; the other 16 - D1 DMA pieces spread
//           over the rest; lgkmcnt(0) at the end
// Near the end the DMA re-fetches tile KT-1 into a stage nobody reads any more, and the last iteration's F0' reads
// load harmless stale fragments (branch-free loop); everything is drained before the epilogue.
// The wave's rows are m * 16 + fq * 4 + j (m = 0..7) and the K order is v3's, so C and the fused column sums are
// bit-identical to v3's.
constexpr int V4_THREADS = 256;
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void v4_mfma(floatx4& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
// the first MFMA into an accumulator: C = 0 as an inline constant, so the accumulators need no zeroing.  (Zeroing
// them in C++ let hipcc copy a zero AGPR into the others with v_accvgpr_mov right before the first asm MFMA, a
// sequence that left every accumulator wrong on the MI355X -- the K = 64 path, where no loop separated the two.)
__device__ __forceinline__ void v4_mfma_first(floatx4& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}

template <int OFF>
__device__ __forceinline__ void v4_read(bf16x8& f, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(addr), "i"(OFF));
}

// one LDS-DMA wave instruction: 64 lanes x 16 B from rsrc + voff + soff into LDS at m0 + lane * 16, with
// m0 = base + IMM set in the same statement (nothing the compiler schedules in between can see or change it)
template <uint32_t IMM>
__device__ __forceinline__ void v4_dma_imm(uint32_t m0_base, uint32_t voff, const i32x4& rsrc, uint32_t soff) {
  asm volatile("s_add_u32 m0, %0, %1\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds"
               :
               : "s"(m0_base), "i"(IMM), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");
}

// The grouped form (lab: gemm_v4_kernel<..., M0G = true>): the buffer instruction's immediate offset is added to
// the global address and to the LDS destination, so four DMAs 1 KiB apart in LDS share one m0 -- the group's first
// sets it (SET), the other three carry OFF = 1, 2, 3 KiB (the 12-bit field's reach) and per-row VGPR offsets
// reduced by OFF.  The later ones rely on m0 surviving the MFMA / ds_read statements in between.
template <uint32_t IMM, uint32_t OFF, bool SET>
__device__ __forceinline__ void v4_dma_grouped(uint32_t m0_base, uint32_t voff, const i32x4& rsrc, uint32_t soff) {
  if constexpr (SET) {
    asm volatile("s_add_u32 m0, %0, %1\n\tbuffer_load_dwordx4 %2, %3, %4 offen offset:%5 lds"
                 :
                 : "s"(m0_base), "i"(IMM), "v"(voff), "s"(rsrc), "s"(soff), "i"(OFF)
                 : "memory");
  } else {
    asm volatile("buffer_load_dwordx4 %0, %1, %2 offen offset:%3 lds"
                 :
                 : "v"(voff), "s"(rsrc), "s"(soff), "i"(OFF)
                 : "memory");
  }
}

__device__ __forceinline__ i32x4 v4_rsrc(const void* base, uint32_t bytes) {
  const uint64_t b = reinterpret_cast<uint64_t>(base);
  i32x4 r;
  r.x = static_cast<int>(b);
  r.y = static_cast<int>(b >> 32);
  r.z = static_cast<int>(bytes);
  r.w = 0x00020000;  // raw buffer, 32-bit data format
  return r;
}

struct V4Frags {
  bf16x8 a[8], b[8];
};

// piece p (0-7: A m-block p, 8-15: B n-block p-8) of a k-step's fragments; m-block offsets (2048 B) are immediates
template <int P>
__device__ __forceinline__ void v4_piece(V4Frags& f, uint32_t a_addr, uint32_t b_addr) {
  if constexpr (P < 8) v4_read<P * 2048>(f.a[P], a_addr);
  else v4_read<(P - 8) * 2048>(f.b[P - 8], b_addr);
}

template <int I, int N, typename F>
__device__ __forceinline__ void v4_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    v4_for<I + 1, N>(f);
  }
}

// In-kernel stamps of the v4 loop (a lab build only: -DDIAG_V4_STAMPS, tools/gemm_w4a_lab.hip --stamps).  Every
// wave records s_memtime deltas into a buffer nothing else reads: [0] prologue, [1] K loop, [2] epilogue up to its
// stores' completion, [3] the middle K-tile's iteration, and the time that iteration spent in [4] X (lgkmcnt +
// barrier), [5] Y (vmcnt + barrier), [6] the closing lgkmcnt.  Each stamp pair waits for its own s_memtime, so
// the stamped build runs a little slower than the production one, which compiles all of this out.
#ifdef DIAG_V4_STAMPS
constexpr bool kV4Stamps = true;
__device__ unsigned long long g_v4_stamps[4096][4][8];
#else
constexpr bool kV4Stamps = false;
#endif

// One recursive-halving step of a 16-lane sum: this lane keeps half `bit` of s[0, 2 * H) (the upper half when bit
// is 1) and adds the partner lane's copy of that half; the partner is the DPP permutation CTRL's image, a lane of
// the other `bit`.  Afterwards s[0, H) holds the kept half.
template <int H, int CTRL>
__device__ __forceinline__ void v4_halve(double (&s)[32], int bit) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const double keep = bit ? s[i + H] : s[i];
    const double send = bit ? s[i] : s[i + H];
    const uint64_t u = __builtin_bit_cast(uint64_t, send);
    const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(u), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(u >> 32), CTRL, 0xf, 0xf, false);
    s[i] = keep + __builtin_bit_cast(double, (static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) |
                                                 static_cast<uint32_t>(lo));
  }
}

#include "v4_plan.h"  // the K-loop plans and their compile-time checks (host-compilable, tests/test_gemm_plans.py)

// ---- fp8 (E4M3) form of the v4 kernel: the same tile, waves, staging (a K-tile is 128 bytes, the fp8 swizzle)
// and epilogue; one v_mfma_f32_16x16x128_f8f6f4 (hipBLASLt's fp8 instruction, unscaled) per output block and
// K-tile, so C is v3's fp8 C bit for bit.  A fragment is a lane's 32 contiguous bytes of a row (two 16-byte
// chunks, 8 VGPRs); the 16 fragments of a K-tile take 128 VGPRs, too many to double-buffer beside 256
// accumulators, so -- as hipBLASLt's MT256x256x128 fp8 kernel does -- the K-tile's 64 MFMAs run by quadrant
// (A0-3 x B0-3, A4-7 x B0-3, A0-3 x B4-7, A4-7 x B4-7) and each fragment is reloaded once its quadrants are done:
// this tile's A4-7 / B4-7 at the start of the K-tile, the next tile's B0-3 / A0-3 at its end.
struct V4F8Frags {
  u32x4 alo[8], ahi[8], blo[8], bhi[8];
};

__device__ __forceinline__ void v4_mfma8(floatx4& acc, const u32x4& alo, const u32x4& ahi, const u32x4& blo,
                                         const u32x4& bhi) {
  const i32x8 a = __builtin_bit_cast(i32x8, __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7));
  const i32x8 b = __builtin_bit_cast(i32x8, __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
  asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void v4_mfma8_first(floatx4& acc, const u32x4& alo, const u32x4& ahi, const u32x4& blo,
                                               const u32x4& bhi) {
  const i32x8 a = __builtin_bit_cast(i32x8, __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7));
  const i32x8 b = __builtin_bit_cast(i32x8, __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
  asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}
template <int OFF>
__device__ __forceinline__ void v4_read4(u32x4& f, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(addr), "i"(OFF));
}
// fp8 read id r: 0-7 this tile's A blocks 4-7 (block 4 + r / 2, chunk half r % 2), 8-15 its B blocks 4-7, 16-23 the
// next tile's A blocks 0-3, 24-31 its B blocks 0-3.  ha / hb: the per-lane addresses of [half] in the stage read.
template <int R>
__device__ __forceinline__ void v4_piece8(V4F8Frags& g, const uint32_t (&ha)[2], const uint32_t (&hb)[2]) {
  constexpr int q = R & 15, blk = (R < 16 ? 4 : 0) + (q & 7) / 2, h = q & 1;
  constexpr bool is_b = q >= 8;
  if constexpr (!is_b) v4_read4<blk * 2048>(h ? g.ahi[blk] : g.alo[blk], ha[h]);
  else v4_read4<blk * 2048>(h ? g.bhi[blk] : g.blo[blk], hb[h]);
}
template <int OUT = OUT_F32, class PLAN = V4PlanA<1, 20, 8, 8, 2>, int GM = 4, bool TR = false, int DT = DT_BF16,
          bool M0G = false>
__global__ void __launch_bounds__(V4_THREADS, 1)
gemm_v4_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, void* __restrict__ Cv,
               double* __restrict__ csum, int M, int N, int K) {
  constexpr bool FP8 = DT == DT_FP8U;
  static_assert(DT == DT_BF16 || DT == DT_FP8U, "v4: bf16 or fp8 (unscaled MFMA)");
  if constexpr (FP8) static_assert(v4f8_plan_ok<PLAN>(), "v4 fp8 plan breaks a read / DMA / barrier ordering rule");
  else static_assert(v4_plan_ok<PLAN>(), "v4 schedule plan breaks a read / DMA / barrier ordering rule");
  static_assert(!M0G || v4_m0_groups_ok<PLAN>(), "grouped m0: each group of 4 DMAs must be issued in order, back to back");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // 2 stages x 64 KiB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the DMA's m0 is an SGPR
  const int wr = wid >> 1, wc = wid & 1;
  const int tiles_m = M / V2_BM, tiles_n = N / V2_BN, nwg = tiles_m * tiles_n;
  int bid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  }
  const int group = bid / (GM * tiles_n);
  const int first_m = group * GM;
  const int gsize = min(tiles_m - first_m, GM);
  const int tm = first_m + (bid % (GM * tiles_n)) % gsize;
  const int tn = (bid % (GM * tiles_n)) / gsize;
  const __bf16* Ab = A + static_cast<size_t>(tm) * V2_BM * K;
  const __bf16* Bb = Bt + static_cast<size_t>(tn) * V2_BN * K;
  const int KT = K / BK;

  // LDS-DMA: wave instruction j (0-15) of a tile: operand j >> 3, rows wid * 64 + 8r + 0..7 with r = j & 7 (lane:
  // row + (lane >> 3), physical chunk lane & 7, source chunk XOR-swizzled by row: one VGPR offset per r), LDS
  // address m0 = the wave's base + an immediate per (stage, j), and the tile's column offset kt * 128 as soffset:
  // two instructions per DMA (s_add_u32 m0 + the load), as hipBLASLt issues them.  The K loop is unrolled by two so
  // the stage's addresses are immediates; that and the lean DMA issue were worth +2.5 % at 4096^3 and +4.7 % at
  // 8192^3 over a loop that selected them per K-tile (profiles/gemm_w4a_lab_mi355x.jsonl): with one wave per SIMD
  // every instruction between MFMAs costs issue cycles.
  const i32x4 rs_a = v4_rsrc(Ab, static_cast<uint32_t>(V2_BM) * K * 2);
  const i32x4 rs_b = v4_rsrc(Bb, static_cast<uint32_t>(V2_BN) * K * 2);
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)smem));
  const uint32_t m0_wave = lds0 + wid * 64 * (BK * 2);
  uint32_t voff_r[8];
  {
    const int rsub = lane >> 3, phys = lane & 7;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = wid * 64 + 8 * r + rsub;
      voff_r[r] = static_cast<uint32_t>((row * K + (phys ^ swz_row_xor(row, FP8)) * 8) * 2) -
                  (M0G ? static_cast<uint32_t>((r & 3) * 8 * (BK * 2)) : 0u);
    }
  }
  auto dma = [&](auto S, auto J, uint32_t soff) {
    constexpr int s = decltype(S)::value, j = decltype(J)::value, op = j >> 3, r = j & 7;
    if constexpr (M0G)
      v4_dma_grouped<s * V2_STAGE_BYTES + op * (V2_BM * BK * 2) + (r >> 2) * 4 * 8 * (BK * 2), (r & 3) * 8 * (BK * 2),
                     (r & 3) == 0>(m0_wave, voff_r[r], op ? rs_b : rs_a, soff);
    else
      v4_dma_imm<s * V2_STAGE_BYTES + op * (V2_BM * BK * 2) + r * 8 * (BK * 2)>(m0_wave, voff_r[r],
                                                                                  op ? rs_b : rs_a, soff);
  };

  // fragment reads: lane (frow, fq); k-step 1 is chunk ^ 4
  const int frow = lane & 15, fq = lane >> 4, x = (frow >> 1) & 7;
  uint32_t ra[2][2], rb[2][2];  // [stage][k-step]
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint32_t c = static_cast<uint32_t>(((fq + 4 * ks) ^ x) * 16);
      ra[s][ks] = lds0 + s * V2_STAGE_BYTES + (wr * 128 + frow) * (BK * 2) + c;
      rb[s][ks] = lds0 + s * V2_STAGE_BYTES + V2_BM * BK * 2 + (wc * 128 + frow) * (BK * 2) + c;
    }

  // fp8: per-lane address of chunk half h (chunk 2 fq + h, swizzled by the row's bits 1 and 3) in each stage
  uint32_t ra8[2][2], rb8[2][2];
  if constexpr (FP8) {
    const int x8 = swz_row_xor(frow, true);
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t c = static_cast<uint32_t>(((2 * fq + h) ^ x8) * 16);
        ra8[st][h] = lds0 + st * V2_STAGE_BYTES + (wr * 128 + frow) * (BK * 2) + c;
        rb8[st][h] = lds0 + st * V2_STAGE_BYTES + V2_BM * BK * 2 + (wc * 128 + frow) * (BK * 2) + c;
      }
  }

  floatx4 acc[8][8];  // written first by the first K-tile's first MFMAs (v4_mfma_first / v4_mfma8_first)

  [[maybe_unused]] uint64_t st_k0 = 0, st_l0 = 0, st_l1 = 0, st_i0 = 0, st_i1 = 0, st_x = 0, st_y = 0, st_e = 0;
  if constexpr (kV4Stamps) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_k0)::"memory");
  // prologue: tiles 0 and 1 into stages 0 and 1, tile 0 waited for, F0 of tile 0 read
  v4_for<0, 16>([&](auto j) { dma(std::integral_constant<int, 0>{}, j, 0u); });
  v4_for<0, 16>([&](auto j) { dma(std::integral_constant<int, 1>{}, j, KT > 1 ? BK * 2u : 0u); });
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  STG_BARRIER();
  [[maybe_unused]] V4Frags f0, f1;
  [[maybe_unused]] V4F8Frags g;
  if constexpr (FP8) v4_for<16, 32>([&](auto r) { v4_piece8<r>(g, ra8[0], rb8[0]); });  // tile 0's A0-3, B0-3
  else v4_for<0, 16>([&](auto p) { v4_piece<p>(f0, ra[0][0], rb[0][0]); });
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (kV4Stamps) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_l0)::"memory");

  // one K-tile kt in stage S (= kt & 1)
  auto iter = [&](auto S, auto FIRST, int kt) {
    constexpr int s = decltype(S)::value;
    constexpr bool first = decltype(FIRST)::value;  // K-tile 0: its k-step-0 MFMAs start the accumulators
    [[maybe_unused]] const uint32_t a1 = ra[s][1], b1 = rb[s][1], a0n = ra[s ^ 1][0], b0n = rb[s ^ 1][0];
    const uint32_t soff = static_cast<uint32_t>(min(kt + 2, KT - 1)) * (BK * 2);  // the tile the DMAs fetch
    [[maybe_unused]] const bool stamp = kV4Stamps && kt == KT / 2;
    if constexpr (kV4Stamps) {
      if (kt == KT / 2) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_i0)::"memory");
      if (kt == KT / 2 + 1) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_i1)::"memory");
    }
    v4_for<0, FP8 ? 64 : 128>([&](auto i) {
      constexpr V4Slot o = PLAN::at(i);
      if constexpr (FP8) {
        constexpr int m = v4f8_m(i), n = v4f8_n(i);
        floatx4& c = acc[m][n];
        if constexpr (first) {
          if constexpr (TR) v4_mfma8_first(c, g.blo[n], g.bhi[n], g.alo[m], g.ahi[m]);
          else v4_mfma8_first(c, g.alo[m], g.ahi[m], g.blo[n], g.bhi[n]);
        } else {
          if constexpr (TR) v4_mfma8(c, g.blo[n], g.bhi[n], g.alo[m], g.ahi[m]);
          else v4_mfma8(c, g.alo[m], g.ahi[m], g.blo[n], g.bhi[n]);
        }
        if constexpr (o.read >= 0 && o.read < 16) v4_piece8<o.read>(g, ra8[s], rb8[s]);
        if constexpr (o.read >= 16) v4_piece8<o.read>(g, ra8[s ^ 1], rb8[s ^ 1]);
      } else {
        const V4Frags& f = i < 64 ? f0 : f1;
        floatx4& c = acc[(i & 63) >> 3][i & 7];
        const bf16x8& fa = f.a[(i & 63) >> 3];
        const bf16x8& fb = f.b[i & 7];
        if constexpr (first && i < 64) {
          if constexpr (TR) v4_mfma_first(c, fb, fa);
          else v4_mfma_first(c, fa, fb);
        } else {
          if constexpr (TR) v4_mfma(c, fb, fa);
          else v4_mfma(c, fa, fb);
        }
        if constexpr (o.read >= 0 && o.read < 16) v4_piece<o.read>(f1, a1, b1);
        if constexpr (o.read >= 16) v4_piece<o.read - 16>(f0, a0n, b0n);
      }
      if constexpr (o.wait == 1) {
        if (stamp) {
          uint64_t t0, t1;
          asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                       : "=s"(t0), "=s"(t1)::"memory");
          st_x += t1 - t0;
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
      }
      if constexpr (o.wait == 2) {
        if (stamp) {
          uint64_t t0, t1;
          asm volatile("s_memtime %0\n\ts_waitcnt vmcnt(%2)\n\ts_barrier\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                       : "=s"(t0), "=s"(t1)
                       : "i"(o.vm)
                       : "memory");
          st_y = t1 - t0;
        } else {
          asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(o.vm) : "memory");
        }
      }
      if constexpr (o.dma >= 0) dma(S, std::integral_constant<int, o.dma>{}, soff);
    });
    if (stamp) {
      uint64_t t0, t1;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                   : "=s"(t0), "=s"(t1)::"memory");
      st_e = t1 - t0;
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  iter(I0{}, std::true_type{}, 0);
  int kt = 1;
  for (; kt + 1 < KT; kt += 2) {
    iter(I1{}, std::false_type{}, kt);
    iter(I0{}, std::false_type{}, kt + 1);
  }
  if (kt < KT) iter(I1{}, std::false_type{}, kt);
  // drain; the s_nops are the wait states between the last MFMA's result and the epilogue's v_accvgpr_read, which
  // hipcc's hazard recognizer cannot insert for an MFMA written in asm
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if constexpr (kV4Stamps) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_l1)::"memory");
#ifdef DIAG_V4_STAMPS
  // after the epilogue's stores (below) the last stamp; written here by a lambda run at the end
  auto write_stamps = [&] {
    uint64_t t;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    if (lane == 0 && blockIdx.x < 4096) {
      unsigned long long* o = g_v4_stamps[blockIdx.x][wid];
      o[0] = st_l0 - st_k0;
      o[1] = st_l1 - st_l0;
      o[2] = t - st_l1;
      o[3] = st_i1 - st_i0;
      o[4] = st_x;
      o[5] = st_y;
      o[6] = st_e;
      o[7] = KT;
    }
  };
#endif

  // The epilogue takes lane / frow / fq afresh from the lane id (v_mbcnt) instead of the values computed for the
  // prologue: those would be live across the K loop, where the 256 accumulators leave no VGPR for them, and the
  // bf16 + column-sum kernels spilled three (fp8: five) to scratch -- the kernel's only scratch use.
  {
  const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int frow = lane & 15, fq = lane >> 4;
  const int row0 = tm * V2_BM + wr * 128, col0 = tn * V2_BN + wc * 128;
  if constexpr (TR) {
    // Transposed blocks (the B fragment is the MFMA's first operand): lane (frow, fq) of block (m, n) holds row
    // m * 16 + frow, columns n * 16 + 4 * fq + 0..3 -- row pieces, stored straight from registers, no LDS.
    if constexpr (OUT == OUT_BF16_CK) {
      // column sums over the wave's 128 rows: 32 per lane (its 4 columns of 8 blocks) summed over m, then over
      // the 16 lanes holding the same columns by recursive halving (each step keeps half the columns and adds the
      // partner lane's half: 16 + 8 + 4 + 2 exchanged sums); lane frow ends with columns 2 * frow, 2 * frow + 1
      // of its 32 (index c = n * 4 + j)
      double s[32];
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        s[c] = 0.0;
#pragma unroll
        for (int m = 0; m < 8; ++m) s[c] += static_cast<double>(acc[m][c >> 2][c & 3]);
      }
      v4_halve<16, 0x140>(s, (frow >> 3) & 1);  // row_mirror: lane i <-> 15 - i (differs in bit 3)
      v4_halve<8, 0x141>(s, (frow >> 2) & 1);   // row_half_mirror: i <-> 7 - i within 8 (bit 2)
      v4_halve<4, 0x4E>(s, (frow >> 1) & 1);    // quad_perm [2,3,0,1]: xor 2
      v4_halve<2, 0xB1>(s, frow & 1);           // quad_perm [1,0,3,2]: xor 1
      const int c0 = 2 * frow;  // columns n * 16 + 4 * fq + j for c = c0, c0 + 1: adjacent
      double2 v;
      v.x = s[0];
      v.y = s[1];
      *reinterpret_cast<double2*>(csum + static_cast<size_t>(row0 / 128) * N + col0 + (c0 >> 2) * 16 + 4 * fq +
                                  (c0 & 3)) = v;
      // bf16 C: block pair (2p, 2p+1) packed to 2 dwords each, then v_permlane16_swap between the 16-lane rows
      // fq even / odd: even rows end with columns 32p + 4fq + 0..7, odd rows with 32p + 16 + 4(fq - 1) + 0..7
      __bf16* __restrict__ Cb = static_cast<__bf16*>(Cv);
      const int cofs = (fq & 1) * 16 + (fq >> 1) * 8;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
          typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
          u32x2 lo = __builtin_bit_cast(u32x2, __builtin_convertvector(acc[m][2 * p], bf16x4));
          u32x2 hi = __builtin_bit_cast(u32x2, __builtin_convertvector(acc[m][2 * p + 1], bf16x4));
          const auto x = __builtin_amdgcn_permlane16_swap(lo.x, hi.x, false, false);
          const auto y = __builtin_amdgcn_permlane16_swap(lo.y, hi.y, false, false);
          const u32x4 out = {x[0], y[0], x[1], y[1]};
          *reinterpret_cast<u32x4*>(Cb + static_cast<size_t>(row0 + m * 16 + frow) * N + col0 + p * 32 + cofs) = out;
        }
      }
    } else {
      float* __restrict__ C = static_cast<float*>(Cv);
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n)
          *reinterpret_cast<floatx4*>(C + static_cast<size_t>(row0 + m * 16 + frow) * N + col0 + n * 16 + 4 * fq) =
              acc[m][n];
    }
#ifdef DIAG_V4_STAMPS
    write_stamps();
#endif
    return;
  }
  // epilogue through each wave's own LDS patch (16 rows x 128 columns of fp32), as v3's
  constexpr int LD = 128 + 4;
  float* patch = reinterpret_cast<float*>(smem) + wid * (16 * LD);
  if constexpr (OUT == OUT_BF16_CK) {
    // column sums over the wave's 128 rows in v3's order (m, then j, then the 4 lanes fq holding the column)
    double cs[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      cs[n] = 0.0;
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[n] += static_cast<double>(acc[m][n][j]);
      cs[n] += __shfl_xor(cs[n], 16);
      cs[n] += __shfl_xor(cs[n], 32);
    }
    if (fq == 0) {
#pragma unroll
      for (int n = 0; n < 8; ++n) csum[static_cast<size_t>(row0 / 128) * N + col0 + n * 16 + frow] = cs[n];
    }
    __bf16* __restrict__ Cb = static_cast<__bf16*>(Cv);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
      // 8 bf16 (16 bytes) per lane: one store instruction covers 4 rows x 256 contiguous bytes
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = q * 4 + (lane >> 4), c8 = (lane & 15) * 8;
        const floatx4 lo = *reinterpret_cast<const floatx4*>(patch + r * LD + c8);
        const floatx4 hi = *reinterpret_cast<const floatx4*>(patch + r * LD + c8 + 4);
        const floatx8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<bf16x8*>(Cb + static_cast<size_t>(row0 + m * 16 + r) * N + col0 + c8) =
            __builtin_convertvector(v, bf16x8);
      }
    }
  } else {
    float* __restrict__ C = static_cast<float*>(Cv);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
      // one store instruction covers 2 rows x 512 contiguous bytes
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = q * 2 + (lane >> 5), c4 = (lane & 31) * 4;
        const floatx4 v = *reinterpret_cast<const floatx4*>(patch + r * LD + c4);
        *reinterpret_cast<floatx4*>(C + static_cast<size_t>(row0 + m * 16 + r) * N + col0 + c4) = v;
      }
    }
  }
  }  // the epilogue's scope
#ifdef DIAG_V4_STAMPS
  write_stamps();
#endif
}

// ---------------------------------------------------------------------------
// v4's tail wave.  A grid of 256x256 tiles that is not a whole number of 256-CU waves leaves most of the chip idle in
// its last wave: 6144^3 is 576 tiles, 2.25 waves, so the third wave runs 64 tiles on 64 CUs while 192 wait (6144^3
// bf16 at 0.917 of hipBLASLt against 0.97 at 4096^3 and 8192^3, profiles/gemm_v4_sizes_ab_mi355x.jsonl).  The v4
// launch then covers only the whole waves -- V4_TAIL_MAIN(nwg) workgroups; v4's XCD remap leaves each XCD's last
// chunk of tile indices uncomputed -- and this kernel computes those tiles as four 128x128 quadrants each, 4x the
// workgroups for the same work, with v1's K loop (the same v_mfma_f32_16x16x32_bf16 per 32-wide K chunk, in the same
// order as v3 / v4: every C element and every fp64 column sum bit-identical to theirs).  Each 128x128 quadrant's
// column sums continue, in wave wr = 1, the partial sums wave wr = 0 left in LDS, so they follow v4's own order over
// the 128-row band (m, then j, then the xor-16 / xor-32 lane exchange).
__host__ __device__ constexpr int v4_tail_main(int nwg) { return nwg / 256 * 256; }
// only a short tail is worth it: a quarter wave of 256^2 tiles is one 2-per-CU wave of 128^2 quadrants
__host__ __device__ constexpr bool v4_tail_applies(int nwg) { return nwg > 256 && nwg % 256 != 0 && nwg % 256 <= 64; }

// fp8 (E4M3) form of v1's K-tile for the tail: a K-tile is 128 bytes, one v_mfma_f32_16x16x128_f8f6f4 per block on
// the lane's 32 contiguous bytes (chunks 2fq, 2fq + 1, the fp8 swizzle) -- v3 / v4's fp8 fragments and instruction
__device__ __forceinline__ void tail_compute_fp8(floatx4 (&acc)[4][4], const u32x4 (&buf)[2][TILE_CHUNKS], int wr,
                                                 int wc, int frow, int fq) {
  i32x8 af[4], bfr[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) stg_load(af[m], buf[0], wr * 64 + m * 16 + frow, fq);
#pragma unroll
  for (int n = 0; n < 4; ++n) stg_load(bfr[n], buf[1], wc * 64 + n * 16 + frow, fq);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
      acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bfr[n], acc[m][n], 0, 0, 0, 0, 0, 0);
}

template <int OUT, int GM = 4, int DT = DT_BF16>
__global__ void __launch_bounds__(THREADS, 2)
gemm_v4_tail_kernel(const u32x4* __restrict__ A, const u32x4* __restrict__ Bt, void* __restrict__ Cv,
                    double* __restrict__ csum, int M, int N, int K) {
  static_assert(DT == DT_BF16 || DT == DT_FP8U, "the tail runs v4's dtypes");
  constexpr bool FP8 = DT == DT_FP8U;
  __shared__ u32x4 lds[2][2][TILE_CHUNKS];  // [buffer][A|B][chunk] = 64 KiB
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  // which 256^2 tile (v4's numbering) and which quadrant of it
  const int tiles_m = M / V2_BM, tiles_n = N / V2_BN, nwg = tiles_m * tiles_n;
  const int q = nwg / 8, r = nwg % 8, qmain = v4_tail_main(nwg) / 8;
  int t = static_cast<int>(blockIdx.x) >> 2;
  int idx = -1;
  for (int x = 0; x < 8; ++x) {  // XCD x's tiles are [base, base + cnt); v4 computed the first qmain of them
    const int cnt = q + (x < r ? 1 : 0), base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    if (t < cnt - qmain) {
      idx = base + qmain + t;
      break;
    }
    t -= cnt - qmain;
  }
  if (idx < 0) return;  // the launch covers exactly the tail (host side); no workgroup reaches this
  const int group = idx / (GM * tiles_n), first_m = group * GM, gsize = min(tiles_m - first_m, GM);
  const int tm = first_m + (idx % (GM * tiles_n)) % gsize, tn = (idx % (GM * tiles_n)) / gsize;
  const int quad = static_cast<int>(blockIdx.x) & 3;
  const int rm = 2 * tm + (quad >> 1), rn = 2 * tn + (quad & 1);  // the 128x128 tile

  const int kchunks = K / 8;
  const u32x4* Ablk = A + static_cast<size_t>(rm) * BM * kchunks;
  const u32x4* Bblk = Bt + static_cast<size_t>(rn) * BN * kchunks;
  u32x4 ra[LOADS_PER_THREAD], rb[LOADS_PER_THREAD];
  int g_off[LOADS_PER_THREAD], l_off[LOADS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < LOADS_PER_THREAD; ++i) {
    const int ch = tid + i * THREADS;
    const int rr = ch / CHUNKS_PER_ROW, c = ch % CHUNKS_PER_ROW;
    g_off[i] = rr * kchunks + c;
    l_off[i] = FP8 ? swz8(rr, c) : swz(rr, c);
  }
  floatx4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int KT = K / BK;  // K-tiles of 64 bf16 columns = 128 fp8 bytes
  const int frow = lane & 15, fq = lane >> 4;
  auto compute = [&](const u32x4(&buf)[2][TILE_CHUNKS]) {
    if constexpr (FP8) tail_compute_fp8(acc, buf, wr, wc, frow, fq);
    else gemm_compute(acc, buf, wr, wc, frow, fq);
  };
  gemm_gload(ra, rb, Ablk, Bblk, g_off, 0);
  gemm_lstore(lds[0], ra, rb, l_off);
  __syncthreads();
  for (int kt = 0; kt < KT; kt += 2) {
    const bool more1 = kt + 1 < KT;
    if (more1) gemm_gload(ra, rb, Ablk, Bblk, g_off, kt + 1);
    compute(lds[0]);
    if (more1) gemm_lstore(lds[1], ra, rb, l_off);
    __syncthreads();
    if (!more1) break;
    const bool more2 = kt + 2 < KT;
    if (more2) gemm_gload(ra, rb, Ablk, Bblk, g_off, kt + 2);
    compute(lds[1]);
    if (more2) gemm_lstore(lds[0], ra, rb, l_off);
    __syncthreads();
  }
  // every wave is past its last LDS read (the loop ends on a barrier): the operand buffers are free for the epilogue
  const int row0 = rm * BM + wr * 64, col0 = rn * BN + wc * 64;
  unsigned char* scratch = reinterpret_cast<unsigned char*>(&lds[0][0][0]);
  if constexpr (OUT == OUT_BF16_CK) {
    // column sums of the 128-row band rm: wave wr = 0 sums its rows (m, then j) and hands the partials over, wave
    // wr = 1 continues them over its own rows -- v4's wave order over the band's 128 rows -- then the lane exchange
    double* part = reinterpret_cast<double*>(scratch) + wc * (4 * 64);  // [wc][n][lane]
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    if (wr == 0) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) cs[n] += static_cast<double>(acc[m][n][j]);
        part[n * 64 + lane] = cs[n];
      }
    }
    __syncthreads();
    if (wr == 1) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        cs[n] = part[n * 64 + lane];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) cs[n] += static_cast<double>(acc[m][n][j]);
        cs[n] += __shfl_xor(cs[n], 16);
        cs[n] += __shfl_xor(cs[n], 32);
      }
      if (fq == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) csum[static_cast<size_t>(rm) * N + rn * BN + wc * 64 + n * 16 + frow] = cs[n];
      }
    }
    __syncthreads();  // the partials are read: the scratch becomes the waves' store patches
    // bf16 C through each wave's own patch (16 rows x 64 fp32 columns): 16-byte row pieces per lane
    constexpr int LD = 64 + 4;
    float* patch = reinterpret_cast<float*>(scratch) + wid * (16 * LD);
    __bf16* __restrict__ Cb = static_cast<__bf16*>(Cv);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
      // a wave's writes to its own patch are visible to its own later reads (one wave, in order: s_waitcnt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rr = h * 8 + (lane >> 3), c8 = (lane & 7) * 8;
        const floatx4 lo = *reinterpret_cast<const floatx4*>(patch + rr * LD + c8);
        const floatx4 hi = *reinterpret_cast<const floatx4*>(patch + rr * LD + c8 + 4);
        const floatx8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<bf16x8*>(Cb + static_cast<size_t>(row0 + m * 16 + rr) * N + col0 + c8) =
            __builtin_convertvector(v, bf16x8);
      }
    }
  } else {
    float* __restrict__ C = static_cast<float*>(Cv);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          C[static_cast<size_t>(row0 + m * 16 + fq * 4 + j) * N + col0 + n * 16 + frow] = acc[m][n][j];
  }
}

}  // namespace
