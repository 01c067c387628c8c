// GEMM v3: the v2 tile on a staggered 4-phase schedule; bf16, MX-fp8 (scaled and unscaled) and MX-fp4.
#pragma once

#include "gemm_v2.h"

namespace {

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

// One 16 KiB region of a stage: 16 LDS-DMA wave-instructions of 8 rows, 2 per wave.  Instruction g's first row:
__device__ __forceinline__ int stg_row0(int region, int g) {
  return region == 0 || region == 3 ? (g >> 3) * 128 + (region == 0 ? 0 : 64) + (g & 7) * 8
                                    : (g >> 2) * 64 + (region == 1 ? 0 : 32) + (g & 3) * 8;
}

template <bool FP8>
__device__ __forceinline__ void stg_region(unsigned char* lds_stage, const __bf16* __restrict__ A,
                                           const __bf16* __restrict__ Bt, int K, int kt, int region, int i, int wid,
                                           int lane) {
  const int rsub = lane >> 3, phys = lane & 7;
  const int g = wid * 2 + i;
  const bool is_a = region == 0 || region == 3;
  const int row0 = stg_row0(region, g);
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
  const int row0 = stg_row0(region, g);
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

// MFMAs are not memory operations, so IR passes may sink them past the next s_barrier into the
// other group's slot; an empty volatile asm that reads and writes each result of a phase pins them there.
__device__ __forceinline__ void pin_acc(floatx4 (&acc)[8][4], int m0, int n0) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(acc[m0 + m][n0 + n]));
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
  pin_acc(acc, m0, n0);
}

// MX-fp8 (E4M3, unit E8M0 scales): one v_mfma_scale_f32_16x16x128_f8f6f4 covers the K-tile's 128 bytes.  SCALE = 0
// is the same K-tile on the unscaled instruction (zero scale operands select v_mfma_f32_16x16x128_f8f6f4): with unit
// scales the two compute the same products, so the knob only changes which matrix-core path runs.
template <int SCALE = 127>
__device__ __forceinline__ void stg_mfma(floatx4 (&acc)[8][4], const i32x8 (&af)[4], const i32x8 (&bf)[2], int m0,
                                         int n0) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      acc[m0 + m][n0 + n] =
          __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bf[n], acc[m0 + m][n0 + n], 0, 0, 0, SCALE, 0, SCALE);
  pin_acc(acc, m0, n0);
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
  pin_acc(acc, m0, n0);
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
  if constexpr (DT == DT_FP8U) stg_mfma<0>(acc, af, bf, m0, n0);
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
    using W = PatchWalk<4, 8>;
    constexpr int LD = W::LD;
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
      for (int q = 0; q < W::STEPS; ++q) {
        const int r = W::row(lane, q), c8 = W::col(lane);
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
    using W = PatchWalk<4, 4>;
    constexpr int LD = W::LD;
    __builtin_amdgcn_s_barrier();
    float* patch = reinterpret_cast<float*>(smem) + wid * (16 * LD);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[(fq * 4 + j) * LD + n * 16 + frow] = acc[m][n][j];
#pragma unroll
      for (int q = 0; q < W::STEPS; ++q) {
        const int r = W::row(lane, q), c4 = W::col(lane);
        const floatx4 v = *reinterpret_cast<const floatx4*>(patch + r * LD + c4);
#ifdef DIAG_GEMM_NO_STORE  // lab build (tools/gemm_stamps.py --no-store): everything but the C write itself
        if (N > (1 << 30))
#endif
        *reinterpret_cast<floatx4*>(C + static_cast<size_t>(row0 + m * 16 + r) * N + col0 + c4) = v;
      }
    }
  } else {
    store_acc_f32(C, N, row0, col0, frow, fq, acc);
  }
}

}  // namespace
