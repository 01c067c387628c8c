// GEMM v4: 4 waves of 128x128 on a plan written out in asm, and its tail of 128x128 quadrants on v1's K loop.
#pragma once

#include "gemm_v1.h"
#include "gemm_v3.h"

namespace {

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

// a fragment's two 16-byte chunks as the MFMA's 32-byte operand
__device__ __forceinline__ i32x8 v4_op8(const u32x4& lo, const u32x4& hi) {
  return __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ void v4_mfma8(floatx4& acc, const u32x4& alo, const u32x4& ahi, const u32x4& blo,
                                         const u32x4& bhi) {
  const i32x8 a = v4_op8(alo, ahi), b = v4_op8(blo, bhi);
  asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void v4_mfma8_first(floatx4& acc, const u32x4& alo, const u32x4& ahi, const u32x4& blo,
                                               const u32x4& bhi) {
  const i32x8 a = v4_op8(alo, ahi), b = v4_op8(blo, bhi);
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
  const auto [tm, tn] = tile_of(xcd_remap(blockIdx.x, nwg), tiles_m, tiles_n, GM);
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
  constexpr int LD = PatchWalk<8, 4>::LD;
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
      // 8 bf16 (16 bytes) per lane: one store instruction covers 4 rows x 256 contiguous bytes.  PatchWalk<8, 8>,
      // with its shifts and masks written out: the compiler does not know v_mbcnt's lane id to be non-negative
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
      // one store instruction covers 2 rows x 512 contiguous bytes (PatchWalk<8, 4> written out, as above)
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
// launch then covers only the whole waves -- v4_tail_main(nwg) workgroups (tile_order.h); v4's XCD remap leaves each
// XCD's last chunk of tile indices uncomputed -- and this kernel computes those tiles as four 128x128 quadrants each,
// 4x the workgroups for the same work, with v1's K loop (the same v_mfma_f32_16x16x32_bf16 per 32-wide K chunk, in
// the same order as v3 / v4: every C element and every fp64 column sum bit-identical to theirs).  Each 128x128
// quadrant's column sums continue, in wave wr = 1, the partial sums wave wr = 0 left in LDS, so they follow v4's own
// order over the 128-row band (m, then j, then the xor-16 / xor-32 lane exchange).

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
  for (int x = 0; x < 8; ++x) {  // v4 computed the first qmain tiles of XCD x's chunk
    const int cnt = xcd_cnt(x, r, q), base = xcd_base(x, r, q);
    if (t < cnt - qmain) {
      idx = base + qmain + t;
      break;
    }
    t -= cnt - qmain;
  }
  if (idx < 0) return;  // the launch covers exactly the tail (host side); no workgroup reaches this
  const auto [tm, tn] = tile_of(idx, tiles_m, tiles_n, GM);
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
    using W = PatchWalk<4, 8>;
    constexpr int LD = W::LD;
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
      for (int h = 0; h < W::STEPS; ++h) {
        const int rr = W::row(lane, h), c8 = W::col(lane);
        const floatx4 lo = *reinterpret_cast<const floatx4*>(patch + rr * LD + c8);
        const floatx4 hi = *reinterpret_cast<const floatx4*>(patch + rr * LD + c8 + 4);
        const floatx8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<bf16x8*>(Cb + static_cast<size_t>(row0 + m * 16 + rr) * N + col0 + c8) =
            __builtin_convertvector(v, bf16x8);
      }
    }
  } else {
    store_acc_f32(static_cast<float*>(Cv), N, row0, col0, frow, fq, acc);
  }
}

}  // namespace
