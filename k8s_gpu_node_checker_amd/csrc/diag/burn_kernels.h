// The burn-ins that never leave the CU: matrix cores (MFMA), LDS, the vector register files, the vector ALU.
#pragma once

#include <cstdint>

#include "../common/hip_host.h"
#include "types.h"

namespace {

// ---------------------------------------------------------------------------
// Matrix-core datapath burn-in, one kernel per precision the MI355X computes in (operand lane layouts
// measured by tools/mfma_lab.hip: lane l holds A[l&15][k = (K/4)(l>>4) + e] and B[k][l&15] in element
// e, fp4 low nibble first):
//   0 bf16  v_mfma_f32_16x16x32_bf16          2 MX-fp8 (E4M3)  v_mfma_scale_f32_16x16x128_f8f6f4
//   1 fp8   v_mfma_f32_16x16x128_f8f6f4       3 MX-fp4 (E2M1)  v_mfma_scale_f32_16x16x128_f8f6f4
// Kind 1 is the unscaled f8f6f4 instruction (E4M3, no block scales): what hipBLASLt's fp8 GEMMs issue on gfx950
// (its TensileLibrary_F8F8_*_gfx950.co holds 13,773 of them and 12 of the gfx94x-era v_mfma_f32_16x16x32_fp8_fp8,
// which this kind used to burn; that older datapath ran at the bf16 rate and no production fp8 GEMM depends on
// it).  The builtin with zero scale operands is selected as the unscaled instruction (checked in the ISA).
// Register-resident (no memory traffic), 4 independent accumulators per wave, 2 waves per SIMD on every
// CU.  Operands are {-1, 0, +1}: every product and partial sum is an integer below 2^24, so the fp32
// result is exact and each lane's final sum must equal the host-computed value bit for bit -- a SIMD
// whose matrix core miscomputes is counted, not averaged away.
template <int KIND>
__device__ __forceinline__ floatx4 burn_mfma(const i32x8& a, const i32x8& b, floatx4 c) {
  if constexpr (KIND == 0) {
    bf16x8 av, bv;
    __builtin_memcpy(&av, &a, 16);
    __builtin_memcpy(&bv, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
  } else if constexpr (KIND == 1) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);  // E4M3, unscaled form
  } else if constexpr (KIND == 2) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);  // E4M3, scales 2^0
  } else {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 4, 0, 127, 0, 127);  // E2M1, scales 2^0
  }
}

// The burn-ins' per-CU maps are indexed by wave_slot() (common/hip_host.h): one of its WAVE_SLOTS slots.
constexpr int BURN_SLOTS = WAVE_SLOTS;

template <int KIND>
__global__ void __launch_bounds__(256) mfma_burn_kernel(const i32x8* __restrict__ fa, const i32x8* __restrict__ fb,
                                                        const float* __restrict__ expect, int iters, int inject_block,
                                                        unsigned long long* errors, unsigned long long* cu_map) {
  const long long t0 = wall_clock64();  // constant-rate clock (hipDeviceAttributeWallClockRate)
  const int lane = threadIdx.x & 63;
  const i32x8 a = fa[lane], b = fb[lane];
  floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc0 = burn_mfma<KIND>(a, b, acc0);
      acc1 = burn_mfma<KIND>(b, a, acc1);
      acc2 = burn_mfma<KIND>(a, a, acc2);
      acc3 = burn_mfma<KIND>(b, b, acc3);
    }
  }
  const floatx4 s = acc0 + acc1 + acc2 + acc3;
  float sum = s[0] + s[1] + s[2] + s[3];
  // the self-check of the verifier (diag_mfma_burn): one lane of one workgroup is made wrong by one, which
  // is exact below 2^24 and so always differs
  if (static_cast<int>(blockIdx.x) == inject_block && threadIdx.x == 0) sum += 1.0f;
  const bool bad = sum != expect[lane];
  if (bad) atomicAdd(errors, 1ULL);
  if (cu_map != nullptr) {
    // per physical CU: waves run, wrong lanes, summed wave time -- a miscomputing CU is named, and an
    // XCD whose waves take longer than the others' (its own clock domain) stands out
    const unsigned long long nbad = __popcll(__ballot(bad));
    const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
    if (lane == 0) {
      unsigned long long* row = cu_map + 3 * wave_slot();
      atomicAdd(row, 1ULL);
      if (nbad) atomicAdd(row + 1, nbad);
      atomicAdd(row + 2, dt);
    }
  }
}

// ---------------------------------------------------------------------------
// LDS test: every workgroup takes the CU's whole LDS (160 KiB on gfx950), writes four patterns over it
// (address hash, its inverse, 0x55.., 0xAA..: every bit at 0 and at 1), and reads each back through a
// different thread than the one that wrote it (half-buffer rotation), so a stuck or coupled bit in any
// bank of any CU is counted -- the register-resident burn-in never touches LDS, and the GEMMs only
// sample their outputs.  Errors are attributed to the physical CU (wave_slot()); `inject_block` >= 0
// corrupts one word of that block's first pattern after the write (the test's own self-check).
__device__ __forceinline__ uint32_t lds_pattern(uint32_t i, uint32_t seed, int p) {
  switch (p & 3) {
    case 0: return mix32(static_cast<uint64_t>(i) * 0x9E3779B97F4A7C15ULL + seed);
    case 1: return ~mix32(static_cast<uint64_t>(i) * 0x9E3779B97F4A7C15ULL + seed);
    case 2: return 0x55555555u;
    default: return 0xAAAAAAAAu;
  }
}

__global__ void __launch_bounds__(1024) lds_test_kernel(uint32_t words, uint32_t seed, int inject_block,
                                                        unsigned long long* errors, unsigned long long* cu_map) {
  extern __shared__ uint32_t lds_words[];
  __shared__ unsigned int block_bad;
  if (threadIdx.x == 0) block_bad = 0;
  unsigned int bad = 0;
  for (int p = 0; p < 4; ++p) {
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) lds_words[i] = lds_pattern(i, seed, p);
    __syncthreads();
    if (p == 0 && static_cast<int>(blockIdx.x) == inject_block && threadIdx.x == 0) lds_words[words / 3] ^= 0x10u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) {
      const uint32_t j = i + words / 2 < words ? i + words / 2 : i + words / 2 - words;
      bad += lds_words[j] != lds_pattern(j, seed, p);
    }
    __syncthreads();  // every read of pattern p done before pattern p+1 overwrites it
  }
  if (bad) atomicAdd(&block_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* row = cu_map + 2 * wave_slot();
    atomicAdd(row, 1ULL);
    if (block_bad) {
      atomicAdd(row + 1, static_cast<unsigned long long>(block_bad));
      atomicAdd(errors, static_cast<unsigned long long>(block_bad));
    }
  }
}

// ---------------------------------------------------------------------------
// Register-file test: each SIMD of gfx950 holds 512 registers x 64 lanes x 4 B = 128 KiB (256 VGPRs and 256 AGPRs per
// wave at one wave per SIMD) -- more SRAM per chip than the LDS and the L2 together.  A workgroup of four waves at 512
// registers each takes a whole CU, one wave per SIMD.  Every tested register of every lane takes four patterns in
// turn (a value distinct per register, lane, workgroup and seed; its inverse; 0x55..; 0xAA..: every bit at 0 and at
// 1); all registers of both files are written before the first is read back, with a hold in between, so a write that
// disturbs another register or a cell that does not retain is seen.  Mismatching words are counted per lane and per
// file and attributed to the SIMD (wave_slot() << 2 | HW_ID.SIMD_ID).
//
// The registers are named explicitly in one asm statement (the assembler's .set / .rept / v[sym] / a[sym]): C++
// values kept live through operand barriers are spilled by the thousand, which would test scratch memory.  The
// statement touches no memory.  The compiler owns v0..v(RF_VLO-1): the lane key, two temporaries, the two error
// counts and the injection mask are its operands; every tested register is a clobber, which also makes the kernel
// descriptor allocate all 512.  A VALU result goes through s_nop 1 before a v_accvgpr_write reads it (nothing pads
// the inside of an asm string).  diag_regfile_test refuses to run a build whose kernel has a scratch segment.
constexpr int RF_VLO = 8, RF_VHI = 255, RF_ALO = 0, RF_AHI = 255;
constexpr int RF_NV = RF_VHI - RF_VLO + 1, RF_NA = RF_AHI - RF_ALO + 1;
constexpr int RF_REGS = RF_NV + RF_NA;  // registers of one lane holding a pattern at once
constexpr int RF_SLOTS = SIMD_ROWS;  // rows of its SIMD map: simd_row() of common/hip_host.h
static_assert(RF_REGS >= 500, "the register-file test must hold at least 500 of a lane's 512 registers");

// "p<t>0" .. "p<t>9": ten register names of a clobber list (a range is not accepted there)
#define RF_DEC(p, t) p #t "0", p #t "1", p #t "2", p #t "3", p #t "4", p #t "5", p #t "6", p #t "7", p #t "8", p #t "9"
#define RF_CENT(p, h) RF_DEC(p, h##0), RF_DEC(p, h##1), RF_DEC(p, h##2), RF_DEC(p, h##3), RF_DEC(p, h##4), \
                      RF_DEC(p, h##5), RF_DEC(p, h##6), RF_DEC(p, h##7), RF_DEC(p, h##8), RF_DEC(p, h##9)
#define RF_TENS(p) RF_DEC(p, 1), RF_DEC(p, 2), RF_DEC(p, 3), RF_DEC(p, 4), RF_DEC(p, 5), RF_DEC(p, 6), RF_DEC(p, 7), \
                   RF_DEC(p, 8), RF_DEC(p, 9)
#define RF_FROM_10(p) RF_TENS(p), RF_CENT(p, 1), RF_DEC(p, 20), RF_DEC(p, 21), RF_DEC(p, 22), RF_DEC(p, 23), \
                      RF_DEC(p, 24), p "250", p "251", p "252", p "253", p "254", p "255"
#define RF_CLOBBERS "v8", "v9", RF_FROM_10("v"), "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", RF_FROM_10("a")

// the walk over the registers: rf_r the register, rf_k its constant (rf_nk = ~rf_k), the same in write and check
#define RF_BEGIN ".set rf_r, %[vlo]\n.set rf_k, 0x85EBCA6B\n.set rf_nk, rf_k ^ 0xffffffff\n"
#define RF_NEXT ".set rf_r, rf_r + 1\n.set rf_k, (rf_k + 0x9E3779B1) & 0xffffffff\n.set rf_nk, rf_k ^ 0xffffffff\n"
// EXP leaves the expected word of register rf_r in %[tmp]
#define RF_EXP_HASH "v_add_u32 %[tmp], rf_k, %[key]\n"    // key + k(r)
#define RF_EXP_INV "v_sub_u32 %[tmp], rf_nk, %[key]\n"    // ~(key + k(r)) = ~k(r) - key
#define RF_EXP_55 "v_mov_b32 %[tmp], 0x55555555\n"
#define RF_EXP_AA "v_mov_b32 %[tmp], 0xAAAAAAAA\n"
#define RF_WRITE(EXP)                                                                                        \
  RF_BEGIN ".rept %[nv]\n" EXP "v_mov_b32 v[rf_r], %[tmp]\n" RF_NEXT ".endr\n"                               \
  ".set rf_r, %[alo]\n.rept %[na]\n" EXP "s_nop 1\nv_accvgpr_write_b32 a[rf_r], %[tmp]\n" RF_NEXT ".endr\n"
#define RF_HOLD(ID)                                                                                          \
  "s_mov_b32 %[st], %[hold]\n"                                                                               \
  ".Lrf_hold" ID "_%=:\ns_cmp_eq_u32 %[st], 0\ns_cbranch_scc1 .Lrf_held" ID "_%=\ns_sleep 8\n"                \
  "s_sub_u32 %[st], %[st], 1\ns_branch .Lrf_hold" ID "_%=\n.Lrf_held" ID "_%=:\n"
#define RF_CHECK(EXP)                                                                                        \
  RF_BEGIN ".rept %[nv]\n" EXP "v_cmp_ne_u32 vcc, %[tmp], v[rf_r]\nv_addc_co_u32 %[cv], vcc, 0, %[cv], vcc\n" \
  RF_NEXT ".endr\n"                                                                                          \
  ".set rf_r, %[alo]\n.rept %[na]\nv_accvgpr_read_b32 %[tmp2], a[rf_r]\n" EXP "s_nop 1\n"                    \
  "v_cmp_ne_u32 vcc, %[tmp], %[tmp2]\nv_addc_co_u32 %[ca], vcc, 0, %[ca], vcc\n" RF_NEXT ".endr\n"
// the self-check: %[inj] (one bit in lane 0 of wave 0 of the injected workgroup, 0 elsewhere) is XOR-ed into the
// register %[which] selects -- 0 / 1 the lowest / highest tested VGPR, 2 / 3 the lowest / highest tested AGPR
#define RF_INJECT_V(N, REG)                                                                                  \
  "s_cmp_eq_u32 %[which], " N "\ns_cselect_b32 %[st], -1, 0\nv_and_b32 %[tmp], %[st], %[inj]\n"              \
  "v_xor_b32 v[" REG "], v[" REG "], %[tmp]\n"
#define RF_INJECT_A(N, REG)                                                                                  \
  "s_cmp_eq_u32 %[which], " N "\ns_cselect_b32 %[st], -1, 0\nv_and_b32 %[tmp], %[st], %[inj]\n"              \
  "v_accvgpr_read_b32 %[tmp2], a[" REG "]\ns_nop 1\nv_xor_b32 %[tmp2], %[tmp2], %[tmp]\ns_nop 1\n"           \
  "v_accvgpr_write_b32 a[" REG "], %[tmp2]\n"
#define RF_INJECT RF_INJECT_V("0", "%[vlo]") RF_INJECT_V("1", "%[vhi]") RF_INJECT_A("2", "%[alo]") RF_INJECT_A("3", "%[ahi]")

__global__ void __launch_bounds__(256, 1) regfile_test_kernel(uint32_t seed, int hold, int inject_block, int inject_reg,
                                                              unsigned long long* errors, unsigned long long* simd_map) {
  static_assert(RF_VLO == 8 && RF_VHI == 255 && RF_ALO == 0 && RF_AHI == 255, "RF_CLOBBERS names v8..v255, a0..a255");
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t key = mix32((static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x) * 0x9E3779B97F4A7C15ULL + seed);
  const uint32_t inj = static_cast<int>(blockIdx.x) == inject_block && threadIdx.x == 0 ? 0x10u : 0u;
  uint32_t bad_v = 0, bad_a = 0, tmp, tmp2, st;
  asm volatile(
      RF_WRITE(RF_EXP_HASH) RF_HOLD("0") RF_INJECT RF_CHECK(RF_EXP_HASH)
      RF_WRITE(RF_EXP_INV) RF_HOLD("1") RF_CHECK(RF_EXP_INV)
      RF_WRITE(RF_EXP_55) RF_HOLD("2") RF_CHECK(RF_EXP_55)
      RF_WRITE(RF_EXP_AA) RF_HOLD("3") RF_CHECK(RF_EXP_AA)
      : [cv] "+v"(bad_v), [ca] "+v"(bad_a), [tmp] "=&v"(tmp), [tmp2] "=&v"(tmp2), [st] "=&s"(st)
      : [key] "v"(key), [inj] "v"(inj), [which] "s"(inject_reg), [hold] "s"(hold), [vlo] "n"(RF_VLO), [vhi] "n"(RF_VHI),
        [alo] "n"(RF_ALO), [ahi] "n"(RF_AHI), [nv] "n"(RF_NV), [na] "n"(RF_NA)
      : "vcc", "scc", RF_CLOBBERS);
  unsigned long long* row = simd_map + SIMD_MAP_COLS * simd_row();
  if (lane == 0) atomicAdd(row, 1ULL);
  if (bad_v) {
    atomicAdd(row + 1, static_cast<unsigned long long>(bad_v));
    atomicAdd(errors, static_cast<unsigned long long>(bad_v));
  }
  if (bad_a) {
    atomicAdd(row + 2, static_cast<unsigned long long>(bad_a));
    atomicAdd(errors, static_cast<unsigned long long>(bad_a));
  }
}

// ---------------------------------------------------------------------------
// Vector-ALU burn-in: the datapaths every non-GEMM kernel runs on, which no matrix-core instruction exercises.
//   0 f64     v_fma_f64          1 pk_f32  v_pk_fma_f32          2 i32  v_mad_u64_u32 (the 32-bit multiplier)
// Shaped like mfma_burn_kernel: register-resident, 2 workgroups of 4 waves per CU, VALU_CHAINS independent chains
// per lane, VALU_UNROLL steps of each per iteration.  Operands differ per lane and keep every intermediate normal
// (valu_ref.h, which also computes what each lane must end with): the device must match the host bit for bit.
#include "valu_ref.h"  // the chains and their host expectation (host-compilable, tests/test_simd_diag_cpu.py)

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int KIND>
struct ValuChain;
template <>
struct ValuChain<0> {
  double x, a, b;
  __device__ __forceinline__ void load(const uint64_t* o) {
    x = __longlong_as_double(o[0]), a = __longlong_as_double(o[1]), b = __longlong_as_double(o[2]);
  }
  __device__ __forceinline__ void step() { x = __builtin_fma(x, a, b); }
  __device__ __forceinline__ uint64_t bits() const { return static_cast<uint64_t>(__double_as_longlong(x)); }
};
template <>
struct ValuChain<1> {
  f32x2 x, a, b;
  __device__ __forceinline__ void load(const uint64_t* o) {
    __builtin_memcpy(&x, o, 8), __builtin_memcpy(&a, o + 1, 8), __builtin_memcpy(&b, o + 2, 8);
  }
  __device__ __forceinline__ void step() { x = __builtin_elementwise_fma(x, a, b); }
  __device__ __forceinline__ uint64_t bits() const {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
  }
};
template <>
struct ValuChain<2> {
  uint64_t x, b;
  uint32_t a;
  __device__ __forceinline__ void load(const uint64_t* o) { x = o[0], a = static_cast<uint32_t>(o[1]), b = o[2]; }
  __device__ __forceinline__ void step() { x = static_cast<uint64_t>(static_cast<uint32_t>(x)) * a + b; }
  __device__ __forceinline__ uint64_t bits() const { return x; }
};

template <int KIND>
__global__ void __launch_bounds__(256) valu_burn_kernel(const uint64_t* __restrict__ ops,
                                                        const uint64_t* __restrict__ expect, int iters, int inject_block,
                                                        unsigned long long* errors, unsigned long long* cu_map) {
  const long long t0 = wall_clock64();
  const int lane = threadIdx.x & 63;
  ValuChain<KIND> ch[VALU_CHAINS];
#pragma unroll
  for (int c = 0; c < VALU_CHAINS; ++c) ch[c].load(ops + 3 * (lane * VALU_CHAINS + c));
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < VALU_UNROLL; ++u) {
#pragma unroll
      for (int c = 0; c < VALU_CHAINS; ++c) ch[c].step();
    }
  }
  bool bad = false;
#pragma unroll
  for (int c = 0; c < VALU_CHAINS; ++c) {
    uint64_t got = ch[c].bits();
    // the self-check of the verifier (diag_valu_burn): one bit of one chain of one lane is flipped
    if (c == 0 && static_cast<int>(blockIdx.x) == inject_block && threadIdx.x == 0) got ^= 1ULL;
    bad |= got != expect[lane * VALU_CHAINS + c];
  }
  if (bad) atomicAdd(errors, 1ULL);
  if (cu_map != nullptr) {
    const unsigned long long nbad = __popcll(__ballot(bad));
    const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
    if (lane == 0) {
      unsigned long long* row = cu_map + 3 * wave_slot();
      atomicAdd(row, 1ULL);
      if (nbad) atomicAdd(row + 1, nbad);
      atomicAdd(row + 2, dt);
    }
  }
}

}  // namespace
