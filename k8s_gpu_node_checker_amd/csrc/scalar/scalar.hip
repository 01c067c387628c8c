// libmi355x_scalar.so: the scalar diagnostic (HIP, gfx950).
//
// Every other compute diagnostic runs on the vector side of a CU.  This one tests the scalar side, in three parts:
//   salu   the scalar ALU: one template instantiation per op of scalar_ref.h, one native instruction each through
//          inline asm on SGPR operands, SCC set before it and read after it inside the same statement.  Every wave
//          runs SCALAR_CHAINS independent chains (scalar_ref.h) in scalar registers; all waves run the same chains, and
//          the words a wave must end with come from the host's model of the op (scalar_expected()).  The wave fetches
//          them with a vector load, so a scalar-cache fault cannot excuse a scalar-ALU fault.
//   sgpr   the SGPR file of each SIMD: one asm statement over the explicitly named registers s[SG_LO]..s[SG_HI]
//          under four patterns, written whole, held with s_sleep, then checked register by register.
//   smem   scalar loads through the scalar data cache: every native width of s_load and s_buffer_load over a table
//          the host filled with scalar_smem_word(); a small table that stays cached (hits) and a large one walked
//          with a wave-dependent stride (misses).  Each load waits for lgkmcnt(0) inside its own statement.
// The scalar memory path is used for loads only: every result leaves the wave through vector stores and vector
// atomics.  No LDS allocation, no scratch: every entry point refuses to run a build that has either.  ops/scalar.py
// is its Python side; ops/diag.run(extra=("scalar",)) runs it next to a level's own tests.
//
// Wrong words are located to their SIMD as the register-file test's are: the SIMD map row is simd_row() of
// common/hip_host.h; `slot` below is that row.  The Report a launch leaves, the report() that ends the kernel and the
// host's Run are those of common/simd_report.h.
// The SGPR file is per SIMD; the scalar ALU and the scalar cache are shared, so their faults show on every SIMD of
// a CU (the cache: of its neighbours too).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "scalar_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int SALU_BLOCKS_PER_CU = 4;   // the default grids
constexpr int SGPR_BLOCKS_PER_CU = 7;   // 4 waves each: 7 waves per SIMD, what 112 allocated SGPRs admit
constexpr int SMEM_BLOCKS_PER_CU = 4;
constexpr int MAX_ITERS = 1 << 20;
constexpr uint32_t MAX_TABLE_WORDS = 1u << 24;  // 64 MiB

// Every count here is one wave's, so lane 0 alone calls report().  A record's `where`: SIMD map row << 32 | the part's
// own index (chain; pattern << 8 | register; table word).
__device__ __forceinline__ unsigned long long where_of(unsigned row, unsigned index) {
  return (static_cast<unsigned long long>(row) << 32) | index;
}

// --- salu ------------------------------------------------------------------------------------------------------
// One application of op OP: SCC set from scc_in, the instruction itself, SCC read out, all in one statement.
#define SALU_HEAD "s_cmp_lg_u32 %[sin], 0\n"
#define SALU_TAIL "\ns_cselect_b32 %[so], 1, 0"
#define SALU_STR_(x) #x
#define SALU_STR(x) SALU_STR_(x)

template <int OP>
__device__ __forceinline__ ScalarOut salu(uint64_t a, uint64_t b, uint32_t scc_in);

#define SALU_BODY(D_T, D_INIT, D_CONSTRAINT, TEXT, ...)                                                      \
  D_T d = D_INIT;                                                                                            \
  uint32_t so;                                                                                               \
  asm volatile(SALU_HEAD TEXT SALU_TAIL : [d] D_CONSTRAINT(d), [so] "=s"(so) : [sin] "s"(scc_in), ##__VA_ARGS__ : "scc"); \
  return {static_cast<uint64_t>(d), so};
#define SALU_D32_AB32(M) SALU_BODY(uint32_t, 0, "=s", #M " %[d], %[a], %[b]", [a] "s"(static_cast<uint32_t>(a)), [b] "s"(static_cast<uint32_t>(b)))
#define SALU_D64_AB64(M) SALU_BODY(uint64_t, 0, "=s", #M " %[d], %[a], %[b]", [a] "s"(a), [b] "s"(b))
#define SALU_D64_A64_B32(M) SALU_BODY(uint64_t, 0, "=s", #M " %[d], %[a], %[b]", [a] "s"(a), [b] "s"(static_cast<uint32_t>(b)))
#define SALU_D64_AB32(M) SALU_BODY(uint64_t, 0, "=s", #M " %[d], %[a], %[b]", [a] "s"(static_cast<uint32_t>(a)), [b] "s"(static_cast<uint32_t>(b)))
#define SALU_D32_A32(M) SALU_BODY(uint32_t, 0, "=s", #M " %[d], %[a]", [a] "s"(static_cast<uint32_t>(a)))
#define SALU_D64_A64(M) SALU_BODY(uint64_t, 0, "=s", #M " %[d], %[a]", [a] "s"(a))
#define SALU_D32_A64(M) SALU_BODY(uint32_t, 0, "=s", #M " %[d], %[a]", [a] "s"(a))
#define SALU_D64_A32(M) SALU_BODY(uint64_t, 0, "=s", #M " %[d], %[a]", [a] "s"(static_cast<uint32_t>(a)))
// the destination is an operand too: preset to S1 (bitset, cmov) or to S0 (the SOPK ops)
#define SALU_RMW32_A32(M) SALU_BODY(uint32_t, static_cast<uint32_t>(b), "+s", #M " %[d], %[a]", [a] "s"(static_cast<uint32_t>(a)))
#define SALU_K_ADD(M) SALU_BODY(uint32_t, static_cast<uint32_t>(a), "+s", #M " %[d], " SALU_STR(SCALAR_ADDK_IMM))
#define SALU_K_MUL(M) SALU_BODY(uint32_t, static_cast<uint32_t>(a), "+s", #M " %[d], " SALU_STR(SCALAR_MULK_IMM))
// a compare has no destination: the result is SCC
#define SALU_CMP(M, A, B)                                                                                    \
  uint32_t so;                                                                                               \
  asm volatile(SALU_HEAD #M " %[a], %[b]" SALU_TAIL : [so] "=s"(so) : [sin] "s"(scc_in), [a] "s"(A), [b] "s"(B) : "scc"); \
  return {0, so};
#define SALU_CMP32(M) SALU_CMP(M, static_cast<uint32_t>(a), static_cast<uint32_t>(b))
#define SALU_CMP64(M) SALU_CMP(M, a, b)

#define SCALAR_X_SALU(E, M, F)                                                                   \
  template <>                                                                                    \
  __device__ __forceinline__ ScalarOut salu<E>(uint64_t a, uint64_t b, uint32_t scc_in) {        \
    (void)a, (void)b;                                                                            \
    SALU_##F(M)                                                                                  \
  }
SCALAR_OP_LIST(SCALAR_X_SALU)
#undef SCALAR_X_SALU

// (skip_block, skip_iter): the self-check's instruction that did not execute, on wave 0 of that workgroup at that
// step (-1: none); flip_block: one bit of the final chain-0 word of that workgroup's wave 0 is flipped (-1: none).
// expect: this op's SCALAR_CHAINS words.
template <int OP>
__global__ void __launch_bounds__(THREADS) salu_kernel(const uint32_t* expect, uint64_t seed, int iters, int flip_block,
                                                       int skip_block, int skip_iter, Report* rep,
                                                       unsigned long long* simd_map) {
  static_assert(SCALAR_CHAINS == 4, "lanes 0..3 compare one chain each");
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const bool hooked_wave = wave == 0;
  const int skip_at = hooked_wave && static_cast<int>(blockIdx.x) == skip_block ? skip_iter : -1;  // wave-uniform
  uint32_t x[SCALAR_CHAINS], c[SCALAR_CHAINS];
#pragma unroll
  for (int ch = 0; ch < SCALAR_CHAINS; ++ch) {
    x[ch] = scalar_init(seed, ch);
    c[ch] = scalar_const(seed, ch);
  }
  for (int it = 0; it < iters; ++it) {
    if (it != skip_at) {
#pragma unroll
      for (int ch = 0; ch < SCALAR_CHAINS; ++ch) {
        const ScalarOut o = salu<OP>(scalar_operand_a(x[ch]), scalar_operand_b(x[ch], c[ch]), scalar_scc_in(x[ch]));
        x[ch] = scalar_step(x[ch], o.result, o.scc, c[ch]);
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < SCALAR_CHAINS; ++ch) {
        const ScalarOut o = scalar_skipped(scalar_operand_a(x[ch]), scalar_scc_in(x[ch]));
        x[ch] = scalar_step(x[ch], o.result, o.scc, c[ch]);
      }
    }
  }
  if (hooked_wave && static_cast<int>(blockIdx.x) == flip_block) x[0] ^= 0x10u;
  // lane ch < 4 holds chain ch's word against the expected one, which it loads itself: a per-lane address, so a
  // vector load
  const uint32_t ch = lane & 3u;
  const uint32_t want = expect[ch];
  const uint32_t got = ch == 0 ? x[0] : ch == 1 ? x[1] : ch == 2 ? x[2] : x[3];
  const unsigned long long wrong = __ballot(lane < SCALAR_CHAINS && got != want);
  const unsigned first = wrong ? static_cast<unsigned>(__ffsll(static_cast<long long>(wrong)) - 1) : 0u;
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  const uint32_t first_got = __builtin_amdgcn_readlane(got, static_cast<int>(first));
  const uint32_t first_want = __builtin_amdgcn_readlane(want, static_cast<int>(first));
  if (lane == 0) report(rep, simd_map, row, __popcll(wrong), where_of(row, first), 0, first_got, first_want, dt);
}

// one wave, `n` applications one after the other, returned raw: in[3 i ..] = a, b, scc_in -> out[2 i ..] = result,
// scc_out
template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(const uint64_t* in, uint64_t* out, int n) {
  for (int i = 0; i < n; ++i) {
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(in + 3 * i)[k]);
    const ScalarOut o = salu<OP>((static_cast<uint64_t>(w[1]) << 32) | w[0], (static_cast<uint64_t>(w[3]) << 32) | w[2], w[4]);
    if (threadIdx.x == 0) {
      out[2 * i] = o.result;
      out[2 * i + 1] = o.scc;
    }
  }
}

struct SaluLaunch {
  const uint32_t* expect;
  uint64_t seed;
  int iters, flip_block, skip_block, skip_iter;
  Report* rep;
  unsigned long long* map;
  unsigned blocks;
};

template <int OP>
void launch_op(const SaluLaunch& l) {
  hipLaunchKernelGGL(salu_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.expect, l.seed, l.iters, l.flip_block,
                     l.skip_block, l.skip_iter, l.rep, l.map);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(salu_kernel<OP>));
}
template <int OP>
void launch_apply(const uint64_t* in, uint64_t* out, int n) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, in, out, n);
}

// the tables from op index to instantiation
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const SaluLaunch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(const uint64_t*, uint64_t*, int) = {launch_apply<OP>...};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, SCALAR_OPS>()));

// --- sgpr ------------------------------------------------------------------------------------------------------
// The registers are named explicitly in one asm statement (the assembler's .set / .rept / s[sym]), as the
// register-file test names its VGPRs.  The compiler owns s0..s[SG_LO-1]: the key, the hold count, the two injection
// masks, the counters and three temporaries are its operands; every tested register is a clobber, which also makes
// the kernel descriptor allocate them all.  SG_LO is the lowest register the compiler leaves free in this kernel
// (read off the compiled kernel: its operands and live values reach s16; s17-s19 are margin); SG_HI = 95 is the last of the 96 a wave may
// name besides VCC and the registers above it; s32, the ABI's stack pointer, is reserved and skipped.  The statement
// touches no memory.
constexpr int SG_LO = 20, SG_HI = 95, SG_SKIP = 32;  // s32 is the ABI's stack pointer: reserved, so left alone
constexpr int SG_SPAN = SG_HI - SG_LO + 1;
constexpr int SG_REGS = SG_SPAN - 1;  // registers of one wave holding a pattern at once
static_assert(SG_HI < 128, "scalar_sgpr_word() keeps 128 registers per wave apart");

#define SG_DEC(t) "s" #t "0", "s" #t "1", "s" #t "2", "s" #t "3", "s" #t "4", "s" #t "5", "s" #t "6", "s" #t "7", "s" #t "8", "s" #t "9"
#define SG_CLOBBERS SG_DEC(2), "s30", "s31", "s33", "s34", "s35", "s36", "s37", "s38", "s39", SG_DEC(4), SG_DEC(5), SG_DEC(6), \
                    SG_DEC(7), SG_DEC(8), "s90", "s91", "s92", "s93", "s94", "s95"

// the walk over the registers: sg_r the register, sg_k = sg_r * G its constant, the same in write and check
#define SG_BEGIN ".set sg_r, %[lo]\n"
#define SG_EACH ".rept %[n]\n.if sg_r != %[skip]\n"
#define SG_END ".endif\n" SG_NEXT ".endr\n"
#define SG_K "((sg_r * 0x9E3779B1) & 0xffffffff)"
#define SG_NEXT ".set sg_r, sg_r + 1\n"
// EXP(dst) leaves the expected word of register sg_r in dst
#define SG_EXP_HASH(dst) "s_add_u32 " dst ", %[key], " SG_K "\n"
#define SG_EXP_INV(dst) "s_add_u32 " dst ", %[key], " SG_K "\ns_not_b32 " dst ", " dst "\n"
#define SG_EXP_55(dst) "s_mov_b32 " dst ", 0x55555555\n"
#define SG_EXP_AA(dst) "s_mov_b32 " dst ", 0xAAAAAAAA\n"
#define SG_WRITE(EXP) SG_BEGIN SG_EACH EXP("s[sg_r]") SG_END
#define SG_HOLD(ID)                                                                                          \
  "s_mov_b32 %[st], %[hold]\n"                                                                               \
  ".Lsg_hold" ID "_%=:\ns_cmp_eq_u32 %[st], 0\ns_cbranch_scc1 .Lsg_held" ID "_%=\ns_sleep 8\n"                \
  "s_sub_u32 %[st], %[st], 1\ns_branch .Lsg_hold" ID "_%=\n.Lsg_held" ID "_%=:\n"
// a wrong register adds 1 to %[cnt]; the first of them in the walk (pattern << 8 | register, the smallest) leaves
// its word and the expected one in %[got] / %[want]
#define SG_CHECK(EXP, PAT)                                                                                   \
  SG_BEGIN SG_EACH EXP("%[tmp]")                                                                              \
  "s_cmp_lg_u32 s[sg_r], %[tmp]\ns_cselect_b32 %[t2], (" PAT " << 8) | sg_r, -1\ns_addc_u32 %[cnt], %[cnt], 0\n" \
  "s_cmp_lt_u32 %[t2], %[first]\ns_cselect_b32 %[got], s[sg_r], %[got]\ns_cselect_b32 %[want], %[tmp], %[want]\n" \
  "s_min_u32 %[first], %[first], %[t2]\n" SG_END
// the self-check: one bit in wave 0 of the injected workgroup, 0 elsewhere
#define SG_INJECT "s_xor_b32 s[%[lo]], s[%[lo]], %[injlo]\ns_xor_b32 s[%[hi]], s[%[hi]], %[injhi]\n"

// inject_reg: 0 the lowest, 1 the highest tested register of wave 0 of workgroup inject_block (-1: none)
__global__ void __launch_bounds__(THREADS) sgpr_kernel(uint64_t seed, int hold, int inject_block, int inject_reg, Report* rep,
                                                       unsigned long long* simd_map) {
  static_assert(SG_LO == 20 && SG_HI == 95 && SG_SKIP == 32, "SG_CLOBBERS names s20..s31 and s33..s95");
  const long long t0 = wall_clock64();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t key = scalar_sgpr_key(seed, wave);
  const bool hooked = static_cast<int>(blockIdx.x) == inject_block && (wave & 3u) == 0;
  const uint32_t injlo = hooked && inject_reg == 0 ? 0x10u : 0u, injhi = hooked && inject_reg == 1 ? 0x10u : 0u;
  uint32_t cnt = 0, first = ~0u, got = 0, want = 0, tmp, t2, st;
  asm volatile(
      SG_WRITE(SG_EXP_HASH) SG_HOLD("0") SG_INJECT SG_CHECK(SG_EXP_HASH, "0")
      SG_WRITE(SG_EXP_INV) SG_HOLD("1") SG_CHECK(SG_EXP_INV, "1")
      SG_WRITE(SG_EXP_55) SG_HOLD("2") SG_CHECK(SG_EXP_55, "2")
      SG_WRITE(SG_EXP_AA) SG_HOLD("3") SG_CHECK(SG_EXP_AA, "3")
      : [cnt] "+s"(cnt), [first] "+s"(first), [got] "+s"(got), [want] "+s"(want), [tmp] "=&s"(tmp), [t2] "=&s"(t2),
        [st] "=&s"(st)
      : [key] "s"(key), [hold] "s"(hold), [injlo] "s"(injlo), [injhi] "s"(injhi), [lo] "n"(SG_LO), [hi] "n"(SG_HI),
        [n] "n"(SG_SPAN), [skip] "n"(SG_SKIP), [t0] "s"(t0)  // t0: the clock is read before the statement
      : "scc", SG_CLOBBERS);
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  if ((threadIdx.x & 63u) == 0) report(rep, simd_map, row, cnt, where_of(row, first), 0, got, want, dt);
}

// --- smem ------------------------------------------------------------------------------------------------------
template <int W>
struct Words {
  typedef uint32_t type __attribute__((ext_vector_type(W)));
};
template <>
struct Words<1> {
  typedef uint32_t type;
};
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One load of kind KIND at byte offset `off` of the table, and its wait, in one statement: scalar loads return out
// of order, so only lgkmcnt(0) says this one has landed.  The caller keeps off + 4 * words inside the table.
#define SMEM_LOAD(M, BASE)                                                                                   \
  asm volatile(M " %[d], %[p], %[o]\ns_waitcnt lgkmcnt(0)" : [d] "=&s"(d) : [p] "s"(BASE), [o] "s"(off) : "memory")
template <int KIND>
__device__ __forceinline__ typename Words<SCALAR_SMEM_TABLE[KIND].words>::type smem_load(const uint32_t* table, u32x4 rsrc,
                                                                                         uint32_t off) {
  typename Words<SCALAR_SMEM_TABLE[KIND].words>::type d;
  if constexpr (KIND == SCALAR_SMEM_LOAD_X1) SMEM_LOAD("s_load_dword", table);
  else if constexpr (KIND == SCALAR_SMEM_LOAD_X2) SMEM_LOAD("s_load_dwordx2", table);
  else if constexpr (KIND == SCALAR_SMEM_LOAD_X4) SMEM_LOAD("s_load_dwordx4", table);
  else if constexpr (KIND == SCALAR_SMEM_LOAD_X8) SMEM_LOAD("s_load_dwordx8", table);
  else if constexpr (KIND == SCALAR_SMEM_LOAD_X16) SMEM_LOAD("s_load_dwordx16", table);
  else if constexpr (KIND == SCALAR_SMEM_BUFFER_X1) SMEM_LOAD("s_buffer_load_dword", rsrc);
  else {
    static_assert(KIND == SCALAR_SMEM_BUFFER_X4, "a kind without an instruction");
    SMEM_LOAD("s_buffer_load_dwordx4", rsrc);
  }
  return d;
}

template <int W>
__device__ __forceinline__ uint32_t word_of(const typename Words<W>::type& v, int j) {
  if constexpr (W == 1) return v;
  else return v[j];
}

// Every wave makes `loads` loads of kind KIND over a table of `words` words (a power of two >= 16, checked by the
// host) and compares every word with the pattern it recomputes.  scattered: 0 walks the table in order from its
// start, 1 from a wave-dependent start with a wave-dependent odd stride.
template <int KIND>
__global__ void __launch_bounds__(THREADS) smem_kernel(const uint32_t* table, uint32_t words, uint32_t seed, uint32_t loads,
                                                       int scattered, Report* rep, unsigned long long* simd_map) {
  constexpr int W = SCALAR_SMEM_TABLE[KIND].words;
  const long long t0 = wall_clock64();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6));
  const uint32_t start = scattered ? scalar_mix32(wave) : 0u, stride = scattered ? scalar_smem_stride(wave) : 0u;
  // the raw buffer descriptor of the table: base, stride 0, num_records = its bytes, the gfx9 raw-buffer word 3
  const uint64_t base = reinterpret_cast<uint64_t>(table);
  const u32x4 rsrc = {static_cast<uint32_t>(base), static_cast<uint32_t>(base >> 32) & 0xffffu, words * 4u, 0x00020000u};
  uint32_t nbad = 0, first = ~0u, got = 0, want = 0;
  for (uint32_t k = 0; k < loads; ++k) {
    const uint32_t idx = scalar_smem_index(k, start, stride, W, words);  // a multiple of W, <= words - W
    const auto v = smem_load<KIND>(table, rsrc, idx * 4u);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t g = word_of<W>(v, j), w = scalar_smem_word(seed, idx + j);
      if (g != w) {
        if (!nbad) first = idx + j, got = g, want = w;
        ++nbad;
      }
    }
  }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  if ((threadIdx.x & 63u) == 0) report(rep, simd_map, row, nbad, where_of(row, first), 0, got, want, dt);
}

struct SmemLaunch {
  const uint32_t* table;
  uint32_t words, seed, loads;
  int scattered;
  Report* rep;
  unsigned long long* map;
  unsigned blocks;
};
template <int KIND>
void launch_kind(const SmemLaunch& l) {
  hipLaunchKernelGGL(smem_kernel<KIND>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.table, l.words, l.seed, l.loads,
                     l.scattered, l.rep, l.map);
}
template <int KIND>
hipError_t attributes_kind(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(smem_kernel<KIND>));
}
template <int... K>
struct Kinds {
  static constexpr void (*launch[])(const SmemLaunch&) = {launch_kind<K>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_kind<K>...};
};
template <int... I>
Kinds<I...> kinds_of(std::integer_sequence<int, I...>);
using AllKinds = decltype(kinds_of(std::make_integer_sequence<int, SCALAR_SMEM_KINDS>()));

// --- host ------------------------------------------------------------------------------------------------------
// -3 with a message when a kernel was built with scratch or LDS
int refuse(const hipFuncAttributes& attr, const std::string& what) {
  return refuse_memory("scalar test", what, attr, ": it would test memory, not the scalar unit");
}

}  // namespace

extern "C" {

const char* scalar_last_error(void) { return g_err.c_str(); }

int scalar_device_count(void) { return device_count(); }

int scalar_slots(void) { return SIMD_ROWS; }  // rows of every simd_map below

int scalar_sgpr_lo(void) { return SG_LO; }  // the SGPR file test covers s[lo]..s[hi] of every wave

int scalar_sgpr_hi(void) { return SG_HI; }

int scalar_sgpr_regs(void) { return SG_REGS; }  // how many of them: the reserved s32 in between is left alone

// The scalar ALU.  Every op of `ops[0..nops)` (ScalarOp of scalar_ref.h), one after the other, on `blocks`
// workgroups of 4 waves (0: 4 per CU), `iters` steps of 4 chains per wave: a checked warm-up launch, then `reps`
// timed and checked launches.  Per op k (arrays of the table's length): errors[k] = wrong wave-words over all its
// launches; first_where[k] = slot << 32 | chain of one wrong word of the first launch that had any (~0: none),
// got[k] / want[k] that chain's word and the model's; ms[k] the mean time of a timed launch.  simd_map:
// scalar_slots() x 3 (waves run, wrong words, summed wall_clock64 ticks) per physical SIMD (simd_row()),
// added up over every launch of every op.
//
// Refused with -2 and a message: a bad device, blocks < 0, iters outside 1..2^20, reps < 1, no op or an unknown
// one, a hook outside the list or the grid; with -3: a kernel built with a scratch segment or an LDS allocation.
//
// Self-check hooks, off by default (inject_op -1), both acting in the warm-up launch of op `inject_op`, on wave 0 of
// workgroup `inject_block`:
//   flip  (inject_skip_iter < 0): one bit of the final chain-0 word is flipped before the compare: 1 wrong word,
//         got = want ^ 0x10
//   skip  (inject_skip_iter >= 0): the wave leaves the instruction out of that one step; wrong words > 0
int scalar_salu(int device, int blocks, int iters, int reps, const int* ops, int nops, uint64_t seed, int inject_op,
                int inject_block, int inject_skip_iter, unsigned long long* errors, unsigned long long* first_where,
                unsigned long long* got, unsigned long long* want, double* ms, unsigned long long* simd_map,
                int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || iters < 1 || iters > MAX_ITERS || reps < 1 ||
      !op_list_known(ops, nops, SCALAR_OPS, false)) {
    g_err = "scalar salu: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a list of known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, SALU_BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (!op_list_has_hook(ops, nops, inject_op) || (inject_op >= 0 && !hook_in_range(inject_block, grid, inject_skip_iter, iters))) {
    g_err = "scalar salu: inject_op must be in the list, inject_block inside the grid and inject_skip_iter below iters";
    return -2;
  }
  for (int k = 0; k < SCALAR_OPS; ++k) {
    errors[k] = got[k] = want[k] = 0;
    first_where[k] = ~0ULL;
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf dexp;
  HIP_CHECK(dexp.alloc(device, SCALAR_CHAINS * sizeof(uint32_t)));
  uint32_t expect[SCALAR_CHAINS];
  for (int i = 0; i < nops; ++i) {
    const int k = ops[i];
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse(attr, SCALAR_OP_TABLE[k].name)) return rc;
    scalar_expected(k, seed, iters, -1, expect);
    HIP_CHECK(hipMemcpy(dexp.ptr, expect, sizeof expect, hipMemcpyHostToDevice));
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_iter);
      AllOps::launch[k]({static_cast<const uint32_t*>(dexp.ptr), scalar_op_seed(seed, k), iters, h.flip_block, h.skip_block,
                         h.skip_at, run.rep(), run.map(), grid});
    };
    if (const int rc = run.series(reps, enqueue, errors + k, rec, ms + k)) return rc;
    first_where[k] = rec[0], got[k] = rec[2], want[k] = rec[3];
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// The SGPR file.  `blocks` workgroups of 4 waves (0: 7 per CU); every wave writes s[lo]..s[hi] whole under each of
// four patterns (scalar_sgpr_word() of its key; its inverse; 0x55555555; 0xAAAAAAAA), holds them for `hold` x
// s_sleep 8 and checks every register: a warm-up launch and `reps` timed ones, all checked.  *errors = wrong
// registers over all launches; *first_where = slot << 32 | pattern << 8 | register of the first wrong register in
// one wave's walk (~0: none), *got / *want its word and the expected one; *ms the mean time of a timed launch;
// simd_map as scalar_salu's.  Refusals as scalar_salu's (hold 0..65536).
//
// Self-check hook, in the warm-up launch on wave 0 of workgroup `inject_block`: inject_reg 0 / 1 flips one bit of
// the lowest / highest tested register between the first pattern's write and its check (-1: off).
int scalar_sgpr(int device, int blocks, int reps, int hold, uint64_t seed, int inject_block, int inject_reg,
                unsigned long long* errors, unsigned long long* first_where, unsigned long long* got,
                unsigned long long* want, double* ms, unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || reps < 1 || hold < 0 || hold > 65536 || inject_reg < -1 || inject_reg > 1) {
    g_err = "scalar sgpr: need a valid device, blocks >= 0 (0: 7 per CU), reps >= 1, hold 0..65536 and inject_reg -1, 0 (lowest) or 1 (highest)";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, SGPR_BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (inject_reg >= 0 && (inject_block < 0 || static_cast<unsigned>(inject_block) >= grid)) {
    g_err = "scalar sgpr: inject_block outside the grid";
    return -2;
  }
  *errors = *got = *want = 0;
  *first_where = ~0ULL;
  *ms = 0.0;
  hipFuncAttributes attr;
  HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(sgpr_kernel)));
  if (const int rc = refuse(attr, "the SGPR file")) return rc;
  Run run;
  if (const int rc = run.open(device)) return rc;
  unsigned long long rec[4] = {~0ULL, 0, 0, 0};
  const auto enqueue = [&](int r) {
    hipLaunchKernelGGL(sgpr_kernel, dim3(grid), dim3(THREADS), 0, nullptr, seed + static_cast<uint64_t>(r), hold,
                       r == 0 ? inject_block : -1, r == 0 ? inject_reg : -1, run.rep(), run.map());
  };
  if (const int rc = run.series(reps, enqueue, errors, rec, ms)) return rc;
  *first_where = rec[0], *got = rec[2], *want = rec[3];
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// Scalar loads.  Every kind whose bit is set in `kind_mask` (ScalarSmemKind of scalar_ref.h) on `blocks` workgroups
// of 4 waves (0: 4 per CU): over a table of `small_bytes`, walked in order `passes` times by every wave (after the
// first pass the loads hit the scalar cache), and over one of `large_bytes`, `loads` loads per wave from a
// wave-dependent start with a wave-dependent stride (most miss).  Both sizes are powers of two from 64 B to 64 MiB.
// Each table gets a warm-up launch and `reps` timed ones, all checked.  Per kind k: errors[k] = wrong words;
// first_where[k] = slot << 32 | the table index of one wrong word (~0: none; the small table's launches come
// first), got[k] / want[k]; ms_hit[k] / ms_miss[k] the mean time of a timed launch over the small / large table.
// simd_map as scalar_salu's.
//
// Self-check hook: inject_word >= 0 has the host flip one bit of that word of the small table after the fill.
int scalar_smem(int device, int blocks, int reps, unsigned int small_bytes, unsigned int large_bytes, int passes, int loads,
                unsigned int kind_mask, uint64_t seed, long long inject_word, unsigned long long* errors,
                unsigned long long* first_where, unsigned long long* got, unsigned long long* want, double* ms_hit,
                double* ms_miss, unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  const auto size_ok = [](unsigned b) { return b >= 64 && b / 4 <= MAX_TABLE_WORDS && (b & (b - 1)) == 0; };
  if (device < 0 || device >= n || blocks < 0 || reps < 1 || !size_ok(small_bytes) || !size_ok(large_bytes) || passes < 1 ||
      passes > 4096 || loads < 1 || loads > MAX_ITERS || !kind_mask || (kind_mask >> SCALAR_SMEM_KINDS) ||
      inject_word >= static_cast<long long>(small_bytes / 4)) {
    g_err = "scalar smem: need a valid device, blocks >= 0 (0: 4 per CU), reps >= 1, table sizes that are powers of two "
            "from 64 B to 64 MiB, passes 1..4096, loads 1..2^20, a mask of known kinds and inject_word inside the small table";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, SMEM_BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  for (int k = 0; k < SCALAR_SMEM_KINDS; ++k) {
    errors[k] = got[k] = want[k] = 0;
    first_where[k] = ~0ULL;
    ms_hit[k] = ms_miss[k] = 0.0;
  }
  const uint32_t seed32 = scalar_mix32(seed);
  const uint32_t words[2] = {small_bytes / 4, large_bytes / 4};
  DevBuf table[2];
  for (int t = 0; t < 2; ++t) {
    std::vector<uint32_t> fill(words[t]);
    for (uint32_t i = 0; i < words[t]; ++i) fill[i] = scalar_smem_word(seed32, i);
    HIP_CHECK(table[t].alloc(device, static_cast<size_t>(words[t]) * sizeof(uint32_t)));
    HIP_CHECK(hipMemcpy(table[t].ptr, fill.data(), fill.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (inject_word >= 0)  // inside the small table: checked above
    if (const int rc = flip_word_bit(static_cast<uint32_t*>(table[0].ptr) + inject_word)) return rc;
  Run run;
  if (const int rc = run.open(device)) return rc;
  for (int k = 0; k < SCALAR_SMEM_KINDS; ++k) {
    if (!((kind_mask >> k) & 1u)) continue;
    hipFuncAttributes attr;
    HIP_CHECK(AllKinds::attributes[k](&attr));
    if (const int rc = refuse(attr, SCALAR_SMEM_TABLE[k].name)) return rc;
    const uint32_t width = static_cast<uint32_t>(SCALAR_SMEM_TABLE[k].words);
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};
    for (int t = 0; t < 2; ++t) {
      const uint32_t nloads = t == 0 ? static_cast<uint32_t>(passes) * (words[0] / width) : static_cast<uint32_t>(loads);
      const SmemLaunch l = {static_cast<const uint32_t*>(table[t].ptr), words[t], seed32, nloads, t, run.rep(), run.map(), grid};
      if (const int rc = run.series(reps, [&](int) { AllKinds::launch[k](l); }, errors + k, rec, (t == 0 ? ms_hit : ms_miss) + k))
        return rc;
    }
    first_where[k] = rec[0], got[k] = rec[2], want[k] = rec[3];
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// `n` applications of op `op` by one wave of `device`, one after the other, returned raw: result[i] the destination
// after the instruction on S0 = a[i], S1 = b[i] with SCC = scc_in[i] before it (zero-extended; 0 for a compare),
// scc_out[i] SCC after it.
int scalar_apply(int device, int op, int n, const uint64_t* a, const uint64_t* b, const unsigned int* scc_in,
                 uint64_t* result, unsigned int* scc_out) {
  const int ndev = device_count();
  bool flags = n >= 1 && n <= MAX_ITERS;
  for (int i = 0; flags && i < n; ++i) flags = scc_in[i] <= 1;
  if (device < 0 || device >= ndev || op < 0 || op >= SCALAR_OPS || !flags) {
    g_err = "scalar apply: need a valid device, an op of the table, 1..2^20 rows and scc_in 0 or 1";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  std::vector<uint64_t> in(3 * static_cast<size_t>(n)), out(2 * static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) in[3 * i] = a[i], in[3 * i + 1] = b[i], in[3 * i + 2] = scc_in[i];
  DevBuf din, dout;
  HIP_CHECK(din.alloc(device, in.size() * sizeof(uint64_t)));
  HIP_CHECK(dout.alloc(device, out.size() * sizeof(uint64_t)));
  HIP_CHECK(hipMemcpy(din.ptr, in.data(), in.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  AllOps::apply[op](static_cast<const uint64_t*>(din.ptr), static_cast<uint64_t*>(dout.ptr), n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out.data(), dout.ptr, out.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) result[i] = out[2 * i], scc_out[i] = static_cast<unsigned int>(out[2 * i + 1]);
  return 0;
}

}  // extern "C"
