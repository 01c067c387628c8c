// The scalar diagnostic's ops (scalar.hip) and what a correct wave must compute: a model of every scalar-ALU
// instruction of the table, written from the ISA's definitions, the pattern of the SGPR-file test and the pattern of
// the scalar-load test.  Plain C++ that the host compiler takes alone: scalar.hip includes it for its kernels (the
// op table, the constants, the hash) and its host side (the expected words), and tests/test_scalar_cpu.py compiles
// it with g++ into a stand-alone program.
//
// An op takes two 64-bit operands a (S0) and b (S1) -- the 32-bit instructions read their low halves -- and SCC, and
// leaves a result (zero-extended to 64 bits; 0 for a compare) and SCC.  A chain step is
//     y = ~x;  a = y:x;  b = (x + c):(y ^ c);  scc_in = x[13];  (r, scc) = op(a, b, scc_in);
//     x = scalar_mix32((x << 32 | scalar_fold(r, scc)) + c)
// so every step depends on the previous result and on SCC.  The chain's own word rides in the hash's upper half: an
// op that collapses its inputs (min, bcnt, a compare) would otherwise forget a step that went wrong before it.  S1 is
// not the bare complement of S0: under b = ~a every and / or / xor would see the same operand pair relation at every
// step (and = 0, or = xor = ~0).
#ifndef K8S_GPU_NODE_CHECKER_AMD_SCALAR_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_SCALAR_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCALAR_HD __host__ __device__ inline
#else
#define SCALAR_HD inline
#endif

constexpr int SCALAR_CHAINS = 4;  // independent chains per wave

// the 16-bit immediates of the two SOPK ops (sign-extended by the instruction)
#define SCALAR_ADDK_IMM 0x6b35
#define SCALAR_MULK_IMM -0x2c4b

// X(enum, mnemonic, operand form).  The forms (what scalar.hip writes around the mnemonic):
//   D32_AB32  insn d, a, b          D64_AB64  insn d[2], a[2], b[2]     D64_A64_B32  insn d[2], a[2], b
//   D64_AB32  insn d[2], a, b       D32_A32   insn d, a                 D64_A64      insn d[2], a[2]
//   D32_A64   insn d, a[2]          D64_A32   insn d[2], a              RMW32_A32    insn d, a   (d preset to b)
//   K_ADD / K_MUL  insn d, imm16 (d preset to a)                        CMP32  insn a, b        CMP64  insn a[2], b[2]
#define SCALAR_OP_LIST(X)                                 \
  /* add / sub and the carry chain */                     \
  X(SCALAR_ADD_U32, s_add_u32, D32_AB32)                  \
  X(SCALAR_ADDC_U32, s_addc_u32, D32_AB32)                \
  X(SCALAR_SUB_U32, s_sub_u32, D32_AB32)                  \
  X(SCALAR_SUBB_U32, s_subb_u32, D32_AB32)                \
  X(SCALAR_ADD_I32, s_add_i32, D32_AB32)                  \
  X(SCALAR_SUB_I32, s_sub_i32, D32_AB32)                  \
  X(SCALAR_ABSDIFF_I32, s_absdiff_i32, D32_AB32)          \
  X(SCALAR_LSHL1_ADD_U32, s_lshl1_add_u32, D32_AB32)      \
  X(SCALAR_LSHL2_ADD_U32, s_lshl2_add_u32, D32_AB32)      \
  X(SCALAR_LSHL3_ADD_U32, s_lshl3_add_u32, D32_AB32)      \
  X(SCALAR_LSHL4_ADD_U32, s_lshl4_add_u32, D32_AB32)      \
  X(SCALAR_ADDK_I32, s_addk_i32, K_ADD)                   \
  /* the multiplier */                                    \
  X(SCALAR_MUL_I32, s_mul_i32, D32_AB32)                  \
  X(SCALAR_MUL_HI_U32, s_mul_hi_u32, D32_AB32)            \
  X(SCALAR_MUL_HI_I32, s_mul_hi_i32, D32_AB32)            \
  X(SCALAR_MULK_I32, s_mulk_i32, K_MUL)                   \
  /* logic, 32 and 64 bit */                              \
  X(SCALAR_AND_B32, s_and_b32, D32_AB32)                  \
  X(SCALAR_OR_B32, s_or_b32, D32_AB32)                    \
  X(SCALAR_XOR_B32, s_xor_b32, D32_AB32)                  \
  X(SCALAR_ANDN2_B32, s_andn2_b32, D32_AB32)              \
  X(SCALAR_ORN2_B32, s_orn2_b32, D32_AB32)                \
  X(SCALAR_NAND_B32, s_nand_b32, D32_AB32)                \
  X(SCALAR_NOR_B32, s_nor_b32, D32_AB32)                  \
  X(SCALAR_XNOR_B32, s_xnor_b32, D32_AB32)                \
  X(SCALAR_NOT_B32, s_not_b32, D32_A32)                   \
  X(SCALAR_AND_B64, s_and_b64, D64_AB64)                  \
  X(SCALAR_OR_B64, s_or_b64, D64_AB64)                    \
  X(SCALAR_XOR_B64, s_xor_b64, D64_AB64)                  \
  X(SCALAR_ANDN2_B64, s_andn2_b64, D64_AB64)              \
  X(SCALAR_ORN2_B64, s_orn2_b64, D64_AB64)                \
  X(SCALAR_NAND_B64, s_nand_b64, D64_AB64)                \
  X(SCALAR_NOR_B64, s_nor_b64, D64_AB64)                  \
  X(SCALAR_XNOR_B64, s_xnor_b64, D64_AB64)                \
  X(SCALAR_NOT_B64, s_not_b64, D64_A64)                   \
  /* the shifter */                                       \
  X(SCALAR_LSHL_B32, s_lshl_b32, D32_AB32)                \
  X(SCALAR_LSHR_B32, s_lshr_b32, D32_AB32)                \
  X(SCALAR_ASHR_I32, s_ashr_i32, D32_AB32)                \
  X(SCALAR_LSHL_B64, s_lshl_b64, D64_A64_B32)             \
  X(SCALAR_LSHR_B64, s_lshr_b64, D64_A64_B32)             \
  X(SCALAR_ASHR_I64, s_ashr_i64, D64_A64_B32)             \
  X(SCALAR_BFM_B32, s_bfm_b32, D32_AB32)                  \
  X(SCALAR_BFM_B64, s_bfm_b64, D64_AB32)                  \
  X(SCALAR_BFE_U32, s_bfe_u32, D32_AB32)                  \
  X(SCALAR_BFE_I32, s_bfe_i32, D32_AB32)                  \
  X(SCALAR_BFE_U64, s_bfe_u64, D64_A64_B32)               \
  X(SCALAR_BFE_I64, s_bfe_i64, D64_A64_B32)               \
  /* bit scan, count and permute */                       \
  X(SCALAR_BCNT0_I32_B32, s_bcnt0_i32_b32, D32_A32)       \
  X(SCALAR_BCNT1_I32_B64, s_bcnt1_i32_b64, D32_A64)       \
  X(SCALAR_FF0_I32_B32, s_ff0_i32_b32, D32_A32)           \
  X(SCALAR_FF1_I32_B64, s_ff1_i32_b64, D32_A64)           \
  X(SCALAR_FLBIT_I32_B32, s_flbit_i32_b32, D32_A32)       \
  X(SCALAR_FLBIT_I32, s_flbit_i32, D32_A32)               \
  X(SCALAR_FLBIT_I32_I64, s_flbit_i32_i64, D32_A64)       \
  X(SCALAR_BREV_B32, s_brev_b32, D32_A32)                 \
  X(SCALAR_BREV_B64, s_brev_b64, D64_A64)                 \
  X(SCALAR_BITSET0_B32, s_bitset0_b32, RMW32_A32)         \
  X(SCALAR_BITSET1_B32, s_bitset1_b32, RMW32_A32)         \
  X(SCALAR_WQM_B64, s_wqm_b64, D64_A64)                   \
  X(SCALAR_QUADMASK_B64, s_quadmask_b64, D64_A64)         \
  X(SCALAR_BITREPLICATE_B64_B32, s_bitreplicate_b64_b32, D64_A32) \
  /* select, extend, pack */                              \
  X(SCALAR_MIN_I32, s_min_i32, D32_AB32)                  \
  X(SCALAR_MIN_U32, s_min_u32, D32_AB32)                  \
  X(SCALAR_MAX_I32, s_max_i32, D32_AB32)                  \
  X(SCALAR_MAX_U32, s_max_u32, D32_AB32)                  \
  X(SCALAR_CSELECT_B32, s_cselect_b32, D32_AB32)          \
  X(SCALAR_CSELECT_B64, s_cselect_b64, D64_AB64)          \
  X(SCALAR_CMOV_B32, s_cmov_b32, RMW32_A32)               \
  X(SCALAR_SEXT_I32_I8, s_sext_i32_i8, D32_A32)           \
  X(SCALAR_SEXT_I32_I16, s_sext_i32_i16, D32_A32)         \
  X(SCALAR_ABS_I32, s_abs_i32, D32_A32)                   \
  X(SCALAR_PACK_LL_B32_B16, s_pack_ll_b32_b16, D32_AB32)  \
  X(SCALAR_PACK_LH_B32_B16, s_pack_lh_b32_b16, D32_AB32)  \
  X(SCALAR_PACK_HH_B32_B16, s_pack_hh_b32_b16, D32_AB32)  \
  /* compares: the result is SCC */                       \
  X(SCALAR_CMP_EQ_I32, s_cmp_eq_i32, CMP32)               \
  X(SCALAR_CMP_LG_U32, s_cmp_lg_u32, CMP32)               \
  X(SCALAR_CMP_GT_I32, s_cmp_gt_i32, CMP32)               \
  X(SCALAR_CMP_GE_U32, s_cmp_ge_u32, CMP32)               \
  X(SCALAR_CMP_LT_U32, s_cmp_lt_u32, CMP32)               \
  X(SCALAR_CMP_LT_I32, s_cmp_lt_i32, CMP32)               \
  X(SCALAR_CMP_LE_I32, s_cmp_le_i32, CMP32)               \
  X(SCALAR_CMP_EQ_U64, s_cmp_eq_u64, CMP64)               \
  X(SCALAR_BITCMP0_B32, s_bitcmp0_b32, CMP32)             \
  X(SCALAR_BITCMP1_B32, s_bitcmp1_b32, CMP32)

enum ScalarOp {
#define SCALAR_X_ENUM(E, M, F) E,
  SCALAR_OP_LIST(SCALAR_X_ENUM)
#undef SCALAR_X_ENUM
  SCALAR_OPS,
};
static_assert(SCALAR_OPS >= 48, "the table holds at least 48 ops");

struct ScalarOpInfo {
  const char* name;  // the instruction's mnemonic
};
// the name of op k (the index is the enum's)
inline constexpr ScalarOpInfo SCALAR_OP_TABLE[SCALAR_OPS] = {
#define SCALAR_X_NAME(E, M, F) {#M},
    SCALAR_OP_LIST(SCALAR_X_NAME)
#undef SCALAR_X_NAME
};

struct ScalarOut {
  uint64_t result;  // the destination, zero-extended (0 for a compare)
  uint32_t scc;     // SCC after the instruction
};

// The 64 -> 32 bit hash of the chains: the project's mix32 (common/hip_host.h; murmur3's finalizer), here for both
// compilers.
SCALAR_HD uint32_t scalar_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// a chain's starting word and its per-step constant, distinct per chain and moved by the seed
SCALAR_HD uint32_t scalar_init(uint64_t seed, int chain) {
  return scalar_mix32(seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(chain + 1));
}
SCALAR_HD uint32_t scalar_const(uint64_t seed, int chain) {
  return scalar_mix32(seed + 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(chain + 1));
}
// the seed of op k's chains
SCALAR_HD uint64_t scalar_op_seed(uint64_t seed, int op) { return seed + 0x632BE59BD9B4E019ULL * static_cast<uint64_t>(op + 1); }

// --- helpers of the model (no shift by the type's width, no signed overflow: the host sanitizers run this) -------
SCALAR_HD uint32_t scalar_rotl32(uint32_t v, int n) { return n ? (v << n) | (v >> (32 - n)) : v; }
SCALAR_HD uint32_t scalar_sar32(uint32_t v, int n) {  // arithmetic shift right, n in 0..31
  const uint32_t fill = (v >> 31) && n ? ~0u << (32 - n) : 0u;
  return (v >> n) | fill;
}
SCALAR_HD uint64_t scalar_sar64(uint64_t v, int n) {  // n in 0..63
  const uint64_t fill = (v >> 63) && n ? ~0ULL << (64 - n) : 0ULL;
  return (v >> n) | fill;
}
SCALAR_HD uint32_t scalar_brev32(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
  return r;
}
SCALAR_HD uint32_t scalar_popc64(uint64_t v) {
  uint32_t n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}
// the index of the lowest set bit, -1 (as 32 bits) when there is none
SCALAR_HD uint32_t scalar_ff1_64(uint64_t v) {
  for (int i = 0; i < 64; ++i)
    if ((v >> i) & 1ULL) return static_cast<uint32_t>(i);
  return ~0u;
}
// how many bits from the top (bit width-1) down are 0 before the first 1; -1 when v has no 1
SCALAR_HD uint32_t scalar_flbit(uint64_t v, int width) {
  for (int i = 0; i < width; ++i)
    if ((v >> (width - 1 - i)) & 1ULL) return static_cast<uint32_t>(i);
  return ~0u;
}
// signed overflow of a + b = r and of a - b = r (32 bit)
SCALAR_HD uint32_t scalar_add_ovf(uint32_t a, uint32_t b, uint32_t r) { return ((~(a ^ b) & (a ^ r)) >> 31) & 1u; }
SCALAR_HD uint32_t scalar_sub_ovf(uint32_t a, uint32_t b, uint32_t r) { return (((a ^ b) & (a ^ r)) >> 31) & 1u; }

// S_BFE: the field of `width_bits`-wide S0 at offset S1[4:0] (32) / S1[5:0] (64), S1[22:16] bits wide; width 0 gives
// 0, a field that reaches the top bit is the plain shift, the signed form extends from the field's top bit.
SCALAR_HD uint64_t scalar_bfe(uint64_t s0, uint32_t s1, int width_bits, bool is_signed) {
  const int off = static_cast<int>(s1 & static_cast<uint32_t>(width_bits - 1));
  const int w = static_cast<int>((s1 >> 16) & 0x7fu);
  const uint64_t all = width_bits == 64 ? ~0ULL : 0xffffffffULL;
  if (w == 0) return 0;
  if (off + w >= width_bits) {
    if (!is_signed) return s0 >> off;
    return (width_bits == 64 ? scalar_sar64(s0, off) : scalar_sar32(static_cast<uint32_t>(s0), off)) & all;
  }
  const uint64_t mask = (1ULL << w) - 1;
  uint64_t f = (s0 >> off) & mask;
  if (is_signed && ((f >> (w - 1)) & 1ULL)) f |= ~mask & all;
  return f;
}

// One application of op `op`: a = S0, b = S1 (the 32-bit instructions read the low halves), scc_in = SCC before it.
// An op the ISA says leaves SCC alone returns scc_in.
SCALAR_HD ScalarOut scalar_apply(int op, uint64_t a, uint64_t b, uint32_t scc_in) {
  const uint32_t a32 = static_cast<uint32_t>(a), b32 = static_cast<uint32_t>(b);
  const int32_t ai = static_cast<int32_t>(a32), bi = static_cast<int32_t>(b32);
  const uint32_t cin = scc_in & 1u;
  uint64_t r = 0;
  uint32_t scc = cin;
  enum { KEEP, NONZERO, SET } rule = NONZERO;  // how SCC follows: untouched, result != 0, set by the case itself
  switch (op) {
    // D = S0 + S1; SCC = unsigned carry out
    case SCALAR_ADD_U32: { const uint64_t t = static_cast<uint64_t>(a32) + b32; r = static_cast<uint32_t>(t), scc = static_cast<uint32_t>(t >> 32), rule = SET; break; }
    // D = S0 + S1 + SCC; SCC = unsigned carry out
    case SCALAR_ADDC_U32: { const uint64_t t = static_cast<uint64_t>(a32) + b32 + cin; r = static_cast<uint32_t>(t), scc = static_cast<uint32_t>(t >> 32), rule = SET; break; }
    // D = S0 - S1; SCC = unsigned borrow (S1 > S0)
    case SCALAR_SUB_U32: r = a32 - b32, scc = b32 > a32, rule = SET; break;
    // D = S0 - S1 - SCC; SCC = unsigned borrow (S1 + SCC > S0)
    case SCALAR_SUBB_U32: r = a32 - b32 - cin, scc = static_cast<uint64_t>(b32) + cin > a32, rule = SET; break;
    // the signed forms: the same sum or difference, SCC = signed overflow
    case SCALAR_ADD_I32: r = a32 + b32, scc = scalar_add_ovf(a32, b32, a32 + b32), rule = SET; break;
    case SCALAR_SUB_I32: r = a32 - b32, scc = scalar_sub_ovf(a32, b32, a32 - b32), rule = SET; break;
    // D = S0 - S1 as 32 bits, negated when negative (so 0x80000000 stays); SCC = D != 0
    case SCALAR_ABSDIFF_I32: { const uint32_t d = a32 - b32; r = (d >> 31) ? 0u - d : d; break; }
    // D = (S0 << N) + S1 in 64 bits; SCC = the sum does not fit 32 bits
    case SCALAR_LSHL1_ADD_U32: case SCALAR_LSHL2_ADD_U32: case SCALAR_LSHL3_ADD_U32: case SCALAR_LSHL4_ADD_U32: {
      const uint64_t t = (static_cast<uint64_t>(a32) << (op - SCALAR_LSHL1_ADD_U32 + 1)) + b32;
      r = static_cast<uint32_t>(t), scc = t >= 0x100000000ULL, rule = SET;
      break;
    }
    // D = D + sext(imm16) (D preset to S0); SCC = signed overflow
    case SCALAR_ADDK_I32: { const uint32_t k = static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(SCALAR_ADDK_IMM))); r = a32 + k, scc = scalar_add_ovf(a32, k, a32 + k), rule = SET; break; }
    // the multiplier leaves SCC alone: the low 32 bits, the high 32 bits unsigned and signed, D * sext(imm16)
    case SCALAR_MUL_I32: r = a32 * b32, rule = KEEP; break;
    case SCALAR_MUL_HI_U32: r = (static_cast<uint64_t>(a32) * b32) >> 32, rule = KEEP; break;
    case SCALAR_MUL_HI_I32: r = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(ai) * static_cast<int64_t>(bi)) >> 32), rule = KEEP; break;
    case SCALAR_MULK_I32: r = a32 * static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(SCALAR_MULK_IMM))), rule = KEEP; break;
    // logic: SCC = D != 0; andn2 = S0 & ~S1, orn2 = S0 | ~S1
    case SCALAR_AND_B32: r = a32 & b32; break;
    case SCALAR_OR_B32: r = a32 | b32; break;
    case SCALAR_XOR_B32: r = a32 ^ b32; break;
    case SCALAR_ANDN2_B32: r = a32 & ~b32; break;
    case SCALAR_ORN2_B32: r = a32 | ~b32; break;
    case SCALAR_NAND_B32: r = ~(a32 & b32); break;
    case SCALAR_NOR_B32: r = ~(a32 | b32); break;
    case SCALAR_XNOR_B32: r = ~(a32 ^ b32); break;
    case SCALAR_NOT_B32: r = ~a32; break;
    case SCALAR_AND_B64: r = a & b; break;
    case SCALAR_OR_B64: r = a | b; break;
    case SCALAR_XOR_B64: r = a ^ b; break;
    case SCALAR_ANDN2_B64: r = a & ~b; break;
    case SCALAR_ORN2_B64: r = a | ~b; break;
    case SCALAR_NAND_B64: r = ~(a & b); break;
    case SCALAR_NOR_B64: r = ~(a | b); break;
    case SCALAR_XNOR_B64: r = ~(a ^ b); break;
    case SCALAR_NOT_B64: r = ~a; break;
    // shifts: the count is S1[4:0] (32 bit) or S1[5:0] (64 bit); SCC = D != 0
    case SCALAR_LSHL_B32: r = static_cast<uint32_t>(a32 << (b32 & 31u)); break;
    case SCALAR_LSHR_B32: r = a32 >> (b32 & 31u); break;
    case SCALAR_ASHR_I32: r = scalar_sar32(a32, static_cast<int>(b32 & 31u)); break;
    case SCALAR_LSHL_B64: r = a << (b32 & 63u); break;
    case SCALAR_LSHR_B64: r = a >> (b32 & 63u); break;
    case SCALAR_ASHR_I64: r = scalar_sar64(a, static_cast<int>(b32 & 63u)); break;
    // bit-field mask: S0[4:0] (S0[5:0]) ones, shifted left by S1[4:0] (S1[5:0]); SCC untouched
    case SCALAR_BFM_B32: r = static_cast<uint32_t>(((1u << (a32 & 31u)) - 1u) << (b32 & 31u)), rule = KEEP; break;
    case SCALAR_BFM_B64: r = ((1ULL << (a32 & 63u)) - 1ULL) << (b32 & 63u), rule = KEEP; break;
    // bit-field extract (scalar_bfe); SCC = D != 0
    case SCALAR_BFE_U32: r = scalar_bfe(a32, b32, 32, false); break;
    case SCALAR_BFE_I32: r = scalar_bfe(a32, b32, 32, true); break;
    case SCALAR_BFE_U64: r = scalar_bfe(a, b32, 64, false); break;
    case SCALAR_BFE_I64: r = scalar_bfe(a, b32, 64, true); break;
    // counts: zeros of S0 (32 bit), ones of S0 (64 bit); SCC = D != 0
    case SCALAR_BCNT0_I32_B32: r = 32u - scalar_popc64(a32); break;
    case SCALAR_BCNT1_I32_B64: r = scalar_popc64(a); break;
    // scans leave SCC alone and return -1 when the bit does not occur: the lowest 0, the lowest 1, the highest 1
    // counted from the top, and the run of bits equal to the sign bit (-1 for 0 and for -1)
    case SCALAR_FF0_I32_B32: r = scalar_ff1_64(static_cast<uint32_t>(~a32)), rule = KEEP; break;
    case SCALAR_FF1_I32_B64: r = scalar_ff1_64(a), rule = KEEP; break;
    case SCALAR_FLBIT_I32_B32: r = scalar_flbit(a32, 32), rule = KEEP; break;
    case SCALAR_FLBIT_I32: r = scalar_flbit((a32 >> 31) ? static_cast<uint32_t>(~a32) : a32, 32), rule = KEEP; break;
    case SCALAR_FLBIT_I32_I64: r = scalar_flbit((a >> 63) ? ~a : a, 64), rule = KEEP; break;
    case SCALAR_BREV_B32: r = scalar_brev32(a32), rule = KEEP; break;
    case SCALAR_BREV_B64: r = (static_cast<uint64_t>(scalar_brev32(a32)) << 32) | scalar_brev32(static_cast<uint32_t>(a >> 32)), rule = KEEP; break;
    // D (preset to S1) with bit S0[4:0] cleared / set; SCC untouched
    case SCALAR_BITSET0_B32: r = b32 & ~(1u << (a32 & 31u)), rule = KEEP; break;
    case SCALAR_BITSET1_B32: r = b32 | (1u << (a32 & 31u)), rule = KEEP; break;
    // whole-quad mode: every group of four bits with any bit set becomes 0xf; SCC = D != 0
    case SCALAR_WQM_B64:
      for (int q = 0; q < 16; ++q)
        if ((a >> (4 * q)) & 0xfULL) r |= 0xfULL << (4 * q);
      break;
    // quad mask: bit q = group q of four bits has any bit set (16 groups); SCC = D != 0
    case SCALAR_QUADMASK_B64:
      for (int q = 0; q < 16; ++q)
        if ((a >> (4 * q)) & 0xfULL) r |= 1ULL << q;
      break;
    // every bit of the 32-bit S0 twice: D[2i] = D[2i+1] = S0[i]; SCC untouched
    case SCALAR_BITREPLICATE_B64_B32:
      for (int i = 0; i < 32; ++i)
        if ((a32 >> i) & 1u) r |= 3ULL << (2 * i);
      rule = KEEP;
      break;
    // SCC = S0 was chosen (strictly smaller / larger; a tie takes S1)
    case SCALAR_MIN_I32: scc = ai < bi, r = scc ? a32 : b32, rule = SET; break;
    case SCALAR_MIN_U32: scc = a32 < b32, r = scc ? a32 : b32, rule = SET; break;
    case SCALAR_MAX_I32: scc = ai > bi, r = scc ? a32 : b32, rule = SET; break;
    case SCALAR_MAX_U32: scc = a32 > b32, r = scc ? a32 : b32, rule = SET; break;
    // read SCC, leave it alone: D = SCC ? S0 : S1; cmov: D (preset to S1) = S0 only when SCC
    case SCALAR_CSELECT_B32: r = cin ? a32 : b32, rule = KEEP; break;
    case SCALAR_CSELECT_B64: r = cin ? a : b, rule = KEEP; break;
    case SCALAR_CMOV_B32: r = cin ? a32 : b32, rule = KEEP; break;
    case SCALAR_SEXT_I32_I8: r = static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(a32 & 0xffu))), rule = KEEP; break;
    case SCALAR_SEXT_I32_I16: r = static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(a32 & 0xffffu))), rule = KEEP; break;
    // D = |S0| (0x80000000 stays); SCC = D != 0
    case SCALAR_ABS_I32: r = (a32 >> 31) ? 0u - a32 : a32; break;
    // two 16-bit halves into one word, low half first: ll = S0.lo, S1.lo; lh = S0.lo, S1.hi; hh = S0.hi, S1.hi
    case SCALAR_PACK_LL_B32_B16: r = (a32 & 0xffffu) | (b32 << 16), rule = KEEP; break;
    case SCALAR_PACK_LH_B32_B16: r = (a32 & 0xffffu) | (b32 & 0xffff0000u), rule = KEEP; break;
    case SCALAR_PACK_HH_B32_B16: r = (a32 >> 16) | (b32 & 0xffff0000u), rule = KEEP; break;
    // compares write SCC only
    case SCALAR_CMP_EQ_I32: scc = ai == bi, rule = SET; break;
    case SCALAR_CMP_LG_U32: scc = a32 != b32, rule = SET; break;
    case SCALAR_CMP_GT_I32: scc = ai > bi, rule = SET; break;
    case SCALAR_CMP_GE_U32: scc = a32 >= b32, rule = SET; break;
    case SCALAR_CMP_LT_U32: scc = a32 < b32, rule = SET; break;
    case SCALAR_CMP_LT_I32: scc = ai < bi, rule = SET; break;
    case SCALAR_CMP_LE_I32: scc = ai <= bi, rule = SET; break;
    case SCALAR_CMP_EQ_U64: scc = a == b, rule = SET; break;
    // SCC = bit S1[4:0] of S0 is 0 / is 1
    case SCALAR_BITCMP0_B32: scc = ((a32 >> (b32 & 31u)) & 1u) == 0u, rule = SET; break;
    case SCALAR_BITCMP1_B32: scc = ((a32 >> (b32 & 31u)) & 1u) == 1u, rule = SET; break;
    default: rule = KEEP; break;
  }
  if (rule == NONZERO) scc = r != 0;
  if (rule == KEEP) scc = cin;
  return {r, scc & 1u};
}

// --- the chains ------------------------------------------------------------------------------------------------
// the operands and SCC a chain word x (with its constant c) gives the op
SCALAR_HD uint64_t scalar_operand_a(uint32_t x) { return (static_cast<uint64_t>(~x) << 32) | x; }
SCALAR_HD uint64_t scalar_operand_b(uint32_t x, uint32_t c) { return (static_cast<uint64_t>(x + c) << 32) | (~x ^ c); }
SCALAR_HD uint32_t scalar_scc_in(uint32_t x) { return (x >> 13) & 1u; }
// an op's outputs as one word
SCALAR_HD uint32_t scalar_fold(uint64_t r, uint32_t scc) {
  return static_cast<uint32_t>(r) + scalar_rotl32(static_cast<uint32_t>(r >> 32), 16) + (scc ? 0x9E3779B9u : 0u);
}
// the chain's new word: `own` its word before the op, (r, scc) the op's outputs, c its constant
SCALAR_HD uint32_t scalar_step(uint32_t own, uint64_t r, uint32_t scc, uint32_t c) {
  return scalar_mix32(((static_cast<uint64_t>(own) << 32) | scalar_fold(r, scc)) + c);
}
// What a step whose instruction was left out hands to the hash: SCC as it was and a destination holding a word no op
// of the table computes from these operands (a skipped step must show whatever the op is: cselect with SCC set, a
// shift by 0 or s_abs of a positive word return S0 itself).
constexpr uint64_t SCALAR_SKIP_XOR = 0x5C3A96E1D2B4780FULL;
SCALAR_HD ScalarOut scalar_skipped(uint64_t a, uint32_t scc_in) { return {a ^ SCALAR_SKIP_XOR, scc_in & 1u}; }

// The words every wave must end with: out[chain] after `iters` steps of op `op`'s chains under `seed` (the test's
// seed: scalar_op_seed() is applied here).  skip_iter >= 0 leaves the instruction out of that one step.
inline void scalar_expected(int op, uint64_t seed, int iters, int skip_iter, uint32_t out[SCALAR_CHAINS]) {
  const uint64_t s = scalar_op_seed(seed, op);
  for (int ch = 0; ch < SCALAR_CHAINS; ++ch) {
    uint32_t x = scalar_init(s, ch);
    const uint32_t c = scalar_const(s, ch);
    for (int it = 0; it < iters; ++it) {
      const uint64_t a = scalar_operand_a(x), b = scalar_operand_b(x, c);
      const ScalarOut o = it != skip_iter ? scalar_apply(op, a, b, scalar_scc_in(x)) : scalar_skipped(a, scalar_scc_in(x));
      x = scalar_step(x, o.result, o.scc, c);
    }
    out[ch] = x;
  }
}

// --- the SGPR-file test's pattern ------------------------------------------------------------------------------
// Register r (its number, below 128) of wave `wave` of the launch holds key(seed, wave) + r * G under the first
// pattern: one odd multiple of G per (wave, register), so no two of a launch's registers hold the same word.
constexpr uint32_t SCALAR_SGPR_G = 0x9E3779B1u;
SCALAR_HD uint32_t scalar_sgpr_key(uint64_t seed, uint32_t wave) { return scalar_mix32(seed) + wave * 128u * SCALAR_SGPR_G; }
SCALAR_HD uint32_t scalar_sgpr_word(uint32_t key, int reg) { return key + static_cast<uint32_t>(reg) * SCALAR_SGPR_G; }

// --- the scalar-load test's pattern ----------------------------------------------------------------------------
// word i of a table: a hash of its index a wave recomputes in four scalar instructions
SCALAR_HD uint32_t scalar_smem_word(uint32_t seed, uint32_t i) { return ((i ^ seed) * 0x9E3779B1u) ^ (i >> 3); }

enum ScalarSmemKind {
  SCALAR_SMEM_LOAD_X1 = 0,
  SCALAR_SMEM_LOAD_X2,
  SCALAR_SMEM_LOAD_X4,
  SCALAR_SMEM_LOAD_X8,
  SCALAR_SMEM_LOAD_X16,
  SCALAR_SMEM_BUFFER_X1,
  SCALAR_SMEM_BUFFER_X4,
  SCALAR_SMEM_KINDS,
};
struct ScalarSmemInfo {
  const char* name;  // the instruction's mnemonic
  int words;         // dwords per load
};
inline constexpr ScalarSmemInfo SCALAR_SMEM_TABLE[SCALAR_SMEM_KINDS] = {
    {"s_load_dword", 1},         {"s_load_dwordx2", 2},          {"s_load_dwordx4", 4}, {"s_load_dwordx8", 8},
    {"s_load_dwordx16", 16},     {"s_buffer_load_dword", 1},     {"s_buffer_load_dwordx4", 4},
};
// Load k of a wave's walk over a table of `words` words (a power of two, at least 16): the index of its first word.
// stride 0 walks the table in order (the small table: after the first pass every load hits); a wave-dependent odd
// `stride` (in loads) scatters the walk (the large table).  Always a multiple of `width` below `words`.
SCALAR_HD uint32_t scalar_smem_index(uint32_t k, uint32_t start, uint32_t stride, uint32_t width, uint32_t words) {
  return ((start + k * (stride ? stride : 1u)) * width) & (words - 1u);
}
SCALAR_HD uint32_t scalar_smem_stride(uint32_t wave) { return (scalar_mix32(0x5CA1A4ULL + wave) & 0xffeu) | 1u; }

#endif  // K8S_GPU_NODE_CHECKER_AMD_SCALAR_REF_H_
