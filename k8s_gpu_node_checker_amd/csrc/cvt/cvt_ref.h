// The cvt diagnostic's ops (cvt.hip) and what a correct SIMD must compute: a model of the format conversions of the
// vector ALU, written from the rule -- sign, exponent and significand arithmetic on integers, never a cast through the
// host's own _Float16 / __bf16 / float.  Plain C++ that the host compiler takes alone: cvt.hip includes it for its
// kernels (the op table, the shapes, the hash) and its host side (the expected words), and tests/test_cvt_cpu.py
// compiles it with g++ into a stand-alone program.
//
// An in-range conversion has one correct result, so the host computes it.  A chain step is
//     x = cvt_mix32((x << 32 | cvt_fold(op(cvt_shape(op, x)))) + c[lane][chain])
// where cvt_shape() maps the 32-bit chain word into the op's operand domain (integer operations only, the same on host
// and device) and steers it to where a converter goes wrong: exact ties (to even both ways), one ulp of the source
// either side of a tie, the largest finite result, the smallest normal and the subnormal range of the destination,
// +-0, and two different halves for the packed ops.
//
// THE DOMAIN.  cvt_convert() refuses (returns false; cvt_in_domain() is that answer alone) operands outside it:
//   * every source is finite (no Inf, no NaN; the E4M3 codes 0x7f / 0xff are NaN, fp4 has neither)
//   * every float result lies in the destination's finite range after scaling: normal and subnormal results, no
//     overflow, Inf or NaN.  fp8 is OCP E4M3 (bias 7, largest finite 448), bf8 OCP E5M2 (bias 15, largest finite
//     57344), fp4 E2M1 (bias 1, largest 6)
//   * the scale of a scalef32 op is an exact power of two from 2^-8 to 2^8 (sign 0, mantissa 0), so every reading of
//     the operand agrees on its value.  A narrowing op divides by the scale, a widening op multiplies by it
//   * float-to-integer ops clamp to the destination's range as the ISA states (NaN is still refused);
//     v_cvt_pk_u8_f32 is kept to results 0..255 and sources >= 0
//   * v_cvt_rpi_i32_f32 is floor(x + 0.5): kept to x whose x + 0.5 is exact in fp32, so that a sum computed in fp32
//     and one computed exactly agree; v_cvt_pknorm_* to |x| with at most 9 significant bits (or beyond +-1, the
//     clamp), so that x * 32767 (65535) is exact in fp32 for the same reason
// The model is written for round-to-nearest-even with denormals kept (MODE.FP_ROUND = 0, MODE.FP_DENORM = 0xf); cvt.hip
// reads the wave's MODE and refuses to run under another.
//
// Not built (no kernel, no model; none was tried on a device): the stochastic-rounding (sr) group.
#ifndef K8S_GPU_NODE_CHECKER_AMD_CVT_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_CVT_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CVT_HD __host__ __device__ inline
#else
#define CVT_HD inline
#endif

constexpr int CVT_WAVE = 64;
constexpr int CVT_CHAINS = 4;  // independent chains per lane

enum CvtGroup { CG_CLASSIC = 0, CG_BF16, CG_FP8, CG_SCALEF32 };
// the instruction of an op, without its select
enum CvtKind {
  CK_F16_F32 = 0, CK_F32_F16, CK_F32_F64, CK_F64_F32, CK_I32_F32, CK_U32_F32, CK_I32_F64, CK_U32_F64, CK_F32_I32,
  CK_F32_U32, CK_F64_I32, CK_F64_U32, CK_F32_UBYTE, CK_PKRTZ, CK_PKNORM_I16, CK_PKNORM_U16, CK_PK_U8, CK_RPI, CK_FLR,
  CK_OFF_I4, CK_F16_U16, CK_F16_I16, CK_U16_F16, CK_I16_F16,
  CK_PK_BF16_F32, CK_F32_BF16,
  CK_F32_FP8, CK_F32_BF8, CK_PK_F32_FP8, CK_PK_F32_BF8, CK_PK_FP8_F32, CK_PK_BF8_F32,
  CK_S_PK_FP8_F32, CK_S_PK_BF8_F32, CK_S_PK_F32_FP8, CK_S_PK_F32_BF8, CK_S_F32_FP8, CK_S_F32_BF8, CK_S_PK_FP4_F32,
  CK_S_PK_F32_FP4,
  CK_S_PK_FP8_F16, CK_S_PK_FP8_BF16, CK_S_PK_BF8_F16, CK_S_PK_BF8_BF16, CK_S_PK_F16_FP8, CK_S_PK_BF16_FP8, CK_S_PK_F16_BF8,
  CK_S_PK_BF16_BF8, CK_S_F16_FP8, CK_S_F16_BF8, CK_S_PK_FP4_F16, CK_S_PK_FP4_BF16, CK_S_PK_F16_FP4, CK_S_PK_BF16_FP4,
  // the wide forms: 32 values per lane (CvtWideArgs / CvtWideOut); six that narrow to 6 bits, then six that widen
  CK_W_2XPK16_FP6_F32, CK_W_2XPK16_BF6_F32, CK_W_PK32_FP6_F16, CK_W_PK32_FP6_BF16, CK_W_PK32_BF6_F16, CK_W_PK32_BF6_BF16,
  CK_W_PK32_F32_FP6, CK_W_PK32_F16_FP6, CK_W_PK32_BF16_FP6, CK_W_PK32_F32_BF6, CK_W_PK32_F16_BF6, CK_W_PK32_BF16_BF6,
};

// X(name, instruction, group, kind, select): the select is the byte (b0..b3, ubyte0..3) or word (lo = 0, hi = 1) of
// the source a widening op reads, or of the destination a narrowing op writes (the rest of it is kept);
// v_cvt_scalef32_f16_{fp8,bf8}: source byte | destination half << 2
#define CVT_OP_LIST(X)                                                            \
  X(f16_f32, "v_cvt_f16_f32", CG_CLASSIC, CK_F16_F32, 0)                         \
  X(f32_f16, "v_cvt_f32_f16", CG_CLASSIC, CK_F32_F16, 0)                         \
  X(f32_f64, "v_cvt_f32_f64", CG_CLASSIC, CK_F32_F64, 0)                         \
  X(f64_f32, "v_cvt_f64_f32", CG_CLASSIC, CK_F64_F32, 0)                         \
  X(i32_f32, "v_cvt_i32_f32", CG_CLASSIC, CK_I32_F32, 0)                         \
  X(u32_f32, "v_cvt_u32_f32", CG_CLASSIC, CK_U32_F32, 0)                         \
  X(i32_f64, "v_cvt_i32_f64", CG_CLASSIC, CK_I32_F64, 0)                         \
  X(u32_f64, "v_cvt_u32_f64", CG_CLASSIC, CK_U32_F64, 0)                         \
  X(f32_i32, "v_cvt_f32_i32", CG_CLASSIC, CK_F32_I32, 0)                         \
  X(f32_u32, "v_cvt_f32_u32", CG_CLASSIC, CK_F32_U32, 0)                         \
  X(f64_i32, "v_cvt_f64_i32", CG_CLASSIC, CK_F64_I32, 0)                         \
  X(f64_u32, "v_cvt_f64_u32", CG_CLASSIC, CK_F64_U32, 0)                         \
  X(f32_ubyte0, "v_cvt_f32_ubyte0", CG_CLASSIC, CK_F32_UBYTE, 0)                 \
  X(f32_ubyte1, "v_cvt_f32_ubyte1", CG_CLASSIC, CK_F32_UBYTE, 1)                 \
  X(f32_ubyte2, "v_cvt_f32_ubyte2", CG_CLASSIC, CK_F32_UBYTE, 2)                 \
  X(f32_ubyte3, "v_cvt_f32_ubyte3", CG_CLASSIC, CK_F32_UBYTE, 3)                 \
  X(pkrtz_f16_f32, "v_cvt_pkrtz_f16_f32", CG_CLASSIC, CK_PKRTZ, 0)               \
  X(pknorm_i16_f32, "v_cvt_pknorm_i16_f32", CG_CLASSIC, CK_PKNORM_I16, 0)        \
  X(pknorm_u16_f32, "v_cvt_pknorm_u16_f32", CG_CLASSIC, CK_PKNORM_U16, 0)        \
  X(pk_u8_f32, "v_cvt_pk_u8_f32", CG_CLASSIC, CK_PK_U8, 0)                       \
  X(rpi_i32_f32, "v_cvt_rpi_i32_f32", CG_CLASSIC, CK_RPI, 0)                     \
  X(flr_i32_f32, "v_cvt_flr_i32_f32", CG_CLASSIC, CK_FLR, 0)                     \
  X(off_f32_i4, "v_cvt_off_f32_i4", CG_CLASSIC, CK_OFF_I4, 0)                    \
  X(f16_u16, "v_cvt_f16_u16", CG_CLASSIC, CK_F16_U16, 0)                         \
  X(f16_i16, "v_cvt_f16_i16", CG_CLASSIC, CK_F16_I16, 0)                         \
  X(u16_f16, "v_cvt_u16_f16", CG_CLASSIC, CK_U16_F16, 0)                         \
  X(i16_f16, "v_cvt_i16_f16", CG_CLASSIC, CK_I16_F16, 0)                         \
  X(pk_bf16_f32, "v_cvt_pk_bf16_f32", CG_BF16, CK_PK_BF16_F32, 0)                \
  X(f32_bf16, "v_cvt_f32_bf16", CG_BF16, CK_F32_BF16, 0)                         \
  X(f32_fp8_b0, "v_cvt_f32_fp8", CG_FP8, CK_F32_FP8, 0)                          \
  X(f32_fp8_b1, "v_cvt_f32_fp8", CG_FP8, CK_F32_FP8, 1)                          \
  X(f32_fp8_b2, "v_cvt_f32_fp8", CG_FP8, CK_F32_FP8, 2)                          \
  X(f32_fp8_b3, "v_cvt_f32_fp8", CG_FP8, CK_F32_FP8, 3)                          \
  X(f32_bf8_b0, "v_cvt_f32_bf8", CG_FP8, CK_F32_BF8, 0)                          \
  X(f32_bf8_b1, "v_cvt_f32_bf8", CG_FP8, CK_F32_BF8, 1)                          \
  X(f32_bf8_b2, "v_cvt_f32_bf8", CG_FP8, CK_F32_BF8, 2)                          \
  X(f32_bf8_b3, "v_cvt_f32_bf8", CG_FP8, CK_F32_BF8, 3)                          \
  X(pk_f32_fp8_lo, "v_cvt_pk_f32_fp8", CG_FP8, CK_PK_F32_FP8, 0)                 \
  X(pk_f32_fp8_hi, "v_cvt_pk_f32_fp8", CG_FP8, CK_PK_F32_FP8, 1)                 \
  X(pk_f32_bf8_lo, "v_cvt_pk_f32_bf8", CG_FP8, CK_PK_F32_BF8, 0)                 \
  X(pk_f32_bf8_hi, "v_cvt_pk_f32_bf8", CG_FP8, CK_PK_F32_BF8, 1)                 \
  X(pk_fp8_f32_lo, "v_cvt_pk_fp8_f32", CG_FP8, CK_PK_FP8_F32, 0)                 \
  X(pk_fp8_f32_hi, "v_cvt_pk_fp8_f32", CG_FP8, CK_PK_FP8_F32, 1)                 \
  X(pk_bf8_f32_lo, "v_cvt_pk_bf8_f32", CG_FP8, CK_PK_BF8_F32, 0)                 \
  X(pk_bf8_f32_hi, "v_cvt_pk_bf8_f32", CG_FP8, CK_PK_BF8_F32, 1)                 \
  X(scalef32_pk_fp8_f32_lo, "v_cvt_scalef32_pk_fp8_f32", CG_SCALEF32, CK_S_PK_FP8_F32, 0) \
  X(scalef32_pk_fp8_f32_hi, "v_cvt_scalef32_pk_fp8_f32", CG_SCALEF32, CK_S_PK_FP8_F32, 1) \
  X(scalef32_pk_bf8_f32_lo, "v_cvt_scalef32_pk_bf8_f32", CG_SCALEF32, CK_S_PK_BF8_F32, 0) \
  X(scalef32_pk_bf8_f32_hi, "v_cvt_scalef32_pk_bf8_f32", CG_SCALEF32, CK_S_PK_BF8_F32, 1) \
  X(scalef32_pk_f32_fp8_lo, "v_cvt_scalef32_pk_f32_fp8", CG_SCALEF32, CK_S_PK_F32_FP8, 0) \
  X(scalef32_pk_f32_fp8_hi, "v_cvt_scalef32_pk_f32_fp8", CG_SCALEF32, CK_S_PK_F32_FP8, 1) \
  X(scalef32_pk_f32_bf8_lo, "v_cvt_scalef32_pk_f32_bf8", CG_SCALEF32, CK_S_PK_F32_BF8, 0) \
  X(scalef32_pk_f32_bf8_hi, "v_cvt_scalef32_pk_f32_bf8", CG_SCALEF32, CK_S_PK_F32_BF8, 1) \
  X(scalef32_f32_fp8_b0, "v_cvt_scalef32_f32_fp8", CG_SCALEF32, CK_S_F32_FP8, 0)  \
  X(scalef32_f32_fp8_b1, "v_cvt_scalef32_f32_fp8", CG_SCALEF32, CK_S_F32_FP8, 1)  \
  X(scalef32_f32_fp8_b2, "v_cvt_scalef32_f32_fp8", CG_SCALEF32, CK_S_F32_FP8, 2)  \
  X(scalef32_f32_fp8_b3, "v_cvt_scalef32_f32_fp8", CG_SCALEF32, CK_S_F32_FP8, 3)  \
  X(scalef32_f32_bf8_b0, "v_cvt_scalef32_f32_bf8", CG_SCALEF32, CK_S_F32_BF8, 0)  \
  X(scalef32_f32_bf8_b1, "v_cvt_scalef32_f32_bf8", CG_SCALEF32, CK_S_F32_BF8, 1)  \
  X(scalef32_f32_bf8_b2, "v_cvt_scalef32_f32_bf8", CG_SCALEF32, CK_S_F32_BF8, 2)  \
  X(scalef32_f32_bf8_b3, "v_cvt_scalef32_f32_bf8", CG_SCALEF32, CK_S_F32_BF8, 3)  \
  X(scalef32_pk_fp4_f32_b0, "v_cvt_scalef32_pk_fp4_f32", CG_SCALEF32, CK_S_PK_FP4_F32, 0) \
  X(scalef32_pk_fp4_f32_b1, "v_cvt_scalef32_pk_fp4_f32", CG_SCALEF32, CK_S_PK_FP4_F32, 1) \
  X(scalef32_pk_fp4_f32_b2, "v_cvt_scalef32_pk_fp4_f32", CG_SCALEF32, CK_S_PK_FP4_F32, 2) \
  X(scalef32_pk_fp4_f32_b3, "v_cvt_scalef32_pk_fp4_f32", CG_SCALEF32, CK_S_PK_FP4_F32, 3) \
  X(scalef32_pk_f32_fp4_b0, "v_cvt_scalef32_pk_f32_fp4", CG_SCALEF32, CK_S_PK_F32_FP4, 0) \
  X(scalef32_pk_f32_fp4_b1, "v_cvt_scalef32_pk_f32_fp4", CG_SCALEF32, CK_S_PK_F32_FP4, 1) \
  X(scalef32_pk_f32_fp4_b2, "v_cvt_scalef32_pk_f32_fp4", CG_SCALEF32, CK_S_PK_F32_FP4, 2) \
  X(scalef32_pk_f32_fp4_b3, "v_cvt_scalef32_pk_f32_fp4", CG_SCALEF32, CK_S_PK_F32_FP4, 3) \
  X(scalef32_pk_fp8_f16_lo, "v_cvt_scalef32_pk_fp8_f16", CG_SCALEF32, CK_S_PK_FP8_F16, 0) \
  X(scalef32_pk_fp8_f16_hi, "v_cvt_scalef32_pk_fp8_f16", CG_SCALEF32, CK_S_PK_FP8_F16, 1) \
  X(scalef32_pk_fp8_bf16_lo, "v_cvt_scalef32_pk_fp8_bf16", CG_SCALEF32, CK_S_PK_FP8_BF16, 0) \
  X(scalef32_pk_fp8_bf16_hi, "v_cvt_scalef32_pk_fp8_bf16", CG_SCALEF32, CK_S_PK_FP8_BF16, 1) \
  X(scalef32_pk_bf8_f16_lo, "v_cvt_scalef32_pk_bf8_f16", CG_SCALEF32, CK_S_PK_BF8_F16, 0) \
  X(scalef32_pk_bf8_f16_hi, "v_cvt_scalef32_pk_bf8_f16", CG_SCALEF32, CK_S_PK_BF8_F16, 1) \
  X(scalef32_pk_bf8_bf16_lo, "v_cvt_scalef32_pk_bf8_bf16", CG_SCALEF32, CK_S_PK_BF8_BF16, 0) \
  X(scalef32_pk_bf8_bf16_hi, "v_cvt_scalef32_pk_bf8_bf16", CG_SCALEF32, CK_S_PK_BF8_BF16, 1) \
  X(scalef32_pk_f16_fp8_lo, "v_cvt_scalef32_pk_f16_fp8", CG_SCALEF32, CK_S_PK_F16_FP8, 0) \
  X(scalef32_pk_f16_fp8_hi, "v_cvt_scalef32_pk_f16_fp8", CG_SCALEF32, CK_S_PK_F16_FP8, 1) \
  X(scalef32_pk_bf16_fp8_lo, "v_cvt_scalef32_pk_bf16_fp8", CG_SCALEF32, CK_S_PK_BF16_FP8, 0) \
  X(scalef32_pk_bf16_fp8_hi, "v_cvt_scalef32_pk_bf16_fp8", CG_SCALEF32, CK_S_PK_BF16_FP8, 1) \
  X(scalef32_pk_f16_bf8_lo, "v_cvt_scalef32_pk_f16_bf8", CG_SCALEF32, CK_S_PK_F16_BF8, 0) \
  X(scalef32_pk_f16_bf8_hi, "v_cvt_scalef32_pk_f16_bf8", CG_SCALEF32, CK_S_PK_F16_BF8, 1) \
  X(scalef32_pk_bf16_bf8_lo, "v_cvt_scalef32_pk_bf16_bf8", CG_SCALEF32, CK_S_PK_BF16_BF8, 0) \
  X(scalef32_pk_bf16_bf8_hi, "v_cvt_scalef32_pk_bf16_bf8", CG_SCALEF32, CK_S_PK_BF16_BF8, 1) \
  X(scalef32_f16_fp8_b0_lo, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 0) \
  X(scalef32_f16_fp8_b1_lo, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 1) \
  X(scalef32_f16_fp8_b2_lo, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 2) \
  X(scalef32_f16_fp8_b3_lo, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 3) \
  X(scalef32_f16_fp8_b0_hi, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 4) \
  X(scalef32_f16_fp8_b1_hi, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 5) \
  X(scalef32_f16_fp8_b2_hi, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 6) \
  X(scalef32_f16_fp8_b3_hi, "v_cvt_scalef32_f16_fp8", CG_SCALEF32, CK_S_F16_FP8, 7) \
  X(scalef32_f16_bf8_b0_lo, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 0) \
  X(scalef32_f16_bf8_b1_lo, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 1) \
  X(scalef32_f16_bf8_b2_lo, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 2) \
  X(scalef32_f16_bf8_b3_lo, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 3) \
  X(scalef32_f16_bf8_b0_hi, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 4) \
  X(scalef32_f16_bf8_b1_hi, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 5) \
  X(scalef32_f16_bf8_b2_hi, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 6) \
  X(scalef32_f16_bf8_b3_hi, "v_cvt_scalef32_f16_bf8", CG_SCALEF32, CK_S_F16_BF8, 7) \
  X(scalef32_pk_fp4_f16_b0, "v_cvt_scalef32_pk_fp4_f16", CG_SCALEF32, CK_S_PK_FP4_F16, 0) \
  X(scalef32_pk_fp4_f16_b1, "v_cvt_scalef32_pk_fp4_f16", CG_SCALEF32, CK_S_PK_FP4_F16, 1) \
  X(scalef32_pk_fp4_f16_b2, "v_cvt_scalef32_pk_fp4_f16", CG_SCALEF32, CK_S_PK_FP4_F16, 2) \
  X(scalef32_pk_fp4_f16_b3, "v_cvt_scalef32_pk_fp4_f16", CG_SCALEF32, CK_S_PK_FP4_F16, 3) \
  X(scalef32_pk_fp4_bf16_b0, "v_cvt_scalef32_pk_fp4_bf16", CG_SCALEF32, CK_S_PK_FP4_BF16, 0) \
  X(scalef32_pk_fp4_bf16_b1, "v_cvt_scalef32_pk_fp4_bf16", CG_SCALEF32, CK_S_PK_FP4_BF16, 1) \
  X(scalef32_pk_fp4_bf16_b2, "v_cvt_scalef32_pk_fp4_bf16", CG_SCALEF32, CK_S_PK_FP4_BF16, 2) \
  X(scalef32_pk_fp4_bf16_b3, "v_cvt_scalef32_pk_fp4_bf16", CG_SCALEF32, CK_S_PK_FP4_BF16, 3) \
  X(scalef32_pk_f16_fp4_b0, "v_cvt_scalef32_pk_f16_fp4", CG_SCALEF32, CK_S_PK_F16_FP4, 0) \
  X(scalef32_pk_f16_fp4_b1, "v_cvt_scalef32_pk_f16_fp4", CG_SCALEF32, CK_S_PK_F16_FP4, 1) \
  X(scalef32_pk_f16_fp4_b2, "v_cvt_scalef32_pk_f16_fp4", CG_SCALEF32, CK_S_PK_F16_FP4, 2) \
  X(scalef32_pk_f16_fp4_b3, "v_cvt_scalef32_pk_f16_fp4", CG_SCALEF32, CK_S_PK_F16_FP4, 3) \
  X(scalef32_pk_bf16_fp4_b0, "v_cvt_scalef32_pk_bf16_fp4", CG_SCALEF32, CK_S_PK_BF16_FP4, 0) \
  X(scalef32_pk_bf16_fp4_b1, "v_cvt_scalef32_pk_bf16_fp4", CG_SCALEF32, CK_S_PK_BF16_FP4, 1) \
  X(scalef32_pk_bf16_fp4_b2, "v_cvt_scalef32_pk_bf16_fp4", CG_SCALEF32, CK_S_PK_BF16_FP4, 2) \
  X(scalef32_pk_bf16_fp4_b3, "v_cvt_scalef32_pk_bf16_fp4", CG_SCALEF32, CK_S_PK_BF16_FP4, 3) \
  X(scalef32_2xpk16_fp6_f32, "v_cvt_scalef32_2xpk16_fp6_f32", CG_SCALEF32, CK_W_2XPK16_FP6_F32, 0) \
  X(scalef32_2xpk16_bf6_f32, "v_cvt_scalef32_2xpk16_bf6_f32", CG_SCALEF32, CK_W_2XPK16_BF6_F32, 0) \
  X(scalef32_pk32_fp6_f16, "v_cvt_scalef32_pk32_fp6_f16", CG_SCALEF32, CK_W_PK32_FP6_F16, 0) \
  X(scalef32_pk32_fp6_bf16, "v_cvt_scalef32_pk32_fp6_bf16", CG_SCALEF32, CK_W_PK32_FP6_BF16, 0) \
  X(scalef32_pk32_bf6_f16, "v_cvt_scalef32_pk32_bf6_f16", CG_SCALEF32, CK_W_PK32_BF6_F16, 0) \
  X(scalef32_pk32_bf6_bf16, "v_cvt_scalef32_pk32_bf6_bf16", CG_SCALEF32, CK_W_PK32_BF6_BF16, 0) \
  X(scalef32_pk32_f32_fp6, "v_cvt_scalef32_pk32_f32_fp6", CG_SCALEF32, CK_W_PK32_F32_FP6, 0) \
  X(scalef32_pk32_f16_fp6, "v_cvt_scalef32_pk32_f16_fp6", CG_SCALEF32, CK_W_PK32_F16_FP6, 0) \
  X(scalef32_pk32_bf16_fp6, "v_cvt_scalef32_pk32_bf16_fp6", CG_SCALEF32, CK_W_PK32_BF16_FP6, 0) \
  X(scalef32_pk32_f32_bf6, "v_cvt_scalef32_pk32_f32_bf6", CG_SCALEF32, CK_W_PK32_F32_BF6, 0) \
  X(scalef32_pk32_f16_bf6, "v_cvt_scalef32_pk32_f16_bf6", CG_SCALEF32, CK_W_PK32_F16_BF6, 0) \
  X(scalef32_pk32_bf16_bf6, "v_cvt_scalef32_pk32_bf16_bf6", CG_SCALEF32, CK_W_PK32_BF16_BF6, 0)

#define CVT_X_ENUM(NAME, INSN, GROUP, KIND, SEL) CO_##NAME,
enum CvtOp { CVT_OP_LIST(CVT_X_ENUM) CVT_OPS };
#undef CVT_X_ENUM

struct CvtOpInfo {
  const char* name;
  const char* insn;
  int group, kind, sel;
};
#define CVT_X_ROW(NAME, INSN, GROUP, KIND, SEL) {#NAME, INSN, GROUP, KIND, SEL},
// name, instruction, group, kind and select of op k (the index is the enum's)
inline constexpr CvtOpInfo CVT_OP_TABLE[CVT_OPS] = {CVT_OP_LIST(CVT_X_ROW)};
#undef CVT_X_ROW
// kind and select again, as functions: what the kernels can ask
#define CVT_X_KIND(NAME, INSN, GROUP, KIND, SEL) case CO_##NAME: return KIND;
#define CVT_X_SEL(NAME, INSN, GROUP, KIND, SEL) case CO_##NAME: return SEL;
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CVT_HDC __host__ __device__ constexpr
#else
#define CVT_HDC constexpr
#endif
CVT_HDC int cvt_kind(int op) {
  switch (op) {
    CVT_OP_LIST(CVT_X_KIND)
    default: return -1;
  }
}
CVT_HDC int cvt_sel(int op) {
  switch (op) {
    CVT_OP_LIST(CVT_X_SEL)
    default: return 0;
  }
}
#undef CVT_X_KIND
#undef CVT_X_SEL
// The wide forms convert 32 values per lane: their operands and results are CvtWideArgs / CvtWideOut.
CVT_HDC bool cvt_is_wide(int op) { return cvt_kind(op) >= CK_W_2XPK16_FP6_F32; }
CVT_HDC bool cvt_wide_narrows(int kind) { return kind < CK_W_PK32_F32_FP6; }  // to fp6 / bf6; else from them
CVT_HDC bool cvt_wide_is_fp6(int kind) {
  return kind == CK_W_2XPK16_FP6_F32 || kind == CK_W_PK32_FP6_F16 || kind == CK_W_PK32_FP6_BF16 ||
         (kind >= CK_W_PK32_F32_FP6 && kind <= CK_W_PK32_BF16_FP6);
}
CVT_HDC int cvt_wide_big(int kind) {  // the other format: 0 fp32, 1 f16, 2 bf16
  if (kind <= CK_W_2XPK16_BF6_F32) return 0;
  if (kind < CK_W_PK32_F32_FP6) return kind == CK_W_PK32_FP6_F16 || kind == CK_W_PK32_BF6_F16 ? 1 : 2;
  return (kind - CK_W_PK32_F32_FP6) % 3;
}

// the operands of one application: a, b the sources (a 64-bit source: a low, b high), c the destination before the
// instruction (a narrowing op that keeps part of it) or the byte select of v_cvt_pk_u8_f32's third operand, s the
// scale (fp32 bits).  An op reads only what its instruction reads.
struct CvtArgs {
  uint32_t a, b, c, s;
};
// the result registers: r[1] is 0 for an op that writes one.  A 16-bit result is r[0]'s low half alone (the upper
// half of the register is not compared)
struct CvtOut {
  uint32_t r[2];
};
// ... and of a wide form.  32 fp32 values are v[0..31] (v_cvt_scalef32_2xpk16: the first source register block is
// v[0..15], the second v[16..31]; the instruction interleaves them: code 2 i stems from v[i], code 2 i + 1 from v[16 + i]); 32 f16 / bf16 values are v[0..15], value j in half j % 2 of v[j / 2]; 32 fp6 / bf6
// codes are v[0..5], code j in bits 6 j .. 6 j + 5 of the 192.  Results likewise in r; the words an op does not write
// are 0.  s: the scale.
constexpr int CVT_WIDE = 32, CVT_WIDE_IN = 33, CVT_WIDE_OUT = 32;
struct CvtWideArgs {
  uint32_t v[CVT_WIDE];
  uint32_t s;
};
struct CvtWideOut {
  uint32_t r[CVT_WIDE];
};

// The 64 -> 32 bit hash of the chains: the project's mix32 (common/hip_host.h; murmur3's finalizer), for both compilers
CVT_HD uint32_t cvt_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}
CVT_HD uint32_t cvt_init(uint64_t seed, int lane, int chain) {
  return cvt_mix32(seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(lane * CVT_CHAINS + chain + 1));
}
CVT_HD uint32_t cvt_const(uint64_t seed, int lane, int chain) {
  return cvt_mix32(seed + 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(lane * CVT_CHAINS + chain + 1));
}
CVT_HD uint64_t cvt_op_seed(uint64_t seed, int op) { return seed + 0x632BE59BD9B4E019ULL * static_cast<uint64_t>(op + 1); }
// the n-th further word drawn from chain word w (the second source, the kept destination, the scale)
CVT_HD uint32_t cvt_hash(uint32_t w, uint32_t n) { return cvt_mix32((static_cast<uint64_t>(n + 1) << 32) | w); }
CVT_HD uint32_t cvt_fold(const CvtOut& o) { return o.r[0] + ((o.r[1] << 16) | (o.r[1] >> 16)); }
// every result word of a wide form
CVT_HD uint32_t cvt_fold_wide(const CvtWideOut& o) {
  uint32_t f = 0;
  for (int j = 0; j < CVT_WIDE; ++j) f += j ? (o.r[j] << j) | (o.r[j] >> (32 - j)) : o.r[j];
  return f;
}
CVT_HD uint32_t cvt_step(uint32_t own, uint32_t folded, uint32_t c) {
  return cvt_mix32(((static_cast<uint64_t>(own) << 32) | folded) + c);
}

// --- formats ------------------------------------------------------------------------------------------------------
// sign | ebits of exponent | mbits of significand.  kind 0: IEEE (the top exponent is Inf / NaN); 1: OCP E4M3 (only
// S.1111.111 is a NaN, no Inf); 2: every code is a finite number (fp4)
struct CvtFmt {
  int ebits, mbits, bias, kind;
};
constexpr CvtFmt CVT_F64 = {11, 52, 1023, 0}, CVT_F32 = {8, 23, 127, 0}, CVT_F16 = {5, 10, 15, 0}, CVT_BF16 = {8, 7, 127, 0},
                 CVT_BF8 = {5, 2, 15, 0}, CVT_FP8 = {4, 3, 7, 1}, CVT_FP4 = {2, 1, 1, 2}, CVT_FP6 = {2, 3, 1, 2},
                 CVT_BF6 = {3, 2, 3, 2};
enum CvtRound { CVT_RNE = 0, CVT_RTZ, CVT_FLOOR, CVT_RPI };

CVT_HD int cvt_bits(const CvtFmt f) { return 1 + f.ebits + f.mbits; }
CVT_HD uint64_t cvt_sign_bit(const CvtFmt f) { return 1ULL << (f.ebits + f.mbits); }
// the largest finite magnitude code
CVT_HD uint64_t cvt_max_code(const CvtFmt f) {
  const uint64_t emask = (1ULL << f.ebits) - 1, mmask = (1ULL << f.mbits) - 1;
  if (f.kind == 0) return ((emask - 1) << f.mbits) | mmask;
  if (f.kind == 1) return (emask << f.mbits) | (mmask - 1);
  return (emask << f.mbits) | mmask;
}
CVT_HD bool cvt_finite(const CvtFmt f, uint64_t code) { return (code & (cvt_sign_bit(f) - 1)) <= cvt_max_code(f); }

// an exact finite value: (-1)^neg * m * 2^e; m == 0 is zero (with its sign)
struct CvtVal {
  bool neg;
  uint64_t m;
  int e;
};
CVT_HD int cvt_top_bit(uint64_t m) {  // the index of m's highest set bit; m != 0
  return 63 - __builtin_clzll(m);
}

// Decode: exponent field E == 0 is a subnormal, M * 2^(1 - bias - mbits); else (2^mbits + M) * 2^(E - bias - mbits).
// false for a code that is no finite number.
CVT_HD bool cvt_decode(const CvtFmt f, uint64_t code, CvtVal* v) {
  if (!cvt_finite(f, code)) return false;
  const uint64_t E = (code >> f.mbits) & ((1ULL << f.ebits) - 1), M = code & ((1ULL << f.mbits) - 1);
  v->neg = (code & cvt_sign_bit(f)) != 0;
  v->m = E ? (M | (1ULL << f.mbits)) : M;
  v->e = static_cast<int>(E ? E : 1) - f.bias - f.mbits;
  return true;
}

// Encode under `mode` (CVT_RNE: to nearest, ties to the even significand; CVT_RTZ: towards zero): the value's binade
// gives the exponent of one unit in the last place, q = max(binade, 1 - bias) - mbits (the subnormals share the
// smallest normal's); the significand is m * 2^(e - q) rounded to an integer; a carry out of the significand moves to
// the next binade.  false when the rounded value lies beyond the largest finite number (the code is not written).
CVT_HD bool cvt_encode(const CvtFmt f, const CvtVal& v, CvtRound mode, uint64_t* code) {
  const uint64_t sign = v.neg ? cvt_sign_bit(f) : 0;
  if (v.m == 0) {
    *code = sign;
    return true;
  }
  const int binade = cvt_top_bit(v.m) + v.e, emin = 1 - f.bias;
  int q = (binade > emin ? binade : emin) - f.mbits;
  const int s = q - v.e;  // bits of m below one unit in the last place
  uint64_t sig;
  if (s <= 0) {
    sig = v.m << -s;
  } else if (s >= 64) {
    sig = 0;  // below half of the smallest subnormal (m has at most 63 bits here): rounds to zero either way
  } else {
    sig = v.m >> s;
    const uint64_t rem = v.m & ((1ULL << s) - 1), half = 1ULL << (s - 1);
    if (mode == CVT_RNE && (rem > half || (rem == half && (sig & 1)))) ++sig;
  }
  if (sig >> (f.mbits + 1)) sig >>= 1, ++q;  // the carry: sig was 2^(mbits + 1) exactly
  uint64_t mag;
  if (sig >> f.mbits) mag = (static_cast<uint64_t>(q + f.mbits + f.bias) << f.mbits) | (sig & ((1ULL << f.mbits) - 1));
  else mag = sig;  // a subnormal, or zero
  if (mag > cvt_max_code(f)) return false;
  *code = sign | mag;
  return true;
}

// Float to integer under `mode` (CVT_RTZ: truncate; CVT_FLOOR; CVT_RNE; CVT_RPI: floor(x + 0.5)), clamped to lo..hi
CVT_HD int64_t cvt_to_int(const CvtVal& v, CvtRound mode, int64_t lo, int64_t hi) {
  if (v.m == 0) return 0 < lo ? lo : 0;
  uint64_t ip;  // the integer part of the magnitude
  int frac = 0;  // of the rest: 0 none, 1 below a half, 2 a half, 3 above a half
  if (v.e >= 0) {
    if (cvt_top_bit(v.m) + v.e >= 62) return v.neg ? lo : hi;
    ip = v.m << v.e;
  } else if (-v.e >= 64) {
    ip = 0, frac = 1;
  } else {
    const int s = -v.e;
    const uint64_t rem = v.m & ((1ULL << s) - 1), half = 1ULL << (s - 1);
    ip = v.m >> s;
    frac = rem == 0 ? 0 : rem < half ? 1 : rem == half ? 2 : 3;
  }
  if (ip >> 62) return v.neg ? lo : hi;
  uint64_t mag = ip;
  if (mode == CVT_FLOOR) mag += v.neg && frac ? 1 : 0;
  else if (mode == CVT_RNE) mag += frac == 3 || (frac == 2 && (ip & 1)) ? 1 : 0;
  else if (mode == CVT_RPI) mag += v.neg ? (frac == 3 ? 1 : 0) : (frac >= 2 ? 1 : 0);
  const int64_t r = v.neg ? -static_cast<int64_t>(mag) : static_cast<int64_t>(mag);
  return r < lo ? lo : r > hi ? hi : r;
}

// the scale operand: 2^k with k in -8..8, sign and mantissa clear; false otherwise
CVT_HD bool cvt_scale_exp(uint32_t s, int* k) {
  const int E = static_cast<int>((s >> 23) & 0xffu);
  *k = E - 127;
  return !(s >> 31) && !(s & 0x7fffffu) && *k >= -8 && *k <= 8;
}
CVT_HD uint32_t cvt_scale_of(uint32_t h) { return static_cast<uint32_t>(127 - 8 + static_cast<int>(h % 17u)) << 23; }

// --- the model ----------------------------------------------------------------------------------------------------
// src (format S) / 2^k -> format D under `mode`
CVT_HD bool cvt_float(const CvtFmt S, uint64_t src, int k, const CvtFmt D, CvtRound mode, uint64_t* dst) {
  CvtVal v;
  if (!cvt_decode(S, src, &v)) return false;
  v.e -= k;
  return cvt_encode(D, v, mode, dst);
}
CVT_HD bool cvt_from_int(int64_t i, const CvtFmt D, uint64_t* dst) {
  const CvtVal v = {i < 0, i < 0 ? static_cast<uint64_t>(-i) : static_cast<uint64_t>(i), 0};
  return cvt_encode(D, v, CVT_RNE, dst);
}
CVT_HD bool cvt_float_to_int(const CvtFmt S, uint64_t src, CvtRound mode, int64_t lo, int64_t hi, int64_t* dst) {
  CvtVal v;
  if (!cvt_decode(S, src, &v)) return false;
  *dst = cvt_to_int(v, mode, lo, hi);
  return true;
}
// the significant bits of m: from its highest to its lowest set bit
CVT_HD int cvt_sig_bits(uint64_t m) {
  if (!m) return 0;
  while (!(m & 1)) m >>= 1;
  return cvt_top_bit(m) + 1;
}
// x -> round_to_nearest_even(clamp(x, lo1, 1) * unit): the pknorm ops
CVT_HD bool cvt_norm(uint32_t src, bool is_signed, uint32_t* dst) {
  CvtVal v;
  if (!cvt_decode(CVT_F32, src, &v)) return false;
  const int64_t unit = is_signed ? 32767 : 65535;
  int64_t r;
  if (v.m && cvt_top_bit(v.m) + v.e >= 0) {
    r = v.neg ? (is_signed ? -unit : 0) : unit;  // |x| >= 1: the clamp
  } else {
    if (cvt_sig_bits(v.m) > 9) return false;  // the product must be exact in fp32 (the head comment)
    v.m *= static_cast<uint64_t>(unit);
    r = cvt_to_int(v, CVT_RNE, is_signed ? -unit : 0, unit);
  }
  *dst = static_cast<uint32_t>(r) & 0xffffu;
  return true;
}

// One application of op `op` on `in`: what the instruction must leave in its destination.  false (and *out
// untouched) when the operands lie outside the domain of the head comment.
CVT_HD bool cvt_convert(int op, const CvtArgs& in, CvtOut* out) {
  if (op < 0 || op >= CVT_OPS) return false;
  const int kind = cvt_kind(op), sel = cvt_sel(op);
  const uint64_t a64 = (static_cast<uint64_t>(in.b) << 32) | in.a;
  uint64_t d = 0, d2 = 0;
  int64_t i = 0;
  int k = 0;
  uint32_t r0 = 0, r1 = 0;
  const bool fp8_kind = kind == CK_F32_FP8 || kind == CK_PK_F32_FP8 || kind == CK_PK_FP8_F32 || kind == CK_S_PK_FP8_F32 ||
                        kind == CK_S_PK_F32_FP8 || kind == CK_S_F32_FP8 || kind == CK_S_PK_FP8_F16 || kind == CK_S_PK_FP8_BF16 ||
                        kind == CK_S_PK_F16_FP8 || kind == CK_S_PK_BF16_FP8 || kind == CK_S_F16_FP8;
  const CvtFmt f8 = fp8_kind ? CVT_FP8 : CVT_BF8;
  const bool bf16_kind = kind == CK_S_PK_FP8_BF16 || kind == CK_S_PK_BF8_BF16 || kind == CK_S_PK_BF16_FP8 ||
                         kind == CK_S_PK_BF16_BF8 || kind == CK_S_PK_FP4_BF16 || kind == CK_S_PK_BF16_FP4;
  const CvtFmt h16 = bf16_kind ? CVT_BF16 : CVT_F16;  // the 16-bit format of the scalef32 forms that have one
  switch (kind) {
    case CK_F16_F32:
      if (!cvt_float(CVT_F32, in.a, 0, CVT_F16, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_F32_F16:
      if (!cvt_float(CVT_F16, in.a & 0xffffu, 0, CVT_F32, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_F32_F64:
      if (!cvt_float(CVT_F64, a64, 0, CVT_F32, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_F64_F32:
      if (!cvt_float(CVT_F32, in.a, 0, CVT_F64, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d), r1 = static_cast<uint32_t>(d >> 32);
      break;
    case CK_I32_F32:
    case CK_I32_F64:
      if (!cvt_float_to_int(kind == CK_I32_F32 ? CVT_F32 : CVT_F64, kind == CK_I32_F32 ? in.a : a64, CVT_RTZ, INT32_MIN,
                            INT32_MAX, &i))
        return false;
      r0 = static_cast<uint32_t>(i);
      break;
    case CK_U32_F32:
    case CK_U32_F64:
      if (!cvt_float_to_int(kind == CK_U32_F32 ? CVT_F32 : CVT_F64, kind == CK_U32_F32 ? in.a : a64, CVT_RTZ, 0, UINT32_MAX, &i))
        return false;
      r0 = static_cast<uint32_t>(i);
      break;
    case CK_F32_I32:
    case CK_F32_U32:
      if (!cvt_from_int(kind == CK_F32_I32 ? static_cast<int64_t>(static_cast<int32_t>(in.a)) : static_cast<int64_t>(in.a),
                        CVT_F32, &d))
        return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_F64_I32:
    case CK_F64_U32:
      if (!cvt_from_int(kind == CK_F64_I32 ? static_cast<int64_t>(static_cast<int32_t>(in.a)) : static_cast<int64_t>(in.a),
                        CVT_F64, &d))
        return false;
      r0 = static_cast<uint32_t>(d), r1 = static_cast<uint32_t>(d >> 32);
      break;
    case CK_F32_UBYTE:
      if (!cvt_from_int((in.a >> (8 * sel)) & 0xffu, CVT_F32, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_PKRTZ:
      if (!cvt_float(CVT_F32, in.a, 0, CVT_F16, CVT_RTZ, &d) || !cvt_float(CVT_F32, in.b, 0, CVT_F16, CVT_RTZ, &d2)) return false;
      r0 = static_cast<uint32_t>(d | (d2 << 16));
      break;
    case CK_PKNORM_I16:
    case CK_PKNORM_U16: {
      uint32_t lo, hi;
      if (!cvt_norm(in.a, kind == CK_PKNORM_I16, &lo) || !cvt_norm(in.b, kind == CK_PKNORM_I16, &hi)) return false;
      r0 = lo | (hi << 16);
      break;
    }
    case CK_PK_U8: {  // byte (b & 3) of c replaced by the source rounded to the nearest integer, ties to even (under the wave's rounding
      // mode, unlike v_cvt_u32_f32, which truncates); the other three kept
      CvtVal v;
      if (!cvt_decode(CVT_F32, in.a, &v) || (v.neg && v.m)) return false;
      i = cvt_to_int(v, CVT_RNE, 0, 1 << 20);
      if (i > 255) return false;
      const int sh = 8 * static_cast<int>(in.b & 3u);
      r0 = (in.c & ~(0xffu << sh)) | (static_cast<uint32_t>(i) << sh);
      break;
    }
    case CK_RPI: {  // floor(x + 0.5), for x whose x + 0.5 is exact in fp32
      CvtVal v;
      if (!cvt_decode(CVT_F32, in.a, &v)) return false;
      if (v.m) {
        if (v.e >= 0 ? cvt_top_bit(v.m) + v.e >= 23 : -v.e > 40) return false;
        if (v.e < 0) {
          const int64_t n = (v.neg ? -static_cast<int64_t>(v.m) : static_cast<int64_t>(v.m)) + (1LL << (-v.e - 1));
          if (cvt_sig_bits(static_cast<uint64_t>(n < 0 ? -n : n)) > 24) return false;
        }
      }
      r0 = static_cast<uint32_t>(cvt_to_int(v, CVT_RPI, INT32_MIN, INT32_MAX));
      break;
    }
    case CK_FLR:
      if (!cvt_float_to_int(CVT_F32, in.a, CVT_FLOOR, INT32_MIN, INT32_MAX, &i)) return false;
      r0 = static_cast<uint32_t>(i);
      break;
    case CK_OFF_I4: {  // the low four bits as a signed integer, over 16
      const int n = static_cast<int>(in.a & 0xfu);
      const CvtVal v = {n >= 8, static_cast<uint64_t>(n >= 8 ? 16 - n : n), -4};
      if (!cvt_encode(CVT_F32, v, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    }
    case CK_F16_U16:
    case CK_F16_I16:
      if (!cvt_from_int(kind == CK_F16_U16 ? static_cast<int64_t>(in.a & 0xffffu)
                                           : static_cast<int64_t>(static_cast<int16_t>(in.a & 0xffffu)),
                        CVT_F16, &d))
        return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_U16_F16:
    case CK_I16_F16:
      if (!cvt_float_to_int(CVT_F16, in.a & 0xffffu, CVT_RTZ, kind == CK_U16_F16 ? 0 : -32768, kind == CK_U16_F16 ? 65535 : 32767,
                            &i))
        return false;
      r0 = static_cast<uint32_t>(i) & 0xffffu;
      break;
    case CK_PK_BF16_F32:
      if (!cvt_float(CVT_F32, in.a, 0, CVT_BF16, CVT_RNE, &d) || !cvt_float(CVT_F32, in.b, 0, CVT_BF16, CVT_RNE, &d2)) return false;
      r0 = static_cast<uint32_t>(d | (d2 << 16));
      break;
    case CK_F32_BF16:
      if (!cvt_float(CVT_BF16, in.a & 0xffffu, 0, CVT_F32, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_S_F32_FP8:
    case CK_S_F32_BF8:
      if (!cvt_scale_exp(in.s, &k)) return false;
      [[fallthrough]];
    case CK_F32_FP8:
    case CK_F32_BF8:  // a widening op multiplies by the scale
      if (!cvt_float(f8, (in.a >> (8 * sel)) & 0xffu, -k, CVT_F32, CVT_RNE, &d)) return false;
      r0 = static_cast<uint32_t>(d);
      break;
    case CK_S_PK_F32_FP8:
    case CK_S_PK_F32_BF8:
      if (!cvt_scale_exp(in.s, &k)) return false;
      [[fallthrough]];
    case CK_PK_F32_FP8:
    case CK_PK_F32_BF8: {  // the word's low byte is the first result
      const uint32_t w = (in.a >> (16 * sel)) & 0xffffu;
      if (!cvt_float(f8, w & 0xffu, -k, CVT_F32, CVT_RNE, &d) || !cvt_float(f8, w >> 8, -k, CVT_F32, CVT_RNE, &d2)) return false;
      r0 = static_cast<uint32_t>(d), r1 = static_cast<uint32_t>(d2);
      break;
    }
    case CK_S_PK_FP8_F32:
    case CK_S_PK_BF8_F32:
      if (!cvt_scale_exp(in.s, &k)) return false;
      [[fallthrough]];
    case CK_PK_FP8_F32:
    case CK_PK_BF8_F32: {  // a narrowing op divides by the scale; a into the word's low byte; the other word of c kept
      if (!cvt_float(CVT_F32, in.a, k, f8, CVT_RNE, &d) || !cvt_float(CVT_F32, in.b, k, f8, CVT_RNE, &d2)) return false;
      const uint32_t w = static_cast<uint32_t>(d | (d2 << 8));
      r0 = sel ? (in.c & 0xffffu) | (w << 16) : (in.c & 0xffff0000u) | w;
      break;
    }
    case CK_S_PK_FP4_F32: {  // a into the low nibble of byte `sel` of c, b into the high one; the other bytes kept
      if (!cvt_scale_exp(in.s, &k)) return false;
      if (!cvt_float(CVT_F32, in.a, k, CVT_FP4, CVT_RNE, &d) || !cvt_float(CVT_F32, in.b, k, CVT_FP4, CVT_RNE, &d2)) return false;
      r0 = (in.c & ~(0xffu << (8 * sel))) | (static_cast<uint32_t>(d | (d2 << 4)) << (8 * sel));
      break;
    }
    case CK_S_PK_F32_FP4: {
      if (!cvt_scale_exp(in.s, &k)) return false;
      const uint32_t w = (in.a >> (8 * sel)) & 0xffu;
      if (!cvt_float(CVT_FP4, w & 0xfu, -k, CVT_F32, CVT_RNE, &d) || !cvt_float(CVT_FP4, w >> 4, -k, CVT_F32, CVT_RNE, &d2))
        return false;
      r0 = static_cast<uint32_t>(d), r1 = static_cast<uint32_t>(d2);
      break;
    }
    case CK_S_PK_FP8_F16: case CK_S_PK_FP8_BF16: case CK_S_PK_BF8_F16: case CK_S_PK_BF8_BF16: {
      // the two halves of a, divided by the scale, into word `sel` of c (a's low half into the word's low byte)
      if (!cvt_scale_exp(in.s, &k)) return false;
      if (!cvt_float(h16, in.a & 0xffffu, k, f8, CVT_RNE, &d) || !cvt_float(h16, in.a >> 16, k, f8, CVT_RNE, &d2)) return false;
      const uint32_t w = static_cast<uint32_t>(d | (d2 << 8));
      r0 = sel ? (in.c & 0xffffu) | (w << 16) : (in.c & 0xffff0000u) | w;
      break;
    }
    case CK_S_PK_F16_FP8: case CK_S_PK_BF16_FP8: case CK_S_PK_F16_BF8: case CK_S_PK_BF16_BF8: {
      // the two bytes of word `sel` of a, times the scale, into the two halves of the result
      if (!cvt_scale_exp(in.s, &k)) return false;
      const uint32_t w = (in.a >> (16 * sel)) & 0xffffu;
      if (!cvt_float(f8, w & 0xffu, -k, h16, CVT_RNE, &d) || !cvt_float(f8, w >> 8, -k, h16, CVT_RNE, &d2)) return false;
      r0 = static_cast<uint32_t>(d | (d2 << 16));
      break;
    }
    case CK_S_F16_FP8: case CK_S_F16_BF8: {  // byte (sel & 3) of a, times the scale, into half (sel >> 2) of c; the other kept
      if (!cvt_scale_exp(in.s, &k)) return false;
      if (!cvt_float(f8, (in.a >> (8 * (sel & 3))) & 0xffu, -k, CVT_F16, CVT_RNE, &d)) return false;
      r0 = (sel >> 2) ? (in.c & 0xffffu) | (static_cast<uint32_t>(d) << 16) : (in.c & 0xffff0000u) | static_cast<uint32_t>(d);
      break;
    }
    case CK_S_PK_FP4_F16: case CK_S_PK_FP4_BF16: {
      if (!cvt_scale_exp(in.s, &k)) return false;
      if (!cvt_float(h16, in.a & 0xffffu, k, CVT_FP4, CVT_RNE, &d) || !cvt_float(h16, in.a >> 16, k, CVT_FP4, CVT_RNE, &d2)) return false;
      r0 = (in.c & ~(0xffu << (8 * sel))) | (static_cast<uint32_t>(d | (d2 << 4)) << (8 * sel));
      break;
    }
    case CK_S_PK_F16_FP4: case CK_S_PK_BF16_FP4: {
      if (!cvt_scale_exp(in.s, &k)) return false;
      const uint32_t w = (in.a >> (8 * sel)) & 0xffu;
      if (!cvt_float(CVT_FP4, w & 0xfu, -k, h16, CVT_RNE, &d) || !cvt_float(CVT_FP4, w >> 4, -k, h16, CVT_RNE, &d2)) return false;
      r0 = static_cast<uint32_t>(d | (d2 << 16));
      break;
    }
    default:
      return false;
  }
  out->r[0] = r0, out->r[1] = r1;
  return true;
}
// code j of 32 packed 6-bit codes
CVT_HD uint32_t cvt_get6(const uint32_t* w, int j) {
  const int bit = 6 * j, word = bit >> 5, sh = bit & 31;
  uint32_t v = w[word] >> sh;
  if (sh > 26) v |= w[word + 1] << (32 - sh);
  return v & 63u;
}
CVT_HD void cvt_put6(uint32_t* w, int j, uint32_t code) {
  const int bit = 6 * j, word = bit >> 5, sh = bit & 31;
  w[word] |= code << sh;
  if (sh > 26) w[word + 1] |= code >> (32 - sh);
}
CVT_HD CvtFmt cvt_wide_small_fmt(int kind) { return cvt_wide_is_fp6(kind) ? CVT_FP6 : CVT_BF6; }
CVT_HD CvtFmt cvt_wide_big_fmt(int kind) { return cvt_wide_big(kind) == 0 ? CVT_F32 : cvt_wide_big(kind) == 1 ? CVT_F16 : CVT_BF16; }

// One application of a wide form: 32 values divided by the scale and rounded to 6 bits, or 32 codes times the scale.
// fp6 is E2M3 (bias 1, largest 7.5), bf6 E3M2 (bias 3, largest 28); neither has an Inf or a NaN.
CVT_HD bool cvt_convert_wide(int op, const CvtWideArgs& in, CvtWideOut* out) {
  if (op < 0 || op >= CVT_OPS || !cvt_is_wide(op)) return false;
  const int kind = cvt_kind(op), big = cvt_wide_big(kind);
  const CvtFmt S6 = cvt_wide_small_fmt(kind), B = cvt_wide_big_fmt(kind);
  int k = 0;
  if (!cvt_scale_exp(in.s, &k)) return false;
  CvtWideOut o;
  for (int j = 0; j < CVT_WIDE; ++j) o.r[j] = 0;
  for (int j = 0; j < CVT_WIDE; ++j) {
    uint64_t d = 0;
    if (cvt_wide_narrows(kind)) {
      // 2xpk16 interleaves its two source blocks: code 2 i is value i of the first, code 2 i + 1 value i of the second
      const uint32_t src = big == 0 ? in.v[16 * (j & 1) + j / 2] : (in.v[j / 2] >> (16 * (j & 1))) & 0xffffu;
      if (!cvt_float(B, src, k, S6, CVT_RNE, &d)) return false;
      cvt_put6(o.r, j, static_cast<uint32_t>(d));
    } else {
      if (!cvt_float(S6, cvt_get6(in.v, j), -k, B, CVT_RNE, &d)) return false;
      if (big == 0) o.r[j] = static_cast<uint32_t>(d);
      else o.r[j / 2] |= static_cast<uint32_t>(d) << (16 * (j & 1));
    }
  }
  *out = o;
  return true;
}
CVT_HD bool cvt_in_domain_wide(int op, const CvtWideArgs& in) {
  CvtWideOut o;
  return cvt_convert_wide(op, in, &o);
}
CVT_HD bool cvt_in_domain(int op, const CvtArgs& in) {
  CvtOut o;
  return cvt_convert(op, in, &o);
}

// --- the shapes -----------------------------------------------------------------------------------------------------
// the code of format S nearest below (-1)^neg * m * 2^e (the shapes build exact values; a value that S cannot hold is
// cut, one beyond its range becomes its largest finite number)
CVT_HD uint64_t cvt_make(const CvtFmt S, bool neg, uint64_t m, int e) {
  const CvtVal v = {neg, m, e};
  uint64_t code = 0;
  if (!cvt_encode(S, v, CVT_RTZ, &code)) code = (neg ? cvt_sign_bit(S) : 0) | cvt_max_code(S);
  return code;
}

// A source of format S whose quotient by 2^k is steered across the grid of D.  With c a magnitude code of D and f an
// 8-bit fraction of c's unit in the last place, the source is (c + f / 256) * 2^k, moved by `tweak` units of S:
//   0: a tie (f = 1/2): to the even c, or up to the even c + 1     1, 2: one unit of S above / below a tie
//   3: the largest finite number, or just below the half unit above it     4: D's subnormals
//   5: +-0, less than half the smallest subnormal, the smallest subnormal, the smallest normal     6, 7: anywhere
CVT_HD uint64_t cvt_shape_narrow(uint32_t w, const CvtFmt S, const CvtFmt D, int k) {
  const uint64_t maxc = cvt_max_code(D);
  const bool neg = (w >> 31) != 0;
  const uint32_t cat = w & 7u, h = w >> 3;
  uint64_t c = cvt_hash(w, 7) % (maxc + 1);
  uint32_t frac = h & 0xffu;
  int tweak = 0;
  switch (cat) {
    case 0: case 1: case 2:
      c %= maxc;
      frac = 0x80u;
      tweak = cat == 1 ? 1 : cat == 2 ? -1 : 0;
      break;
    case 3:
      c = maxc - ((h >> 9) & 1u);
      frac = ((h >> 8) & 1u) ? 0u : 0x7fu;
      break;
    case 4:
      c %= 1ULL << D.mbits;
      break;
    case 5:
      frac = 0;
      switch ((h >> 8) & 3u) {
        case 0: c = 0; break;
        case 1: c = 0, frac = h & 0x7fu; break;
        case 2: c = 1ULL << D.mbits; break;
        default: c = 1; break;
      }
      break;
    default:
      if (c == maxc) frac &= 0x7fu;
      break;
  }
  CvtVal v = {false, 0, 0};
  cvt_decode(D, c, &v);
  uint64_t code = cvt_make(S, neg, (v.m << 8) | frac, v.e - 8 + k);
  if (tweak && (code & (cvt_sign_bit(S) - 1))) {
    code += static_cast<uint64_t>(static_cast<int64_t>(tweak));
    if (!cvt_finite(S, code)) code -= static_cast<uint64_t>(static_cast<int64_t>(tweak));  // S's largest number stays
  }
  return code;
}

// A finite code of format S (16 or 32 bits wide), steered to its subnormals, its largest number, +-0 and its smallest
// normal; `pick` chooses
CVT_HD uint64_t cvt_shape_widen(uint64_t code, uint32_t pick, const CvtFmt S) {
  const uint64_t sign = cvt_sign_bit(S), emask = ((1ULL << S.ebits) - 1) << S.mbits;
  code &= (sign << 1) - 1;
  switch (pick & 7u) {
    case 0: code &= ~emask; break;
    case 1: code = (code & sign) | cvt_max_code(S); break;
    case 2: code &= sign; break;
    case 3: code = (code & sign) | (1ULL << S.mbits); break;
    default: break;
  }
  if (!cvt_finite(S, code)) code ^= S.kind == 1 ? 1ULL : (1ULL << S.mbits);
  return code;
}

// A source of format S for a conversion to an integer of `ibits` magnitude bits: halves, the bounds, +-0 and the tiny,
// beyond the range (the clamp), and anywhere from 1/4 up to the bound
CVT_HD uint64_t cvt_shape_to_int(uint32_t w, const CvtFmt S, int ibits) {
  const bool neg = (w >> 31) != 0;
  const uint32_t cat = w & 7u, h = w >> 3;
  uint64_t m;
  int e;
  switch (cat) {
    case 0: m = 2ULL * ((h >> 4) & ((1u << (ibits > 16 ? 16 : ibits - 1)) - 1)) + 1, e = -1; break;
    case 1: m = (1ULL << 24) - (h & 3u), e = ibits - 24; break;
    case 2:
      switch (h & 3u) {
        case 0: m = 0, e = 0; break;
        case 1: return (neg ? cvt_sign_bit(S) : 0) | 1;
        case 2: m = (1ULL << 24) - 1, e = -25; break;
        default: m = (1ULL << 24) - 1, e = -24; break;
      }
      break;
    case 3: m = (1ULL << 23) | (h & 0x7fffffu), e = ibits + static_cast<int>((h >> 23) & 7u) - 23; break;
    default:
      m = (((1ULL << 23) | (h & 0x7fffffu)) << 29) | (cvt_hash(w, 2) & 0x1fffffffu);
      e = static_cast<int>((h >> 23) % static_cast<uint32_t>(ibits + 3)) - 2 - 52;
      break;
  }
  return cvt_make(S, neg, m, e);
}

// An integer of `ibits` bits (signed: two's complement) for a conversion to a format of P significant bits: ties of
// that format and one either side (where the integer is wider than P), the extremes, the first integer P cannot hold,
// and anywhere.  `cap`: the largest magnitude allowed (the f16 destination's range).
CVT_HD uint32_t cvt_shape_from_int(uint32_t w, int ibits, bool is_signed, int P, uint32_t cap) {
  const bool neg = is_signed && (w >> 31);
  const uint32_t cat = w & 7u, h = w >> 3;
  const int mag_bits = ibits - (is_signed ? 1 : 0);
  uint64_t v;
  if (cat <= 2 && mag_bits > P) {
    const int s = 1 + static_cast<int>(h % static_cast<uint32_t>(mag_bits - P));
    const uint64_t m = (1ULL << (P - 1)) | ((h >> 4) & ((1ULL << (P - 1)) - 1));
    v = ((m << s) | (1ULL << (s - 1))) + (cat == 1 ? 1 : 0) - (cat == 2 ? 1 : 0);
  } else if (cat == 3) {
    switch (h & 3u) {
      case 0: v = 0; break;
      case 1: v = (1ULL << mag_bits) - 1; break;
      case 2: v = is_signed ? (1ULL << mag_bits) : 1; break;  // with neg: the most negative
      default: v = P < mag_bits ? (1ULL << P) + 1 : 3; break;
    }
  } else {
    v = cvt_hash(w, 3) & ((1ULL << mag_bits) - 1);
  }
  while (v > cap) v >>= 1;
  const uint32_t mask = ibits == 32 ? 0xffffffffu : (1u << ibits) - 1;
  return static_cast<uint32_t>(neg ? 0 - v : v) & mask;
}

// The operands op `op` gets from chain word w.  Integer operations only: the same on host and device.
CVT_HD CvtArgs cvt_shape(int op, uint32_t w) {
  const int kind = cvt_kind(op);
  const uint32_t w2 = cvt_hash(w, 0);
  CvtArgs in = {w, w2, cvt_hash(w, 1), cvt_scale_of(cvt_hash(w, 4))};
  int k = 0;
  cvt_scale_exp(in.s, &k);
  const bool fp8_kind = kind == CK_PK_FP8_F32 || kind == CK_S_PK_FP8_F32;
  switch (kind) {
    case CK_F16_F32: in.a = static_cast<uint32_t>(cvt_shape_narrow(w, CVT_F32, CVT_F16, 0)); break;
    case CK_F32_F16: in.a = (w & 0xffff0000u) | static_cast<uint32_t>(cvt_shape_widen(w, w >> 16, CVT_F16)); break;
    case CK_F32_BF16: in.a = (w & 0xffff0000u) | static_cast<uint32_t>(cvt_shape_widen(w, w >> 16, CVT_BF16)); break;
    case CK_F32_F64: {
      const uint64_t d = cvt_shape_narrow(w, CVT_F64, CVT_F32, 0);
      in.a = static_cast<uint32_t>(d), in.b = static_cast<uint32_t>(d >> 32);
      break;
    }
    case CK_F64_F32: in.a = static_cast<uint32_t>(cvt_shape_widen(w, w2, CVT_F32)); break;
    case CK_I32_F32: case CK_FLR: in.a = static_cast<uint32_t>(cvt_shape_to_int(w, CVT_F32, 31)); break;
    case CK_U32_F32: in.a = static_cast<uint32_t>(cvt_shape_to_int(w, CVT_F32, 32)); break;
    case CK_I32_F64: case CK_U32_F64: {
      const uint64_t d = cvt_shape_to_int(w, CVT_F64, kind == CK_I32_F64 ? 31 : 32);
      in.a = static_cast<uint32_t>(d), in.b = static_cast<uint32_t>(d >> 32);
      break;
    }
    case CK_F32_I32: in.a = cvt_shape_from_int(w, 32, true, 24, 0xffffffffu); break;
    case CK_F32_U32: in.a = cvt_shape_from_int(w, 32, false, 24, 0xffffffffu); break;
    case CK_F64_I32: in.a = cvt_shape_from_int(w, 32, true, 53, 0xffffffffu); break;
    case CK_F64_U32: in.a = cvt_shape_from_int(w, 32, false, 53, 0xffffffffu); break;
    case CK_F16_U16: in.a = (w2 & 0xffff0000u) | cvt_shape_from_int(w, 16, false, 11, 65519u); break;
    case CK_F16_I16: in.a = (w2 & 0xffff0000u) | cvt_shape_from_int(w, 16, true, 11, 65519u); break;
    case CK_U16_F16: in.a = (w2 & 0xffff0000u) | static_cast<uint32_t>(cvt_shape_to_int(w, CVT_F16, 16)); break;
    case CK_I16_F16: in.a = (w2 & 0xffff0000u) | static_cast<uint32_t>(cvt_shape_to_int(w, CVT_F16, 15)); break;
    case CK_PKRTZ:
      in.a = static_cast<uint32_t>(cvt_shape_narrow(w, CVT_F32, CVT_F16, 0));
      in.b = static_cast<uint32_t>(cvt_shape_narrow(w2, CVT_F32, CVT_F16, 0));
      break;
    case CK_PK_BF16_F32:
      in.a = static_cast<uint32_t>(cvt_shape_narrow(w, CVT_F32, CVT_BF16, 0));
      in.b = static_cast<uint32_t>(cvt_shape_narrow(w2, CVT_F32, CVT_BF16, 0));
      break;
    case CK_PKNORM_I16: case CK_PKNORM_U16: {  // 9 significant bits below 1; +-1; beyond it; +-0
      uint32_t* dst[2] = {&in.a, &in.b};
      const uint32_t src[2] = {w, w2};
      for (int j = 0; j < 2; ++j) {
        const uint32_t u = src[j], cat = u & 7u, h = u >> 3;
        const bool neg = (u >> 31) != 0;
        uint64_t code;
        if (cat == 0) code = cvt_make(CVT_F32, neg, 1, 0);
        else if (cat == 1) code = cvt_make(CVT_F32, neg, (1ULL << 23) | (h & 0x7fffffu), static_cast<int>((h >> 23) & 7u) - 23);
        else if (cat == 2) code = cvt_make(CVT_F32, neg, 0, 0);
        else code = cvt_make(CVT_F32, neg, 0x100u | (h & 0xffu), -9 - static_cast<int>((h >> 8) & 3u));
        *dst[j] = static_cast<uint32_t>(code);
      }
      break;
    }
    case CK_PK_U8:  // 0 .. 255.498 in steps of 1/256: every tie of the integers among them
      in.a = static_cast<uint32_t>(cvt_make(CVT_F32, false, (w >> 3) % (255u * 256u + 0x80u), -8));
      if ((w & 7u) == 0) in.a = static_cast<uint32_t>(cvt_make(CVT_F32, false, 2 * ((w >> 3) % 255u) + 1, -1));
      break;
    case CK_RPI: {  // |x| < 2^14 in steps of 1/256, so x + 0.5 is exact: ties and one step either side among them
      const uint32_t h = w >> 3, cat = w & 7u;
      uint32_t frac = (h >> 14) & 0xffu;
      if (cat == 0) frac = 0x80u;
      else if (cat == 1) frac = 0x81u;
      else if (cat == 2) frac = 0x7fu;
      else if (cat == 3) frac = 0;
      in.a = static_cast<uint32_t>(cvt_make(CVT_F32, (w >> 31) != 0, ((h & 0x3fffu) << 8) | frac, -8));
      break;
    }
    case CK_PK_FP8_F32: case CK_PK_BF8_F32: k = 0; [[fallthrough]];
    case CK_S_PK_FP8_F32: case CK_S_PK_BF8_F32:
      in.a = static_cast<uint32_t>(cvt_shape_narrow(w, CVT_F32, fp8_kind ? CVT_FP8 : CVT_BF8, k));
      in.b = static_cast<uint32_t>(cvt_shape_narrow(w2, CVT_F32, fp8_kind ? CVT_FP8 : CVT_BF8, k));
      break;
    case CK_S_PK_FP4_F32:
      in.a = static_cast<uint32_t>(cvt_shape_narrow(w, CVT_F32, CVT_FP4, k));
      in.b = static_cast<uint32_t>(cvt_shape_narrow(w2, CVT_F32, CVT_FP4, k));
      break;
    case CK_S_PK_FP8_F16: case CK_S_PK_FP8_BF16: case CK_S_PK_BF8_F16: case CK_S_PK_BF8_BF16: case CK_S_PK_FP4_F16:
    case CK_S_PK_FP4_BF16: {  // two 16-bit sources in a (a value the source format cannot hold is cut, or its largest)
      const bool bf = kind == CK_S_PK_FP8_BF16 || kind == CK_S_PK_BF8_BF16 || kind == CK_S_PK_FP4_BF16;
      const CvtFmt S = bf ? CVT_BF16 : CVT_F16;
      const CvtFmt D = kind == CK_S_PK_FP4_F16 || kind == CK_S_PK_FP4_BF16 ? CVT_FP4
                       : kind == CK_S_PK_FP8_F16 || kind == CK_S_PK_FP8_BF16 ? CVT_FP8 : CVT_BF8;
      uint32_t lo = static_cast<uint32_t>(cvt_shape_narrow(w, S, D, k)), hi = static_cast<uint32_t>(cvt_shape_narrow(w2, S, D, k));
      if (lo == hi) hi ^= 0x8000u;  // two different halves
      in.a = lo | (hi << 16);
      break;
    }
    case CK_S_PK_F16_FP8: case CK_S_F16_FP8:  // a finite f16 result: 448 * 2^7 is the most it holds
      if (k > 7) in.s = cvt_scale_of(cvt_hash(w, 4) % 16u);
      [[fallthrough]];
    case CK_F32_FP8: case CK_PK_F32_FP8: case CK_S_F32_FP8: case CK_S_PK_F32_FP8: case CK_S_PK_BF16_FP8:  // every byte a finite code
      for (int j = 0; j < 4; ++j)
        if (((in.a >> (8 * j)) & 0x7fu) == 0x7fu) in.a ^= 1u << (8 * j);
      break;
    case CK_S_PK_F16_BF8: case CK_S_F16_BF8:  // a finite f16 result: 57344 * 2^0 is the most it holds
      if (k > 0) in.s = cvt_scale_of(cvt_hash(w, 4) % 9u);
      [[fallthrough]];
    case CK_F32_BF8: case CK_PK_F32_BF8: case CK_S_F32_BF8: case CK_S_PK_F32_BF8: case CK_S_PK_BF16_BF8:
      for (int j = 0; j < 4; ++j)
        if (((in.a >> (8 * j)) & 0x7cu) == 0x7cu) in.a ^= 4u << (8 * j);
      break;
    default: break;  // f32_ubyte, off_f32_i4, scalef32_pk_f32_fp4: every word is in the domain
  }
  if ((kind == CK_PKRTZ || kind == CK_PK_BF16_F32 || kind == CK_PK_FP8_F32 || kind == CK_PK_BF8_F32 || kind == CK_S_PK_FP8_F32 ||
       kind == CK_S_PK_BF8_F32 || kind == CK_S_PK_FP4_F32) && in.a == in.b)
    in.b ^= 0x80000000u;  // two different halves
  return in;
}

// The operands a wide form gets from chain word w: 32 sources steered across the 6-bit grid each by its own draw, or
// six words of codes (every code is a number).
CVT_HD CvtWideArgs cvt_shape_wide(int op, uint32_t w) {
  const int kind = cvt_kind(op), big = cvt_wide_big(kind);
  CvtWideArgs in;
  in.s = cvt_scale_of(cvt_hash(w, 4));
  int k = 0;
  cvt_scale_exp(in.s, &k);
  for (int j = 0; j < CVT_WIDE; ++j) in.v[j] = 0;
  if (cvt_wide_narrows(kind)) {
    const CvtFmt S6 = cvt_wide_small_fmt(kind), B = cvt_wide_big_fmt(kind);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < CVT_WIDE; ++j) {
      const uint32_t e = static_cast<uint32_t>(cvt_shape_narrow(cvt_hash(w, 16u + static_cast<uint32_t>(j)), B, S6, k));
      if (big == 0) in.v[j] = e;
      else in.v[j / 2] |= e << (16 * (j & 1));
    }
  } else {
    for (int j = 0; j < 6; ++j) in.v[j] = cvt_hash(w, 16u + static_cast<uint32_t>(j));
  }
  return in;
}

// The words every wave must end with: out[lane * CVT_CHAINS + chain] after `iters` steps of op `op`'s chains under
// `seed` (the test's seed: cvt_op_seed() is applied here).  false when a shaped operand left the domain: the model
// does not run outside it.
inline bool cvt_expected(int op, uint64_t seed, int iters, uint32_t out[CVT_WAVE * CVT_CHAINS]) {
  const uint64_t s = cvt_op_seed(seed, op);
  for (int lane = 0; lane < CVT_WAVE; ++lane)
    for (int ch = 0; ch < CVT_CHAINS; ++ch) {
      uint32_t x = cvt_init(s, lane, ch);
      const uint32_t c = cvt_const(s, lane, ch);
      for (int it = 0; it < iters; ++it) {
        if (cvt_is_wide(op)) {
          CvtWideOut o;
          if (!cvt_convert_wide(op, cvt_shape_wide(op, x), &o)) return false;
          x = cvt_step(x, cvt_fold_wide(o), c);
          continue;
        }
        CvtOut o;
        if (!cvt_convert(op, cvt_shape(op, x), &o)) return false;
        x = cvt_step(x, cvt_fold(o), c);
      }
      out[lane * CVT_CHAINS + ch] = x;
    }
  return true;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_CVT_REF_H_
