// libmi355x_cvt.so: the cvt diagnostic (HIP, gfx950).
//
// Every quantised workload narrows its activations through the vector ALU's format converters and widens them back,
// and no other diagnostic executes one.  This one runs every conversion of cvt_ref.h's op table -- the classic ones
// (f16 / f32 / f64 / integers, pkrtz, pknorm, pk_u8, rpi, flr, off_i4), bf16, fp8 / bf8 with every byte and word
// select, and the gfx950 scalef32 forms of fp8, bf8, fp4, fp6 and bf6 from and to f32, f16 and bf16 -- one template instantiation per op, one native
// instruction each: the __builtin_amdgcn_cvt_* builtin where the compiler has one, an asm statement that names the
// instruction where it has none or where a cast could be vectorised into another one, a plain cast for the 64-bit
// forms (tests/test_cvt_cpu.py counts every op's mnemonic in its kernels).  ops/cvt.py is its Python side;
// ops/diag.run(extra=("cvt",)) runs it next to a level's own tests.
//
// Every lane runs CVT_CHAINS chains of  x = mix32((x << 32 | fold(op(shape(x)))) + c[lane][chain]):  shape() maps the
// chain word into the op's operand domain (ties, the largest finite result, subnormals, +-0: cvt_ref.h), so every
// step's input depends on the previous conversion and a wrong result propagates.  All waves run the same chains; the
// 64 x 4 words a wave must end with come from the host's model (cvt_expected()), and every lane compares bit for bit.
// No LDS allocation, no scratch: cvt_test refuses to run a build that has either.  Every launch also writes the
// wave's float mode (MODE bits 7:0) with a vector store: the model holds for round-to-nearest-even with denormals
// kept, and cvt_test refuses (-3) to judge a device that runs in another mode.
//
// Wrong words are located to their SIMD: the SIMD map row is simd_row() of common/hip_host.h.  The Report a launch
// leaves, the report() that ends the kernel and the host's Run are those of common/simd_report.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "cvt_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int BLOCKS_PER_CU = 4;  // the default grid
constexpr int MAX_ITERS = 1 << 16;
constexpr int MAX_ROWS = 4096;    // of one cvt_apply_many call
constexpr int ROWS_PER_LAUNCH = 64;
constexpr uint32_t MODE_WANT = 0xf0u;  // FP_ROUND (bits 3:0) nearest even for all widths, FP_DENORM (bits 7:4) all kept

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef _Float16 f16x32 __attribute__((ext_vector_type(32)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
struct Words16 {
  uint32_t w[16];
};

__device__ __forceinline__ float as_f(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t as_u(float f) { return __builtin_bit_cast(uint32_t, f); }

// an instruction the compiler has no builtin for; the pads are inside the string, where the compiler adds none
#define CVT_ASM1(M, D, A) asm volatile("s_nop 1\n" M " %0, %1\ns_nop 1" : "=v"(D) : "v"(A))
#define CVT_ASM2(M, D, A, B) asm volatile("s_nop 1\n" M " %0, %1, %2\ns_nop 1" : "=v"(D) : "v"(A), "v"(B))

// One application of op OP: the instruction itself on this lane's operands.
template <int OP>
__device__ __forceinline__ CvtOut convert(const CvtArgs& in) {
  constexpr int K = cvt_kind(OP), SEL = cvt_sel(OP);
  uint32_t r0 = 0, r1 = 0;
  if constexpr (K == CK_F16_F32) {
    CVT_ASM1("v_cvt_f16_f32", r0, in.a);  // (a cast in a loop is paired with its neighbour's into v_cvt_pk_f16_f32)
    r0 &= 0xffffu;
  } else if constexpr (K == CK_F32_F16) {
    CVT_ASM1("v_cvt_f32_f16", r0, in.a);
  } else if constexpr (K == CK_F32_F64 || K == CK_I32_F64 || K == CK_U32_F64) {
    const double d = __builtin_bit_cast(double, (static_cast<uint64_t>(in.b) << 32) | in.a);
    if constexpr (K == CK_F32_F64) r0 = as_u(static_cast<float>(d));
    else if constexpr (K == CK_I32_F64) asm volatile("s_nop 1\nv_cvt_i32_f64 %0, %1\ns_nop 1" : "=v"(r0) : "v"(d));
    else asm volatile("s_nop 1\nv_cvt_u32_f64 %0, %1\ns_nop 1" : "=v"(r0) : "v"(d));
  } else if constexpr (K == CK_F64_F32 || K == CK_F64_I32 || K == CK_F64_U32) {
    double d;
    if constexpr (K == CK_F64_F32) d = static_cast<double>(as_f(in.a));
    else if constexpr (K == CK_F64_I32) d = static_cast<double>(static_cast<int32_t>(in.a));
    else d = static_cast<double>(in.a);
    const uint64_t u = __builtin_bit_cast(uint64_t, d);
    r0 = static_cast<uint32_t>(u), r1 = static_cast<uint32_t>(u >> 32);
  } else if constexpr (K == CK_I32_F32) {  // a cast out of range is undefined in C++: the instruction is named
    CVT_ASM1("v_cvt_i32_f32", r0, in.a);
  } else if constexpr (K == CK_U32_F32) {
    CVT_ASM1("v_cvt_u32_f32", r0, in.a);
  } else if constexpr (K == CK_F32_I32) {
    CVT_ASM1("v_cvt_f32_i32", r0, in.a);
  } else if constexpr (K == CK_F32_U32) {
    CVT_ASM1("v_cvt_f32_u32", r0, in.a);
  } else if constexpr (K == CK_F32_UBYTE) {
    if constexpr (SEL == 0) CVT_ASM1("v_cvt_f32_ubyte0", r0, in.a);
    else if constexpr (SEL == 1) CVT_ASM1("v_cvt_f32_ubyte1", r0, in.a);
    else if constexpr (SEL == 2) CVT_ASM1("v_cvt_f32_ubyte2", r0, in.a);
    else CVT_ASM1("v_cvt_f32_ubyte3", r0, in.a);
  } else if constexpr (K == CK_PKRTZ) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(as_f(in.a), as_f(in.b)));
  } else if constexpr (K == CK_PKNORM_I16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(as_f(in.a), as_f(in.b)));
  } else if constexpr (K == CK_PKNORM_U16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_u16(as_f(in.a), as_f(in.b)));
  } else if constexpr (K == CK_PK_U8) {
    r0 = __builtin_amdgcn_cvt_pk_u8_f32(as_f(in.a), in.b, in.c);
  } else if constexpr (K == CK_RPI) {
    CVT_ASM1("v_cvt_rpi_i32_f32", r0, in.a);
  } else if constexpr (K == CK_FLR) {
    CVT_ASM1("v_cvt_flr_i32_f32", r0, in.a);
  } else if constexpr (K == CK_OFF_I4) {
    r0 = as_u(__builtin_amdgcn_cvt_off_f32_i4(static_cast<int>(in.a)));
  } else if constexpr (K == CK_F16_U16) {  // the 16-bit forms read and write a register's low half
    CVT_ASM1("v_cvt_f16_u16", r0, in.a);
    r0 &= 0xffffu;
  } else if constexpr (K == CK_F16_I16) {
    CVT_ASM1("v_cvt_f16_i16", r0, in.a);
    r0 &= 0xffffu;
  } else if constexpr (K == CK_U16_F16) {
    CVT_ASM1("v_cvt_u16_f16", r0, in.a);
    r0 &= 0xffffu;
  } else if constexpr (K == CK_I16_F16) {
    CVT_ASM1("v_cvt_i16_f16", r0, in.a);
    r0 &= 0xffffu;
  } else if constexpr (K == CK_PK_BF16_F32) {
    CVT_ASM2("v_cvt_pk_bf16_f32", r0, in.a, in.b);
  } else if constexpr (K == CK_F32_BF16) {
    CVT_ASM1("v_cvt_f32_bf16", r0, in.a);
  } else if constexpr (K == CK_F32_FP8) {
    r0 = as_u(__builtin_amdgcn_cvt_f32_fp8(static_cast<int>(in.a), SEL));
  } else if constexpr (K == CK_F32_BF8) {
    r0 = as_u(__builtin_amdgcn_cvt_f32_bf8(static_cast<int>(in.a), SEL));
  } else if constexpr (K == CK_PK_F32_FP8) {
    const f32x2 r = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(in.a), SEL != 0);
    r0 = as_u(r.x), r1 = as_u(r.y);
  } else if constexpr (K == CK_PK_F32_BF8) {
    const f32x2 r = __builtin_amdgcn_cvt_pk_f32_bf8(static_cast<int>(in.a), SEL != 0);
    r0 = as_u(r.x), r1 = as_u(r.y);
  } else if constexpr (K == CK_PK_FP8_F32) {
    r0 = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(as_f(in.a), as_f(in.b), static_cast<int>(in.c), SEL != 0));
  } else if constexpr (K == CK_PK_BF8_F32) {
    r0 = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_bf8_f32(as_f(in.a), as_f(in.b), static_cast<int>(in.c), SEL != 0));
  } else if constexpr (K == CK_S_PK_FP8_F32) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(__builtin_bit_cast(i16x2, in.c), as_f(in.a),
                                                                               as_f(in.b), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_BF8_F32) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(__builtin_bit_cast(i16x2, in.c), as_f(in.a),
                                                                               as_f(in.b), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_F32_FP8) {
    const f32x2 r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(in.a, as_f(in.s), SEL != 0);
    r0 = as_u(r.x), r1 = as_u(r.y);
  } else if constexpr (K == CK_S_PK_F32_BF8) {
    const f32x2 r = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(in.a, as_f(in.s), SEL != 0);
    r0 = as_u(r.x), r1 = as_u(r.y);
  } else if constexpr (K == CK_S_F32_FP8) {
    r0 = as_u(__builtin_amdgcn_cvt_scalef32_f32_fp8(static_cast<int>(in.a), as_f(in.s), SEL));
  } else if constexpr (K == CK_S_F32_BF8) {
    r0 = as_u(__builtin_amdgcn_cvt_scalef32_f32_bf8(static_cast<int>(in.a), as_f(in.s), SEL));
  } else if constexpr (K == CK_S_PK_FP4_F32) {
    r0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(in.c, as_f(in.a), as_f(in.b), as_f(in.s), SEL);
  } else if constexpr (K == CK_S_PK_FP8_F16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(__builtin_bit_cast(i16x2, in.c),
                                                                               __builtin_bit_cast(f16x2, in.a), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_FP8_BF16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(__builtin_bit_cast(i16x2, in.c),
                                                                                __builtin_bit_cast(bf16x2, in.a), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_BF8_F16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(__builtin_bit_cast(i16x2, in.c),
                                                                               __builtin_bit_cast(f16x2, in.a), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_BF8_BF16) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(__builtin_bit_cast(i16x2, in.c),
                                                                                __builtin_bit_cast(bf16x2, in.a), as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_F16_FP8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(in.a, as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_BF16_FP8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(in.a, as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_F16_BF8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(in.a, as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_PK_BF16_BF8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(in.a, as_f(in.s), SEL != 0));
  } else if constexpr (K == CK_S_F16_FP8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_f16_fp8(__builtin_bit_cast(f16x2, in.c), static_cast<int>(in.a),
                                                                            as_f(in.s), SEL & 3, (SEL >> 2) != 0));
  } else if constexpr (K == CK_S_F16_BF8) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_f16_bf8(__builtin_bit_cast(f16x2, in.c), static_cast<int>(in.a),
                                                                            as_f(in.s), SEL & 3, (SEL >> 2) != 0));
  } else if constexpr (K == CK_S_PK_FP4_F16) {
    r0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(in.c, __builtin_bit_cast(f16x2, in.a), as_f(in.s), SEL);
  } else if constexpr (K == CK_S_PK_FP4_BF16) {
    r0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(in.c, __builtin_bit_cast(bf16x2, in.a), as_f(in.s), SEL);
  } else if constexpr (K == CK_S_PK_F16_FP4) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(in.a, as_f(in.s), SEL));
  } else if constexpr (K == CK_S_PK_BF16_FP4) {
    r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(in.a, as_f(in.s), SEL));
  } else {
    static_assert(K == CK_S_PK_F32_FP4, "an op without an instruction");
    const f32x2 r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(in.a, as_f(in.s), SEL);
    r0 = as_u(r.x), r1 = as_u(r.y);
  }
  return {{r0, r1}};
}

// One application of a wide form (cvt_is_wide): 32 values per lane through one instruction.
template <int OP>
__device__ __forceinline__ CvtWideOut convert_wide(const CvtWideArgs& in) {
  constexpr int K = cvt_kind(OP);
  CvtWideOut out;
#pragma unroll
  for (int j = 0; j < CVT_WIDE; ++j) out.r[j] = 0;
  const float scale = as_f(in.s);
  if constexpr (cvt_wide_narrows(K)) {
    u32x6 r;
    if constexpr (K == CK_W_2XPK16_FP6_F32 || K == CK_W_2XPK16_BF6_F32) {
      f32x16 a, b;
#pragma unroll
      for (int j = 0; j < 16; ++j) a[j] = as_f(in.v[j]), b[j] = as_f(in.v[16 + j]);
      if constexpr (K == CK_W_2XPK16_FP6_F32) r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
      else r = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, scale);
    } else {
      Words16 src;
#pragma unroll
      for (int j = 0; j < 16; ++j) src.w[j] = in.v[j];
      if constexpr (K == CK_W_PK32_FP6_F16) r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(__builtin_bit_cast(f16x32, src), scale);
      else if constexpr (K == CK_W_PK32_BF6_F16) r = __builtin_amdgcn_cvt_scalef32_pk32_bf6_f16(__builtin_bit_cast(f16x32, src), scale);
      else if constexpr (K == CK_W_PK32_FP6_BF16) r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, src), scale);
      else r = __builtin_amdgcn_cvt_scalef32_pk32_bf6_bf16(__builtin_bit_cast(bf16x32, src), scale);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) out.r[j] = r[j];
  } else {
    const u32x6 src = {in.v[0], in.v[1], in.v[2], in.v[3], in.v[4], in.v[5]};
    if constexpr (K == CK_W_PK32_F32_FP6 || K == CK_W_PK32_F32_BF6) {
      f32x32 r;
      if constexpr (K == CK_W_PK32_F32_FP6) r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(src, scale);
      else r = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(src, scale);
#pragma unroll
      for (int j = 0; j < 32; ++j) out.r[j] = as_u(r[j]);
    } else {
      Words16 r;
      if constexpr (K == CK_W_PK32_F16_FP6) r = __builtin_bit_cast(Words16, __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(src, scale));
      else if constexpr (K == CK_W_PK32_F16_BF6) r = __builtin_bit_cast(Words16, __builtin_amdgcn_cvt_scalef32_pk32_f16_bf6(src, scale));
      else if constexpr (K == CK_W_PK32_BF16_FP6) r = __builtin_bit_cast(Words16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(src, scale));
      else r = __builtin_bit_cast(Words16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(src, scale));
#pragma unroll
      for (int j = 0; j < 16; ++j) out.r[j] = r.w[j];
    }
  }
  return out;
}

// one chain step of op OP on chain word x (converted, or -- the self-check's skipped step -- the sources folded as they are)
template <int OP>
__device__ __forceinline__ uint32_t chain_step(uint32_t x, uint32_t c, bool converted) {
  if constexpr (cvt_is_wide(OP)) {
    const CvtWideArgs in = cvt_shape_wide(OP, x);
    CvtWideOut o;
    if (converted) {
      o = convert_wide<OP>(in);
    } else {
#pragma unroll
      for (int j = 0; j < CVT_WIDE; ++j) o.r[j] = in.v[j];
    }
    return cvt_step(x, cvt_fold_wide(o), c);
  } else {
    const CvtArgs in = cvt_shape(OP, x);
    return cvt_step(x, cvt_fold(converted ? convert<OP>(in) : CvtOut{{in.a, in.b}}), c);
  }
}

// (skip_block, skip_iter): the self-check's conversion that did not happen, on wave 0 of that workgroup at that step
// (-1: none): the chains fold the sources as they are; flip_block: one bit of lane 0's final chain-0 word of that
// workgroup's wave 0 is flipped (-1: none).  mode_out: the wave's MODE bits 7:0, written by lane 0 of workgroup 0.
template <int OP>
__global__ void __launch_bounds__(THREADS) cvt_kernel(const uint32_t* __restrict__ expect, uint64_t seed, int iters, int flip_block,
                                                      int skip_block, int skip_iter, Report* rep, unsigned long long* simd_map,
                                                      uint32_t* mode_out) {
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int skip_at = wave == 0 && static_cast<int>(blockIdx.x) == skip_block ? skip_iter : -1;  // wave-uniform
  const uint32_t mode = __builtin_amdgcn_s_getreg((7 << 11) | (0 << 6) | 1);                     // MODE[7:0]
  uint32_t x[CVT_CHAINS], c[CVT_CHAINS];
#pragma unroll
  for (int ch = 0; ch < CVT_CHAINS; ++ch) {
    x[ch] = cvt_init(seed, static_cast<int>(lane), ch);
    c[ch] = cvt_const(seed, static_cast<int>(lane), ch);
  }
  for (int it = 0; it < iters; ++it) {
    if (it != skip_at) {
#pragma unroll
      for (int ch = 0; ch < CVT_CHAINS; ++ch) x[ch] = chain_step<OP>(x[ch], c[ch], true);
    } else {
#pragma unroll
      for (int ch = 0; ch < CVT_CHAINS; ++ch) x[ch] = chain_step<OP>(x[ch], c[ch], false);
    }
  }
  if (static_cast<int>(blockIdx.x) == flip_block && threadIdx.x == 0) x[0] ^= 0x10u;
  if (blockIdx.x == 0 && threadIdx.x == 0) *mode_out = mode;
  unsigned nbad = 0, first_chain = 0;
  uint32_t got = 0, want = 0;
#pragma unroll
  for (int ch = CVT_CHAINS - 1; ch >= 0; --ch) {  // ends at the first wrong chain
    const uint32_t w = expect[lane * CVT_CHAINS + ch];
    if (x[ch] != w) ++nbad, first_chain = ch, got = x[ch], want = w;
  }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  // a record's `where`: SIMD map row << 16 | lane << 8 | the lane's first wrong chain
  const unsigned long long where = (static_cast<unsigned long long>(row) << 16) | (lane << 8) | first_chain;
  report(rep, simd_map, row, nbad, where, 0, got, want, dt);
}

// the words of one operand row and of one result row of op `op`: (a, b, c, s) and two registers, or a wide form's
// 32 words and the scale, and 32 words
constexpr int in_words(int op) { return cvt_is_wide(op) ? CVT_WIDE_IN : 4; }
constexpr int out_words(int op) { return cvt_is_wide(op) ? CVT_WIDE_OUT : 2; }

// one wave, `n` applications one after the other, returned raw: row i's lane l reads in[(i * 64 + l) * in_words ..]
// and writes out[(i * 64 + l) * out_words ..]
template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  for (int i = 0; i < n; ++i) {
    const size_t k = static_cast<size_t>(i) * 64u + threadIdx.x;
    if constexpr (cvt_is_wide(OP)) {
      CvtWideArgs a;
#pragma unroll
      for (int j = 0; j < CVT_WIDE; ++j) a.v[j] = in[CVT_WIDE_IN * k + j];
      a.s = in[CVT_WIDE_IN * k + CVT_WIDE];
      const CvtWideOut r = convert_wide<OP>(a);
#pragma unroll
      for (int j = 0; j < CVT_WIDE; ++j) out[CVT_WIDE_OUT * k + j] = r.r[j];
    } else {
      const CvtArgs a = {in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3]};
      const CvtOut r = convert<OP>(a);
      out[2 * k] = r.r[0];
      out[2 * k + 1] = r.r[1];
    }
  }
}

struct Launch {
  const uint32_t* expect;
  uint64_t seed;
  int iters, flip_block, skip_block, skip_iter;
  Report* rep;
  unsigned long long* map;
  uint32_t* mode;
  unsigned blocks;
};

template <int OP>
void launch_op(const Launch& l) {
  hipLaunchKernelGGL(cvt_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.expect, l.seed, l.iters, l.flip_block,
                     l.skip_block, l.skip_iter, l.rep, l.map, l.mode);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(cvt_kernel<OP>));
}
template <int OP>
void launch_apply(const uint32_t* in, uint32_t* out, int n) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, in, out, n);
}
template <int OP>
hipError_t attributes_apply(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(apply_kernel<OP>));
}

// the tables from op index to instantiation
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const Launch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(const uint32_t*, uint32_t*, int) = {launch_apply<OP>...};
  static constexpr hipError_t (*apply_attributes[])(hipFuncAttributes*) = {attributes_apply<OP>...};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, CVT_OPS>()));

int refuse(const hipFuncAttributes& attr, const std::string& what) {
  return refuse_memory("cvt test", what, attr, ": it would test memory, not the converter");
}

}  // namespace

extern "C" {

const char* cvt_last_error(void) { return g_err.c_str(); }

int cvt_device_count(void) { return device_count(); }

int cvt_slots(void) { return SIMD_ROWS; }  // rows of cvt_test's simd_map

int cvt_ops(void) { return CVT_OPS; }  // the op table's length

// The words of one operand row and of one result row of op `op` in the three calls below: 4 (a, b, c, s: CvtArgs) and
// 2 (the result registers), or, for a wide form, 33 (32 words of values, then the scale: CvtWideArgs) and 32.
int cvt_row_words(int op, int* operand_words, int* result_words) {
  if (op < 0 || op >= CVT_OPS) {
    g_err = "cvt row_words: need an op of the table";
    return -2;
  }
  *operand_words = in_words(op), *result_words = out_words(op);
  return 0;
}

// The host's side of an application, no GPU used.  cvt_shape_rows: the operand rows that op `op`'s shape gives the n
// chain words cvt_mix32(seed + i).  cvt_model_rows: the model's result row per row of `rows`, with ok[i] = 0 (and
// zeros) where the operands lie outside the model's domain.  -2: an unknown op, n < 1.
int cvt_shape_rows(int op, uint64_t seed, int n, unsigned int* rows) {
  if (op < 0 || op >= CVT_OPS || n < 1 || rows == nullptr) {
    g_err = "cvt shape_rows: need an op of the table and n >= 1";
    return -2;
  }
  for (int i = 0; i < n; ++i) {
    const uint32_t w = cvt_mix32(seed + static_cast<uint64_t>(i));
    if (cvt_is_wide(op)) {
      const CvtWideArgs a = cvt_shape_wide(op, w);
      for (int j = 0; j < CVT_WIDE; ++j) rows[CVT_WIDE_IN * i + j] = a.v[j];
      rows[CVT_WIDE_IN * i + CVT_WIDE] = a.s;
      continue;
    }
    const CvtArgs a = cvt_shape(op, w);
    rows[4 * i] = a.a, rows[4 * i + 1] = a.b, rows[4 * i + 2] = a.c, rows[4 * i + 3] = a.s;
  }
  return 0;
}

int cvt_model_rows(int op, const unsigned int* rows, int n, unsigned int* out, unsigned char* ok) {
  if (op < 0 || op >= CVT_OPS || n < 1 || rows == nullptr) {
    g_err = "cvt model_rows: need an op of the table and n >= 1";
    return -2;
  }
  for (int i = 0; i < n && cvt_is_wide(op); ++i) {
    CvtWideArgs a;
    CvtWideOut o;
    for (int j = 0; j < CVT_WIDE; ++j) a.v[j] = rows[CVT_WIDE_IN * i + j], o.r[j] = 0;
    a.s = rows[CVT_WIDE_IN * i + CVT_WIDE];
    ok[i] = cvt_convert_wide(op, a, &o) ? 1 : 0;
    for (int j = 0; j < CVT_WIDE; ++j) out[CVT_WIDE_OUT * i + j] = o.r[j];
  }
  for (int i = 0; i < n && !cvt_is_wide(op); ++i) {
    CvtOut o = {{0, 0}};
    ok[i] = cvt_convert(op, {rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]}, &o) ? 1 : 0;
    out[2 * i] = o.r[0], out[2 * i + 1] = o.r[1];
  }
  return 0;
}

// Every op of `ops[0..nops)` (CvtOp of cvt_ref.h), one after the other, on `blocks` workgroups of 4 waves (0: 4 per
// CU), `iters` steps of 4 chains per lane: a checked warm-up launch, then `reps` timed and checked launches.  Per op k
// (arrays of the table's length): errors[k] = wrong chain words over all its launches; first[4 k ..] = where (SIMD map
// row << 16 | lane << 8 | chain; ~0: none), 0, got, want of one wrong word of the first launch that had any; ms[k] the
// mean time of a timed launch.  mode[0] = the float mode the first warm-up launch ran in (MODE bits 7:0: FP_ROUND in
// 3:0, FP_DENORM in 7:4).  simd_map: cvt_slots() x 3 (waves run, wrong words, summed wall_clock64 ticks) per physical
// SIMD (simd_row()), added up over every launch of every op.
//
// Refused with -2 and a message: a bad device, blocks < 0, iters outside 1..2^16, reps < 1, no op, an unknown or
// repeated one, a hook outside the list or the grid; with -3: a kernel built with a scratch segment or an LDS
// allocation, a float mode other than round-to-nearest-even with denormals kept (the message names the field), or a
// shaped operand outside the model's domain.
//
// Self-check hooks, off by default (inject_op -1), both acting in the warm-up launch of op `inject_op`, on wave 0 of
// workgroup `inject_block`:
//   flip  (inject_skip_iter < 0): one bit of lane 0's final chain-0 word is flipped before the compare: 1 wrong word,
//         got = want ^ 0x10
//   skip  (inject_skip_iter >= 0): the wave leaves the conversion out of that one step (the chains fold the sources
//         unconverted); wrong words > 0
int cvt_test(int device, int blocks, int iters, int reps, const int* ops, int nops, uint64_t seed, int inject_op, int inject_block,
             int inject_skip_iter, unsigned long long* errors, unsigned long long* first, double* ms, unsigned int* mode,
             unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || iters < 1 || iters > MAX_ITERS || reps < 1 ||
      !op_list_known(ops, nops, CVT_OPS, true)) {
    g_err = "cvt test: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^16, reps >= 1 and a list of distinct known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (!op_list_has_hook(ops, nops, inject_op) || (inject_op >= 0 && !hook_in_range(inject_block, grid, inject_skip_iter, iters))) {
    g_err = "cvt test: inject_op must be in the list, inject_block inside the grid and inject_skip_iter below iters";
    return -2;
  }
  for (int k = 0; k < CVT_OPS; ++k) {
    errors[k] = 0;
    no_record(first + 4 * k);
    ms[k] = 0.0;
  }
  *mode = 0;
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf dexp, dmode;
  HIP_CHECK(dexp.alloc(device, CVT_WAVE * CVT_CHAINS * sizeof(uint32_t)));
  HIP_CHECK(dmode.alloc(device, sizeof(uint32_t)));
  HIP_CHECK(hipMemset(dmode.ptr, 0xff, sizeof(uint32_t)));
  std::vector<uint32_t> expect(CVT_WAVE * CVT_CHAINS);
  for (int i = 0; i < nops; ++i) {
    const int k = ops[i];
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse(attr, CVT_OP_TABLE[k].name)) return rc;
    if (!cvt_expected(k, seed, iters, expect.data())) {
      g_err = std::string("cvt test: a shaped operand of ") + CVT_OP_TABLE[k].name + " left the model's domain";
      return -3;
    }
    HIP_CHECK(hipMemcpy(dexp.ptr, expect.data(), expect.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_iter);
      AllOps::launch[k]({static_cast<const uint32_t*>(dexp.ptr), cvt_op_seed(seed, k), iters, h.flip_block, h.skip_block,
                         h.skip_at, run.rep(), run.map(), static_cast<uint32_t*>(dmode.ptr), grid});
    };
    const auto judge_mode = [&](int r) {  // the mode of the first warm-up: nothing is judged under another
      if (i != 0 || r != 0) return 0;
      uint32_t m = 0;
      HIP_CHECK(hipMemcpy(&m, dmode.ptr, sizeof m, hipMemcpyDeviceToHost));
      *mode = m;
      if ((m & 0xffu) != MODE_WANT) {
        g_err = std::string("cvt test: the waves run with MODE.") + ((m & 0xfu) ? "FP_ROUND" : "FP_DENORM") + " = " +
                std::to_string((m & 0xfu) ? (m & 0xfu) : ((m >> 4) & 0xfu)) +
                ": the model holds for round-to-nearest-even (0) with denormals kept (15)";
        return -3;
      }
      return 0;
    };
    if (const int rc = run.series(reps, enqueue, errors + k, first + 4 * k, ms + k, judge_mode)) return rc;
  }
  return run.read_map(simd_map);
}

// Single applications of op `op` by one wave of `device`, returned raw, ROWS_PER_LAUNCH rows of 64 lanes per launch:
// rows[(i * 64 + lane) * operand_words ..] = the operands of row i's lane, out[(i * 64 + lane) * result_words ..] =
// its result registers (cvt_row_words(); a register the op does not write is 0).  Any operand may be given: this is how
// NaN, Inf and overflowing sources are probed.  Refused with -2: a bad device or op, nrows outside 1..4096.
int cvt_apply_many(int device, int op, const unsigned int* rows, int nrows, unsigned int* out) {
  const int n = device_count();
  if (device < 0 || device >= n || op < 0 || op >= CVT_OPS || rows == nullptr || nrows < 1 || nrows > MAX_ROWS) {
    g_err = "cvt apply: need a valid device, an op of the table and 1..4096 rows of 64 lanes";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  hipFuncAttributes attr;
  HIP_CHECK(AllOps::apply_attributes[op](&attr));
  if (const int rc = refuse(attr, std::string("apply of ") + CVT_OP_TABLE[op].name)) return rc;
  const size_t lanes = static_cast<size_t>(nrows) * CVT_WAVE;
  DevBuf din, dout;
  const size_t iw = static_cast<size_t>(in_words(op)), ow = static_cast<size_t>(out_words(op));
  HIP_CHECK(din.alloc(device, lanes * iw * 4));
  HIP_CHECK(dout.alloc(device, lanes * ow * 4));
  HIP_CHECK(hipMemcpy(din.ptr, rows, lanes * iw * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(dout.ptr, 0, lanes * ow * 4));
  for (int at = 0; at < nrows; at += ROWS_PER_LAUNCH) {
    const int count = nrows - at < ROWS_PER_LAUNCH ? nrows - at : ROWS_PER_LAUNCH;
    AllOps::apply[op](static_cast<const uint32_t*>(din.ptr) + static_cast<size_t>(at) * CVT_WAVE * iw,
                      static_cast<uint32_t*>(dout.ptr) + static_cast<size_t>(at) * CVT_WAVE * ow, count);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out, dout.ptr, lanes * ow * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
