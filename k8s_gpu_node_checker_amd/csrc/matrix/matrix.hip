// libmi355x_matrix.so: the matrix diagnostic (HIP, gfx950).
//
// The matrix-core burn-in runs four encodings of one 16x16 shape on {-1, 0, +1} operands and checks a lane sum.  This
// one issues the MFMA families of matrix_ref.h's table -- fp32, fp16, bf16, int8 and fp64 inputs, the gfx94x-era bf8
// instructions, bf8 / fp6 / bf6 / fp4 of f8f6f4 with and without block scales in both shapes, and the gfx94x-era sparse
// v_smfmac_* -- on operands that exercise the significand multipliers and the exponent alignment, and compares every
// element of the accumulator bit for bit.  ops/matrix.py is its Python side; ops/diag.run(extra=("matrix",)) runs it
// next to a level's own tests.
//
// One template instantiation per op of matrix_ref.h, one native instruction each (control immediates 0).  Every wave
// loads MATRIX_STEPS operand sets and C once and keeps them in registers; a round is
//     acc = C;  for s in 0..3: acc = op(A_s, B_s, acc)
// (dependent through the accumulator, as a K loop's steps are), and after every round each lane compares its
// elements of acc with the host model's (matrix_expect() of matrix_ref.h) as raw bits.  The operands obey the
// header's exactness rule, so the result has one value whatever the order the hardware adds in.  No LDS, no scratch:
// matrix_test refuses to run a build that has either.
//
// Wrong elements are located to their SIMD as the register-file test's are: the SIMD map row is simd_row() of
// common/hip_host.h.  The Report a launch leaves, the report() that ends the kernel and the host's Run are those of
// common/simd_report.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "matrix_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int BLOCKS_PER_CU = 2;        // the default grid
constexpr int MAX_ITERS = 1 << 20;

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef int intx2 __attribute__((ext_vector_type(2)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef int intx16 __attribute__((ext_vector_type(16)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx16 __attribute__((ext_vector_type(16)));
typedef short shortx4 __attribute__((ext_vector_type(4)));
typedef short shortx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

// the accumulator type of op OP
template <int OP>
struct Acc {
  static constexpr MatrixOpInfo o = MATRIX_OP_TABLE[OP];
  using type = std::conditional_t<o.cfmt == MF_F64, doublex4,
               std::conditional_t<o.cfmt == MF_I32, std::conditional_t<o.M == 32, intx16, intx4>,
                                  std::conditional_t<o.M == 32, floatx16, floatx4>>>;
};

// a lane's register words as the builtin's operand type
template <class T>
__device__ __forceinline__ T as(const uint32_t* w) {
  T t;
  __builtin_memcpy(&t, w, sizeof(T));
  return t;
}

#define MX_IS(SP, AF, BF, M_, K_) (o.sparse == SP && !o.f8f6f4 && o.afmt == AF && o.bfmt == BF && o.M == M_ && o.K == K_)

// One application of op OP: the instruction itself on this lane's registers (a, b: MATRIX_AW words, those past the
// op's own are zero), its accumulator, and the index / scale registers where the op has them.
template <int OP>
__device__ __forceinline__ typename Acc<OP>::type mfma(const uint32_t* a, const uint32_t* b, typename Acc<OP>::type c,
                                                       int idx, int sa, int sb) {
  constexpr MatrixOpInfo o = MATRIX_OP_TABLE[OP];
  if constexpr (o.f8f6f4 && o.scaled && o.M == 16) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(as<intx8>(a), as<intx8>(b), c, o.cbsz, o.blgp, 0, sa, 0, sb);
  } else if constexpr (o.f8f6f4 && o.scaled) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(as<intx8>(a), as<intx8>(b), c, o.cbsz, o.blgp, 0, sa, 0, sb);
  } else if constexpr (o.f8f6f4 && o.M == 16) {  // zero scale operands select the unscaled instruction
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(as<intx8>(a), as<intx8>(b), c, o.cbsz, o.blgp, 0, 0, 0, 0);
  } else if constexpr (o.f8f6f4) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(as<intx8>(a), as<intx8>(b), c, o.cbsz, o.blgp, 0, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F32, MF_F32, 32, 2)) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(as<float>(a), as<float>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F32, MF_F32, 16, 4)) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(as<float>(a), as<float>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F16, MF_F16, 32, 8)) {
    return __builtin_amdgcn_mfma_f32_32x32x8f16(as<halfx4>(a), as<halfx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F16, MF_F16, 16, 16)) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(as<halfx4>(a), as<halfx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F16, MF_F16, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(as<halfx8>(a), as<halfx8>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F16, MF_F16, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(as<halfx8>(a), as<halfx8>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF16, MF_BF16, 32, 8)) {
    return __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(as<shortx4>(a), as<shortx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF16, MF_BF16, 16, 16)) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as<shortx4>(a), as<shortx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF16, MF_BF16, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as<bf16x8>(a), as<bf16x8>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF16, MF_BF16, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as<bf16x8>(a), as<bf16x8>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_I8, MF_I8, 32, 16)) {
    return __builtin_amdgcn_mfma_i32_32x32x16_i8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_I8, MF_I8, 16, 32)) {
    return __builtin_amdgcn_mfma_i32_16x16x32_i8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_I8, MF_I8, 32, 32)) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(as<intx4>(a), as<intx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_I8, MF_I8, 16, 64)) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(as<intx4>(a), as<intx4>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_F64, MF_F64, 16, 4)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(as<double>(a), as<double>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_FP8, MF_FP8, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_FP8, MF_BF8, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF8, MF_FP8, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF8, MF_BF8, 16, 32)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_FP8, MF_FP8, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_FP8, MF_BF8, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_bf8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF8, MF_FP8, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf8_fp8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(0, MF_BF8, MF_BF8, 32, 16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(as<long>(a), as<long>(b), c, 0, 0, 0);
  } else if constexpr (MX_IS(1, MF_F16, MF_F16, 16, 32)) {  // the sparse ops: cbsz = abid = 0
    return __builtin_amdgcn_smfmac_f32_16x16x32_f16(as<halfx4>(a), as<halfx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_F16, MF_F16, 32, 16)) {
    return __builtin_amdgcn_smfmac_f32_32x32x16_f16(as<halfx4>(a), as<halfx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_F16, MF_F16, 16, 64)) {
    return __builtin_amdgcn_smfmac_f32_16x16x64_f16(as<halfx8>(a), as<halfx16>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_F16, MF_F16, 32, 32)) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_f16(as<halfx8>(a), as<halfx16>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF16, MF_BF16, 16, 32)) {
    return __builtin_amdgcn_smfmac_f32_16x16x32_bf16(as<shortx4>(a), as<shortx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF16, MF_BF16, 32, 16)) {
    return __builtin_amdgcn_smfmac_f32_32x32x16_bf16(as<shortx4>(a), as<shortx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF16, MF_BF16, 16, 64)) {
    return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(as<bf16x8>(a), as<bf16x16>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF16, MF_BF16, 32, 32)) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_bf16(as<bf16x8>(a), as<bf16x16>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_I8, MF_I8, 16, 64)) {
    return __builtin_amdgcn_smfmac_i32_16x16x64_i8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_I8, MF_I8, 32, 32)) {
    return __builtin_amdgcn_smfmac_i32_32x32x32_i8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_I8, MF_I8, 16, 128)) {
    return __builtin_amdgcn_smfmac_i32_16x16x128_i8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_I8, MF_I8, 32, 64)) {
    return __builtin_amdgcn_smfmac_i32_32x32x64_i8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_FP8, MF_FP8, 16, 64)) {
    return __builtin_amdgcn_smfmac_f32_16x16x64_fp8_fp8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_FP8, MF_FP8, 32, 32)) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_fp8_fp8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_FP8, MF_FP8, 16, 128)) {
    return __builtin_amdgcn_smfmac_f32_16x16x128_fp8_fp8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_FP8, MF_FP8, 32, 64)) {
    return __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF8, MF_BF8, 16, 64)) {
    return __builtin_amdgcn_smfmac_f32_16x16x64_bf8_bf8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF8, MF_BF8, 32, 32)) {
    return __builtin_amdgcn_smfmac_f32_32x32x32_bf8_bf8(as<intx2>(a), as<intx4>(b), c, idx, 0, 0);
  } else if constexpr (MX_IS(1, MF_BF8, MF_BF8, 16, 128)) {
    return __builtin_amdgcn_smfmac_f32_16x16x128_bf8_bf8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  } else {
    static_assert(MX_IS(1, MF_BF8, MF_BF8, 32, 64), "an op without an instruction");
    return __builtin_amdgcn_smfmac_f32_32x32x64_bf8_bf8(as<intx4>(a), as<intx8>(b), c, idx, 0, 0);
  }
}
#undef MX_IS

// the words of a lane's operand block the op reads (the rest of the builtin's operand is zero)
template <int OP>
struct Words {
  static constexpr MatrixOpInfo o = MATRIX_OP_TABLE[OP];
  static constexpr int a = matrix_a_words(o), b = matrix_b_words(o), c = matrix_cd_words(o);
  static constexpr int per_elem = matrix_fmt(o.cfmt).bits / 32;
};

// (flip_block, skip_block): the self-check's workgroup (-1: none).  flip: wave 0's lane 0 flips bit 4 of register 0
// of the last round's accumulator before the compare.  skip: wave 0 leaves step `skip_step` out of the last round.
template <int OP>
__global__ void __launch_bounds__(THREADS) matrix_kernel(const MatrixOperands* __restrict__ in, int iters, int flip_block,
                                                         int skip_block, int skip_step, Report* rep,
                                                         unsigned long long* simd_map) {
  using W = Words<OP>;
  using CT = typename Acc<OP>::type;
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int skip_at = wave == 0 && static_cast<int>(blockIdx.x) == skip_block ? skip_step : -1;  // wave-uniform
  const bool flip = static_cast<int>(blockIdx.x) == flip_block && threadIdx.x == 0;
  uint32_t a[MATRIX_STEPS][MATRIX_AW] = {}, b[MATRIX_STEPS][MATRIX_AW] = {}, cw[W::c], want[W::c];
  int idx[MATRIX_STEPS], sa[MATRIX_STEPS], sb[MATRIX_STEPS];
#pragma unroll
  for (int s = 0; s < MATRIX_STEPS; ++s) {
#pragma unroll
    for (int w = 0; w < W::a; ++w) a[s][w] = in->A[s][lane * MATRIX_AW + w];
#pragma unroll
    for (int w = 0; w < W::b; ++w) b[s][w] = in->B[s][lane * MATRIX_AW + w];
    idx[s] = static_cast<int>(in->idx[s][lane]);
    sa[s] = static_cast<int>(in->scale_a[s][lane]);
    sb[s] = static_cast<int>(in->scale_b[s][lane]);
  }
#pragma unroll
  for (int w = 0; w < W::c; ++w) cw[w] = in->C[lane * MATRIX_CW + w], want[w] = in->D[lane * MATRIX_CW + w];
  const CT c = as<CT>(cw);
  unsigned nbad = 0;
  int first = -1;
  unsigned long long first_got = 0, first_want = 0;
  for (int it = 0; it < iters; ++it) {
    CT acc = c;
    asm volatile("" : "+v"(acc));  // the round's input is opaque: its four instructions are issued every round
    const int skip = it == iters - 1 ? skip_at : -1;
#pragma unroll
    for (int s = 0; s < MATRIX_STEPS; ++s)
      if (s != skip) acc = mfma<OP>(a[s], b[s], acc, idx[s], sa[s], sb[s]);
    uint32_t got[W::c];
    __builtin_memcpy(got, &acc, sizeof got);
    if (flip && it == iters - 1) got[0] ^= 0x10u;
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < W::c; ++w) diff |= got[w] ^ want[w];
    if (diff) {
#pragma unroll
      for (int r = 0; r < W::c / W::per_elem; ++r) {
        unsigned long long g = got[r * W::per_elem], e = want[r * W::per_elem];
        if constexpr (W::per_elem == 2) {
          g |= static_cast<unsigned long long>(got[2 * r + 1]) << 32;
          e |= static_cast<unsigned long long>(want[2 * r + 1]) << 32;
        }
        if (g != e) {
          ++nbad;
          if (first < 0) first = r, first_got = g, first_want = e;
        }
      }
    }
  }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  // a record's `where`: SIMD map row << 16 | lane << 8 | register element of the lane's first wrong element
  const unsigned long long where =
      (static_cast<unsigned long long>(row) << 16) | (lane << 8) | static_cast<unsigned>(first);
  report(rep, simd_map, row, nbad, where, 0, first_got, first_want, dt);
}

// what matrix_apply hands one wave: raw registers in, raw D out
struct ApplyIo {
  uint32_t A[MATRIX_WAVE * MATRIX_AW], B[MATRIX_WAVE * MATRIX_AW], C[MATRIX_WAVE * MATRIX_CW];
  uint32_t idx[MATRIX_WAVE], scale_a[MATRIX_WAVE], scale_b[MATRIX_WAVE];
  uint32_t D[MATRIX_WAVE * MATRIX_CW];
};

template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(ApplyIo* io) {
  using W = Words<OP>;
  using CT = typename Acc<OP>::type;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t a[MATRIX_AW] = {}, b[MATRIX_AW] = {}, cw[W::c];
#pragma unroll
  for (int w = 0; w < W::a; ++w) a[w] = io->A[lane * MATRIX_AW + w];
#pragma unroll
  for (int w = 0; w < W::b; ++w) b[w] = io->B[lane * MATRIX_AW + w];
#pragma unroll
  for (int w = 0; w < W::c; ++w) cw[w] = io->C[lane * MATRIX_CW + w];
  const CT d = mfma<OP>(a, b, as<CT>(cw), static_cast<int>(io->idx[lane]), static_cast<int>(io->scale_a[lane]),
                        static_cast<int>(io->scale_b[lane]));
  uint32_t out[W::c];
  __builtin_memcpy(out, &d, sizeof out);
#pragma unroll
  for (int w = 0; w < W::c; ++w) io->D[lane * MATRIX_CW + w] = out[w];
}

struct Launch {
  const MatrixOperands* in;
  int iters, flip_block, skip_block, skip_step;
  Report* rep;
  unsigned long long* map;
  unsigned blocks;
};

template <int OP>
void launch_op(const Launch& l) {
  hipLaunchKernelGGL(matrix_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.in, l.iters, l.flip_block,
                     l.skip_block, l.skip_step, l.rep, l.map);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(matrix_kernel<OP>));
}
template <int OP>
void launch_apply(ApplyIo* io) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, io);
}

// the tables from op index to instantiation
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const Launch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(ApplyIo*) = {launch_apply<OP>...};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, MATRIX_OPS>()));

}  // namespace

extern "C" {

const char* matrix_last_error(void) { return g_err.c_str(); }

int matrix_device_count(void) { return device_count(); }

int matrix_slots(void) { return SIMD_ROWS; }  // rows of matrix_test's simd_map

// Every op of `ops` (n_ops indices into MATRIX_OP_TABLE), one after the other, on `blocks` workgroups of 4 waves (0: 2
// per CU), `iters` rounds of MATRIX_STEPS dependent instructions: a checked warm-up launch, then `reps` timed and
// checked launches.  The result arrays hold MATRIX_OPS entries, indexed by op.  Per op k: errors[k] = wrong elements
// over all its launches; first_where[k] = row << 16 | lane << 8 | register element of one wrong element of the first
// launch that had any (~0: none), got[k] / want[k] that element's bits and the model's; ms[k] the mean time of a timed
// launch.  simd_map: matrix_slots() x 3 (waves run, wrong elements, summed wall_clock64 ticks) per physical SIMD
// (simd_row()), added up over every launch of every op.
//
// Refused with -2 and a message: a bad device, blocks < 0, iters outside 1..2^20, reps < 1, no op, an unknown or
// repeated op, a hook outside the ops or the grid, operands the model refuses; with -3: a kernel built with a scratch
// segment or an LDS allocation (it would test memory, not the matrix core).
//
// Self-check hooks, off by default (inject_op -1), both acting in the warm-up launch of op `inject_op`, on wave 0 of
// workgroup `inject_block`:
//   flip  (inject_skip_step < 0): one bit of lane 0's register 0 of the last round's accumulator is flipped before the
//         compare: 1 wrong element, got = want ^ 0x10
//   skip  (inject_skip_step 0..3): the wave leaves that one instruction out of its last round; wrong elements > 0
int matrix_test(int device, int blocks, int iters, int reps, const int* ops, int n_ops, uint64_t seed, int inject_op,
                int inject_block, int inject_skip_step, unsigned long long* errors, unsigned long long* first_where,
                unsigned long long* got, unsigned long long* want, double* ms, unsigned long long* simd_map,
                int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || iters < 1 || iters > MAX_ITERS || reps < 1 ||
      !op_list_known(ops, n_ops, MATRIX_OPS, true)) {
    g_err = "matrix test: need a valid device, blocks >= 0 (0: 2 per CU), iters 1..2^20, reps >= 1 and a list of "
            "distinct known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (!op_list_has_hook(ops, n_ops, inject_op) ||
      (inject_op >= 0 && !hook_in_range(inject_block, grid, inject_skip_step, MATRIX_STEPS))) {
    g_err = "matrix test: inject_op must be among the ops, inject_block inside the grid and inject_skip_step below 4";
    return -2;
  }
  for (int k = 0; k < MATRIX_OPS; ++k) {
    errors[k] = got[k] = want[k] = 0;
    first_where[k] = ~0ULL;
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf din;
  HIP_CHECK(din.alloc(device, sizeof(MatrixOperands)));
  std::vector<MatrixOperands> host(1);
  for (int i = 0; i < n_ops; ++i) {
    const int k = ops[i];
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse_memory("matrix test", MATRIX_OP_TABLE[k].name, attr,
                                     ": it would test memory, not the matrix core"))
      return rc;
    if (const int rc = matrix_expect(k, seed, 0, -1, host.data()); rc < 0) {
      g_err = std::string("matrix test: the model refuses the operands of ") + MATRIX_OP_TABLE[k].name + " (" +
              std::to_string(rc) + ")";
      return -2;
    }
    HIP_CHECK(hipMemcpy(din.ptr, host.data(), sizeof(MatrixOperands), hipMemcpyHostToDevice));
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_step);
      AllOps::launch[k]({static_cast<const MatrixOperands*>(din.ptr), iters, h.flip_block, h.skip_block, h.skip_at, run.rep(),
                         run.map(), grid});
    };
    if (const int rc = run.series(reps, enqueue, errors + k, rec, ms + k)) return rc;
    first_where[k] = rec[0], got[k] = rec[2], want[k] = rec[3];
  }
  return run.read_map(simd_map);
}

// One application of op `op` by one wave of `device`, on raw per-lane registers: a and b hold MATRIX_AW (8) words per
// lane, c and d MATRIX_CW (16); idx, scale_a, scale_b one word per lane (read by the ops that have them).  d = the
// accumulator registers after the instruction.
int matrix_apply(int device, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* idx,
                 const uint32_t* scale_a, const uint32_t* scale_b, uint32_t* d) {
  const int n = device_count();
  if (device < 0 || device >= n || op < 0 || op >= MATRIX_OPS) {
    g_err = "matrix apply: need a valid device and an op of the table";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  std::vector<ApplyIo> host(1);
  ApplyIo& h = host[0];
  __builtin_memcpy(h.A, a, sizeof h.A);
  __builtin_memcpy(h.B, b, sizeof h.B);
  __builtin_memcpy(h.C, c, sizeof h.C);
  __builtin_memcpy(h.idx, idx, sizeof h.idx);
  __builtin_memcpy(h.scale_a, scale_a, sizeof h.scale_a);
  __builtin_memcpy(h.scale_b, scale_b, sizeof h.scale_b);
  __builtin_memset(h.D, 0, sizeof h.D);
  DevBuf io;
  HIP_CHECK(io.alloc(device, sizeof(ApplyIo)));
  HIP_CHECK(hipMemcpy(io.ptr, &h, sizeof h, hipMemcpyHostToDevice));
  AllOps::apply[op](static_cast<ApplyIo*>(io.ptr));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(&h, io.ptr, sizeof h, hipMemcpyDeviceToHost));
  __builtin_memcpy(d, h.D, sizeof h.D);
  return 0;
}

}  // extern "C"
