// Vector types and GEMM enumerations that several parts of the diagnostics share.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // native 16-byte vector (SROA-friendly, unlike uint4)
typedef int i32x8 __attribute__((ext_vector_type(8)));            // 32 fp8 / 64 fp4 operand bytes

// operand type and output form of the GEMM kernels (template arguments; DT_BF16 / DT_FP8 are also the C ABI's `dt`);
// the forms are described at gemm_v3_kernel
enum GemmDtype { DT_BF16 = 0, DT_FP8 = 1, DT_FP4 = 2, DT_FP8U = 3 /* fp8 operands, unscaled MFMA */ };
enum GemmOut { OUT_F32 = 0, OUT_BF16_CK = 1 };

}  // namespace
