// The bf16 / fp8 / fp4 MFMA GEMM kernels, one header per generation.  The order is the order of the kernel
// definitions in the translation unit.
#pragma once

#include "gemm_common.h"
#include "gemm_v1.h"
#include "gemm_v2.h"
#include "gemm_v3.h"
#include "gemm_v4.h"
