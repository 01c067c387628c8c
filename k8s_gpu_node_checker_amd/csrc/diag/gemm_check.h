// What the GEMM runs are checked with: the operand fills, the sampled reference kernels and the whole-output
// tile checksums.
#pragma once

#include <cmath>
#include <cstdint>

#include "../common/hip_host.h"
#include "gemm_verdict.h"
#include "types.h"

namespace {

// fp32 reference for sampled outputs: one thread per (row, col) sample.
__global__ void gemm_ref_kernel(const __bf16* A, const __bf16* Bt, const int* rows, const int* cols, float* out,
                                int nsamp, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsamp) return;
  const __bf16* a = A + static_cast<size_t>(rows[i]) * K;
  const __bf16* b = Bt + static_cast<size_t>(cols[i]) * K;
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += static_cast<float>(a[k]) * static_cast<float>(b[k]);
  out[i] = s;
}

template <typename T>
__global__ void gather_kernel(const T* C, const int* rows, const int* cols, float* out, int nsamp, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nsamp) out[i] = static_cast<float>(C[static_cast<size_t>(rows[i]) * N + cols[i]]);
}

// Deterministic pseudo-random bf16 in [-1, 1]: the fp32 value lies in [-1, 1), and the hashes within 2^-9 of the
// top round to bf16 1.0.
__global__ void fill_bf16_kernel(__bf16* p, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const uint32_t h = mix32(i * 0x9E3779B97F4A7C15ULL + seed);
    p[i] = static_cast<__bf16>((h >> 8) * (2.0f / 16777216.0f) - 1.0f);
  }
}

// Finite OCP E4M3 bytes (exponent field <= 8, so |x| < 4 and no NaN encoding), hashed from the index.
__global__ void fill_fp8_kernel(uint8_t* p, size_t n, uint64_t seed) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ULL ^ seed;
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ULL;
    h ^= h >> 29;
    const uint32_t e = static_cast<uint32_t>(h % 9), m = static_cast<uint32_t>((h >> 8) & 7), s = (h >> 12) & 1;
    p[i] = static_cast<uint8_t>((s << 7) | (e << 3) | m);
  }
}

// fp64 reference (operands decoded by gemm_verdict.h's e4m3_value) of sampled fp8 outputs, plus sum |a*b| (the scale of the MX MFMA's accumulation error)
__global__ void gemm_ref_fp8_kernel(const uint8_t* A, const uint8_t* Bt, const int* rows, const int* cols,
                                    double* out, double* mag, int nsamp, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsamp) return;
  const uint8_t* a = A + static_cast<size_t>(rows[i]) * K;
  const uint8_t* b = Bt + static_cast<size_t>(cols[i]) * K;
  double acc = 0.0, m = 0.0;
  for (int k = 0; k < K; ++k) {
    const double p = e4m3_value(a[k]) * e4m3_value(b[k]);
    acc += p;
    m += fabs(p);
  }
  out[i] = acc;
  mag[i] = m;
}

// ---------------------------------------------------------------- whole-output GEMM check
// The sampled check above reads 4,096 of the 67 M outputs of an 8192^2 GEMM: a matrix core that corrupts the
// tiles of one workgroup slot is found only if a sample lands there.  Checksums cover every output at the cost
// of one pass over C (Huang & Abraham's algorithm-based fault tolerance): for each tile-high block of rows tb,
// sum_i C[i][j] (i in tb) must equal sum_k (sum_i A[i][k]) Bt[j][k].  Both sides are formed in fp64 from the
// exact operand values, so the only difference is the GEMM's own fp32 rounding, bounded by
// mag[tb][j] = sum_k (sum_i |A[i][k]|) |Bt[j][k]|; a column whose difference exceeds tol * mag marks the tile
// (tb, j / tile width) bad, and the launch's blockIdx -> tile order names the XCD that computed it.
template <int DT>
__device__ __forceinline__ double ck_value(const void* p, size_t i) {
  if constexpr (DT == DT_BF16) return static_cast<double>(static_cast<const __bf16*>(p)[i]);
  else return e4m3_value(static_cast<const uint8_t*>(p)[i]);
}

// asum[tb][k] = sum of the RB rows of block tb in column k, aabs the same over |A|; thread per column (coalesced)
template <int DT>
__global__ void __launch_bounds__(256) ck_asum_kernel(const void* A, double* asum, double* aabs, int K, int RB) {
  const int k = blockIdx.x * 256 + threadIdx.x, tb = blockIdx.y;
  if (k >= K) return;
  double s = 0.0, m = 0.0;
  for (int i = 0; i < RB; ++i) {
    const double v = ck_value<DT>(A, static_cast<size_t>(tb * RB + i) * K + k);
    s += v;
    m += fabs(v);
  }
  asum[static_cast<size_t>(tb) * K + k] = s;
  aabs[static_cast<size_t>(tb) * K + k] = m;
}

// ref[tb][j] = asum[tb] . Bt[j], mag[tb][j] = aabs[tb] . |Bt[j]|: thread per column j, CK_TB row blocks per
// workgroup, Bt staged through LDS 32 k at a time (coalesced along k; the +1 pad keeps the column reads apart)
constexpr int CK_TB = 8, CK_KC = 32;
template <int DT>
__global__ void __launch_bounds__(256) ck_ref_kernel(const void* Bt, const double* asum, const double* aabs,
                                                     double* ref, double* mag, int N, int K, int nblk) {
  __shared__ float bs[256][CK_KC + 1];
  __shared__ double as[CK_TB][CK_KC], am[CK_TB][CK_KC];
  const int tid = threadIdx.x, j0 = blockIdx.x * 256, tb0 = blockIdx.y * CK_TB;
  double r[CK_TB], g[CK_TB];
#pragma unroll
  for (int t = 0; t < CK_TB; ++t) r[t] = g[t] = 0.0;
  for (int k0 = 0; k0 < K; k0 += CK_KC) {
    for (int idx = tid; idx < 256 * CK_KC; idx += 256) {
      const int row = idx / CK_KC, kk = idx % CK_KC;
      bs[row][kk] = j0 + row < N ? static_cast<float>(ck_value<DT>(Bt, static_cast<size_t>(j0 + row) * K + k0 + kk))
                                 : 0.f;
    }
    for (int idx = tid; idx < CK_TB * CK_KC; idx += 256) {
      const int t = idx / CK_KC, kk = idx % CK_KC;
      const bool ok = tb0 + t < nblk;
      as[t][kk] = ok ? asum[static_cast<size_t>(tb0 + t) * K + k0 + kk] : 0.0;
      am[t][kk] = ok ? aabs[static_cast<size_t>(tb0 + t) * K + k0 + kk] : 0.0;
    }
    __syncthreads();
    for (int kk = 0; kk < CK_KC; ++kk) {
      const double b = bs[tid][kk], bb = fabs(b);
#pragma unroll
      for (int t = 0; t < CK_TB; ++t) {
        r[t] += as[t][kk] * b;
        g[t] += am[t][kk] * bb;
      }
    }
    __syncthreads();
  }
  if (j0 + tid >= N) return;
#pragma unroll
  for (int t = 0; t < CK_TB; ++t)
    if (tb0 + t < nblk) {
      ref[static_cast<size_t>(tb0 + t) * N + j0 + tid] = r[t];
      mag[static_cast<size_t>(tb0 + t) * N + j0 + tid] = g[t];
    }
}

// csum[tb][j] = sum of the RB rows of block tb of C in column j, in fp64; thread per column (coalesced)
__global__ void __launch_bounds__(256) ck_csum_kernel(const float* C, double* csum, int N, int RB) {
  const int j = blockIdx.x * 256 + threadIdx.x, tb = blockIdx.y;
  if (j >= N) return;
  double s = 0.0;
  for (int i = 0; i < RB; ++i) s += C[static_cast<size_t>(tb * RB + i) * N + j];
  csum[static_cast<size_t>(tb) * N + j] = s;
}

}  // namespace
