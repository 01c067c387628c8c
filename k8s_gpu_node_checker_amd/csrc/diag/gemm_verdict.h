// The host half of the GEMM diagnostics' verdict, free of any HIP call: the E4M3 decode of the reference kernels,
// the sample positions, what a bf16 output's rounding forgives, the whole-output checksum verdict over host arrays
// and the sampled-error reduction.  gemm_check.h (the device side) and gemm_host.h / diag.hip (the runners) call
// these.  Plain C++ on tile_order.h, no HIP include: tests/test_gemm_verdict_cpu.py compiles it with the host compiler.
#ifndef K8S_GPU_NODE_CHECKER_AMD_GEMM_VERDICT_H_
#define K8S_GPU_NODE_CHECKER_AMD_GEMM_VERDICT_H_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "tile_order.h"

// the reference kernels decode on the device, the host compiler reads the same text
#if defined(__HIPCC__)
#define GEMM_VERDICT_HD __host__ __device__
#else
#define GEMM_VERDICT_HD
#endif

namespace {

// The value of an OCP E4M3 (float8_e4m3fn) byte: 4 exponent bits (bias 7), 3 mantissa bits, subnormals m / 8 * 2^-6
// at exponent field 0, no infinities; 0x7F / 0xFF are the format's NaN.
GEMM_VERDICT_HD inline double e4m3_value(uint8_t b) {
  const int e = (b >> 3) & 15, m = b & 7;
  if (e == 15 && m == 7) return std::numeric_limits<double>::quiet_NaN();
  const double v = e == 0 ? m / 8.0 * 0.015625 : (1.0 + m / 8.0) * ldexp(1.0, e - 7);
  return (b & 0x80) ? -v : v;
}

// Output tiles of a launch and the group_m of their blockIdx regrouping (tile_order.h, which also maps a tile back
// to the XCD that computed it: tile_xcds).
struct TileGeom {
  int rows, cols, group_m;
};

// |got - ref| beyond the rounding of a bf16 output (at most half an ulp: 2^-8 of |value|, with margin), so the
// sampled checks of the bf16-output kernel keep the tolerances of the fp32 one
// (a NaN stays NaN: std::max would turn it into 0)
inline double beyond_bf16_rounding(double got, double ref) {
  const double e = std::fabs(got - ref) - std::ldexp(std::max(std::fabs(got), std::fabs(ref)), -8) * 1.01;
  return e > 0.0 || std::isnan(e) ? e : 0.0;
}

// The `nsamp` (row, column) pairs of an M x N output that a diagnostic run checks against its reference kernel
inline void sample_indices(uint64_t seed, int nsamp, int M, int N, std::vector<int>& rows, std::vector<int>& cols) {
  rows.resize(nsamp);
  cols.resize(nsamp);
  uint64_t x = seed;
  for (int i = 0; i < nsamp; ++i) {
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    rows[i] = static_cast<int>((x >> 33) % static_cast<uint64_t>(M));
    x = x * 6364136223846793005ULL + 1442695040888963407ULL;
    cols[i] = static_cast<int>((x >> 33) % static_cast<uint64_t>(N));
  }
}

// The sampled check's result: the worst |got - ref| over its denominator, max(1, |ref|) for the fp32 reference
// (`by_mag` false) or the sample's sum |a*b| (`by_mag`: mag[] is read).  With `fused` (bf16 C) the error is what lies
// beyond the output's own rounding.  A NaN difference gives HUGE_VAL.
inline double sampled_worst(const float* got, const double* ref, const double* mag, int nsamp, bool fused,
                            bool by_mag) {
  double worst = 0.0;
  for (int i = 0; i < nsamp; ++i) {
    const double d = fused ? beyond_bf16_rounding(got[i], ref[i]) : std::fabs(static_cast<double>(got[i]) - ref[i]);
    const double denom = by_mag ? std::max(mag[i], 1e-30) : std::max(1.0, std::fabs(ref[i]));
    worst = std::max(worst, std::isnan(d) ? HUGE_VAL : d / denom);
  }
  return worst;
}

// Whole-output verdict over host arrays.  ref / mag are [nblk][N] (one row per tile-high block of rows); csum is
// [nblk * halves][N], the `halves` partial column sums of a row block in consecutive rows (the fused kernels give one
// per 128 rows: 2 for a 256-row tile), added here in fp64; out_csum (optional, [nblk][N]) receives the sums judged.
// ck_out[0] bad tiles, [1] bad columns, [2..9] bad tiles per XCD, [10] / [11] the first bad tile's (row, column) in
// tiles or -1; *max_err the worst |csum - ref| / mag.  A column fails when that exceeds tol; a NaN or infinite sum
// counts as bad and makes *max_err infinite.  *floor_out (optional) = tol * the largest mag of any column: an output
// wrong by more than that (plus the healthy residual) is flagged whichever column it is in.
constexpr int kCkOut = 12;
inline void checksum_verdict(const double* ref, const double* mag, const double* csum, int halves, int nblk, int N,
                             TileGeom g, double tol, double* max_err, long long* ck_out, double* floor_out,
                             double* out_csum = nullptr) {
  const int tiles_n = N / g.cols;
  const size_t cnt = static_cast<size_t>(nblk) * N;
  const std::vector<int> xcd = tile_xcds(nblk, tiles_n, g.group_m);
  std::vector<char> bad(static_cast<size_t>(nblk) * tiles_n, 0);
  double worst = 0.0, max_mag = 0.0;
  long long cols = 0;
  for (size_t i = 0; i < cnt; ++i) {
    const size_t tb = i / N, j = i % N;
    double sum = 0.0;
    for (int h = 0; h < halves; ++h) sum += csum[(tb * halves + h) * N + j];
    if (out_csum != nullptr) out_csum[i] = sum;
    max_mag = std::max(max_mag, mag[i]);
    const double e = std::fabs(sum - ref[i]) / std::max(mag[i], 1e-30);
    if (!(e <= tol)) {  // also NaN
      ++cols;
      bad[tb * tiles_n + j / g.cols] = 1;
    }
    worst = std::isfinite(e) ? std::max(worst, e) : HUGE_VAL;
  }
  for (int i = 0; i < kCkOut; ++i) ck_out[i] = 0;
  ck_out[1] = cols;
  ck_out[10] = ck_out[11] = -1;
  for (size_t t = 0; t < bad.size(); ++t) {
    if (!bad[t]) continue;
    ++ck_out[0];
    if (xcd[t] >= 0) ++ck_out[2 + xcd[t]];
    if (ck_out[10] < 0) {
      ck_out[10] = static_cast<long long>(t / tiles_n);
      ck_out[11] = static_cast<long long>(t % tiles_n);
    }
  }
  *max_err = worst;
  if (floor_out != nullptr) *floor_out = tol * max_mag;
}

}  // namespace

#endif  // K8S_GPU_NODE_CHECKER_AMD_GEMM_VERDICT_H_
