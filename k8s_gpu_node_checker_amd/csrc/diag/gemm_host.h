// Host side of the GEMM diagnostics: the per-thread knobs, the launch dispatch over the kernel variants, the
// whole-output checksum runner and the self-check hooks on the output.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../common/hip_host.h"
#include "gemm_check.h"
#include "gemm_kernels.h"
#include "gemm_verdict.h"

namespace {

// GEMM knobs are per calling thread: the node agent runs one diagnostic thread per GPU at once, and a
// test or tool that switches a variant must not change what another GPU's thread launches.
thread_local int g_gemm_variant = 0;
thread_local int g_gemm_schedule = 1;  // v3 restaging order (V3_PHASE): 1 = LDS-DMA pieces per phase 0/2/2/4, 0 = 2/0/4/2
thread_local int g_gemm_buffer_loads = 0;  // v3 operand staging: 0 = global_load_lds, 1 = buffer_load ... lds
// fp8 v3 MFMA: 1 = the unscaled v_mfma_f32_16x16x128_f8f6f4 (hipBLASLt's fp8 form, the default: +5.6 % over the
// scaled form at 4096^3 and 8192^3 with bit-identical C, profiles/gemm_fp8_mfma_ab_mi355x.jsonl), 0 = the
// v_mfma_scale_..._f8f6f4 MX path with unit E8M0 scales (kept for A/B)
thread_local int g_gemm_fp8_unscaled = 1;
// v4 bf16: a short last wave of 256^2 tiles runs as 128^2 quadrants (gemm_v4_tail_kernel; 0 = off, for A/B)
thread_local int g_gemm_tail = 1;
thread_local int g_gemm_epilogue = 1;  // 0 = direct 4-byte stores, 1 = LDS-staged 16-byte row pieces (v3
                                       // kernels; measured +2..12 %, profiles/gemm_fp8_mi355x.jsonl)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: it is set once for
// every (kernel, device) pair, on the device current to the calling thread, before that pair's first
// launch.  Devices run concurrently (one agent thread per GPU, up to 64 in CPX), hence one once_flag per
// ordinal rather than one process-wide bool.
constexpr int kMaxDevices = 256;
struct LdsAttrOnce {
  std::once_flag once[kMaxDevices];
  hipError_t result[kMaxDevices] = {};
};

int ensure_dynamic_lds(LdsAttrOnce& slot, const void* kernel, int bytes, const char* what) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) {
    HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
  }
  std::call_once(slot.once[dev], [&] {
    slot.result[dev] = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  });
  if (slot.result[dev] != hipSuccess) {
    g_err = std::string(what) + ": hipFuncSetAttribute(MaxDynamicSharedMemorySize) on device " +
            std::to_string(dev) + ": " + hipGetErrorString(slot.result[dev]);
    return -1;
  }
  return 0;
}

template <int DT, bool EPI, bool BUF, int SCHED = 1, int OUT = OUT_F32, bool PRIO = DT == DT_BF16 || DT == DT_FP8U>
int launch_v3_inst(const void* A, const void* Bt, void* C, double* csum, int M, int N, int Kcols,
                   hipStream_t stream) {
  static LdsAttrOnce attr;
  if (ensure_dynamic_lds(attr, reinterpret_cast<const void*>(gemm_v3_kernel<DT, EPI, BUF, SCHED, OUT, PRIO>),
                         2 * V2_STAGE_BYTES, "gemm v3") != 0)
    return -1;
  const int nwg = (M / V2_BM) * (N / V2_BN);
  hipLaunchKernelGGL((gemm_v3_kernel<DT, EPI, BUF, SCHED, OUT, PRIO>), dim3(nwg), dim3(V2_THREADS),
                     2 * V2_STAGE_BYTES, stream, static_cast<const __bf16*>(A), static_cast<const __bf16*>(Bt), C,
                     csum, M, N, Kcols);
  return 0;
}
template <int DT, bool EPI, bool BUF, int SCHED = 1>
int launch_v3_inst(const void* A, const void* Bt, float* C, int M, int N, int Kcols, hipStream_t stream) {
  return launch_v3_inst<DT, EPI, BUF, SCHED, OUT_F32>(A, Bt, C, nullptr, M, N, Kcols, stream);
}

// bf16 C + fused 128-row column sums (OUT_BF16_CK), restaging order per g_gemm_schedule
template <int DT>
int launch_v3_ck(const void* A, const void* Bt, __bf16* C, double* csum, int M, int N, int Kcols,
                 hipStream_t stream) {
  return g_gemm_schedule == 0
             ? launch_v3_inst<DT, true, false, 0, OUT_BF16_CK>(A, Bt, C, csum, M, N, Kcols, stream)
             : launch_v3_inst<DT, true, false, 1, OUT_BF16_CK>(A, Bt, C, csum, M, N, Kcols, stream);
}

// fp8 operands on the MFMA form the thread's knob picks (g_gemm_fp8_unscaled); the unscaled form raises the second
// wave group's priority as the bf16 kernel does
int launch_v3_ck_fp8(const void* A, const void* Bt, __bf16* C, double* csum, int M, int N, int Kcols,
                     hipStream_t stream) {
  return g_gemm_fp8_unscaled ? launch_v3_ck<DT_FP8U>(A, Bt, C, csum, M, N, Kcols, stream)
                             : launch_v3_ck<DT_FP8>(A, Bt, C, csum, M, N, Kcols, stream);
}

// v4 launch (bf16; M, N multiples of 256, K of 64): fp32 C, or bf16 C + fused column sums (OUT_BF16_CK)
template <int OUT, bool TR, int DT>
int launch_v4_inst(const void* A, const void* Bt, void* C, double* csum, int M, int N, int K, hipStream_t stream) {
  using Plan = std::conditional_t<DT == DT_FP8U, V4PlanF8<8, 10, 26, 27, 42>, V4PlanA<1, 20, 8, 8, 2>>;
  constexpr auto kern = gemm_v4_kernel<OUT, Plan, 4, TR, DT>;
  if (static_cast<uint64_t>(V2_BM) * static_cast<uint64_t>(K) * 2 >= (1ull << 32)) {
    // the buffer resources cover a 256-row panel with 32-bit byte offsets
    g_err = "gemm v4: a 256-row operand panel must stay under 4 GiB (K < 8,388,608 bf16 columns)";
    return -2;
  }
  static LdsAttrOnce attr;
  if (ensure_dynamic_lds(attr, reinterpret_cast<const void*>(kern), 2 * V2_STAGE_BYTES, "gemm v4") != 0) return -1;
  const int nwg = (M / V2_BM) * (N / V2_BN);
  // a short last wave: v4 on the whole waves, the rest as 128^2 quadrants (gemm_v4_tail_kernel)
  const bool tail = g_gemm_tail && v4_tail_applies(nwg);
  const int main_wg = tail ? v4_tail_main(nwg) : nwg;
  hipLaunchKernelGGL(kern, dim3(main_wg), dim3(V4_THREADS), 2 * V2_STAGE_BYTES, stream, static_cast<const __bf16*>(A),
                     static_cast<const __bf16*>(Bt), C, csum, M, N, K);
  if (tail)
    hipLaunchKernelGGL((gemm_v4_tail_kernel<OUT, 4, DT>), dim3(4 * (nwg - main_wg)), dim3(THREADS), 0, stream,
                       static_cast<const u32x4*>(A), static_cast<const u32x4*>(Bt), C, csum, M, N, K);
  return 0;
}
// v4 with the LDS-patch epilogue (variant 4) or the transposed, register-direct one (variant 5); K in bf16 columns
// (fp8: row bytes / 2)
template <int OUT, int DT = DT_BF16>
int launch_v4(int variant, const void* A, const void* Bt, void* C, double* csum, int M, int N, int K,
              hipStream_t stream) {
  return variant == 5 ? launch_v4_inst<OUT, true, DT>(A, Bt, C, csum, M, N, K, stream)
                      : launch_v4_inst<OUT, false, DT>(A, Bt, C, csum, M, N, K, stream);
}

// The fp8 kernel the calling thread's knobs select: v4 (4 or 5) for auto / v4 / v4t with the unscaled MFMA, else v3
int fp8_variant() {
  const int v = g_gemm_variant == 0 ? 4 : g_gemm_variant;
  return v >= 4 && g_gemm_fp8_unscaled ? v : 3;
}

// fp8 bf16 C + fused column sums on the selected kernel (Kcols = row bytes / 2)
int launch_fp8_ck(const void* A, const void* Bt, __bf16* C, double* csum, int M, int N, int Kcols,
                  hipStream_t stream) {
  const int v = fp8_variant();
  return v >= 4 ? launch_v4<OUT_BF16_CK, DT_FP8U>(v, A, Bt, C, csum, M, N, Kcols, stream)
                : launch_v3_ck_fp8(A, Bt, C, csum, M, N, Kcols, stream);
}

// The diagnostic runs (diag_gemm_bf16 / diag_gemm_fp8 in diag.hip) take the bf16-output kernel wherever the production v3 configuration
// would run (LDS-staged epilogue, global_load_lds staging); other knob settings keep fp32 C.  v4 has one
// configuration, always LDS-staged: it always has the bf16 output.
bool v3_ck_path() { return g_gemm_epilogue == 1 && !g_gemm_buffer_loads; }

// v3 launch (M, N multiples of 256; Kcols = bf16 columns, K8 / 2 for fp8), epilogue per g_gemm_epilogue,
// operand staging per g_gemm_buffer_loads, restaging order per g_gemm_schedule (the buffer path: order 1)
template <int DT>
int launch_v3(const void* A, const void* Bt, float* C, int M, int N, int Kcols, hipStream_t stream) {
  if (g_gemm_buffer_loads)
    return g_gemm_epilogue ? launch_v3_inst<DT, true, true>(A, Bt, C, M, N, Kcols, stream)
                           : launch_v3_inst<DT, false, true>(A, Bt, C, M, N, Kcols, stream);
  if (g_gemm_schedule == 0)
    return g_gemm_epilogue ? launch_v3_inst<DT, true, false, 0>(A, Bt, C, M, N, Kcols, stream)
                           : launch_v3_inst<DT, false, false, 0>(A, Bt, C, M, N, Kcols, stream);
  return g_gemm_epilogue ? launch_v3_inst<DT, true, false, 1>(A, Bt, C, M, N, Kcols, stream)
                         : launch_v3_inst<DT, false, false, 1>(A, Bt, C, M, N, Kcols, stream);
}

// The bf16 kernel diag_gemm_bf16_launch runs for M x N: 1 = v1 (128^2 tiles), 2 = v2, 3 = v3, 4 = v4 (256^2).
// v2-v4 need 256-multiples and enough 256^2 tiles to occupy the 256 CUs (one block per CU); below that the 128^2
// kernel's 4x larger grid wins (measured: 2048^3 v1 543 vs v2 321 TFLOP/s).
int bf16_variant(int M, int N) {
  const bool big_ok = M % V2_BM == 0 && N % V2_BN == 0 && (M / V2_BM) * (N / V2_BN) >= 256;
  return g_gemm_variant == 0 ? (big_ok ? 4 : 1) : g_gemm_variant;
}

// the bf16 launch with bf16 C + fused column sums: v4 when the thread's variant resolves to it, else v3
int launch_bf16_ck(const void* A, const void* Bt, __bf16* C, double* csum, int M, int N, int K, hipStream_t stream) {
  const int v = bf16_variant(M, N);
  return v >= 4 ? launch_v4<OUT_BF16_CK>(v, A, Bt, C, csum, M, N, K, stream)
                : launch_v3_ck<DT_BF16>(A, Bt, C, csum, M, N, K, stream);
}

// Does the diagnostic run of `dt` (DT_BF16 / DT_FP8) at M x N write bf16 C with fused column sums (else fp32 C)?
// The one answer for the runners, diag_gemm_ck_path and whoever calls diag_gemm_launch_ck.
bool gemm_fused(int dt, int M, int N) {
  const int v = dt == DT_FP8 ? fp8_variant() : bf16_variant(M, N);
  return v >= 4 || (v == 3 && v3_ck_path());
}

// The tiles of the 128^2 kernel (v1) and of the 256^2 ones (TileGeom: gemm_verdict.h)
constexpr TileGeom kGeomV1{BM, BN, 8}, kGeomV3{V2_BM, V2_BN, 4};

// Whole-output check of C = A . Bt^T: the ck_* kernels form ref, mag and (fp32 C) the column sums, and
// checksum_verdict (gemm_verdict.h, which documents *max_err, ck_out[kCkOut] and *floor_out) judges them on the host.
// With `fused` (the OUT_BF16_CK kernel's csum[M / 128][N], device memory) the column sums come from the
// kernel itself, its 128-row halves added per tile row in fp64, and C is not read.  out_ref / out_mag / out_csum
// (optional, host, [M / g.rows][N] each) receive what was judged.
template <int DT>
int gemm_checksum(int device, const void* A, const void* Bt, const float* C, int M, int N, int K, TileGeom g,
                  double tol, double* max_err, long long* ck_out, const double* fused = nullptr,
                  double* floor_out = nullptr, double* out_ref = nullptr, double* out_mag = nullptr,
                  double* out_csum = nullptr) {
  const int rb = g.rows;
  const int nblk = M / rb;
  const size_t kb = sizeof(double) * static_cast<size_t>(nblk) * K, nb = sizeof(double) * static_cast<size_t>(nblk) * N;
  DevBuf asum, aabs, ref, mag, csum;
  HIP_CHECK(asum.alloc(device, kb));
  HIP_CHECK(aabs.alloc(device, kb));
  HIP_CHECK(ref.alloc(device, nb));
  HIP_CHECK(mag.alloc(device, nb));
  if (!fused) HIP_CHECK(csum.alloc(device, nb));
  double* as = static_cast<double*>(asum.ptr);
  double* am = static_cast<double*>(aabs.ptr);
  hipLaunchKernelGGL(ck_asum_kernel<DT>, dim3((K + 255) / 256, nblk), dim3(256), 0, nullptr, A, as, am, K, rb);
  hipLaunchKernelGGL(ck_ref_kernel<DT>, dim3((N + 255) / 256, (nblk + CK_TB - 1) / CK_TB), dim3(256), 0, nullptr, Bt,
                     as, am, static_cast<double*>(ref.ptr), static_cast<double*>(mag.ptr), N, K, nblk);
  if (!fused)
    hipLaunchKernelGGL(ck_csum_kernel, dim3((N + 255) / 256, nblk), dim3(256), 0, nullptr, C,
                       static_cast<double*>(csum.ptr), N, rb);
  HIP_CHECK(hipGetLastError());
  const size_t cnt = static_cast<size_t>(nblk) * N;
  const int halves = fused ? rb / 128 : 1;
  std::vector<double> hr(cnt), hm(cnt), hc(cnt * halves);
  HIP_CHECK(hipMemcpy(hr.data(), ref.ptr, nb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hm.data(), mag.ptr, nb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hc.data(), fused ? fused : csum.ptr, nb * halves, hipMemcpyDeviceToHost));
  checksum_verdict(hr.data(), hm.data(), hc.data(), halves, nblk, N, g, tol, max_err, ck_out, floor_out, out_csum);
  if (out_ref != nullptr) std::copy(hr.begin(), hr.end(), out_ref);
  if (out_mag != nullptr) std::copy(hm.begin(), hm.end(), out_mag);
  return 0;
}

// A test hook: overwrite output element `elem` of C with 1e6 (an error every check must see) or, with a `delta`
// that is not NaN, with its own value plus delta (the smallest error the checksums must see).
hipError_t inject_output(float* C, long long elem, long long count, double delta) {
  if (elem < 0 || elem >= count) return hipSuccess;
  float v = 1e6f;
  if (!std::isnan(delta)) {
    float old;
    const hipError_t e = hipMemcpy(&old, C + elem, sizeof(old), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    v = static_cast<float>(static_cast<double>(old) + delta);
  }
  return hipMemcpy(C + elem, &v, sizeof(v), hipMemcpyHostToDevice);
}

// The same for the bf16-output kernel: the element becomes 1e6 in C and in its 128-row block's fused column
// sum, as if the matrix core had produced that value.  With `delta` the fused sum (formed from the fp32
// accumulators, before the rounding) moves by exactly delta and C holds the rounded old + delta.
hipError_t inject_output_ck(__bf16* C, double* csum, long long elem, int M, int N, double delta) {
  if (elem < 0 || elem >= static_cast<long long>(M) * N) return hipSuccess;
  __bf16 old;
  hipError_t e = hipMemcpy(&old, C + elem, sizeof(old), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  const bool by_delta = !std::isnan(delta);
  const __bf16 v = static_cast<__bf16>(by_delta ? static_cast<float>(static_cast<float>(old) + delta) : 1e6f);
  if ((e = hipMemcpy(C + elem, &v, sizeof(v), hipMemcpyHostToDevice)) != hipSuccess) return e;
  double* cs = csum + (elem / N) / 128 * N + elem % N;
  double sum;
  if ((e = hipMemcpy(&sum, cs, sizeof(sum), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  sum += by_delta ? delta : static_cast<double>(static_cast<float>(v)) - static_cast<double>(static_cast<float>(old));
  return hipMemcpy(cs, &sum, sizeof(sum), hipMemcpyHostToDevice);
}

}  // namespace
