// Active MI355X diagnostics (gfx950 / CDNA4 only): the "deep" health checks the
// node agent can run besides the passive amd-smi probe.  A node can be
// Ready=True with clean ECC counters and still have a GPU that computes wrong
// results, runs at a fraction of its matrix rate (stuck clocks, throttling) or
// has a weak HBM stack; these kernels measure exactly that.
//
//   gemm_bf16   C[M,N] = A[M,K] . Bt[N,K]^T, bf16 in / fp32 out on MFMA
//               (v_mfma_f32_16x16x32_bf16), XOR-swizzled LDS (conflict-free
//               ds_read_b128 fragment loads), XCD-aware tile order.
//               v4: 256x256x64 tiles, 4 waves of 128x128 each, the loop's MFMA /
//                   ds_read / LDS-DMA interleave written out in asm on a checked
//                   plan (v4_plan.h); bf16 and fp8 (16x16x128, by quadrant), the
//                   default for large GEMMs;
//               v3: the same tile, 8 waves in two barrier-staggered groups, LDS-DMA
//                   restaged region by region (MX-fp4, the scaled MX-fp8 form, and
//                   bf16 / fp8 for A/B);
//               v2: the same tile, one barrier per K-tile (kept for A/B);
//               v1: 128x128x64 tiles, 4 waves, register-staged (small grids).
//               Verified against an fp32 reference kernel on sampled outputs.
//   hbm_copy / hbm_read / hbm_write
//               16-byte nontemporal streams, 8 loads in flight per thread,
//               32 blocks per CU; TB/s against the 8 TB/s HBM3E spec.
//   memtest     address-hash patterns written and verified (plus the
//               bit-inverted pass), mismatches counted with one atomic per
//               failing 16-byte word.
//   p2p_copy    xGMI pair check: peer copies between two GPUs of the node,
//               timed, and the received pattern verified on the destination.
//   host_link   pinned host <-> device copy bandwidth over the PCIe link.
//   mfma_burn   matrix-core datapath burn-in per precision (bf16, fp8, MX-fp8,
//               MX-fp4), register-resident, every lane's exact result checked.
//   regfile     both vector register files of every SIMD (512 registers x 64
//               lanes) under four patterns, errors located to the SIMD.
//   valu_burn   vector-ALU burn-in (fp64 FMA, packed fp32 FMA, 32-bit integer
//               multiply-add), every lane bit-exact against the host (valu_ref.h).
//
// C ABI (ctypes, ops/diag.py).  Every HIP call is checked; on failure the
// function returns a negative code and diag_last_error() says what failed.
//
// This file holds the entry points (every extern "C" block) and the runners only they use.  The kernels are in
// gemm_kernels.h (gemm_common.h and gemm_v1.h to gemm_v4.h, one GEMM generation each, on tile_order.h and v4_plan.h),
// gemm_check.h, mem_kernels.h, burn_kernels.h and xcd_kernels.h, the GEMM launch dispatch in gemm_host.h, the HIP-free
// half of the GEMM verdict in gemm_verdict.h, the host helpers shared with the other libraries in ../common/hip_host.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../common/hip_host.h"
#include "gemm_kernels.h"
#include "gemm_check.h"
#include "mem_kernels.h"
#include "burn_kernels.h"
#include "xcd_kernels.h"
#include "gemm_host.h"

namespace {

// one thread per 16-byte element (grid-stride kernels launched with it run their loop once)
unsigned flat_grid(size_t n) { return static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 0x7FFFFFFFu)); }

// Self-check hook of the per-XCD readers: one bit of 32-bit word `word` of XCD `xcd`'s slice is flipped from the host
// (after the fill, before the first launch).  Returns -2 with g_err set when the word lies outside the slice.
int flip_slice_word(void* buf, uint32_t slice_vec, int xcd, long long word, const char* what) {
  if (xcd < 0) return 0;
  if (xcd > 7 || word < 0 || word >= 4LL * slice_vec) {
    g_err = std::string(what) + ": inject_xcd 0..7 and inject_word inside the slice";
    return -2;
  }
  return flip_word_bit(static_cast<uint32_t*>(buf) + 4ULL * slice_vec * static_cast<unsigned>(xcd) + word);
}

int grid_for(int device, int blocks_per_cu) { return cu_count(device) * blocks_per_cu; }

float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return -1.f;  // no time: a negative rate, which every rate check fails, rather than an infinite one
  }
  return ms;
}

// The error counter a verifying kernel adds to and, optionally, its per-slot table (`slots` rows of `cols` counters:
// where on the chip the waves ran and the errors were).
struct ErrMap {
  DevBuf cnt, tab;
  size_t map_bytes = 0;
  int alloc(int device, int slots, int cols, bool with_map = true) {
    HIP_CHECK(cnt.alloc(device, sizeof(unsigned long long)));
    if (with_map) {
      map_bytes = static_cast<size_t>(slots) * cols * sizeof(unsigned long long);
      HIP_CHECK(tab.alloc(device, map_bytes));
    }
    return 0;
  }
  unsigned long long* errors() const { return static_cast<unsigned long long*>(cnt.ptr); }
  unsigned long long* map() const { return static_cast<unsigned long long*>(tab.ptr); }  // null without a map
  int zero() {
    HIP_CHECK(hipMemset(cnt.ptr, 0, sizeof(unsigned long long)));
    if (tab.ptr) HIP_CHECK(hipMemset(tab.ptr, 0, map_bytes));
    return 0;
  }
  // copies back the counter and the table; either destination may be null
  int read(unsigned long long* errors_out, unsigned long long* map_out) {
    if (errors_out) HIP_CHECK(hipMemcpy(errors_out, cnt.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (map_out && tab.ptr) HIP_CHECK(hipMemcpy(map_out, tab.ptr, map_bytes, hipMemcpyDeviceToHost));
    return 0;
  }
};

// The run every burn-in shares once its tables are on the device: a checked warm-up launch (with `inject_block`,
// the verifier's self-check), `reps` timed launches, then the wrong-lane count and (cu_map != NULL) the BURN_SLOTS
// x 3 table over every launch.  `launch(inj, errors, map)` queues one launch of `blocks` workgroups.
template <typename F>
int burn_run(int device, int reps, int inject_block, F&& launch, unsigned long long* errors,
             unsigned long long* cu_map, float* ms) {
  ErrMap em;
  if (em.alloc(device, BURN_SLOTS, 3, cu_map != nullptr) || em.zero()) return -1;
  launch(inject_block < 0 ? -1 : inject_block, em.errors(), em.map());  // warm-up (also checked)
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  Timer tm;
  HIP_CHECK(tm.create());
  const auto timed = [&] {
    for (int r = 0; r < reps; ++r) launch(-1, em.errors(), em.map());
    return 0;
  };
  if (const int rc = tm.timed(timed, ms)) return rc;
  return em.read(errors, cu_map);
}

}  // namespace

// One entry point per diagnostic: the test hooks and optional outputs are parameters of it, and each comment below
// says which argument values mean "no hook" and which out-pointers may be null.
extern "C" {

const char* diag_last_error(void) { return g_err.c_str(); }

// 0 = auto (bf16: v4 four-wave 256x256 tiles when M, N are multiples of 256 and the grid fills the chip, else
// v1), 1 = force v1 (128x128 register-staged), 2 = force v2, 3 = force v3 (8 waves, staggered), 4 = force v4,
// 5 = v4 with the transposed register-direct epilogue.  fp8: auto / 4 / 5 run v4 on the unscaled MFMA (the MX form,
// fp8_unscaled = 0, and 1-3 run v3); fp4 always runs v3.
void diag_set_gemm_variant(int v) { g_gemm_variant = v; }
void diag_set_gemm_epilogue(int e) { g_gemm_epilogue = e; }
void diag_set_gemm_tail(int t) { g_gemm_tail = t ? 1 : 0; }
int diag_get_gemm_tail(void) { return g_gemm_tail; }
void diag_set_gemm_buffer_loads(int b) { g_gemm_buffer_loads = b; }
void diag_set_gemm_schedule(int s) { g_gemm_schedule = s; }
int diag_get_gemm_schedule(void) { return g_gemm_schedule; }
void diag_set_gemm_fp8_unscaled(int u) { g_gemm_fp8_unscaled = u ? 1 : 0; }
int diag_get_gemm_fp8_unscaled(void) { return g_gemm_fp8_unscaled; }
int diag_get_gemm_variant(void) { return g_gemm_variant; }
int diag_get_gemm_epilogue(void) { return g_gemm_epilogue; }
int diag_get_gemm_buffer_loads(void) { return g_gemm_buffer_loads; }

#ifdef DIAG_GEMM_STAMPS
// the stamps of the last v3 launch (8 x 2 x 4 x 4 64-bit clock values, diagnostic build only)
int diag_gemm_stamps(unsigned long long* out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gemm_stamps), sizeof(g_gemm_stamps)));
  return 0;
}
#endif

int diag_device_count(void) { return device_count(); }

// "arch|name|CUs|bytes|PCI BDF" of a HIP device (arch e.g. "gfx950:sramecc+:xnack-").
int diag_device_arch(int device, char* buf, int len) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  snprintf(buf, static_cast<size_t>(len), "%s|%s|%d|%zu|%04x:%02x:%02x.0", prop.gcnArchName, prop.name,
           prop.multiProcessorCount, static_cast<size_t>(prop.totalGlobalMem), prop.pciDomainID, prop.pciBusID,
           prop.pciDeviceID);
  return 0;
}

// Raw kernel on caller-owned device pointers (used by the numerics tests with
// torch tensors).  M, N multiples of 128; K multiple of 64.
int diag_gemm_bf16_launch(const void* A, const void* Bt, float* C, int M, int N, int K, void* stream) {
  if (M % BM || N % BN || K % BK || M <= 0 || N <= 0 || K <= 0) {
    g_err = "gemm_bf16: M, N must be multiples of 128 and K a multiple of 64";
    return -2;
  }
  const int variant = bf16_variant(M, N);
  if (variant >= 2 && variant <= 5) {
    if (M % V2_BM || N % V2_BN) {
      g_err = "gemm_bf16 v2-v5: M, N must be multiples of 256";
      return -2;
    }
    if (variant >= 4) {
      const int rc = launch_v4<OUT_F32>(variant, A, Bt, C, nullptr, M, N, K, static_cast<hipStream_t>(stream));
      if (rc != 0) return rc;
    } else if (variant == 2) {
      static LdsAttrOnce attr;
      if (ensure_dynamic_lds(attr, reinterpret_cast<const void*>(gemm_bf16_v2_kernel), 2 * V2_STAGE_BYTES,
                             "gemm v2") != 0)
        return -1;
      const int nwg = (M / V2_BM) * (N / V2_BN);
      hipLaunchKernelGGL(gemm_bf16_v2_kernel, dim3(nwg), dim3(V2_THREADS), 2 * V2_STAGE_BYTES,
                         static_cast<hipStream_t>(stream), static_cast<const __bf16*>(A),
                         static_cast<const __bf16*>(Bt), C, M, N, K);
    } else if (launch_v3<DT_BF16>(A, Bt, C, M, N, K, static_cast<hipStream_t>(stream)) != 0) {
      return -1;
    }
  } else {
    const int nwg = (M / BM) * (N / BN);
    hipLaunchKernelGGL(gemm_bf16_kernel, dim3(nwg), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const u32x4*>(A), static_cast<const u32x4*>(Bt), C, M, N, K);
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

// MX-fp8 GEMM on caller-owned device pointers: C[M,N] (fp32) = A[M,K] . Bt[N,K]^T with OCP E4M3
// operands (one byte each) and unit block scales.  M, N multiples of 256; K a multiple of 128.
int diag_gemm_fp8_launch(const void* A, const void* Bt, float* C, int M, int N, int K, void* stream) {
  if (M % V2_BM || N % V2_BN || K % 128 || M <= 0 || N <= 0 || K <= 0) {
    g_err = "gemm_fp8: M, N must be multiples of 256 and K a multiple of 128";
    return -2;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int v = fp8_variant();
  const int rc = v >= 4 ? launch_v4<OUT_F32, DT_FP8U>(v, A, Bt, C, nullptr, M, N, K / 2, st)
                 : g_gemm_fp8_unscaled ? launch_v3<DT_FP8U>(A, Bt, C, M, N, K / 2, st)
                                       : launch_v3<DT_FP8>(A, Bt, C, M, N, K / 2, st);
  if (rc != 0) return rc;
  HIP_CHECK(hipGetLastError());
  return 0;
}

// MX-fp4 GEMM: OCP E2M1 operands packed two per byte (element 2i in the low nibble), unit block
// scales, fp32 C.  M, N multiples of 256; K (elements) a multiple of 256.
int diag_gemm_fp4_launch(const void* A, const void* Bt, float* C, int M, int N, int K, void* stream) {
  if (M % V2_BM || N % V2_BN || K % 256 || M <= 0 || N <= 0 || K <= 0) {
    g_err = "gemm_fp4: M, N must be multiples of 256 and K a multiple of 256";
    return -2;
  }
  if (launch_v3<DT_FP4>(A, Bt, C, M, N, K / 4, static_cast<hipStream_t>(stream)) != 0) return -1;
  HIP_CHECK(hipGetLastError());
  return 0;
}

// The v3 kernel with bf16 output and fused column sums (what the diagnostic runs time and check):
// C[M,N] (bf16) = A . Bt^T, csum[M / 128][N] (fp64) = each column's sum over every 128-row block, formed from
// the fp32 accumulators.  bf16 (dt 0) or MX-fp8 (dt 1) operands; M, N multiples of 256, K of 64 (bf16) or 128.
int diag_gemm_launch_ck(int dt, const void* A, const void* Bt, void* C, double* csum, int M, int N, int K,
                        void* stream) {
  if (M % V2_BM || N % V2_BN || K % (dt == DT_FP8 ? 128 : BK) || M <= 0 || N <= 0 || K <= 0 ||
      (dt != DT_BF16 && dt != DT_FP8)) {
    g_err = "gemm_ck: bf16 or fp8, M, N multiples of 256, K a multiple of 64 (bf16) or 128 (fp8)";
    return -2;
  }
  if (!A || !Bt || !C || !csum) {
    g_err = "gemm_ck: null operand, output or column-sum pointer";
    return -2;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = dt == DT_FP8 ? launch_fp8_ck(A, Bt, static_cast<__bf16*>(C), csum, M, N, K / 2, st)
                              : launch_bf16_ck(A, Bt, static_cast<__bf16*>(C), csum, M, N, K, st);
  if (rc != 0) return rc;
  HIP_CHECK(hipGetLastError());
  return 0;
}

// 1 when diag_gemm_bf16 (dt 0) / diag_gemm_fp8 (dt 1) at M x N would time the bf16-output kernel with fused
// column sums under the calling thread's knobs, 0 when it would write fp32 C
int diag_gemm_ck_path(int dt, int M, int N) { return gemm_fused(dt, M, N) ? 1 : 0; }

}  // extern "C"

namespace {

// What differs between the bf16 and the fp8 diagnostic run (gemm_run): the operands and their fill, the sampled
// reference (`Ref` values from launch_ref, each error divided by denom()), the launches, the checksums' type and tiles.
struct GemmBf16 {
  static constexpr int DT = DT_BF16;
  static constexpr size_t kElemBytes = sizeof(__bf16);
  static constexpr uint64_t kSeedA = 0x1234ULL, kSeedBt = 0xBEEFULL, kSampleSeed = 0x243F6A8885A308D3ULL;
  using Ref = float;  // the fp32 reference kernel; an error is relative to max(1, |ref|)
  static constexpr bool kMag = false;
  static void fill(void* p, size_t n, uint64_t seed) {
    hipLaunchKernelGGL(fill_bf16_kernel, dim3(2048), dim3(256), 0, nullptr, static_cast<__bf16*>(p), n, seed);
  }
  static void launch_ref(const void* A, const void* Bt, const int* rows, const int* cols, void* ref, void*, int nsamp,
                         int K) {
    hipLaunchKernelGGL(gemm_ref_kernel, dim3((nsamp + 255) / 256), dim3(256), 0, nullptr,
                       static_cast<const __bf16*>(A), static_cast<const __bf16*>(Bt), rows, cols,
                       static_cast<float*>(ref), nsamp, K);
  }
  static double denom(double ref, double) { return std::max(1.0, std::fabs(ref)); }
  static int launch_ck(const void* A, const void* Bt, __bf16* C, double* cs, int M, int N, int K) {
    return launch_bf16_ck(A, Bt, C, cs, M, N, K, nullptr);
  }
  static int launch_f32(const void* A, const void* Bt, float* C, int M, int N, int K) {
    return diag_gemm_bf16_launch(A, Bt, C, M, N, K, nullptr);
  }
  // the v4 / v3 kernels compute 256^2 tiles, the v1 kernel 128^2
  static TileGeom geom(int M, int N) { return bf16_variant(M, N) == 1 ? kGeomV1 : kGeomV3; }
};

struct GemmFp8 {
  static constexpr int DT = DT_FP8;
  static constexpr size_t kElemBytes = 1;
  static constexpr uint64_t kSeedA = 0x5151ULL, kSeedBt = 0xA7A7ULL, kSampleSeed = 0x13198A2E03707344ULL;
  using Ref = double;  // the fp64 reference kernel, which also gives mag = sum|a*b|; an error is relative to mag
  static constexpr bool kMag = true;
  static void fill(void* p, size_t n, uint64_t seed) {
    hipLaunchKernelGGL(fill_fp8_kernel, dim3(2048), dim3(256), 0, nullptr, static_cast<uint8_t*>(p), n, seed);
  }
  static void launch_ref(const void* A, const void* Bt, const int* rows, const int* cols, void* ref, void* mag,
                         int nsamp, int K) {
    hipLaunchKernelGGL(gemm_ref_fp8_kernel, dim3((nsamp + 255) / 256), dim3(256), 0, nullptr,
                       static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(Bt), rows, cols,
                       static_cast<double*>(ref), static_cast<double*>(mag), nsamp, K);
  }
  static double denom(double, double mag) { return std::max(mag, 1e-30); }
  static int launch_ck(const void* A, const void* Bt, __bf16* C, double* cs, int M, int N, int K) {
    return launch_fp8_ck(A, Bt, C, cs, M, N, K / 2, nullptr);
  }
  static int launch_f32(const void* A, const void* Bt, float* C, int M, int N, int K) {
    return diag_gemm_fp8_launch(A, Bt, C, M, N, K, nullptr);
  }
  static TileGeom geom(int, int) { return kGeomV3; }
};

// Optional host copies of what gemm_verify judged (any pointer may be null): the sample positions, the sampled
// reference and magnitude (zeros where the type forms none) and the checksums' per-(row block, column) arrays.
struct VerifyOut {
  int *rows = nullptr, *cols = nullptr;
  double *ref = nullptr, *mag = nullptr, *ck_ref = nullptr, *ck_mag = nullptr, *ck_csum = nullptr;
};

// The referee of a diagnostic run, on device buffers the caller owns: `nsamp` sampled outputs of C against the
// reference kernel (*max_err) and, with ck_tol >= 0, every output by tile checksums over the tiles `g`
// (gemm_checksum: *ck_err, ck_out[kCkOut], *ck_floor).  `cs` != NULL: C is bf16 and cs the fused csum[M / 128][N];
// NULL: C is fp32.  The shape is the caller's to check.
template <typename T>
int gemm_verify(int device, const void* A, const void* Bt, const void* Cv, const double* cs, int M, int N, int K,
                TileGeom g, int nsamp, double ck_tol, double* max_err, double* ck_err, long long* ck_out,
                double* ck_floor, const VerifyOut& vo = VerifyOut()) {
  using Ref = typename T::Ref;
  const bool fused = cs != nullptr;
  DevBuf bref, bmag, brows, bcols, bgot;
  HIP_CHECK(bref.alloc(device, sizeof(Ref) * nsamp));
  if (T::kMag) HIP_CHECK(bmag.alloc(device, sizeof(double) * nsamp));
  HIP_CHECK(brows.alloc(device, sizeof(int) * nsamp));
  HIP_CHECK(bcols.alloc(device, sizeof(int) * nsamp));
  HIP_CHECK(bgot.alloc(device, sizeof(float) * nsamp));
  const int* rows = static_cast<const int*>(brows.ptr);
  const int* cols = static_cast<const int*>(bcols.ptr);
  float* got = static_cast<float*>(bgot.ptr);
  std::vector<int> hr, hc;
  sample_indices(T::kSampleSeed, nsamp, M, N, hr, hc);
  HIP_CHECK(hipMemcpy(brows.ptr, hr.data(), sizeof(int) * nsamp, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(bcols.ptr, hc.data(), sizeof(int) * nsamp, hipMemcpyHostToDevice));
  T::launch_ref(A, Bt, rows, cols, bref.ptr, bmag.ptr, nsamp, K);
  // gather the sampled outputs on the device: one copy instead of nsamp tiny ones
  if (fused)
    hipLaunchKernelGGL(gather_kernel<__bf16>, dim3((nsamp + 255) / 256), dim3(256), 0, nullptr,
                       static_cast<const __bf16*>(Cv), rows, cols, got, nsamp, N);
  else
    hipLaunchKernelGGL(gather_kernel<float>, dim3((nsamp + 255) / 256), dim3(256), 0, nullptr,
                       static_cast<const float*>(Cv), rows, cols, got, nsamp, N);
  HIP_CHECK(hipGetLastError());
  std::vector<Ref> href(nsamp);
  std::vector<double> hmag(nsamp, 0.0);
  std::vector<float> hC(nsamp);
  HIP_CHECK(hipMemcpy(href.data(), bref.ptr, sizeof(Ref) * nsamp, hipMemcpyDeviceToHost));
  if (T::kMag) HIP_CHECK(hipMemcpy(hmag.data(), bmag.ptr, sizeof(double) * nsamp, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hC.data(), bgot.ptr, sizeof(float) * nsamp, hipMemcpyDeviceToHost));
  const std::vector<double> ref64(href.begin(), href.end());
  *max_err = sampled_worst(hC.data(), ref64.data(), hmag.data(), nsamp, fused, T::kMag);
  if (vo.rows) std::copy(hr.begin(), hr.end(), vo.rows);
  if (vo.cols) std::copy(hc.begin(), hc.end(), vo.cols);
  if (vo.ref) std::copy(ref64.begin(), ref64.end(), vo.ref);
  if (vo.mag) std::copy(hmag.begin(), hmag.end(), vo.mag);
  if (ck_tol >= 0.0)
    return gemm_checksum<T::DT>(device, A, Bt, static_cast<const float*>(Cv), M, N, K, g, ck_tol, ck_err, ck_out, cs,
                                ck_floor, vo.ck_ref, vo.ck_mag, vo.ck_csum);
  return 0;
}

// Self-contained MFMA burn-in: allocate, fill, run `iters` GEMMs, time them, then the referee (gemm_verify): `nsamp`
// sampled outputs against the reference kernel and, with ck_tol >= 0, every output by tile checksums
// (*ck_err, ck_out[kCkOut], *ck_floor).  `inject_elem` >= 0 overwrites that output between the timing and the
// checks: with 1e6, or (inject_delta not NaN) with its own value plus inject_delta.  The shape is the caller's to check.
template <typename T>
int gemm_run(int device, int M, int N, int K, int warmup, int iters, int nsamp, long long inject_elem,
             double inject_delta, double ck_tol, double* tflops, double* max_err, double* ms_per_iter, double* ck_err,
             long long* ck_out, double* ck_floor) {
  HIP_CHECK(hipSetDevice(device));
  // bf16 C and the kernel's own column sums (OUT_BF16_CK), or fp32 C
  const bool fused = gemm_fused(T::DT, M, N);
  DevBuf bA, bBt, bC, bcs;
  HIP_CHECK(bA.alloc(device, T::kElemBytes * static_cast<size_t>(M) * K));
  HIP_CHECK(bBt.alloc(device, T::kElemBytes * static_cast<size_t>(N) * K));
  HIP_CHECK(bC.alloc(device, (fused ? sizeof(__bf16) : sizeof(float)) * static_cast<size_t>(M) * N));
  if (fused) HIP_CHECK(bcs.alloc(device, sizeof(double) * static_cast<size_t>(M / 128) * N));
  double* cs = static_cast<double*>(bcs.ptr);
  float* C = static_cast<float*>(bC.ptr);
  __bf16* Cb = static_cast<__bf16*>(bC.ptr);
  auto run = [&]() -> int {
    return fused ? T::launch_ck(bA.ptr, bBt.ptr, Cb, cs, M, N, K) : T::launch_f32(bA.ptr, bBt.ptr, C, M, N, K);
  };
  T::fill(bA.ptr, static_cast<size_t>(M) * K, T::kSeedA);
  T::fill(bBt.ptr, static_cast<size_t>(N) * K, T::kSeedBt);
  HIP_CHECK(hipGetLastError());
  Timer tm;
  HIP_CHECK(tm.create());
  for (int i = 0; i < warmup; ++i)
    if (run()) return -1;
  const auto timed = [&] {
    for (int i = 0; i < iters; ++i)
      if (run()) return -1;
    return 0;
  };
  float t_ms = 0.f;
  if (const int rc = tm.timed(timed, &t_ms)) return rc;
  const double ms = t_ms / std::max(iters, 1);
  if (fused) HIP_CHECK(inject_output_ck(Cb, cs, inject_elem, M, N, inject_delta));
  else HIP_CHECK(inject_output(C, inject_elem, static_cast<long long>(M) * N, inject_delta));
  *ms_per_iter = ms;
  *tflops = 2.0 * M * N * static_cast<double>(K) / (ms * 1e-3) / 1e12;
  return gemm_verify<T>(device, bA.ptr, bBt.ptr, bC.ptr, fused ? cs : nullptr, M, N, K, T::geom(M, N), nsamp, ck_tol,
                        max_err, ck_err, ck_out, ck_floor);
}

}  // namespace

extern "C" {

// bf16 GEMM burn-in (gemm_run): *max_rel_err = max |C - ref| / max(1, |ref|) over the samples.  No hook:
// inject_elem = -1 (inject_delta is then unused; NaN = the 1e6 overwrite).  ck_tol < 0: no checksums, and ck_err,
// ck_out and ck_floor may be null; with checksums ck_floor may still be null.
int diag_gemm_bf16(int device, int M, int N, int K, int warmup, int iters, int nsamp, long long inject_elem,
                   double inject_delta, double ck_tol, double* tflops, double* max_rel_err, double* ms_per_iter,
                   double* ck_err, long long* ck_out, double* ck_floor) {
  if (inject_elem >= static_cast<long long>(M) * N) {
    g_err = "gemm: inject_elem outside the output";
    return -2;
  }
  if (M % BM || N % BN || K % BK) {
    g_err = "gemm_bf16: M, N must be multiples of 128 and K a multiple of 64";
    return -2;
  }
  return gemm_run<GemmBf16>(device, M, N, K, warmup, iters, nsamp, inject_elem, inject_delta, ck_tol, tflops,
                            max_rel_err, ms_per_iter, ck_err, ck_out, ck_floor);
}

// MX-fp8 counterpart of diag_gemm_bf16 (the same hooks; ck_floor, and without checksums ck_err and ck_out, may be
// null): *max_err = max |C - ref| / sum|a*b| over the samples.
int diag_gemm_fp8(int device, int M, int N, int K, int warmup, int iters, int nsamp, long long inject_elem,
                  double inject_delta, double ck_tol, double* tflops, double* max_err, double* ms_per_iter,
                  double* ck_err, long long* ck_out, double* ck_floor) {
  if (inject_elem >= static_cast<long long>(M) * N) {
    g_err = "gemm: inject_elem outside the output";
    return -2;
  }
  if (M % V2_BM || N % V2_BN || K % 128 || nsamp < 1) {
    g_err = "gemm_fp8: M, N must be multiples of 256, K a multiple of 128";
    return -2;
  }
  return gemm_run<GemmFp8>(device, M, N, K, warmup, iters, nsamp, inject_elem, inject_delta, ck_tol, tflops, max_err,
                           ms_per_iter, ck_err, ck_out, ck_floor);
}

// The diagnostics' referee (gemm_verify) on caller-owned device buffers of the current device, for the tests: dt 0 =
// bf16, 1 = E4M3 operands A[M][K], Bt[N][K]; geom 0 = 128/128/8 tiles (bf16 only), 1 = 256/256/4.  csum != NULL: C is
// bf16 and csum the fused csum[M / 128][N] (geom 1 only); NULL: C is fp32.  ck_tol < 0: no checksums (ck_err, ck_out,
// ck_floor untouched, and they may be null; with checksums ck_floor may still be null).  Optional host arrays, each
// of which may be null: rows / cols / ref / mag[nsamp] (mag: zeros for bf16) and ck_ref / ck_mag / ck_csum, each
// [M / tile rows][N].  Nothing is launched on a refused argument (-2).
int diag_gemm_verify(int dt, const void* A, const void* Bt, const void* C, const double* csum, int M, int N, int K,
                     int geom, int nsamp, double ck_tol, double* max_err, double* ck_err, long long* ck_out,
                     double* ck_floor, int* rows, int* cols, double* ref, double* mag, double* ck_ref,
                     double* ck_mag, double* ck_csum) {
  if ((dt != DT_BF16 && dt != DT_FP8) || (geom != 0 && geom != 1) || (dt == DT_FP8 && geom == 0)) {
    g_err = "gemm_verify: dt 0 (bf16) or 1 (fp8), geom 0 (128^2 tiles, bf16 only) or 1 (256^2 tiles)";
    return -2;
  }
  const int tile = geom ? V2_BM : BM, kmul = dt == DT_FP8 ? 128 : BK;
  if (M <= 0 || N <= 0 || K <= 0 || M % tile || N % tile || K % kmul) {
    g_err = "gemm_verify: M, N must be multiples of the tile (128 for geom 0, 256 for geom 1), K of 64 (bf16) or 128 "
            "(fp8)";
    return -2;
  }
  if (nsamp < 1) {
    g_err = "gemm_verify: nsamp must be at least 1";
    return -2;
  }
  if (!A || !Bt || !C || !max_err || (ck_tol >= 0.0 && (!ck_err || !ck_out))) {
    g_err = "gemm_verify: null operand, output or result pointer";
    return -2;
  }
  if (csum && geom == 0) {
    g_err = "gemm_verify: fused column sums come with 256^2 tiles (geom 1) only";
    return -2;
  }
  int device = 0;
  HIP_CHECK(hipGetDevice(&device));
  VerifyOut vo;
  vo.rows = rows, vo.cols = cols, vo.ref = ref, vo.mag = mag;
  vo.ck_ref = ck_ref, vo.ck_mag = ck_mag, vo.ck_csum = ck_csum;
  const TileGeom g = geom ? kGeomV3 : kGeomV1;
  return dt == DT_FP8 ? gemm_verify<GemmFp8>(device, A, Bt, C, csum, M, N, K, g, nsamp, ck_tol, max_err, ck_err,
                                             ck_out, ck_floor, vo)
                      : gemm_verify<GemmBf16>(device, A, Bt, C, csum, M, N, K, g, nsamp, ck_tol, max_err, ck_err,
                                              ck_out, ck_floor, vo);
}

// The diagnostics' own operand fill (dt 0: fill_bf16_kernel, 1: fill_fp8_kernel) of `n` elements at device pointer
// `ptr`, complete on return.
int diag_gemm_fill(int dt, void* ptr, size_t n, unsigned long long seed) {
  if ((dt != DT_BF16 && dt != DT_FP8) || !ptr || n == 0) {
    g_err = "gemm_fill: dt 0 (bf16) or 1 (fp8), a buffer of at least one element";
    return -2;
  }
  if (dt == DT_FP8) GemmFp8::fill(ptr, n, seed);
  else GemmBf16::fill(ptr, n, seed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return 0;
}

// HBM streams over `bytes` per buffer: copy (read+write), read-only, write-only, in TB/s.  The bytes the rates are
// computed from are checked outside the timed loops (stream_verify_kernel): after the copy phase every 16-byte
// element of the destination holds the source's fill, after the write phase the written value; *errors = elements
// that did not.  `inject_word` >= 0 (the verifier's self-check) overwrites that element of the destination from the
// host before the verification of `inject_phase` (0 = the copy's, 1 = the write's); -1 = no hook.
int diag_hbm_bandwidth(int device, size_t bytes, int iters, long long inject_word, int inject_phase,
                       double* copy_tbs, double* read_tbs, double* write_tbs, unsigned long long* errors) {
  HIP_CHECK(hipSetDevice(device));
  const size_t n = bytes / sizeof(f32x4);
  if (inject_word >= 0 && (static_cast<size_t>(inject_word) >= n || inject_phase < 0 || inject_phase > 1)) {
    g_err = "hbm: inject_word outside the buffer (or inject_phase not 0 / 1)";
    return -2;
  }
  DevBuf ba, bb, bsink, berr;
  HIP_CHECK(berr.alloc(device, sizeof(unsigned long long)));
  HIP_CHECK(hipMemset(berr.ptr, 0, sizeof(unsigned long long)));
  auto verify = [&](int phase, float want) -> int {
    f32x4* dst = static_cast<f32x4*>(bb.ptr);
    if (inject_word >= 0 && phase == inject_phase) {
      const float bad[4] = {want, -want, want, want};  // one lane of the element wrong
      HIP_CHECK(hipMemcpy(dst + inject_word, bad, sizeof bad, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(stream_verify_kernel, dim3(flat_grid(n)), dim3(256), 0, nullptr, dst, n, want,
                       static_cast<unsigned long long*>(berr.ptr));
    HIP_CHECK(hipGetLastError());
    return 0;
  };
  HIP_CHECK(ba.alloc(device, n * sizeof(f32x4)));
  HIP_CHECK(bb.alloc(device, n * sizeof(f32x4)));
  HIP_CHECK(bsink.alloc(device, sizeof(float)));
  f32x4* a = static_cast<f32x4*>(ba.ptr);
  f32x4* b = static_cast<f32x4*>(bb.ptr);
  float* sink = static_cast<float*>(bsink.ptr);
  const unsigned grid = flat_grid(n);
  hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, nullptr, a, n, 1.0f);
  hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, nullptr, b, n, 2.0f);
  HIP_CHECK(hipGetLastError());
  Timer tm;
  HIP_CHECK(tm.create());
  const size_t nb = n * sizeof(f32x4);
  // one phase: an untimed launch, then `iters` timed ones; the rate over `traffic` x the buffer's bytes per launch
  auto phase = [&](auto&& launch, double traffic, double* tbs) -> int {
    float t_ms = 0.f;
    launch();
    const auto loop = [&] {
      for (int i = 0; i < iters; ++i) launch();
      return 0;
    };
    if (const int rc = tm.timed(loop, &t_ms)) return rc;
    *tbs = traffic * nb * iters / (t_ms * 1e-3) / 1e12;
    return 0;
  };
  if (phase([&] { hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, nullptr, a, b, n); }, 2.0, copy_tbs))
    return -1;
  if (phase([&] { hipLaunchKernelGGL(read_kernel, dim3(grid), dim3(256), 0, nullptr, a, n, sink); }, 1.0, read_tbs))
    return -1;
  if (verify(0, 1.0f)) return -1;  // b is still the copy of a (the read phase only reads a)
  if (phase([&] { hipLaunchKernelGGL(write_kernel, dim3(grid), dim3(256), 0, nullptr, b, n, 3.0f); }, 1.0, write_tbs))
    return -1;
  if (verify(1, 3.0f)) return -1;
  HIP_CHECK(hipMemcpy(errors, berr.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

// Pattern test over `bytes` of HBM; `passes` x (pattern, inverted pattern).
// `inject_word` >= 0: that 16-byte word is overwritten (0xA5 bytes) between one write and its verify -- the write
// of pass `inject_pass`, its inverted half when `inject_invert` -- the fault-injection check that a corrupted word
// is counted and located (diag.memtest(inject_word=...)); `inject_word2` >= 0 is a second word of the same write.
// No hook: inject_word = inject_word2 = -1 (inject_pass and inject_invert are then unused).
int diag_memtest(int device, size_t bytes, uint64_t seed, int passes, long long inject_word,
                 long long inject_word2, int inject_pass, int inject_invert, unsigned long long* errors,
                 unsigned long long* first_bad_byte, double* gbps) {
  HIP_CHECK(hipSetDevice(device));
  for (const long long w : {inject_word, inject_word2})
    if (w >= 0 && static_cast<size_t>(w) >= bytes / sizeof(uint4)) {
      g_err = "memtest: inject_word outside the buffer";
      return -2;
    }
  if ((inject_word >= 0 || inject_word2 >= 0) && (inject_pass < 0 || inject_pass >= passes)) {
    g_err = "memtest: inject_pass outside the passes";
    return -2;
  }
  const size_t n = bytes / sizeof(uint4);
  DevBuf bp, bdev;
  HIP_CHECK(bp.alloc(device, n * sizeof(uint4)));
  HIP_CHECK(bdev.alloc(device, 2 * sizeof(unsigned long long)));
  uint4* p = static_cast<uint4*>(bp.ptr);
  unsigned long long* dev = static_cast<unsigned long long*>(bdev.ptr);
  const unsigned long long init[2] = {0ULL, ~0ULL};
  HIP_CHECK(hipMemcpy(dev, init, sizeof init, hipMemcpyHostToDevice));
  const unsigned grid = flat_grid(n);
  Timer tm;
  HIP_CHECK(tm.create());
  const auto all_passes = [&]() -> int {
    for (int pass = 0; pass < passes; ++pass) {
      for (int inv = 0; inv < 2; ++inv) {
        const uint64_t s = seed + static_cast<uint64_t>(pass) * 0x9E3779B97F4A7C15ULL;
        hipLaunchKernelGGL(mt_write_kernel, dim3(grid), dim3(256), 0, nullptr, p, n, s, inv);
        if (pass == inject_pass && inv == (inject_invert ? 1 : 0))
          for (const long long w : {inject_word, inject_word2})
            if (w >= 0) HIP_CHECK(hipMemsetAsync(p + w, 0xA5, sizeof(uint4), nullptr));
        hipLaunchKernelGGL(mt_verify_kernel, dim3(grid), dim3(256), 0, nullptr, p, n, s, inv, dev, dev + 1);
      }
    }
    return 0;
  };
  float t_ms = 0.f;
  if (const int rc = tm.timed(all_passes, &t_ms)) return rc;
  unsigned long long h[2];
  HIP_CHECK(hipMemcpy(h, dev, sizeof h, hipMemcpyDeviceToHost));
  *errors = h[0];
  *first_bad_byte = h[0] ? h[1] * sizeof(uint4) : ~0ULL;
  *gbps = 4.0 * passes * static_cast<double>(n * sizeof(uint4)) / (t_ms * 1e-3) / 1e9;
  return 0;
}

// xGMI point-to-point check between two GPUs of the node: `iters` copies of `bytes` from `src` to
// `dst` (hipMemcpyPeerAsync on a src-device stream, peer access enabled both ways when the pair
// supports it -- on an MI355X hive every pair is one xGMI hop), timed with events; the received
// buffer is then verified against the address-hash pattern on `dst`.  *peer = 1 if direct peer
// access was available.  A slow pair (a link trained down or retrying) shows up as an outlier
// against the node's other pairs; a corrupting one as errors.
//
// `timeout_ms` > 0 bounds the copies and the verification: the completion events are polled rather than
// waited on, and a pair that has not finished by then returns -4 ("hung") instead of blocking the agent's
// node-level thread forever on a link that stopped making progress.  On that path the buffers, events and
// stream are deliberately leaked: freeing memory an in-flight copy still targets would block (hipFree
// synchronises the device) or let the engine write into a reused allocation.  timeout_ms = 0: a blocking wait.
int diag_p2p_copy(int src, int dst, size_t bytes, int iters, double timeout_ms, double* gbps,
                  unsigned long long* errors, int* peer) {
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  if (src < 0 || dst < 0 || src >= n || dst >= n || src == dst || iters < 1 || bytes < 16) {
    g_err = "p2p: need two distinct devices, iters >= 1, bytes >= 16";
    return -2;
  }
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  int can_sd = 0, can_ds = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&can_sd, src, dst));
  HIP_CHECK(hipDeviceCanAccessPeer(&can_ds, dst, src));
  *peer = can_sd && can_ds;
  if (*peer) {
    HIP_CHECK(enable_peer(src, dst));
    HIP_CHECK(enable_peer(dst, src));
  }
  const size_t nvec = bytes / sizeof(uint4);
  const size_t nbytes = nvec * sizeof(uint4);
  DevBuf a, b, cnt;
  HIP_CHECK(a.alloc(src, nbytes));
  HIP_CHECK(b.alloc(dst, nbytes));
  HIP_CHECK(cnt.alloc(dst, 2 * sizeof(unsigned long long)));
  const uint64_t seed = 0xC0FFEEULL + static_cast<uint64_t>(src) * 131 + static_cast<uint64_t>(dst);
  // pattern on src, junk on dst
  HIP_CHECK(hipSetDevice(src));
  hipLaunchKernelGGL(mt_write_kernel, dim3(grid_for(src, 4)), dim3(256), 0, nullptr, static_cast<uint4*>(a.ptr), nvec,
                     seed, 0);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipSetDevice(dst));
  HIP_CHECK(hipMemset(b.ptr, 0xA5, nbytes));
  const unsigned long long init[2] = {0ULL, ~0ULL};
  HIP_CHECK(hipMemcpy(cnt.ptr, init, sizeof init, hipMemcpyHostToDevice));
  HIP_CHECK(hipDeviceSynchronize());
  // timed copies on a stream of the source device
  HIP_CHECK(hipSetDevice(src));
  Timer tm;
  HIP_CHECK(tm.create(true));
  hipEvent_t e0 = tm.e0, e1 = tm.e1;
  hipStream_t st = tm.stream;
  HIP_CHECK(hipMemcpyPeerAsync(b.ptr, dst, a.ptr, src, nbytes, st));  // warm-up (maps, engine)
  HIP_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) HIP_CHECK(hipMemcpyPeerAsync(b.ptr, dst, a.ptr, src, nbytes, st));
  HIP_CHECK(hipEventRecord(e1, st));
  const PollDeadline dl(timeout_ms);
  Timer tv;  // the verification's completion event lives on `dst`
  auto hung = [&](const char* stage) {
    a.ptr = b.ptr = cnt.ptr = nullptr;
    tm.e0 = tm.e1 = tv.e0 = tv.e1 = nullptr;
    tm.stream = nullptr;
    (void)hipSetDevice(cur);
    char msg[192];
    std::snprintf(msg, sizeof msg, "p2p %d->%d: %s did not complete within %.0f ms (xGMI link or engine hung)", src,
                  dst, stage, timeout_ms);
    g_err = msg;
    return -4;
  };
  hipError_t w = wait_event_polled(e1, dl);
  if (w == hipErrorNotReady) return hung("copies");
  HIP_CHECK(w);
  float ms = 0.f;
  HIP_CHECK(event_ms(e0, e1, &ms));
  *gbps = ms > 0.f ? static_cast<double>(iters) * static_cast<double>(nbytes) / (ms * 1e-3) / 1e9 : 0.0;
  // verify what arrived
  HIP_CHECK(hipSetDevice(dst));
  HIP_CHECK(tv.create(false));
  unsigned long long* c = static_cast<unsigned long long*>(cnt.ptr);
  hipLaunchKernelGGL(mt_verify_kernel, dim3(grid_for(dst, 4)), dim3(256), 0, nullptr,
                     static_cast<const uint4*>(b.ptr), nvec, seed, 0, c, c + 1);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(tv.e0, nullptr));
  w = wait_event_polled(tv.e0, dl);
  if (w == hipErrorNotReady) return hung("verification");
  HIP_CHECK(w);
  unsigned long long h[2];
  HIP_CHECK(hipMemcpy(h, cnt.ptr, sizeof h, hipMemcpyDeviceToHost));
  *errors = h[0];
  HIP_CHECK(hipSetDevice(cur));
  return 0;
}

// Self-test of the polled deadline the pair copies wait with (wait_event_polled), on one GPU: queue `launches`
// full-buffer writes of 1 GiB (finite work, ~0.15 ms each on MI355X) on a stream of their own, wait for them
// with a `deadline_ms` deadline -- *timed_out = 1 when the deadline passed first, *waited_ms how long that
// took -- then drain the stream (*drained_ms) before freeing, so nothing is left running.  The hung-pair path
// of diag_p2p_copy cannot be provoked on a healthy node; this shows the same wait returning at its deadline.
int diag_poll_selftest(int device, int launches, double deadline_ms, int* timed_out, double* waited_ms,
                       double* drained_ms) {
  if (launches < 1 || launches > 100000 || deadline_ms <= 0.0) {
    g_err = "poll selftest: launches in [1, 100000] and a positive deadline";
    return -2;
  }
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  constexpr size_t bytes = size_t(1) << 30;
  DevBuf buf;
  HIP_CHECK(buf.alloc(device, bytes));
  Timer tm;
  HIP_CHECK(tm.create(true));
  const size_t n = bytes / sizeof(f32x4);
  for (int i = 0; i < launches; ++i)
    hipLaunchKernelGGL(write_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, tm.stream,
                       static_cast<f32x4*>(buf.ptr), n, 1.0f);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(tm.e1, tm.stream));
  const auto t0 = SteadyClock::now();
  const hipError_t w = wait_event_polled(tm.e1, PollDeadline(deadline_ms));
  const auto t1 = SteadyClock::now();
  *timed_out = w == hipErrorNotReady;
  *waited_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  const hipError_t d = hipEventSynchronize(tm.e1);  // finite work: drain before the buffer is freed
  *drained_ms = std::chrono::duration<double, std::milli>(SteadyClock::now() - t1).count();
  if (w != hipSuccess && w != hipErrorNotReady) HIP_CHECK(w);
  HIP_CHECK(d);
  HIP_CHECK(hipSetDevice(cur));
  return 0;
}

// The "fan" pass of the xGMI check: `src` copies to all `ndst` peers at once, so every one of its links carries
// traffic together (the pair pass loads one link at a time; a link that holds up alone but not under load -- a
// marginal lane retraining, an engine shared with another link -- only shows here).  One source buffer with the
// address-hash pattern, one destination buffer per peer, one non-blocking stream per peer on `src`; every stream
// waits on a common start event, runs `iters` hipMemcpyPeerAsync of `bytes` and records its own end, so
// gbps[i] = the rate peer i saw while all were running and *total_gbps = all bytes over the slowest stream's end.
// Each destination is then verified against the pattern (errors[i]); peer[i] = direct peer access both ways.
// `timeout_ms` > 0 bounds copies and verification as in diag_p2p_copy (-4 "hung", resources leaked on purpose); 0 =
// a blocking wait.
int diag_p2p_fan(int src, const int* dsts, int ndst, size_t bytes, int iters, double timeout_ms, double* gbps,
                 unsigned long long* errors, int* peer, double* total_gbps) {
  constexpr int kMaxFan = 64;  // a CPX hive: 63 peers
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  if (src < 0 || src >= n || ndst < 1 || ndst > kMaxFan || iters < 1 || bytes < 16) {
    g_err = "p2p fan: need a valid source, 1..64 peers, iters >= 1, bytes >= 16";
    return -2;
  }
  for (int i = 0; i < ndst; ++i) {
    if (dsts[i] < 0 || dsts[i] >= n || dsts[i] == src) {
      g_err = "p2p fan: every peer must be a device other than the source";
      return -2;
    }
    for (int j = 0; j < i; ++j)
      if (dsts[j] == dsts[i]) {
        g_err = "p2p fan: a peer is listed twice";
        return -2;
      }
  }
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  for (int i = 0; i < ndst; ++i) {
    int sd = 0, ds = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&sd, src, dsts[i]));
    HIP_CHECK(hipDeviceCanAccessPeer(&ds, dsts[i], src));
    peer[i] = sd && ds;
    if (peer[i]) {
      HIP_CHECK(enable_peer(src, dsts[i]));
      HIP_CHECK(enable_peer(dsts[i], src));
    }
    errors[i] = 0;
    gbps[i] = 0.0;
  }
  *total_gbps = 0.0;
  const size_t nvec = bytes / sizeof(uint4);
  const size_t nbytes = nvec * sizeof(uint4);
  const uint64_t seed = 0xFA17ULL + static_cast<uint64_t>(src) * 131;
  DevBuf a;
  DevBuf b[kMaxFan], cnt[kMaxFan];
  HIP_CHECK(a.alloc(src, nbytes));
  HIP_CHECK(hipSetDevice(src));
  hipLaunchKernelGGL(mt_write_kernel, dim3(grid_for(src, 4)), dim3(256), 0, nullptr, static_cast<uint4*>(a.ptr), nvec,
                     seed, 0);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  const unsigned long long init[2] = {0ULL, ~0ULL};
  for (int i = 0; i < ndst; ++i) {
    HIP_CHECK(b[i].alloc(dsts[i], nbytes));
    HIP_CHECK(cnt[i].alloc(dsts[i], sizeof init));
    HIP_CHECK(hipMemset(b[i].ptr, 0xA5, nbytes));
    HIP_CHECK(hipMemcpy(cnt[i].ptr, init, sizeof init, hipMemcpyHostToDevice));
    HIP_CHECK(hipDeviceSynchronize());
  }
  // streams and events on the source device: a head stream records the common start, each peer's stream waits
  // on it, then copies (after one untimed warm-up copy per peer, mapping the pages and waking the engines)
  HIP_CHECK(hipSetDevice(src));
  Timer head;
  HIP_CHECK(head.create(true));
  Timer per[kMaxFan];
  for (int i = 0; i < ndst; ++i) {
    HIP_CHECK(per[i].create(true));
    HIP_CHECK(hipMemcpyPeerAsync(b[i].ptr, dsts[i], a.ptr, src, nbytes, per[i].stream));
    HIP_CHECK(hipEventRecord(per[i].e0, per[i].stream));
  }
  for (int i = 0; i < ndst; ++i) HIP_CHECK(hipStreamWaitEvent(head.stream, per[i].e0, 0));  // warm-ups done
  HIP_CHECK(hipEventRecord(head.e0, head.stream));
  for (int i = 0; i < ndst; ++i) {
    HIP_CHECK(hipStreamWaitEvent(per[i].stream, head.e0, 0));
    for (int it = 0; it < iters; ++it) HIP_CHECK(hipMemcpyPeerAsync(b[i].ptr, dsts[i], a.ptr, src, nbytes, per[i].stream));
    HIP_CHECK(hipEventRecord(per[i].e1, per[i].stream));
  }
  const PollDeadline dl(timeout_ms);
  Timer verify[kMaxFan];
  auto hung = [&](int i, const char* stage) {
    // in-flight copies may still target these buffers: leak everything rather than free under them
    a.ptr = nullptr;
    for (int j = 0; j < ndst; ++j) {
      b[j].ptr = cnt[j].ptr = nullptr;
      per[j].e0 = per[j].e1 = nullptr;
      per[j].stream = nullptr;
      verify[j].e0 = verify[j].e1 = nullptr;
    }
    head.e0 = head.e1 = nullptr;
    head.stream = nullptr;
    (void)hipSetDevice(cur);
    char msg[192];
    std::snprintf(msg, sizeof msg, "p2p fan %d->%d: %s did not complete within %.0f ms (xGMI link or engine hung)",
                  src, dsts[i], stage, timeout_ms);
    g_err = msg;
    return -4;
  };
  float slowest = 0.f;
  for (int i = 0; i < ndst; ++i) {
    hipError_t w = wait_event_polled(per[i].e1, dl);
    if (w == hipErrorNotReady) return hung(i, "copies");
    HIP_CHECK(w);
    float ms = 0.f;
    HIP_CHECK(event_ms(head.e0, per[i].e1, &ms));
    gbps[i] = ms > 0.f ? static_cast<double>(iters) * static_cast<double>(nbytes) / (ms * 1e-3) / 1e9 : 0.0;
    slowest = std::max(slowest, ms);
  }
  *total_gbps = slowest > 0.f
                    ? static_cast<double>(ndst) * iters * static_cast<double>(nbytes) / (slowest * 1e-3) / 1e9
                    : 0.0;
  for (int i = 0; i < ndst; ++i) {
    HIP_CHECK(hipSetDevice(dsts[i]));
    HIP_CHECK(verify[i].create(false));
    unsigned long long* c = static_cast<unsigned long long*>(cnt[i].ptr);
    hipLaunchKernelGGL(mt_verify_kernel, dim3(grid_for(dsts[i], 4)), dim3(256), 0, nullptr,
                       static_cast<const uint4*>(b[i].ptr), nvec, seed, 0, c, c + 1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(verify[i].e0, nullptr));
  }
  for (int i = 0; i < ndst; ++i) {
    hipError_t w = wait_event_polled(verify[i].e0, dl);
    if (w == hipErrorNotReady) return hung(i, "verification");
    HIP_CHECK(w);
    unsigned long long h[2];
    HIP_CHECK(hipSetDevice(dsts[i]));
    HIP_CHECK(hipMemcpy(h, cnt[i].ptr, sizeof h, hipMemcpyDeviceToHost));
    errors[i] = h[0];
  }
  HIP_CHECK(hipSetDevice(cur));
  return 0;
}

int diag_mfma_burn_slots(void) { return BURN_SLOTS; }

// Matrix-core burn-in of one precision (`kind` as mfma_burn_kernel): `reps` launches of `iters`
// iterations on every CU; *tflops = dense rate, *errors = wave-lanes whose exact result differed; (cu_map != NULL)
// a BURN_SLOTS x 3 table of (waves, wrong lanes, wave time in wall-clock ticks) per physical CU slot (wave_slot()),
// over every launch including the warm-up.
// `inject_block` >= 0 (the verifier's self-check): in the warm-up launch only -- it is checked and mapped like the
// others, and a block index lands on another CU in every launch -- lane 0 of wave 0 of that workgroup is made wrong;
// -1 = no hook.  cu_map may be null (no map wanted).
int diag_mfma_burn(int device, int kind, int iters, int reps, int inject_block, double* tflops,
                   unsigned long long* errors, unsigned long long* cu_map) {
  if (kind < 0 || kind > 3 || iters < 1 || iters > 65536 || reps < 1) {
    g_err = "mfma_burn: kind 0..3, 1 <= iters <= 65536, reps >= 1";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  static const int kK[4] = {32, 128, 128, 128};
  const int K = kK[kind], per = K / 4;
  // a lane's final sum is bounded by 16 outputs * K * 4 MFMA per accumulator-iteration * iters
  if (16.0 * K * 4 * iters >= 16777216.0) {
    g_err = "mfma_burn: iters too large for an exact fp32 check (< 2048 at K=128, < 8192 at K=32)";
    return -2;
  }
  // operands in {-1, 0, +1}, per lane (the same in every wave, so every wave has the same answer)
  uint64_t st = 0x9E3779B97F4A7C15ULL ^ static_cast<uint64_t>(kind);
  auto rnd3 = [&st]() {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return static_cast<int>(st % 3) - 1;
  };
  std::vector<int> va(64 * per), vb(64 * per);
  for (int& x : va) x = rnd3();
  for (int& x : vb) x = rnd3();
  std::vector<uint8_t> fa(64 * 32, 0), fb(64 * 32, 0);
  auto encode = [&](std::vector<uint8_t>& f, const std::vector<int>& v) {
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < per; ++e) {
        const int x = v[l * per + e];
        if (kind == 0) {
          const uint16_t bits = x == 0 ? 0 : (x > 0 ? 0x3F80 : 0xBF80);
          memcpy(&f[l * 32 + 2 * e], &bits, 2);
        } else if (kind == 3) {
          const uint8_t nib = x == 0 ? 0 : (x > 0 ? 0x2 : 0xA);
          f[l * 32 + e / 2] |= static_cast<uint8_t>(nib << ((e & 1) ? 4 : 0));
        } else {
          f[l * 32 + e] = x == 0 ? 0 : (x > 0 ? 0x38 : 0xB8);
        }
      }
  };
  encode(fa, va);
  encode(fb, vb);
  // host reference: C_xy[i][j] = sum_k x(lane i + 16(k/per), k%per) * y(lane j + 16(k/per), k%per)
  auto prod = [&](const std::vector<int>& x, const std::vector<int>& y, int i, int j) {
    long acc = 0;
    for (int k = 0; k < K; ++k) acc += static_cast<long>(x[(i + 16 * (k / per)) * per + k % per]) *
                                       y[(j + 16 * (k / per)) * per + k % per];
    return acc;
  };
  std::vector<float> expect(64);
  for (int l = 0; l < 64; ++l) {
    long tot = 0;
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * (l >> 4) + r, col = l & 15;
      tot += prod(va, vb, row, col) + prod(vb, va, row, col) + prod(va, va, row, col) + prod(vb, vb, row, col);
    }
    expect[l] = static_cast<float>(tot * 4L * iters);  // exact: bounded below 2^24 by the check above
  }
  DevBuf dfa, dfb, dex;
  HIP_CHECK(dfa.alloc(device, fa.size()));
  HIP_CHECK(dfb.alloc(device, fb.size()));
  HIP_CHECK(dex.alloc(device, expect.size() * sizeof(float)));
  HIP_CHECK(hipMemcpy(dfa.ptr, fa.data(), fa.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dfb.ptr, fb.data(), fb.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dex.ptr, expect.data(), expect.size() * sizeof(float), hipMemcpyHostToDevice));
  const int blocks = grid_for(device, 2);  // 8 waves per CU = 2 per SIMD
  if (inject_block >= blocks) {
    g_err = "mfma_burn: inject_block outside the grid";
    return -2;
  }
  auto launch = [&](int inj, unsigned long long* c, unsigned long long* m) {
    const i32x8* a = static_cast<const i32x8*>(dfa.ptr);
    const i32x8* b = static_cast<const i32x8*>(dfb.ptr);
    const float* ex = static_cast<const float*>(dex.ptr);
    switch (kind) {
      case 0: hipLaunchKernelGGL(mfma_burn_kernel<0>, dim3(blocks), dim3(256), 0, nullptr, a, b, ex, iters, inj, c, m); break;
      case 1: hipLaunchKernelGGL(mfma_burn_kernel<1>, dim3(blocks), dim3(256), 0, nullptr, a, b, ex, iters, inj, c, m); break;
      case 2: hipLaunchKernelGGL(mfma_burn_kernel<2>, dim3(blocks), dim3(256), 0, nullptr, a, b, ex, iters, inj, c, m); break;
      default: hipLaunchKernelGGL(mfma_burn_kernel<3>, dim3(blocks), dim3(256), 0, nullptr, a, b, ex, iters, inj, c, m);
    }
  };
  float ms = 0.f;
  if (const int rc = burn_run(device, reps, inject_block, launch, errors, cu_map, &ms)) return rc;
  const double flop = static_cast<double>(blocks) * 4 /*waves*/ * iters * 16 /*MFMA per iter*/ * 2.0 * 16 * 16 * K;
  *tflops = ms > 0.f ? flop * reps / (ms * 1e-3) / 1e12 : 0.0;
  return 0;
}

// LDS test over `rounds` x CUs workgroups of the largest LDS allocation a workgroup may take.
// cu_map: BURN_SLOTS x 2 (workgroups run, bad words) per physical CU slot; *lds_bytes = bytes per CU tested.
int diag_lds_test(int device, int rounds, uint32_t seed, int inject_block, unsigned long long* errors,
                  unsigned long long* cu_map, int* lds_bytes, double* ms) {
  if (rounds < 1 || rounds > 64) {
    g_err = "lds_test: 1 <= rounds <= 64";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  int max_lds = 0;
  HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  if (max_lds < 65536 || max_lds > (1 << 20)) {
    g_err = "lds_test: unexpected LDS size " + std::to_string(max_lds);
    return -2;
  }
  // the kernel's own 4-byte counter shares the allocation
  const uint32_t dyn = static_cast<uint32_t>(max_lds) - 16u;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_test_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(dyn)));
  ErrMap em;
  if (em.alloc(device, BURN_SLOTS, 2) || em.zero()) return -1;
  const int blocks = grid_for(device, rounds);
  Timer tm;
  HIP_CHECK(tm.create());
  float t_ms = 0.f;
  const auto launch = [&] {
    hipLaunchKernelGGL(lds_test_kernel, dim3(blocks), dim3(1024), dyn, nullptr, dyn / 4u, seed, inject_block,
                       em.errors(), em.map());
    return 0;
  };
  if (const int rc = tm.timed(launch, &t_ms)) return rc;
  *ms = t_ms;
  *lds_bytes = static_cast<int>(dyn);
  return em.read(errors, cu_map);
}

// Register-file test over `rounds` x CUs workgroups of four 512-register waves (one per SIMD of a CU), each word held
// for `hold` x 512 clocks between write and read-back.  simd_map: diag_regfile_slots() x 3 (waves run, bad VGPR
// words, bad AGPR words) per physical SIMD (wave_slot() << 2 | SIMD_ID); *regs_per_lane = registers of a lane under
// a pattern at once; *scratch_bytes = the kernel's private segment, and anything but 0 is an error: such a build
// would test scratch memory.  `inject_block` >= 0 (the verifier's self-check): one bit of register `inject_reg`
// (0 / 1 lowest / highest tested VGPR, 2 / 3 lowest / highest tested AGPR) of lane 0 of wave 0 of that workgroup is
// flipped between the write and the check of the first pattern.
int diag_regfile_slots(void) { return RF_SLOTS; }

int diag_regfile_test(int device, int rounds, uint32_t seed, int hold, int inject_block, int inject_reg,
                      unsigned long long* errors, unsigned long long* simd_map, int* regs_per_lane, int* scratch_bytes,
                      double* ms) {
  if (rounds < 1 || rounds > 64 || hold < 0 || hold > 65536) {
    g_err = "regfile_test: 1 <= rounds <= 64, 0 <= hold <= 65536";
    return -2;
  }
  if (inject_block >= 0 && (inject_reg < 0 || inject_reg > 3)) {
    g_err = "regfile_test: inject_reg 0..3 (lowest / highest VGPR, lowest / highest AGPR)";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  hipFuncAttributes attr;
  HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(regfile_test_kernel)));
  *regs_per_lane = RF_REGS;
  *scratch_bytes = static_cast<int>(attr.localSizeBytes);
  if (attr.localSizeBytes != 0) {
    g_err = "regfile_test: the kernel was built with " + std::to_string(attr.localSizeBytes) +
            " bytes of scratch per lane: it would test memory, not registers";
    return -3;
  }
  const int blocks = grid_for(device, rounds);
  if (inject_block >= blocks) {
    g_err = "regfile_test: inject_block outside the grid";
    return -2;
  }
  ErrMap em;
  if (em.alloc(device, RF_SLOTS, 3) || em.zero()) return -1;
  Timer tm;
  HIP_CHECK(tm.create());
  float t_ms = 0.f;
  const auto launch = [&] {
    hipLaunchKernelGGL(regfile_test_kernel, dim3(blocks), dim3(256), 0, nullptr, seed, hold, inject_block,
                       inject_reg, em.errors(), em.map());
    return 0;
  };
  if (const int rc = tm.timed(launch, &t_ms)) return rc;
  *ms = t_ms;
  return em.read(errors, simd_map);
}

// Vector-ALU burn-in of one kind (0 f64, 1 pk_f32, 2 i32; valu_burn_kernel): `reps` timed launches of `iters`
// iterations on every CU after a checked warm-up; *gops = G(FL)OP/s (an FMA or a multiply-add counts 2 per element),
// *errors = lanes whose final values differ from the host's in any bit; cu_map as diag_mfma_burn's (BURN_SLOTS
// x 3).  `inject_block` >= 0 (the verifier's self-check): lane 0 of wave 0 of that workgroup is made wrong in the
// warm-up launch; -1 = no hook.
int diag_valu_burn(int device, int kind, int iters, int reps, int inject_block, double* gops,
                   unsigned long long* errors, unsigned long long* cu_map) {
  if (kind < 0 || kind >= VALU_KINDS || iters < 1 || iters > 65536 || reps < 1) {
    g_err = "valu_burn: kind 0..2, 1 <= iters <= 65536, reps >= 1";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  const int blocks = grid_for(device, 2);  // 8 waves per CU = 2 per SIMD
  if (inject_block >= blocks) {
    g_err = "valu_burn: inject_block outside the grid";
    return -2;
  }
  // per lane (the same in every wave, so every wave has the same answer)
  std::vector<uint64_t> ops(3 * VALU_LANES * VALU_CHAINS), expect(VALU_LANES * VALU_CHAINS);
  valu_tables(kind, static_cast<long>(iters) * VALU_UNROLL, ops.data(), expect.data());
  DevBuf dops, dex;
  HIP_CHECK(dops.alloc(device, ops.size() * 8));
  HIP_CHECK(dex.alloc(device, expect.size() * 8));
  HIP_CHECK(hipMemcpy(dops.ptr, ops.data(), ops.size() * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dex.ptr, expect.data(), expect.size() * 8, hipMemcpyHostToDevice));
  auto launch = [&](int inj, unsigned long long* c, unsigned long long* m) {
    const uint64_t* o = static_cast<const uint64_t*>(dops.ptr);
    const uint64_t* ex = static_cast<const uint64_t*>(dex.ptr);
    switch (kind) {
      case 0: hipLaunchKernelGGL(valu_burn_kernel<0>, dim3(blocks), dim3(256), 0, nullptr, o, ex, iters, inj, c, m); break;
      case 1: hipLaunchKernelGGL(valu_burn_kernel<1>, dim3(blocks), dim3(256), 0, nullptr, o, ex, iters, inj, c, m); break;
      default: hipLaunchKernelGGL(valu_burn_kernel<2>, dim3(blocks), dim3(256), 0, nullptr, o, ex, iters, inj, c, m);
    }
  };
  float ms = 0.f;
  if (const int rc = burn_run(device, reps, inject_block, launch, errors, cu_map, &ms)) return rc;
  const double per_step = kind == 1 ? 4.0 : 2.0;  // a float2 FMA is two FMAs
  const double op = static_cast<double>(blocks) * 256 * iters * VALU_UNROLL * VALU_CHAINS * per_step;
  *gops = ms > 0.f ? op * reps / (ms * 1e-3) / 1e9 : 0.0;
  return 0;
}

// L2 read bandwidth per XCD: 8 slices of `slice_bytes` (one per XCD id), `passes` reads of its slice by
// every workgroup, `blocks_per_cu` workgroups of 4 waves per CU.  *tbs = aggregate bytes read / timed launch; cu_map as
// diag_mfma_burn's (BURN_SLOTS x 3).  `inject_xcd` >= 0 (the verifier's self-check): flip_slice_word; -1 = no hook.
int diag_l2_bandwidth(int device, size_t slice_bytes, int passes, int blocks_per_cu, uint32_t seed, int inject_xcd,
                      long long inject_word, double* tbs, unsigned long long* errors, unsigned long long* cu_map) {
  if (slice_bytes < 4096 || slice_bytes > (64u << 20) || slice_bytes % 16 || passes < 1 || passes > 1024 ||
      blocks_per_cu < 1 || blocks_per_cu > 8) {
    g_err = "l2_bandwidth: 4 KiB <= slice_bytes <= 64 MiB (multiple of 16), 1 <= passes <= 1024, 1..8 blocks/CU";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  const uint32_t slice_vec = static_cast<uint32_t>(slice_bytes / 16);
  const uint32_t n_vec = 8u * slice_vec;  // XCC_ID is 0..7
  DevBuf dbuf;
  ErrMap em;
  HIP_CHECK(dbuf.alloc(device, static_cast<size_t>(n_vec) * 16));
  if (em.alloc(device, BURN_SLOTS, 3)) return -1;
  hipLaunchKernelGGL(l2_fill_kernel, dim3(1024), dim3(256), 0, nullptr, static_cast<uint4*>(dbuf.ptr), n_vec, seed);
  HIP_CHECK(hipGetLastError());
  if (const int rc = flip_slice_word(dbuf.ptr, slice_vec, inject_xcd, inject_word, "l2_bandwidth")) return rc;
  const int blocks = grid_for(device, blocks_per_cu);
  const auto launch = [&] {
    hipLaunchKernelGGL(l2_read_kernel, dim3(blocks), dim3(256), 0, nullptr, static_cast<const uint4*>(dbuf.ptr),
                       slice_vec, passes, seed, em.errors(), em.map());
    return 0;
  };
  launch();  // untimed: brings every slice into its XCD's L2 (its counts are cleared below)
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (em.zero()) return -1;
  Timer tm;
  HIP_CHECK(tm.create());
  float ms = 0.f;
  if (const int rc = tm.timed(launch, &ms)) return rc;
  if (em.read(errors, cu_map)) return -1;
  const double bytes = static_cast<double>(blocks) * passes * static_cast<double>(slice_bytes);
  *tbs = ms > 0.f ? bytes / (ms * 1e-3) / 1e12 : 0.0;
  return 0;
}

// HBM per XCD (hbm_xcd_kernel): `slice_bytes` per XCD (8 slices, a multiple of 128 KiB, at most 512 MiB),
// read `passes` times by the XCD's own workgroups, all XCDs at once: aggregate read TB/s, wrong words,
// per-CU map.  With `xcd_tbs` (8 doubles) each XCD then streams its slice alone: its own read TB/s (0 for an
// XCD without CUs on this device).  *errors counts the timed full-chip run and the lone runs; cu_map is the timed
// full-chip run's.  `inject_xcd` >= 0 (the verifier's self-check): flip_slice_word; -1 = no hook.  xcd_tbs may be null.
int diag_hbm_xcd(int device, size_t slice_bytes, int passes, int blocks_per_cu, uint32_t seed, int inject_xcd,
                 long long inject_word, double* tbs, unsigned long long* errors, unsigned long long* cu_map,
                 double* xcd_tbs) {
  const size_t chunk = static_cast<size_t>(HBM_XCD_CHUNK_VEC) * 16;
  if (slice_bytes < chunk || slice_bytes > (512u << 20) || slice_bytes % chunk || passes < 1 || passes > 64 ||
      blocks_per_cu < 1 || blocks_per_cu > 8) {
    g_err = "hbm_xcd: 128 KiB <= slice_bytes <= 512 MiB (multiple of 128 KiB), 1 <= passes <= 64, 1..8 blocks/CU";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  const uint32_t slice_vec = static_cast<uint32_t>(slice_bytes / 16);
  const uint32_t n_vec = 8u * slice_vec;  // XCC_ID is 0..7; 8 x 512 MiB keeps word indices in 32 bits
  DevBuf dbuf, dnext;
  ErrMap em;
  HIP_CHECK(dbuf.alloc(device, static_cast<size_t>(n_vec) * 16));
  HIP_CHECK(dnext.alloc(device, 8 * sizeof(unsigned int)));
  if (em.alloc(device, BURN_SLOTS, 3)) return -1;
  hipLaunchKernelGGL(l2_fill_kernel, dim3(4096), dim3(256), 0, nullptr, static_cast<uint4*>(dbuf.ptr), n_vec, seed);
  HIP_CHECK(hipGetLastError());
  if (const int rc = flip_slice_word(dbuf.ptr, slice_vec, inject_xcd, inject_word, "hbm_xcd")) return rc;
  const int blocks = grid_for(device, blocks_per_cu);
  Timer tm;
  HIP_CHECK(tm.create());
  // one timed run (the queue counters reset first); returns its milliseconds, < 0 on a HIP error
  auto timed = [&](int only_xcd) -> float {
    if (hipMemset(dnext.ptr, 0, 8 * sizeof(unsigned int)) != hipSuccess) return -1.f;
    if (hipEventRecord(tm.e0, nullptr) != hipSuccess) return -1.f;
    hipLaunchKernelGGL(hbm_xcd_kernel, dim3(blocks), dim3(256), 0, nullptr, static_cast<const uint4*>(dbuf.ptr),
                       slice_vec, passes, seed, only_xcd, static_cast<unsigned int*>(dnext.ptr), em.errors(),
                       em.map());
    if (hipGetLastError() != hipSuccess || hipEventRecord(tm.e1, nullptr) != hipSuccess ||
        hipEventSynchronize(tm.e1) != hipSuccess)
      return -1.f;
    return elapsed_ms(tm.e0, tm.e1);
  };
  if (timed(-1) < 0.f) HIP_CHECK(hipGetLastError());  // untimed warm-up: page tables, clocks up
  if (em.zero()) return -1;
  const float ms = timed(-1);
  if (ms < 0.f) {
    HIP_CHECK(hipGetLastError());
    g_err = "hbm_xcd: timed run failed";
    return -1;
  }
  if (em.read(nullptr, cu_map)) return -1;  // the timed full-chip run's map; the count goes on through the lone runs
  // bytes actually read: every XCD that has CUs reads its slice `passes` times
  bool present[8] = {false, false, false, false, false, false, false, false};
  int xcds_seen = 0;
  for (int x = 0; x < 8; ++x) {
    for (int sl = 0; sl < 128 && !present[x]; ++sl) present[x] = cu_map[3 * (x * 128 + sl)] != 0;
    xcds_seen += present[x];
  }
  const double bytes = static_cast<double>(xcds_seen) * passes * static_cast<double>(slice_bytes);
  *tbs = ms > 0.f ? bytes / (ms * 1e-3) / 1e12 : 0.0;
  if (xcd_tbs != nullptr) {
    // untimed: the first lone-XCD run of a process measured ~8 % low (one XCD's clocks and queues ramping
    // after the full-chip run), so the first present XCD streams once before the timed ones
    for (int x = 0; x < 8; ++x)
      if (present[x]) {
        if (timed(x) < 0.f) HIP_CHECK(hipGetLastError());
        break;
      }
    for (int x = 0; x < 8; ++x) {
      xcd_tbs[x] = 0.0;
      if (!present[x]) continue;
      const float xms = timed(x);
      if (xms < 0.f) {
        HIP_CHECK(hipGetLastError());
        g_err = "hbm_xcd: isolated run failed";
        return -1;
      }
      xcd_tbs[x] = xms > 0.f ? passes * static_cast<double>(slice_bytes) / (xms * 1e-3) / 1e12 : 0.0;
    }
  }
  return em.read(errors, nullptr);
}

// Host link check: pinned host <-> device copies of `bytes`, `iters` each way (SDMA over PCIe),
// timed with events.  A slot trained down to x8 / an older generation shows up here at half rate.
int diag_host_link(int device, size_t bytes, int iters, double* h2d_gbps, double* d2h_gbps) {
  if (bytes < 4096 || iters < 1) {
    g_err = "host_link: bytes >= 4096 and iters >= 1";
    return -2;
  }
  HIP_CHECK(hipSetDevice(device));
  void* host = nullptr;
  HIP_CHECK(hipHostMalloc(&host, bytes, hipHostMallocDefault));
  struct HostFree {
    void* p;
    ~HostFree() { (void)hipHostFree(p); }
  } hf{host};
  memset(host, 0x5A, bytes);
  DevBuf dev;
  HIP_CHECK(dev.alloc(device, bytes));
  // on the null stream, as every single-device test: a stream of its own would be one more hardware queue, and each
  // queue the runtime creates holds ~170 MiB of host memory for the rest of the process (tools/hip_rss_probe.hip)
  Timer tm;
  HIP_CHECK(tm.create());
  for (int dir = 0; dir < 2; ++dir) {
    auto copy = [&]() {
      return dir == 0 ? hipMemcpyAsync(dev.ptr, host, bytes, hipMemcpyHostToDevice, nullptr)
                      : hipMemcpyAsync(host, dev.ptr, bytes, hipMemcpyDeviceToHost, nullptr);
    };
    HIP_CHECK(copy());  // warm-up
    const auto copies = [&]() -> int {
      for (int i = 0; i < iters; ++i) HIP_CHECK(copy());
      return 0;
    };
    float ms = 0.f;
    if (const int rc = tm.timed(copies, &ms)) return rc;
    const double gbps = ms > 0.f ? static_cast<double>(iters) * static_cast<double>(bytes) / (ms * 1e-3) / 1e9 : 0.0;
    *(dir == 0 ? h2d_gbps : d2h_gbps) = gbps;
  }
  return 0;
}

}  // extern "C"
