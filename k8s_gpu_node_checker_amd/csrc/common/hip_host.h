// The host-side HIP plumbing every diagnostic library shares: the error string behind *_last_error(), the checked
// call, the current-device scope, device allocations, timing events, polled completion, peer access, the self-check's
// bit flip and a wave's physical location.  simd_report.h builds the SIMD-located diagnostics' report on it.
//
// Include it from exactly one translation unit per library.  Everything lives in an anonymous namespace, so each
// .so keeps its own g_err (and with it its own *_last_error()) and exports none of this.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <string>
#include <thread>

namespace {

thread_local std::string g_err;  // what failed in the calling thread's last entry point

// Every HIP call goes through this: on failure the enclosing function returns -1 and g_err names the call.
#define HIP_CHECK(expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      (void)hipGetLastError(); /* a failed allocation must not fail the next call's check */ \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
      return -1;                                                                          \
    }                                                                                     \
  } while (0)

// HIP devices visible to the process; 0 when the runtime cannot say (no error is left behind)
inline int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

inline int cu_count(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    cus = 256;  // the MI355X's CU count (a grid size only: any value is correct, this one fills the chip)
  }
  return cus;
}

// The time between two completed events, for HIP_CHECK: a failure is reported as the error it is
inline hipError_t event_ms(hipEvent_t a, hipEvent_t b, float* ms) {
  *ms = 0.f;
  return hipEventElapsedTime(ms, a, b);
}

// The calling thread's current device for the length of an entry point: `device` once enter() returned 0, the
// caller's own again on every return path, a refusal or a failed HIP call included.
struct DeviceScope {
  int cur = -1;
  DeviceScope() = default;
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  int enter(int device) {
    int c = 0;
    HIP_CHECK(hipGetDevice(&c));
    cur = c;
    HIP_CHECK(hipSetDevice(device));
    return 0;
  }
  ~DeviceScope() {
    if (cur >= 0) (void)hipSetDevice(cur);
  }
};

// Device allocation owned by its device: freed on every return path, with that device current.
struct DevBuf {
  int device = -1;
  void* ptr = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  hipError_t alloc(int dev, size_t bytes) {
    device = dev;
    hipError_t e = hipSetDevice(dev);
    return e != hipSuccess ? e : hipMalloc(&ptr, bytes);
  }
  ~DevBuf() {
    if (ptr) {
      int cur = 0;
      if (hipGetDevice(&cur) == hipSuccess && hipSetDevice(device) == hipSuccess) {
        (void)hipFree(ptr);
        (void)hipSetDevice(cur);
      }
    }
  }
};

// A pair of timing events and an optional stream, released on every return path: the agent calls the entry
// points for the life of its pod, so an early HIP_CHECK return must not leak them.
struct Timer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t stream = nullptr;
  Timer() = default;
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  hipError_t create(bool own_stream = false) {
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess && own_stream) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    return e;
  }
  ~Timer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
  }
  // One timed section on stream `st`: record, `enqueue()` (queues the work; 0, or a negative code with g_err set),
  // record, wait for it, check the last error.  0 with the section's milliseconds in *ms, else a negative code.
  template <typename F>
  int timed(F&& enqueue, float* ms, hipStream_t st = nullptr) {
    HIP_CHECK(hipEventRecord(e0, st));
    if (const int rc = enqueue()) return rc;
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(event_ms(e0, e1, ms));
    return 0;
  }
};

inline hipError_t enable_peer(int from, int to) {
  hipError_t e = hipSetDevice(from);
  if (e != hipSuccess) return e;
  e = hipDeviceEnablePeerAccess(to, 0);
  if (e == hipErrorPeerAccessAlreadyEnabled) {
    (void)hipGetLastError();  // sticky-free: clear it
    return hipSuccess;
  }
  return e;
}

// Polled completion with a deadline: a hung copy engine or link must not block the caller.
using SteadyClock = std::chrono::steady_clock;
struct PollDeadline {
  double limit_ms;
  SteadyClock::time_point t0 = SteadyClock::now();
  explicit PollDeadline(double ms) : limit_ms(ms) {}
  bool bounded() const { return limit_ms > 0.0; }
  bool passed() const {
    return bounded() && std::chrono::duration<double, std::milli>(SteadyClock::now() - t0).count() >= limit_ms;
  }
};
// hipSuccess once `ev` completed, hipErrorNotReady when the deadline passed first, else the query's error.
inline hipError_t wait_event_polled(hipEvent_t ev, const PollDeadline& dl) {
  if (!dl.bounded()) return hipEventSynchronize(ev);
  for (;;) {
    hipError_t q = hipEventQuery(ev);
    if (q != hipErrorNotReady) return q;
    if (dl.passed()) return hipErrorNotReady;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

// The verifiers' self-check: bit 4 of the 32-bit word at device address `w` is flipped from the host, with the
// word's device current.  The caller checks that `w` lies inside its buffer.
inline int flip_word_bit(uint32_t* w) {
  uint32_t v = 0;
  HIP_CHECK(hipMemcpy(&v, w, sizeof v, hipMemcpyDeviceToHost));
  v ^= 0x10u;
  HIP_CHECK(hipMemcpy(w, &v, sizeof v, hipMemcpyHostToDevice));
  return 0;
}

// The 64 -> 32 bit hash of the address patterns and fills (murmur3's finalizer)
__device__ __forceinline__ uint32_t mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// Physical location of the calling wave: XCD (XCC_ID), shader engine, shader array and CU (HW_ID), packed
// as xcd<<7 | se<<5 | sh<<4 | cu -- one of WAVE_SLOTS slots; the CUs of one MI355X occupy 256 of them.
constexpr int WAVE_SLOTS = 1024;
__device__ __forceinline__ unsigned wave_slot() {
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);   // HW_ID, all 32 bits
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // XCC_ID[3:0]
  return ((xcc & 7u) << 7) | (((hw >> 13) & 3u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);
}

// ... and its SIMD inside that CU: wave_slot() << 2 | HW_ID.SIMD_ID, one of SIMD_ROWS rows of a SIMD map.  A row has
// SIMD_MAP_COLS columns: waves run, then two counters of the map's owner (the register-file test: wrong VGPR and wrong
// AGPR words; simd_report.h: wrong words and summed wall_clock64 ticks).
constexpr int SIMD_ROWS = WAVE_SLOTS * 4;
constexpr int SIMD_MAP_COLS = 3;
__device__ __forceinline__ unsigned simd_row() {
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);  // HW_ID; SIMD_ID = bits 5:4
  return (wave_slot() << 2) | ((hw >> 4) & 3u);
}

}  // namespace
