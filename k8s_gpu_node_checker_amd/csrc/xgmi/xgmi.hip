// libmi355x_xgmi.so: the kernel-driven xGMI test (HIP, gfx950).
//
// The copy-engine path (diag_p2p_copy / diag_p2p_fan in csrc/diag/diag.hip) moves every byte with
// hipMemcpyPeerAsync, so a slow result there is a slow link OR a slow SDMA engine.  RCCL, which every real job
// runs, loads the links with loads and stores issued by the CUs; this library does the same.  One source GPU
// writes into (or reads from) a buffer on each of its peers from a kernel, verifies every byte, and times each
// destination with the wall clock.  ops/xgmi.py is its Python side; ops/diag.p2p_matrix(kernel=True) sets its
// rates next to the copy path's to tell a link from an engine.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../common/hip_host.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // native 16-byte vector (one dwordx4 access)

constexpr int kMaxFan = 64;       // a CPX hive: 63 peers
constexpr unsigned THREADS = 256;
constexpr unsigned U = 8;         // independent 16-byte accesses in flight per lane (as l2_read_kernel)
constexpr size_t CHUNK = static_cast<size_t>(U) * THREADS;  // elements one workgroup moves per step: 32 KiB
constexpr int XCDS = 8;
constexpr int SLOT_WORDS = 4;     // per destination: first start, last end, bad elements, lowest bad element

// the address-hash pattern of the memtest and the copy-path pair test: element i holds four hashed words
__device__ __forceinline__ u32x4 pattern(size_t i, uint64_t seed) {
  u32x4 v;
  v.x = mix32(4 * i + seed);
  v.y = mix32(4 * i + 1 + seed);
  v.z = mix32(4 * i + 2 + seed);
  v.w = mix32(4 * i + 3 + seed);
  return v;
}

__device__ __host__ __forceinline__ uint64_t dst_seed(uint64_t seed, int d) {
  return seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(d + 1);
}

struct FanArgs {
  u32x4* buf[kMaxFan];  // destination i's buffer (peer memory, or src's own when dsts[i] == src)
};

// One launch on `src` serves every destination (a stream per destination would be capped by the process's
// hardware queues: 4 by default, so seven peers could never run together).
//
// Mapping of workgroups to destinations.  The hardware deals workgroups round-robin to the 8 XCDs (workgroup b
// runs on XCD b % 8), so `b % ndst` would pin a destination to a subset of the XCDs whenever ndst shares a factor
// with 8.  Instead 8 consecutive workgroups -- one per XCD -- form a group, and the groups are dealt round-robin
// to the destinations:
//     group g = b / 8,  destination d = g % ndst,  rank within d:  r = (g / ndst) * 8 + b % 8.
// The grid is 8 * ndst * groups workgroups, so every destination owns `groups` workgroups on each XCD, whatever
// ndst is.  Rank r of a destination's W = 8 * groups workgroups moves chunks r, r + W, ... of CHUNK elements; the
// last chunk may be short (every access of it is bounds-checked).
//
// MODE 0, store: the lane forms pattern(i, seed_d) in registers and stores it into the peer's buffer.  No source
// buffer is read, so the rate is the link's write rate alone.  Plain stores: 16 bytes per lane, 8 per lane issued
// back to back.
// MODE 1, load: the lane reads the peer's buffer and compares every element in registers; bad elements and the
// lowest bad index go to the destination's slot in src-local memory.  The loads are nontemporal
// (__builtin_nontemporal_load -> global_load_dwordx4 ... nt), the one non-default flavour a 16-byte load can be
// given from C++: like sc1 loads they bypass the CU's L1, so nothing read in one iteration is served from src's
// L1 in the next, and they cost 0-3 % against plain loads at 16 bytes.  Neither flavour bypasses the L2: what keeps
// an iteration from being served out of src's 8 x 4 MiB of L2 is the buffer's size (256 MiB by default) together
// with nt marking the lines as streaming, so a small test buffer may be re-read from L2 (its rate is not a link
// rate; its verification is unaffected, as the buffer does not change between iterations).
//
// Timing: every workgroup that moves at least one element stamps the wall clock (the constant-rate counter of the
// burn-in kernels, 10 ns ticks) before its first access and after its last has completed (each wave waits for
// its own accesses, then the workgroup's barrier), and folds the stamps into its destination's slot with
// atomicMin / atomicMax.  A workgroup without work would only widen the window with its scheduling time.
template <int MODE>
__global__ void __launch_bounds__(THREADS) fan_kernel(FanArgs args, int ndst, unsigned groups, size_t nvec,
                                                      uint64_t seed, unsigned long long* slots) {
  const unsigned g = blockIdx.x / XCDS;
  const int d = static_cast<int>(g % static_cast<unsigned>(ndst));
  const size_t rank = static_cast<size_t>(g / static_cast<unsigned>(ndst)) * XCDS + blockIdx.x % XCDS;
  const size_t wgs = static_cast<size_t>(groups) * XCDS;
  const size_t nchunks = (nvec + CHUNK - 1) / CHUNK;
  if (rank >= nchunks) return;  // uniform per workgroup: no barrier is skipped by part of it
  unsigned long long* slot = slots + SLOT_WORDS * d;
  const long long t0 = wall_clock64();
  u32x4* __restrict__ buf = args.buf[d];
  const uint64_t sd = dst_seed(seed, d);
  unsigned int bad = 0;
  unsigned long long first = ~0ULL;
  for (size_t c = rank; c < nchunks; c += wgs) {
    const size_t base = c * CHUNK + threadIdx.x;
    if ((c + 1) * CHUNK <= nvec) {
      if constexpr (MODE == 0) {
        u32x4 v[U];
#pragma unroll
        for (unsigned k = 0; k < U; ++k) v[k] = pattern(base + k * THREADS, sd);
#pragma unroll
        for (unsigned k = 0; k < U; ++k) buf[base + k * THREADS] = v[k];
      } else {
        u32x4 v[U];
#pragma unroll
        for (unsigned k = 0; k < U; ++k) v[k] = __builtin_nontemporal_load(buf + base + k * THREADS);
#pragma unroll
        for (unsigned k = 0; k < U; ++k) {
          const size_t i = base + k * THREADS;
          const u32x4 e = pattern(i, sd);
          if (v[k].x != e.x || v[k].y != e.y || v[k].z != e.z || v[k].w != e.w) {
            ++bad;
            first = first < i ? first : i;
          }
        }
      }
    } else {  // the ragged last chunk
      for (unsigned k = 0; k < U; ++k) {
        const size_t i = base + k * THREADS;
        if (i >= nvec) break;
        if constexpr (MODE == 0) {
          buf[i] = pattern(i, sd);
        } else {
          const u32x4 v = __builtin_nontemporal_load(buf + i);
          const u32x4 e = pattern(i, sd);
          if (v.x != e.x || v.y != e.y || v.z != e.z || v.w != e.w) {
            ++bad;
            first = first < i ? first : i;
          }
        }
      }
    }
  }
  if (bad) {  // rare: vector atomics into src-local memory, one per lane that saw a bad element
    atomicAdd(slot + 2, static_cast<unsigned long long>(bad));
    atomicMin(slot + 3, first);
  }
  // s_waitcnt vmcnt(0) (gfx9 encoding: expcnt and lgkmcnt left at their maxima): this wave's stores have been
  // acknowledged ...  (a workgroup-scope fence emits no wait on gfx950, so the wait is asked for by name)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();  // ... and so have every other wave's of the workgroup
  if (threadIdx.x == 0) {
    atomicMin(slot, static_cast<unsigned long long>(t0));
    atomicMax(slot + 1, static_cast<unsigned long long>(wall_clock64()));
  }
}

__global__ void __launch_bounds__(THREADS) fill_kernel(u32x4* p, size_t n, uint64_t seed) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride)
    p[i] = pattern(i, seed);
}

__global__ void __launch_bounds__(THREADS) verify_kernel(const u32x4* p, size_t n, uint64_t seed,
                                                         unsigned long long* errors, unsigned long long* first_bad) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    const u32x4 v = p[i];
    const u32x4 e = pattern(i, seed);
    if (v.x != e.x || v.y != e.y || v.z != e.z || v.w != e.w) {
      atomicAdd(errors, 1ULL);
      atomicMin(first_bad, static_cast<unsigned long long>(i));
    }
  }
}

// grid of the grid-stride fill / verify kernels: 4 workgroups per CU, never more than one thread per element
unsigned flat_grid(int device, size_t n) {
  return static_cast<unsigned>(std::min<size_t>((n + THREADS - 1) / THREADS, static_cast<size_t>(cu_count(device)) * 4));
}

// Self-check hook: one bit of 32-bit word `word` of `buf` is flipped from the host (the entry point checks the range).
int flip_word(void* buf, long long word) { return flip_word_bit(static_cast<uint32_t*>(buf) + word); }

}  // namespace

extern "C" {

const char* xgmi_last_error(void) { return g_err.c_str(); }

int xgmi_device_count(void) { return device_count(); }

// `src` stores to (mode 0) or loads from (mode 1) a buffer of `bytes` (rounded down to 16) on every one of the
// `ndst` devices in `dsts`, all from ONE kernel launch per iteration on `src` (fan_kernel): ndst = 1 is the pair
// test, ndst > 1 loads every listed link of `src` at once.  dsts[i] may be any valid device; each entry gets its
// own buffer.  `src` itself and repeats are allowed: that is how a one-GPU box runs the kernel, the slicing and the
// verification (its rates are then local-HBM rates, not link rates).
//
// gbps[i]: iters * bytes over (last end - first start) of destination i's workgroups across the timed launches,
// from the wall clock; *total_gbps: all bytes over the HIP-event time of the timed launches.  One untimed warm-up
// launch comes first (it maps the pages).  peer[i] = 1 for src itself, else hipDeviceCanAccessPeer both ways (peer
// access is then enabled, as diag_p2p_fan does); a destination without peer access is refused with -2, as a kernel
// cannot reach it.
//
// Store mode: the destinations start as 0xA5 junk, the seed differs per destination and per iteration, and after
// the last launch each destination verifies its buffer on its own device against the LAST iteration's seed:
// errors[i] = bad 16-byte elements, first_bad[i] = the lowest bad element (~0 when none).  Only the last
// iteration's bytes are verified; every earlier iteration's were overwritten in place.
// Load mode: every destination fills its buffer with its own pattern on its own device; src's lanes compare every
// element of every timed launch in registers, so errors[i] adds up over the `iters` launches.
//
// Self-check hook, inject_dst >= 0 (-1: none): the host flips one bit of 32-bit word `inject_word` of that
// destination's buffer -- in store mode after the last launch and before the verification (1 error, first_bad =
// inject_word / 4), in load mode after the fill (the warm-up is not counted: errors = iters).  -2 when the
// destination or the word is out of range.
//
// `timeout_ms` > 0 bounds launches and verification as in diag_p2p_fan: completion is polled, and a miss returns -4
// with the pair named in xgmi_last_error.  On that path every buffer, event and stream is leaked on purpose: a
// kernel still in flight may be writing them.  0 = a blocking wait.
int xgmi_kernel_fan(int src, const int* dsts, int ndst, size_t bytes, int iters, int mode, double timeout_ms,
                    int inject_dst, long long inject_word, double* gbps, unsigned long long* errors,
                    unsigned long long* first_bad, int* peer, double* total_gbps) {
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  if (src < 0 || src >= n || ndst < 1 || ndst > kMaxFan || iters < 1 || bytes < 16 || (mode != 0 && mode != 1)) {
    g_err = "xgmi kernel fan: need a valid source, 1..64 destinations, iters >= 1, bytes >= 16, mode 0 or 1";
    return -2;
  }
  for (int i = 0; i < ndst; ++i)
    if (dsts[i] < 0 || dsts[i] >= n) {
      g_err = "xgmi kernel fan: every destination must be a valid device";
      return -2;
    }
  const size_t nvec = bytes / sizeof(u32x4);
  const size_t nbytes = nvec * sizeof(u32x4);
  if (inject_dst >= ndst || (inject_dst >= 0 && (inject_word < 0 || static_cast<size_t>(inject_word) >= 4 * nvec))) {
    g_err = "xgmi kernel fan: inject_dst below ndst and inject_word inside the buffer";
    return -2;
  }
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  for (int i = 0; i < ndst; ++i) {
    errors[i] = 0;
    first_bad[i] = ~0ULL;
    gbps[i] = 0.0;
    peer[i] = 1;
    if (dsts[i] == src) continue;
    int sd = 0, ds = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&sd, src, dsts[i]));
    HIP_CHECK(hipDeviceCanAccessPeer(&ds, dsts[i], src));
    peer[i] = sd && ds;
    if (!peer[i]) {
      char msg[128];
      std::snprintf(msg, sizeof msg, "xgmi kernel fan %d->%d: no peer access, a kernel on %d cannot reach %d's memory",
                    src, dsts[i], src, dsts[i]);
      g_err = msg;
      return -2;
    }
    HIP_CHECK(enable_peer(src, dsts[i]));
    HIP_CHECK(enable_peer(dsts[i], src));
  }
  *total_gbps = 0.0;
  const uint64_t seed0 = 0x5A17C0DEULL + static_cast<uint64_t>(src) * 131;
  // store mode: iteration `it` (-1 = the warm-up) has its own seed; load mode: one seed, set by the fill
  auto iter_seed = [&](int it) {
    return mode == 0 ? seed0 + 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(it + 2) : seed0;
  };
  DevBuf b[kMaxFan], cnt[kMaxFan], slots;
  FanArgs args = {};
  const unsigned long long cnt_init[2] = {0ULL, ~0ULL};
  for (int i = 0; i < ndst; ++i) {
    HIP_CHECK(b[i].alloc(dsts[i], nbytes));
    args.buf[i] = static_cast<u32x4*>(b[i].ptr);
    if (mode == 0) {
      HIP_CHECK(cnt[i].alloc(dsts[i], sizeof cnt_init));
      HIP_CHECK(hipMemcpy(cnt[i].ptr, cnt_init, sizeof cnt_init, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(b[i].ptr, 0xA5, nbytes));
    } else {
      hipLaunchKernelGGL(fill_kernel, dim3(flat_grid(dsts[i], nvec)), dim3(THREADS), 0, nullptr, args.buf[i], nvec,
                         dst_seed(iter_seed(0), i));
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  }
  if (mode == 1 && inject_dst >= 0) {
    HIP_CHECK(hipSetDevice(dsts[inject_dst]));
    if (const int rc = flip_word(b[inject_dst].ptr, inject_word)) return rc;
  }
  // slots in src-local memory: [0] the warm-up's (discarded), [1] the timed launches'
  HIP_CHECK(hipSetDevice(src));
  unsigned long long slot_init[2][kMaxFan][SLOT_WORDS];
  for (auto& set : slot_init)
    for (auto& s : set) s[0] = ~0ULL, s[1] = 0ULL, s[2] = 0ULL, s[3] = ~0ULL;
  HIP_CHECK(slots.alloc(src, sizeof slot_init));
  HIP_CHECK(hipMemcpy(slots.ptr, slot_init, sizeof slot_init, hipMemcpyHostToDevice));
  HIP_CHECK(hipDeviceSynchronize());
  int clock_khz = 0;  // the wall clock's rate: 100 MHz on the MI355X
  if (hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, src) != hipSuccess || clock_khz <= 0) {
    (void)hipGetLastError();
    clock_khz = 100000;
  }
  // about 4 workgroups per CU in all, a whole number of 8-workgroup groups per destination
  const unsigned groups = std::max(1u, static_cast<unsigned>(cu_count(src)) * 4u / (XCDS * static_cast<unsigned>(ndst)));
  const dim3 grid(XCDS * static_cast<unsigned>(ndst) * groups);
  Timer tm;
  HIP_CHECK(tm.create(true));
  unsigned long long* warm = static_cast<unsigned long long*>(slots.ptr);
  unsigned long long* timed = warm + kMaxFan * SLOT_WORDS;
  auto launch = [&](int it, unsigned long long* sl) {
    if (mode == 0)
      hipLaunchKernelGGL(fan_kernel<0>, grid, dim3(THREADS), 0, tm.stream, args, ndst, groups, nvec, iter_seed(it), sl);
    else
      hipLaunchKernelGGL(fan_kernel<1>, grid, dim3(THREADS), 0, tm.stream, args, ndst, groups, nvec, iter_seed(it), sl);
  };
  launch(-1, warm);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(tm.e0, tm.stream));
  for (int it = 0; it < iters; ++it) launch(it, timed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(tm.e1, tm.stream));
  const PollDeadline dl(timeout_ms);
  Timer verify[kMaxFan];
  auto hung = [&](int i, const char* stage) {
    // the kernel may still be writing these buffers: leak everything rather than free under it
    slots.ptr = nullptr;
    for (int j = 0; j < ndst; ++j) {
      b[j].ptr = cnt[j].ptr = nullptr;
      verify[j].e0 = verify[j].e1 = nullptr;
    }
    tm.e0 = tm.e1 = nullptr;
    tm.stream = nullptr;
    (void)hipSetDevice(cur);
    char msg[192];
    std::snprintf(msg, sizeof msg, "xgmi kernel %s %d->%d: %s did not complete within %.0f ms (xGMI link hung)",
                  mode == 0 ? "store" : "load", src, dsts[i], stage, timeout_ms);
    g_err = msg;
    return -4;
  };
  hipError_t w = wait_event_polled(tm.e1, dl);
  if (w == hipErrorNotReady) return hung(0, "the launches");  // one kernel for all: no destination to single out
  HIP_CHECK(w);
  float ms = 0.f;
  HIP_CHECK(event_ms(tm.e0, tm.e1, &ms));
  *total_gbps = ms > 0.f ? static_cast<double>(ndst) * iters * static_cast<double>(nbytes) / (ms * 1e-3) / 1e9 : 0.0;
  unsigned long long got[kMaxFan][SLOT_WORDS];
  HIP_CHECK(hipMemcpy(got, timed, sizeof got, hipMemcpyDeviceToHost));
  for (int i = 0; i < ndst; ++i) {
    // a window shorter than one tick of the clock counts as one tick
    const unsigned long long ticks = got[i][1] > got[i][0] ? got[i][1] - got[i][0] : 1ULL;
    const double s = static_cast<double>(ticks) / (static_cast<double>(clock_khz) * 1e3);
    gbps[i] = static_cast<double>(iters) * static_cast<double>(nbytes) / s / 1e9;
    if (mode == 1) {
      errors[i] = got[i][2];
      first_bad[i] = got[i][3];
    }
  }
  if (mode == 0) {
    if (inject_dst >= 0) {
      HIP_CHECK(hipSetDevice(dsts[inject_dst]));
      if (const int rc = flip_word(b[inject_dst].ptr, inject_word)) return rc;
    }
    for (int i = 0; i < ndst; ++i) {
      HIP_CHECK(hipSetDevice(dsts[i]));
      HIP_CHECK(verify[i].create(false));
      unsigned long long* c = static_cast<unsigned long long*>(cnt[i].ptr);
      hipLaunchKernelGGL(verify_kernel, dim3(flat_grid(dsts[i], nvec)), dim3(THREADS), 0, nullptr,
                         static_cast<const u32x4*>(b[i].ptr), nvec, dst_seed(iter_seed(iters - 1), i), c, c + 1);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(verify[i].e0, nullptr));
    }
    for (int i = 0; i < ndst; ++i) {
      w = wait_event_polled(verify[i].e0, dl);
      if (w == hipErrorNotReady) return hung(i, "verification");
      HIP_CHECK(w);
      unsigned long long h[2];
      HIP_CHECK(hipSetDevice(dsts[i]));
      HIP_CHECK(hipMemcpy(h, cnt[i].ptr, sizeof h, hipMemcpyDeviceToHost));
      errors[i] = h[0];
      first_bad[i] = h[1];
    }
  }
  HIP_CHECK(hipSetDevice(cur));
  return 0;
}

}  // extern "C"
