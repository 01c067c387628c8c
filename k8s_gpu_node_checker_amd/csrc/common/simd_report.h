// What the SIMD-located diagnostics (lanes, matrix, scalar, vmem) share beyond hip_host.h: the record a launch
// leaves, the end of every kernel that writes it, and the host's run of checked, timed launches around it.
//
// Include it after hip_host.h, from the same one translation unit per library; the same anonymous namespace.
#pragma once

#include <string>

#include "hip_host.h"

namespace {

// what a launch reports besides the map (device memory, zeroed by the host before every launch)
struct Report {
  unsigned long long errors;   // wrong words, in the library's own unit (lanes, elements, registers, bytes)
  unsigned long long claimed;  // 1 once a lane has written the record below
  unsigned long long where;    // packed by the library: the SIMD map row above what locates the word inside the wave
  unsigned long long index;    // the library's own index of the word (0 where `where` says it all)
  unsigned long long got, want;
};

// A lane's `nbad` (> 0) wrong words: added to row `row` of the SIMD map (SIMD_ROWS x SIMD_MAP_COLS: waves run, wrong
// words, summed wall_clock64 ticks) and to the launch's count; one lane of the launch writes the record of its first.
__device__ __forceinline__ void report_wrong(Report* rep, unsigned long long* simd_map, unsigned row, unsigned nbad,
                                             unsigned long long where, unsigned long long index, unsigned long long got,
                                             unsigned long long want) {
  atomicAdd(simd_map + SIMD_MAP_COLS * row + 1, static_cast<unsigned long long>(nbad));
  atomicAdd(&rep->errors, static_cast<unsigned long long>(nbad));
  if (atomicCAS(&rep->claimed, 0ULL, 1ULL) == 0ULL) {
    rep->where = where;
    rep->index = index;
    rep->got = got;
    rep->want = want;
  }
}

// The end of every kernel, on every lane: a lane with wrong words reports them, lane 0 adds its wave and the wave's
// `dt` ticks to its SIMD's row.  A count held per wave is passed on lane 0 alone.  Vector stores and vector atomics
// only, nothing that crosses lanes, no LDS, no scratch.
__device__ __forceinline__ void report(Report* rep, unsigned long long* simd_map, unsigned row, unsigned nbad,
                                       unsigned long long where, unsigned long long index, unsigned long long got,
                                       unsigned long long want, unsigned long long dt) {
  if (nbad) report_wrong(rep, simd_map, row, nbad, where, index, got, want);
  if ((threadIdx.x & 63u) == 0) {
    unsigned long long* r = simd_map + SIMD_MAP_COLS * row;
    atomicAdd(r, 1ULL);
    atomicAdd(r + 2, dt);
  }
}

// -3 with a message when a kernel was built with scratch, or with another LDS allocation than it may have: it would
// test memory.  The message reads `<prefix>: the kernel of <what> was built with ... bytes of LDS<tail>`.
inline int refuse_memory(const char* prefix, const std::string& what, const hipFuncAttributes& attr,
                         const std::string& tail, size_t lds_allowed = 0) {
  if (attr.localSizeBytes == 0 && attr.sharedSizeBytes == lds_allowed) return 0;
  g_err = std::string(prefix) + ": the kernel of " + what + " was built with " + std::to_string(attr.localSizeBytes) +
          " bytes of scratch per lane and " + std::to_string(attr.sharedSizeBytes) + " bytes of LDS" + tail;
  return -3;
}

// the grid of an entry point: `blocks` workgroups as asked for, or (0) `per_cu` for every CU of `device`
inline unsigned default_grid(int device, int blocks, int per_cu) {
  return blocks ? static_cast<unsigned>(blocks) : static_cast<unsigned>(cu_count(device)) * per_cu;
}

// the report and the map of one entry point, and its checked, timed launches
struct Run {
  static constexpr size_t MAP_BYTES = static_cast<size_t>(SIMD_ROWS) * SIMD_MAP_COLS * sizeof(unsigned long long);
  DevBuf drep, dmap;
  Timer tm;
  int open(int device) {
    HIP_CHECK(drep.alloc(device, sizeof(Report)));
    HIP_CHECK(dmap.alloc(device, MAP_BYTES));
    HIP_CHECK(hipMemset(dmap.ptr, 0, MAP_BYTES));
    HIP_CHECK(tm.create());
    return 0;
  }
  Report* rep() const { return static_cast<Report*>(drep.ptr); }
  unsigned long long* map() const { return static_cast<unsigned long long*>(dmap.ptr); }
  int clear() {
    HIP_CHECK(hipMemset(drep.ptr, 0, sizeof(Report)));
    return 0;
  }
  // the time of what `enqueue` queues; the report is read by collect()
  template <typename F>
  int launch(F&& enqueue, float* ms) {
    const auto go = [&] {
      enqueue();
      return 0;
    };
    return tm.timed(go, ms);
  }
  // adds the wrong words since clear() to *errors and keeps the first record seen: rec[0..4) = where, index, got, want
  // (rec[0] == ~0: none yet)
  int collect(unsigned long long* errors, unsigned long long* rec) {
    Report h;
    HIP_CHECK(hipMemcpy(&h, drep.ptr, sizeof h, hipMemcpyDeviceToHost));
    *errors += h.errors;
    if (h.claimed && rec[0] == ~0ULL) rec[0] = h.where, rec[1] = h.index, rec[2] = h.got, rec[3] = h.want;
    return 0;
  }
  // the usual launch: clear(), launch() and collect() in one
  template <typename F>
  int checked(F&& enqueue, float* ms, unsigned long long* errors, unsigned long long* rec) {
    if (const int rc = clear()) return rc;
    if (const int rc = launch(enqueue, ms)) return rc;
    return collect(errors, rec);
  }
  // The usual series: launch r = 0, the warm-up (which carries the self-check hooks), then `reps` timed launches, each
  // of what enqueue(r) queues and each checked(); *mean_ms = the mean time of the timed ones.  after(r) runs once
  // launch r has been collected.  Ends at the first non-zero code, of a launch or of after(), and returns it.
  template <typename F, typename A>
  int series(int reps, F&& enqueue, unsigned long long* errors, unsigned long long* rec, double* mean_ms, A&& after) {
    double total_ms = 0.0;
    for (int r = 0; r <= reps; ++r) {
      float t = 0.f;
      if (const int rc = checked([&] { enqueue(r); }, &t, errors, rec)) return rc;
      if (const int rc = after(r)) return rc;
      if (r > 0) total_ms += t;
    }
    *mean_ms = total_ms / reps;
    return 0;
  }
  template <typename F>
  int series(int reps, F&& enqueue, unsigned long long* errors, unsigned long long* rec, double* mean_ms) {
    return series(reps, enqueue, errors, rec, mean_ms, [](int) { return 0; });
  }
  int read_map(unsigned long long* simd_map) {
    HIP_CHECK(hipMemcpy(simd_map, dmap.ptr, MAP_BYTES, hipMemcpyDeviceToHost));
    return 0;
  }
};

}  // namespace
