// libmi355x_scratch.so: the scratch diagnostic (HIP, gfx950).
//
// Private (scratch) memory is the one path almost every real kernel uses and every other diagnostic here is built to
// avoid: the frame base the dispatcher hands every wave slot, the compiler's own scratch accesses, generic pointers
// into private memory at call depth, and the backing store the runtime sizes and hands out.  Two parts, every row
// selectable (scratch_ref.h holds the models and the classifier, and says what is not here):
//   isolate  one kernel with a 1 KiB-per-lane frame on a grid of twice the device's wave slots, so that slots are
//            reused inside the launch.  Per round a wave writes its frame with runtime-indexed C++ stores, dwells for a
//            CONSTANT number of s_sleep (it waits on nobody), reads the frame back and compares.  The written word is a
//            bijection of (round, wave, lane, word), so the host says whose a wrong word is.  wall_clock64 after the
//            writes and before the reads gives the co-residency that the host reports and never judges.
//   frames   scratch_frames_index and scratch_frames_calls of scratch_ref.h on every lane, compared bit for bit with
//            the host's run of the same routines.
// No kernel spins on another wave's data; every loop has a fixed trip count.  A kernel built WITHOUT a private
// segment is refused (-3): the mirror image of the other libraries' check.  ops/scratch.py is the Python side;
// ops/diag.run(extra=("scratch",)) runs it next to a level's own tests.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../common/hip_host.h"
#include "../common/simd_report.h"
#include "scratch_ref.h"

namespace {

constexpr unsigned THREADS = SCRATCH_THREADS;
constexpr unsigned WAVES_PER_BLOCK = THREADS / SCRATCH_WAVE;
typedef __attribute__((address_space(5))) volatile uint32_t* private_ptr;
#define DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// ---- isolate ---------------------------------------------------------------------------------------------------

struct IsoArgs {
  unsigned long long* times;  // waves x rounds x {after the writes, before the reads}
  uint32_t* rows;             // waves: the SIMD map row a wave ran on
  Report* rep;
  unsigned long long* map;
  uint32_t seed, stride;
  int rounds;
  int hook_wave, hook_round;  // -1: no hook
  int hook_flip, hook_alias, hook_stale;  // which one (hook_stale: the word, -1: none)
};

__global__ void __launch_bounds__(THREADS) isolate_kernel(IsoArgs a) {
  volatile uint32_t cells[SCRATCH_ISO_WORDS];  // 1 KiB per lane
  const private_ptr frame = (private_ptr)cells;
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  uint32_t nbad = 0, bad_cell = 0, bad_got = 0, bad_want = 0;
#pragma nounroll
  for (int r = 0; r < a.rounds; ++r) {
    const bool hook_now = static_cast<int>(wave) == a.hook_wave && r == a.hook_round;
    const int stale = hook_now && lane == 0 ? a.hook_stale : -1;
#pragma nounroll
    for (uint32_t i = 0; i < SCRATCH_ISO_WORDS; ++i) {  // the compiler's own scratch stores, a runtime index
      const uint32_t j = scratch_iso_index(i, lane, a.stride);
      if (static_cast<int>(j) != stale) frame[j] = scratch_iso_word(a.seed, r, wave, lane, j);
    }
    DRAIN();
    const unsigned long long tw = wall_clock64();
    for (int s = 0; s < SCRATCH_ISO_DWELL; ++s) __builtin_amdgcn_s_sleep(16);  // a constant: nobody is waited for
    const unsigned long long tr = wall_clock64();
#pragma nounroll
    for (uint32_t i = 0; i < SCRATCH_ISO_WORDS; ++i) {
      const uint32_t j = scratch_iso_index(i, lane, a.stride);
      uint32_t got = frame[j];
      const uint32_t want = scratch_iso_word(a.seed, r, wave, lane, j);
      if (hook_now && lane == 0 && j == 0) {
        if (a.hook_flip) got ^= 0x10u;
        if (a.hook_alias) got = scratch_iso_word(a.seed, r, wave + 1, lane, j);  // what wave + 1 wrote to this cell
      }
      if (got != want) {
        if (!nbad) bad_cell = scratch_pack(r, wave, lane, j), bad_got = got, bad_want = want;
        ++nbad;
      }
    }
    if (lane == 0) {
      a.times[(static_cast<size_t>(wave) * a.rounds + r) * 2] = tw;
      a.times[(static_cast<size_t>(wave) * a.rounds + r) * 2 + 1] = tr;
    }
  }
  const unsigned row = simd_row();
  if (lane == 0) a.rows[wave] = row;
  // a record's `where`: SIMD map row << 16 | lane; its index: scratch_pack(round, wave, lane, word) of the reader's cell
  report(a.rep, a.map, row, nbad, (static_cast<unsigned long long>(row) << 16) | lane, bad_cell, bad_got, bad_want,
         static_cast<unsigned long long>(wall_clock64() - t0));
}

// ---- frames ----------------------------------------------------------------------------------------------------

struct FramesArgs {
  uint32_t* out;   // waves x 64 lanes x SCRATCH_FRAMES_OUT
  uint32_t* rows;  // waves
  Report* rep;
  unsigned long long* map;
  uint32_t seed;
  int steps;
};

template <int CALLS>
__global__ void __launch_bounds__(THREADS) frames_kernel(FramesArgs a) {
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  uint32_t o[SCRATCH_FRAMES_OUT];
  if constexpr (CALLS) scratch_frames_calls(a.seed, wave, lane, a.steps, o);
  else scratch_frames_index(a.seed, wave, lane, a.steps, o);
  uint32_t* out = a.out + (static_cast<size_t>(wave) * SCRATCH_WAVE + lane) * SCRATCH_FRAMES_OUT;
  for (int k = 0; k < SCRATCH_FRAMES_OUT; ++k) out[k] = o[k];
  const unsigned row = simd_row();
  if (lane == 0) a.rows[wave] = row;
  report(a.rep, a.map, row, 0, 0, 0, 0, 0, static_cast<unsigned long long>(wall_clock64() - t0));
}

// ---- host ------------------------------------------------------------------------------------------------------

std::string row_name(int row) {
  return row == SCRATCH_ROW_ISOLATE ? "isolate/1k" : row == SCRATCH_ROW_FRAMES_INDEX ? "frames/index" : "frames/calls";
}

hipError_t row_attributes(int row, hipFuncAttributes* attr) {
  if (row == SCRATCH_ROW_ISOLATE) return hipFuncGetAttributes(attr, reinterpret_cast<const void*>(isolate_kernel));
  if (row == SCRATCH_ROW_FRAMES_INDEX) return hipFuncGetAttributes(attr, reinterpret_cast<const void*>(frames_kernel<0>));
  return hipFuncGetAttributes(attr, reinterpret_cast<const void*>(frames_kernel<1>));
}

// pinned host memory for the read-back, released on every return path
struct HostBuf {
  void* ptr = nullptr;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  hipError_t alloc(size_t bytes) { return hipHostMalloc(&ptr, bytes, hipHostMallocDefault); }
  ~HostBuf() {
    if (ptr) (void)hipHostFree(ptr);
  }
};

constexpr int FIRST = 10;  // words of a row's record
struct Found {             // what the host's compare adds to a row
  unsigned long long* errors;
  unsigned long long* first;  // FIRST words; first[0] == ~0: none yet
  std::vector<unsigned long long>* map;
  int launch;
  void wrong(uint32_t simd, uint32_t lane, uint32_t wave, uint32_t word, uint32_t got, uint32_t want) {
    ++*errors;
    (*map)[SIMD_MAP_COLS * simd + 1] += 1;
    if (first[0] != ~0ULL) return;
    first[0] = (static_cast<unsigned long long>(simd) << 16) | lane, first[1] = wave, first[2] = word, first[3] = got;
    first[4] = want, first[5] = SCRATCH_CLASS_CORRUPT, first[6] = 0, first[7] = ~0ULL, first[8] = 0;
    first[9] = static_cast<unsigned long long>(launch);
  }
};

}  // namespace

extern "C" {

const char* scratch_last_error(void) { return g_err.c_str(); }

int scratch_device_count(void) { return device_count(); }

int scratch_slots(void) { return SIMD_ROWS; }  // rows of the simd_map below

int scratch_rows(void) { return SCRATCH_ROWS; }

// The rows `rows[0..nrows)` (SCRATCH_ROW_ISOLATE, SCRATCH_ROW_FRAMES_INDEX or _CALLS), one after the other: a checked
// warm-up launch, then `reps` timed and checked launches each.  The frames rows run `blocks` workgroups of 256 threads
// (0: one per CU); the isolate row
// runs `iso_blocks` workgroups (0: twice the device's wave slots, 2 x CUs x 32 waves, at most 16,384 waves) for
// `rounds` rounds.  Arrays of scratch_rows() rows, indexed by the row:
//   errors[k]      wrong 32-bit words over all its launches
//   words[k]       words compared over all its launches
//   ms[k]          the mean time of a timed launch
//   first[10 k..]  where (SIMD map row << 16 | lane; ~0: none), wave, word (isolate: the cell; frames: the output
//                  word), got, want, the ScratchClass, the age, the writer's wave (~0: none), the writer's SIMD map
//                  row, the launch (0: the warm-up) of one wrong word of the first launch that had any
//   frame_bytes[k] the kernel's private segment per lane (hipFuncGetAttributes)
// info[0..8): co_resident_waves (the most isolate frames live at once, from the waves' own clocks; reported, never
// judged), the free device memory that the first isolate launch of this call took and still holds afterwards, the
// most it held while it ran, the isolate grid's waves, the frames grid's workgroups, the isolate grid's, 0, 0.
// simd_map: scratch_slots() x 3 (waves run, wrong words, summed wall_clock64 ticks) per physical SIMD, added up over
// every launch of every row; a wrong word counts for the SIMD that read it.
//
// Refused with -2 and a message: a bad device, rounds outside 1..16,
// reps < 1, no row or an unknown one, an isolate grid above 16,384 waves, a hook outside the rows or the grid, an
// alias hook on the last wave, a stale hook outside the frame or in round 0, hooks on a row that has none; with -3: a
// kernel built with NO private segment or with more than SCRATCH_MAX_SEGMENT_BYTES per lane.
//
// Self-check hooks, off by default (inject_row -1), acting in the warm-up launch of row `inject_row` on wave
// `inject_wave`:
//   flip   (neither of the two below) frames: bit 4 of the first word lane 0 of that wave handed back is
//          flipped before the compare; isolate: bit 4 of the word lane 0 read from cell 0 in round `inject_round`: 1
//          wrong word, got = want ^ 0x10
//   alias  (inject_alias, isolate) the compare is given the word that wave + 1 wrote to the same cell
//   stale  (inject_stale_word >= 0, isolate, inject_round >= 1) lane 0 skips writing that word: it reads the round before
int scratch_test(int device, const int* rows, int nrows, int blocks, int iso_blocks, int rounds,
                 int reps, uint32_t seed, int inject_row, int inject_wave, int inject_round, int inject_alias,
                 int inject_stale_word, unsigned long long* errors, unsigned long long* words, double* ms,
                 unsigned long long* first, int* frame_bytes, unsigned long long* info, unsigned long long* simd_map) {
  const int n = device_count();
  bool known = rows != nullptr && nrows >= 1 && nrows <= SCRATCH_ROWS, hook_listed = inject_row < 0;
  for (int i = 0; known && i < nrows; ++i) {
    known = rows[i] >= 0 && rows[i] < SCRATCH_ROWS;
    hook_listed = hook_listed || rows[i] == inject_row;
  }
  if (device < 0 || device >= n || rounds < 1 || rounds > SCRATCH_ISO_MAX_ROUNDS || reps < 1 || blocks < 0 || iso_blocks < 0 || !known) {
    g_err = "scratch: need a valid device, rounds 1..16, reps >= 1 and a list of known rows";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const int cus = cu_count(device);
  const int G = blocks ? blocks : cus;
  const long long iso_default = std::min<long long>(2LL * cus * 32 / WAVES_PER_BLOCK, SCRATCH_ISO_MAX_WAVES / WAVES_PER_BLOCK);
  const long long IG = iso_blocks ? iso_blocks : iso_default;
  if (IG * WAVES_PER_BLOCK > SCRATCH_ISO_MAX_WAVES || G > 4096) {
    g_err = "scratch: the isolate grid may have at most " + std::to_string(SCRATCH_ISO_MAX_WAVES) + " waves (" +
            std::to_string(SCRATCH_ISO_MAX_WAVES / WAVES_PER_BLOCK) + " workgroups: the wave's field of the written word "
            "has 14 bits), not " + std::to_string(IG) + " workgroups; the frames grid at most 4096 workgroups";
    return -2;
  }
  const int fwaves = G * WAVES_PER_BLOCK, iwaves = static_cast<int>(IG) * WAVES_PER_BLOCK;
  if (!hook_listed) {
    g_err = "scratch: inject_row must be in the list";
    return -2;
  }
  if (inject_row >= 0) {
    const bool iso = inject_row == SCRATCH_ROW_ISOLATE;
    const int waves = iso ? iwaves : fwaves;
    if (inject_wave < 0 || inject_wave >= waves || (!iso && (inject_alias || inject_stale_word >= 0 || inject_round != 0)) ||
        inject_round < 0 || inject_round >= rounds || (inject_alias && inject_wave + 1 >= waves) ||
        inject_stale_word >= SCRATCH_ISO_WORDS || (inject_stale_word >= 0 && inject_round < 1) ||
        (inject_alias && inject_stale_word >= 0)) {
      g_err = "scratch: inject_wave must lie inside the row's grid (an alias needs wave + 1 there too), inject_round inside "
              "the rounds, inject_stale_word inside the frame and in a round >= 1 (round 0 has no round before), one hook at "
              "a time, and only the isolate row has the alias and stale hooks and rounds";
      return -2;
    }
  }
  for (int k = 0; k < SCRATCH_ROWS; ++k) {
    errors[k] = words[k] = 0;
    for (int j = 0; j < FIRST; ++j) first[FIRST * k + j] = 0;
    first[FIRST * k] = ~0ULL;
    frame_bytes[k] = 0;
    ms[k] = 0.0;
  }
  for (int j = 0; j < 8; ++j) info[j] = 0;
  info[3] = static_cast<unsigned long long>(iwaves), info[4] = static_cast<unsigned long long>(G);
  info[5] = static_cast<unsigned long long>(IG);

  Run run;
  if (const int rc = run.open(device)) return rc;
  const size_t frames_words = static_cast<size_t>(fwaves) * SCRATCH_WAVE * SCRATCH_FRAMES_OUT;
  const size_t times_words = static_cast<size_t>(iwaves) * rounds * 2;
  bool any_iso = false, any_frames = false;
  for (int i = 0; i < nrows; ++i) (rows[i] == SCRATCH_ROW_ISOLATE ? any_iso : any_frames) = true;
  const size_t out_words = any_frames ? frames_words : 0;
  const int max_waves = std::max(fwaves, iwaves);
  DevBuf dout, dwave, dtimes;
  HostBuf hout;
  if (out_words) {
    HIP_CHECK(dout.alloc(device, out_words * sizeof(uint32_t)));
    HIP_CHECK(hout.alloc(out_words * sizeof(uint32_t)));
  }
  HIP_CHECK(dwave.alloc(device, static_cast<size_t>(max_waves) * sizeof(uint32_t)));
  if (any_iso) HIP_CHECK(dtimes.alloc(device, times_words * sizeof(unsigned long long)));
  uint32_t* out = static_cast<uint32_t*>(hout.ptr);
  std::vector<uint32_t> per_wave(max_waves);
  std::vector<unsigned long long> times(any_iso ? times_words : 0), pad(any_iso ? 2 * times_words : 0);
  std::vector<unsigned long long> host_map(static_cast<size_t>(SIMD_ROWS) * SIMD_MAP_COLS, 0);
  bool measured = false;

  for (int i = 0; i < nrows; ++i) {
    const int k = rows[i];
    hipFuncAttributes attr;
    HIP_CHECK(row_attributes(k, &attr));
    frame_bytes[k] = static_cast<int>(attr.localSizeBytes);
    if (attr.localSizeBytes == 0 || attr.localSizeBytes > SCRATCH_MAX_SEGMENT_BYTES) {
      g_err = "scratch: the kernel of " + row_name(k) + " was built with " + std::to_string(attr.localSizeBytes) +
              " bytes of scratch per lane: it must have a private segment (this library tests it), of at most " +
              std::to_string(SCRATCH_MAX_SEGMENT_BYTES) + " bytes (1 KiB of locals and what the compiler adds)";
      return -3;
    }
    double total_ms = 0.0;
    unsigned long long rec4[4] = {~0ULL, 0, 0, 0};
    for (int r = 0; r <= reps; ++r) {  // r == 0: the warm-up, which carries the hooks
      const bool hooked = r == 0 && k == inject_row;
      Found found = {errors + k, first + FIRST * k, &host_map, r};
      float t = 0.f;
      unsigned long long device_errors = 0;
      if (k == SCRATCH_ROW_ISOLATE) {
        const IsoArgs a = {static_cast<unsigned long long*>(dtimes.ptr), static_cast<uint32_t*>(dwave.ptr), run.rep(), run.map(),
                           seed, 37u, rounds, hooked ? inject_wave : -1, hooked ? inject_round : -1,
                           hooked && !inject_alias && inject_stale_word < 0 ? 1 : 0, hooked && inject_alias ? 1 : 0,
                           hooked ? inject_stale_word : -1};
        size_t free0 = 0, free1 = 0, low = 0, total = 0;
        const bool measure = !measured;
        if (measure) HIP_CHECK(hipMemGetInfo(&free0, &total));
        low = free0;
        if (const int rc = run.clear()) return rc;
        HIP_CHECK(hipEventRecord(run.tm.e0, nullptr));
        hipLaunchKernelGGL(isolate_kernel, dim3(static_cast<unsigned>(IG)), dim3(THREADS), 0, nullptr, a);
        HIP_CHECK(hipEventRecord(run.tm.e1, nullptr));
        for (int polls = 0; measure && polls < 4096 && hipEventQuery(run.tm.e1) == hipErrorNotReady; ++polls) {
          size_t f = 0;  // how much the runtime holds while the launch runs
          if (hipMemGetInfo(&f, &total) == hipSuccess && f < low) low = f;
        }
        (void)hipGetLastError();  // hipErrorNotReady of the query is no error
        HIP_CHECK(hipEventSynchronize(run.tm.e1));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(event_ms(run.tm.e0, run.tm.e1, &t));
        if (measure) {
          HIP_CHECK(hipMemGetInfo(&free1, &total));
          info[1] = free0 > free1 ? free0 - free1 : 0;
          info[2] = free0 > low ? free0 - low : 0;
          measured = true;
        }
        const bool had = rec4[0] != ~0ULL;
        if (const int rc = run.collect(&device_errors, rec4)) return rc;
        errors[k] += device_errors;
        HIP_CHECK(hipMemcpy(per_wave.data(), dwave.ptr, static_cast<size_t>(iwaves) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(times.data(), dtimes.ptr, times_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const uint32_t live = scratch_co_resident(times.data(), times_words / 2, pad.data());
        if (live > info[0]) info[0] = live;
        if (!had && rec4[0] != ~0ULL) {  // this launch's record: classify the word and name its writer
          const uint32_t cell = static_cast<uint32_t>(rec4[1]), got = static_cast<uint32_t>(rec4[2]);
          const ScratchVerdict v = scratch_classify(seed, cell, got, static_cast<uint32_t>(iwaves), static_cast<uint32_t>(rounds));
          unsigned long long* f = first + FIRST * k;
          f[0] = rec4[0], f[1] = (cell >> 14) & 16383u, f[2] = cell, f[3] = rec4[2], f[4] = rec4[3];
          f[5] = static_cast<unsigned long long>(v.cls), f[6] = static_cast<unsigned long long>(v.age);
          f[7] = v.cls == SCRATCH_CLASS_ALIAS ? v.wave : ~0ULL;
          f[8] = v.cls == SCRATCH_CLASS_ALIAS ? per_wave[v.wave] % SIMD_ROWS : 0;
          f[9] = static_cast<unsigned long long>(r);
        }
        words[k] += static_cast<unsigned long long>(iwaves) * SCRATCH_WAVE * SCRATCH_ISO_WORDS * rounds;
      } else {
        const FramesArgs a = {static_cast<uint32_t*>(dout.ptr), static_cast<uint32_t*>(dwave.ptr), run.rep(), run.map(), seed,
                              SCRATCH_FRAMES_STEPS};
        const auto go = [&] {
          if (k == SCRATCH_ROW_FRAMES_CALLS) hipLaunchKernelGGL(frames_kernel<1>, dim3(G), dim3(THREADS), 0, nullptr, a);
          else hipLaunchKernelGGL(frames_kernel<0>, dim3(G), dim3(THREADS), 0, nullptr, a);
        };
        if (const int rc = run.checked(go, &t, &device_errors, rec4)) return rc;
        if (hooked)
          if (const int rc = flip_word_bit(a.out + static_cast<size_t>(inject_wave) * SCRATCH_WAVE * SCRATCH_FRAMES_OUT)) return rc;
        HIP_CHECK(hipMemcpy(out, dout.ptr, frames_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(per_wave.data(), dwave.ptr, static_cast<size_t>(fwaves) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int w = 0; w < fwaves; ++w)
          for (uint32_t l = 0; l < SCRATCH_WAVE; ++l) {
            uint32_t want[SCRATCH_FRAMES_OUT];
            if (k == SCRATCH_ROW_FRAMES_CALLS) scratch_frames_calls(seed, static_cast<uint32_t>(w), l, SCRATCH_FRAMES_STEPS, want);
            else scratch_frames_index(seed, static_cast<uint32_t>(w), l, SCRATCH_FRAMES_STEPS, want);
            const uint32_t* got = out + (static_cast<size_t>(w) * SCRATCH_WAVE + l) * SCRATCH_FRAMES_OUT;
            for (int j = 0; j < SCRATCH_FRAMES_OUT; ++j)
              if (got[j] != want[j])
                found.wrong(per_wave[w] % SIMD_ROWS, l, static_cast<uint32_t>(w), static_cast<uint32_t>(j), got[j], want[j]);
          }
        words[k] += frames_words;
      }
      if (r > 0) total_ms += t;
    }
    ms[k] = total_ms / reps;
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  for (size_t j = 0; j < host_map.size(); ++j) simd_map[j] += host_map[j];  // the words the host found wrong
  return 0;
}

}  // extern "C"
