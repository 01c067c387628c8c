// libmi355x_hbmscan.so: the hbmscan diagnostic (HIP, gfx950).
//
// The probe reads what the hardware has already caught (ECC counters, retired pages); the memtest of the levels
// (csrc/diag) writes one address hash and its inverse over 8 GiB, under 3 % of an MI355X's 288 GB, and answers with a
// count and the first bad byte.  This library tests every byte hipMalloc will give it, minus a reserve, and names what
// it found: a stuck bit, an address alias, one bad region, or scattered errors.  ops/hbmscan.py is its Python side;
// ops/diag.run(extra=("hbmscan",)) runs it next to a level's own tests.
//
// The tested set is a list of chunks (hbmscan_ref.h: the plan), and every step of every phase (hbmscan_ref.h: the
// expected word) is one launch per chunk, all chunks in the same order, then one synchronize.  Three kernels, each in
// the form tools/hbm_explore.hip measured fastest (csrc/diag/mem_kernels.h): one 16-byte word per thread, a flat grid
// over the chunk, no grid-stride loop; nontemporal loads, nontemporal stores beside a load and plain stores alone
// (write 6.87 against 6.65 TB/s nontemporal).  Indices are 64-bit throughout: a chunk has up to 2^30 words and the
// global index, which the addr phase writes raw, runs over the whole set.
//
// Offsets in the results are virtual: into the chunks this process was given.  The project has no map from an address
// to an HBM stack or channel.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <thread>
#include <vector>

#include "../common/hip_host.h"
#include "hbmscan_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int MAX_FLIPS = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// what the verifying launches report (device memory, zeroed once per scan: the counts run over the whole scan)
struct Report {
  unsigned long long errors;  // wrong words
  HbmscanRecord records[HBMSCAN_MAX_RECORDS];
  unsigned long long hist[HBMSCAN_HIST];
};

// where a launch is in the scan: what a record says besides the words
struct Where {
  int phase, step;
  unsigned chunk;
  uint64_t g0;  // global index of the chunk's first word
};

__device__ __forceinline__ u32x4 as_vec(const HbmscanWord& w) { return u32x4{w.w[0], w.w[1], w.w[2], w.w[3]}; }

// The mismatch path: rare, and bounded whatever the memory does.  One atomic per wave that saw a wrong word -- the
// add of its count, whose returned value numbers the wave's wrong words -- so a wholly bad chunk costs one atomic per
// 64 words, not one per word, and the first HBMSCAN_MAX_RECORDS wrong words own a record slot each with no second
// counter.  Only the first HBMSCAN_HIST_WORDS add their flipped bits to the histogram.
__device__ void report_bad(Report* rep, unsigned long long ballot, bool bad, const Where& at, uint64_t i, u32x4 got,
                           const HbmscanWord& want) {
  const unsigned lane = threadIdx.x & 63u;
  const int leader = __ffsll(ballot) - 1;
  unsigned long long base = 0;
  if (static_cast<int>(lane) == leader) base = atomicAdd(&rep->errors, static_cast<unsigned long long>(__popcll(ballot)));
  base = __shfl(base, leader);
  if (!bad) return;
  const unsigned long long ordinal = base + __popcll(ballot & ((1ULL << lane) - 1ULL));
  if (ordinal < static_cast<unsigned long long>(HBMSCAN_MAX_RECORDS)) {
    HbmscanRecord& r = rep->records[ordinal];
    r.phase = static_cast<uint32_t>(at.phase);
    r.step = static_cast<uint32_t>(at.step);
    r.chunk = at.chunk;
    r.pad = 0;
    r.word = i;
    r.global = at.g0 + i;
    for (int l = 0; l < 4; ++l) {
      r.got[l] = got[l];
      r.want[l] = want.w[l];
    }
  }
  if (ordinal < static_cast<unsigned long long>(HBMSCAN_HIST_WORDS)) {
    for (int l = 0; l < 4; ++l) {
      uint32_t x = got[l] ^ want.w[l];
      while (x) {
        const int b = __ffs(x) - 1;
        x &= x - 1;
        atomicAdd(&rep->hist[2 * (32 * l + b) + ((got[l] >> b) & 1u)], 1ULL);
      }
    }
  }
}

__global__ void __launch_bounds__(THREADS) write_kernel(u32x4* __restrict__ p, uint64_t n, uint64_t g0, HbmscanContent c) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
  if (i < n) p[i] = as_vec(hbmscan_word(c, g0 + i));
}

// verify (WRITE false), or verify and write the inverse (WRITE true): one load, one compare and one store per word by
// the same thread.  The stored word comes from the expected one, so a wrong word is not carried into the next step.
template <bool WRITE>
__global__ void __launch_bounds__(THREADS) verify_kernel(u32x4* __restrict__ p, uint64_t n, HbmscanContent c, Where at,
                                                         Report* rep) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x;
  bool bad = false;
  u32x4 got = {0u, 0u, 0u, 0u};
  HbmscanWord want = {{0u, 0u, 0u, 0u}};
  if (i < n) {
    got = __builtin_nontemporal_load(p + i);
    want = hbmscan_word(c, at.g0 + i);
    bad = got[0] != want.w[0] || got[1] != want.w[1] || got[2] != want.w[2] || got[3] != want.w[3];
    if (WRITE) __builtin_nontemporal_store(~as_vec(want), p + i);
  }
  const unsigned long long ballot = __builtin_amdgcn_ballot_w64(bad);  // the whole wave is here: no lane left early
  if (ballot) report_bad(rep, ballot, bad, at, i, got, want);
}

struct Chunk {
  u32x4* ptr;
  uint64_t words;
  uint64_t base;  // index of its first word in the tested set (without index_base)
};

// the device address of 32-bit lane `lane` of word `word` of the tested set (the caller checked the range)
uint32_t* lane_of(const std::vector<Chunk>& chunks, uint64_t word, int lane) {
  for (const Chunk& c : chunks)
    if (word - c.base < c.words) return reinterpret_cast<uint32_t*>(c.ptr + (word - c.base)) + lane;
  return nullptr;
}

// Hook: bit `bit` (0..127) of a word flipped (value < 0) or forced to `value`, from the host.
int poke_bit(const std::vector<Chunk>& chunks, uint64_t word, int bit, int value) {
  uint32_t* w = lane_of(chunks, word, bit / 32);
  uint32_t v = 0;
  HIP_CHECK(hipMemcpy(&v, w, sizeof v, hipMemcpyDeviceToHost));
  const uint32_t m = 1u << (bit % 32);
  v = value < 0 ? v ^ m : value ? v | m : v & ~m;
  HIP_CHECK(hipMemcpy(w, &v, sizeof v, hipMemcpyHostToDevice));
  return 0;
}

double seconds_since(SteadyClock::time_point t0) { return std::chrono::duration<double>(SteadyClock::now() - t0).count(); }

}  // namespace

extern "C" {

const char* hbmscan_last_error(void) { return g_err.c_str(); }

int hbmscan_device_count(void) { return device_count(); }

// hbmscan_ref.h's plan: chunk sizes (bytes) into plan_out, room for 4096; returns their number, or -2.
int hbmscan_plan(unsigned long long free_bytes, unsigned long long total_bytes, unsigned long long reserve,
                 unsigned long long limit, unsigned long long chunk, unsigned long long* plan_out) {
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "plan_out is uint64_t");
  const int n = hbmscan_ref_plan(free_bytes, total_bytes, reserve, limit, chunk, reinterpret_cast<uint64_t*>(plan_out));
  if (n < 0) g_err = "hbmscan plan: need free <= total, a target (min(limit, free - reserve)) of at least 16 bytes, a "
                     "chunk that is a multiple of 16 in 16 .. 16 GiB and at most 4096 chunks";
  return n;
}

// hbmscan_ref.h's expected word after step `step` of `phase` into out[4]; -2 for a phase or step that does not exist.
int hbmscan_want(int phase, int step, unsigned long long global_word, uint64_t seed, unsigned int* out) {
  if (phase < 0 || phase >= HBMSCAN_PHASES || step < 0 || step >= hbmscan_steps(phase, HBMSCAN_MAX_RANDOM_PASSES)) {
    g_err = "hbmscan want: no such phase or step";
    return -2;
  }
  const HbmscanWord w = hbmscan_ref_want(phase, step, global_word, seed);
  for (int l = 0; l < 4; ++l) out[l] = w.w[l];
  return 0;
}

// hbmscan_ref.h's classifier over n records and the 256-entry histogram.
int hbmscan_classify(const HbmscanRecord* records, int n, const unsigned long long* hist, unsigned long long index_base,
                     unsigned long long tested_words, HbmscanFinding* finding_out) {
  if (n < 0 || n > HBMSCAN_MAX_RECORDS) {
    g_err = "hbmscan classify: 0 .. 64 records";
    return -2;
  }
  hbmscan_ref_classify(records, n, reinterpret_cast<const uint64_t*>(hist), index_base, tested_words, finding_out);
  return 0;
}

// The scan of `device`.  The plan is hbmscan_plan(free, total, reserve, limit, chunk) of hipMemGetInfo's numbers
// (limit 0: everything free but the reserve).  Every planned chunk is allocated; one that fails is halved, down to
// min_chunk, and retried, and when a piece of min_chunk fails too the scan goes on with what it holds: an allocation
// failure is never a finding, it only lowers the tested bytes.  Every chunk is freed on every return path.
//
// Outputs.  totals[16]: 0 total bytes, 1 free bytes, 2 planned bytes, 3 tested bytes, 4 chunks held, 5 wrong words,
// 6 records, 7 complete, 8 cached (tested under 2 GiB: verified word for word, but the caches may have answered),
// 9 / 10 the phase and step last completed, 11 chunks halved, 12 allocations that failed.  Per phase: wrong words, the
// sweeps' milliseconds (launch to synchronize, summed), the wall milliseconds with holds and hooks, the bytes of traffic
// (a step that verifies and writes counts twice).  records[64], hist[256], the finding: hbmscan_ref.h.
//
// deadline_s > 0 is held against the wall clock after every step's synchronize: a scan that runs out returns what it
// has with complete = 0.  Incomplete is reported, not failed.
//
// Self-check hooks, all off by default, applied by the host between launches (words are indices into the tested set):
//   flips[4 * k .. ] = (phase, step, word, bit), n_flips of them (at most 4): that bit is flipped once, after that
//       step's write (so `step` must be a writing step); the next step, which verifies it, reports it
//   stuck_word >= 0: bit stuck_bit of it is forced to stuck_value after every writing step
//   alias_a, alias_b >= 0: in addr, after the first write, word alias_a is copied over word alias_b
//   index_base: the global index of the first word (just under 2^32: the carry into the high half, without 64 GiB)
//   fail_alloc_at = k > 0: the k-th hipMalloc of a chunk is taken as failed
// Refused with -2 and a message: anything out of range, a hook outside the tested set included.
int hbmscan_test(int device, unsigned long long limit, unsigned long long reserve, unsigned long long chunk,
                 unsigned long long min_chunk, int hold_ms, int random_passes, uint64_t seed, double deadline_s,
                 unsigned long long index_base, const long long* flips, int n_flips, long long stuck_word, int stuck_bit,
                 int stuck_value, long long alias_a, long long alias_b, int fail_alloc_at, unsigned long long* totals,
                 unsigned long long* phase_errors, double* phase_ms, double* phase_wall_ms, double* phase_bytes,
                 HbmscanRecord* records, unsigned long long* hist, HbmscanFinding* finding) {
  const auto t_start = SteadyClock::now();
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev || chunk < HBMSCAN_WORD || chunk > HBMSCAN_MAX_CHUNK || chunk % HBMSCAN_WORD ||
      min_chunk < HBMSCAN_WORD || min_chunk % HBMSCAN_WORD || hold_ms < 0 || hold_ms > 60000 || random_passes < 1 ||
      random_passes > HBMSCAN_MAX_RANDOM_PASSES || !(deadline_s >= 0.0) || std::isinf(deadline_s) ||
      index_base > (1ULL << 62) || fail_alloc_at < 0) {
    g_err = "hbmscan test: need a valid device, chunk and min_chunk multiples of 16 (chunk up to 16 GiB), hold_ms "
            "0..60000, random_passes 1..64, deadline_s >= 0, index_base <= 2^62 and fail_alloc_at >= 0";
    return -2;
  }
  if (n_flips < 0 || n_flips > MAX_FLIPS || (n_flips && !flips) || stuck_word < -1 || alias_a < -1 || alias_b < -1 ||
      (alias_a < 0) != (alias_b < 0) || (alias_a >= 0 && alias_a == alias_b) ||
      (stuck_word >= 0 && (stuck_bit < 0 || stuck_bit > 127 || stuck_value < 0 || stuck_value > 1))) {
    g_err = "hbmscan test: at most 4 flips, stuck_bit 0..127 with stuck_value 0 or 1, and two different alias words";
    return -2;
  }
  for (int k = 0; k < n_flips; ++k) {
    const long long ph = flips[4 * k], st = flips[4 * k + 1], word = flips[4 * k + 2], bit = flips[4 * k + 3];
    if (ph < 0 || ph >= HBMSCAN_PHASES || st < 0 || st >= hbmscan_steps(static_cast<int>(ph), random_passes) ||
        hbmscan_step_kind(static_cast<int>(ph), static_cast<int>(st)) == HBMSCAN_VERIFY || word < 0 || bit < 0 || bit > 127) {
      g_err = "hbmscan test: a flip needs a phase, a step of it that writes, a word >= 0 and a bit 0..127";
      return -2;
    }
  }
  for (int i = 0; i < 16; ++i) totals[i] = 0;
  for (int ph = 0; ph < HBMSCAN_PHASES; ++ph) {
    phase_errors[ph] = 0;
    phase_ms[ph] = phase_wall_ms[ph] = phase_bytes[ph] = 0.0;
  }
  for (int i = 0; i < HBMSCAN_HIST; ++i) hist[i] = 0;
  *finding = HbmscanFinding{HBMSCAN_NONE, -1, -1, -1, 0, 0, 0};

  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  totals[0] = total_b;
  totals[1] = free_b;
  std::vector<uint64_t> plan(HBMSCAN_MAX_CHUNKS);
  const int planned = hbmscan_ref_plan(free_b, total_b, reserve, limit, chunk, plan.data());
  if (planned < 0) {
    char msg[256];
    snprintf(msg, sizeof msg, "hbmscan test: nothing to test: %llu bytes free of %llu, reserve %llu, limit %llu, chunk "
             "%llu (or more than 4096 chunks)", static_cast<unsigned long long>(free_b),
             static_cast<unsigned long long>(total_b), reserve, limit, chunk);
    g_err = msg;
    return -2;
  }
  uint64_t planned_bytes = 0;
  for (int i = 0; i < planned; ++i) planned_bytes += plan[i];
  totals[2] = planned_bytes;

  // allocate: the planned sizes in order; a failed one is split in two and both halves tried in its place
  std::deque<DevBuf> bufs;  // (a deque: DevBuf does not move)
  std::vector<Chunk> chunks;
  std::deque<uint64_t> todo(plan.begin(), plan.begin() + planned);
  uint64_t tested_words = 0;
  int mallocs = 0;
  while (!todo.empty() && chunks.size() < static_cast<size_t>(HBMSCAN_MAX_CHUNKS)) {
    const uint64_t bytes = todo.front();
    todo.pop_front();
    bufs.emplace_back();
    ++mallocs;
    const hipError_t e = mallocs == fail_alloc_at ? hipErrorOutOfMemory : bufs.back().alloc(device, bytes);
    if (e == hipSuccess) {
      chunks.push_back({static_cast<u32x4*>(bufs.back().ptr), bytes / HBMSCAN_WORD, tested_words});
      tested_words += bytes / HBMSCAN_WORD;
      continue;
    }
    (void)hipGetLastError();  // not sticky: the next call's check must not see it
    bufs.pop_back();
    ++totals[12];
    uint64_t half = bytes / 2;
    half -= half % HBMSCAN_WORD;
    if (half < min_chunk) break;  // go on with what is held
    ++totals[11];
    todo.push_front(bytes - half);
    todo.push_front(half);
  }
  totals[3] = tested_words * HBMSCAN_WORD;
  totals[4] = chunks.size();
  totals[8] = totals[3] < HBMSCAN_CACHED_BELOW ? 1 : 0;
  if (!tested_words) {
    g_err = "hbmscan test: no chunk could be allocated";
    return -1;
  }
  for (int k = 0; k < n_flips; ++k)
    if (static_cast<uint64_t>(flips[4 * k + 2]) >= tested_words) {
      g_err = "hbmscan test: a flip's word lies outside the tested set";
      return -2;
    }
  for (const long long w : {stuck_word, alias_a, alias_b})
    if (w >= 0 && static_cast<uint64_t>(w) >= tested_words) {
      g_err = "hbmscan test: a hook's word lies outside the tested set";
      return -2;
    }

  DevBuf report;
  HIP_CHECK(report.alloc(device, sizeof(Report)));
  Report* rep = static_cast<Report*>(report.ptr);
  HIP_CHECK(hipMemset(rep, 0, sizeof(Report)));

  unsigned long long errors = 0;
  bool complete = true;
  for (int ph = 0; ph < HBMSCAN_PHASES && complete; ++ph) {
    const int steps = hbmscan_steps(ph, random_passes);
    const auto t_phase = SteadyClock::now();
    for (int st = 0; st < steps; ++st) {
      const int kind = hbmscan_step_kind(ph, st);
      // a verifying step compares against what the step before left; a step that writes too leaves its inverse
      const HbmscanContent c = hbmscan_content(ph, kind == HBMSCAN_WRITE ? st : st - 1, seed);
      const auto t0 = SteadyClock::now();
      for (size_t k = 0; k < chunks.size(); ++k) {
        const Chunk& ch = chunks[k];
        const dim3 grid(static_cast<unsigned>((ch.words + THREADS - 1) / THREADS));
        const Where at = {ph, st, static_cast<unsigned>(k), index_base + ch.base};
        if (kind == HBMSCAN_WRITE)
          hipLaunchKernelGGL(write_kernel, grid, dim3(THREADS), 0, nullptr, ch.ptr, ch.words, at.g0, c);
        else if (kind == HBMSCAN_VERIFY_WRITE)
          hipLaunchKernelGGL(verify_kernel<true>, grid, dim3(THREADS), 0, nullptr, ch.ptr, ch.words, c, at, rep);
        else
          hipLaunchKernelGGL(verify_kernel<false>, grid, dim3(THREADS), 0, nullptr, ch.ptr, ch.words, c, at, rep);
      }
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
      phase_ms[ph] += seconds_since(t0) * 1e3;
      phase_bytes[ph] += static_cast<double>(tested_words * HBMSCAN_WORD) * (kind == HBMSCAN_VERIFY_WRITE ? 2.0 : 1.0);
      if (kind != HBMSCAN_WRITE) {
        unsigned long long now = 0;
        HIP_CHECK(hipMemcpy(&now, &rep->errors, sizeof now, hipMemcpyDeviceToHost));
        phase_errors[ph] += now - errors;
        errors = now;
      }
      if (kind != HBMSCAN_VERIFY) {  // the hooks act on what this step wrote
        for (int k = 0; k < n_flips; ++k)
          if (flips[4 * k] == ph && flips[4 * k + 1] == st)
            if (const int rc = poke_bit(chunks, static_cast<uint64_t>(flips[4 * k + 2]), static_cast<int>(flips[4 * k + 3]), -1))
              return rc;
        if (ph == HBMSCAN_ADDR && st == 0 && alias_a >= 0)
          HIP_CHECK(hipMemcpy(lane_of(chunks, static_cast<uint64_t>(alias_b), 0), lane_of(chunks, static_cast<uint64_t>(alias_a), 0),
                              HBMSCAN_WORD, hipMemcpyDeviceToDevice));
        if (stuck_word >= 0)
          if (const int rc = poke_bit(chunks, static_cast<uint64_t>(stuck_word), stuck_bit, stuck_value)) return rc;
        if (ph == HBMSCAN_FADE && hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(hold_ms));
      }
      totals[9] = static_cast<unsigned long long>(ph);
      totals[10] = static_cast<unsigned long long>(st);
      const bool last = ph == HBMSCAN_PHASES - 1 && st == steps - 1;
      if (deadline_s > 0.0 && !last && seconds_since(t_start) >= deadline_s) {
        complete = false;
        break;
      }
    }
    phase_wall_ms[ph] = seconds_since(t_phase) * 1e3;
  }

  std::vector<Report> h(1);
  HIP_CHECK(hipMemcpy(h.data(), rep, sizeof(Report), hipMemcpyDeviceToHost));
  const int nrec = static_cast<int>(std::min<unsigned long long>(h[0].errors, HBMSCAN_MAX_RECORDS));
  for (int i = 0; i < nrec; ++i) records[i] = h[0].records[i];
  for (int i = 0; i < HBMSCAN_HIST; ++i) hist[i] = h[0].hist[i];
  totals[5] = h[0].errors;
  totals[6] = static_cast<unsigned long long>(nrec);
  totals[7] = complete ? 1 : 0;
  hbmscan_ref_classify(records, nrec, reinterpret_cast<const uint64_t*>(hist), index_base, tested_words, finding);
  return 0;
}

}  // extern "C"
