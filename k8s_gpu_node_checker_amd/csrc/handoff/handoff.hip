// libmi355x_handoff.so: the handoff diagnostic (HIP, gfx950).
//
// Every other diagnostic lets data cross from one workgroup to another only at a kernel boundary.  This one hands
// data from one CU to another INSIDE a launch, which is what the L2 write-back (buffer_wbl2 sc1), the L1 invalidate
// (buffer_inv sc1), write-through sc1 stores, L1-bypassing sc1 loads and agent-scope flags and atomic adds exist for:
// the eight per-XCD L2s are not coherent with each other, and a CU's vector L1 is never refreshed by another CU's
// stores.
//
// G workgroups of 256 threads form a ring of ping-pong hand-offs.  Workgroup w owns one 4 KiB slab, one flag word and
// one ack word (each flag and ack on a 128-byte line of its own) and consumes the slab of handoff_producer(w)
// (handoff_ref.h): w + 1 in the `cross` placement, w + 8 in `same`.  Round r, epoch = r + 1:
//   1. w waits until ack[w] >= r: its consumer has read round r - 1, the slab is free
//   2. every wave pre-reads its lines of the PARTNER's slab with plain loads: the consumer's L1 is warm, so a missing
//      invalidate shows
//   3. uneven load: handoff_sleeps() s_sleep, and hash-chosen workgroups store up to 16 KiB into a private region,
//      which leaves dirty lines in the L2 for the write-back to carry
//   4. w writes its slab with handoff_word(seed, w, r, i) and publishes the epoch, per form
//   5. w waits for its partner's signal, makes the form's acquire and loads the partner's whole slab; every lane
//      compares every word with handoff_word(seed, p, r, i), computed in registers
//   6. s_waitcnt vmcnt(0), a barrier, then lane 0 stores ack[p] = epoch (relaxed, agent)
// The four forms, one template instantiation each:
//   fence    plain global_store_dwordx4; every wave vmcnt(0); barrier; lane 0 fence(release, agent), asm vmcnt(0),
//            relaxed agent flag store | lane 0 relaxed agent poll, fence(acquire, agent), asm vmcnt(0), barrier, plain
//            global_load_dwordx4
//   wt       16-byte sc1 stores; every wave vmcnt(0); barrier; lane 0 sc1 flag store | lane 0 sc1 poll, barrier,
//            global_load_dwordx4 sc1, no fence
//   wt_add   as wt, but the signal is an agent-scope atomic add to a counter (each 128-byte line is written whole by
//            one store instruction of one wave) | global_load_dword sc1 poll of the counter, barrier, sc1 loads
//   granule  512 naturally aligned 8-byte {tag = epoch, value} granules, one relaxed agent store each, no flag and no
//            fence | each wave sweeps its granules with relaxed agent 8-byte loads until every tag is the epoch
//
// Every spin is bounded: one lane (the granule form: one wave) polls relaxed with s_sleep between polls, against a
// wall_clock64 deadline.  The first wave that gives up records who waited for what with agent atomics and sets an
// abort word that every spin also polls, so every workgroup then stops handing off, reports and returns.  HIP
// promises no co-residency and another tenant may hold CUs: a timeout is reported, not failed.
//
// Each kernel declares HANDOFF_LDS_BYTES of LDS, more than half a CU's, so at most one workgroup is resident per CU
// and a grid of at most the CU count is co-resident on an idle device.  Placement is only observed: every workgroup
// records where it ran.  ops/handoff.py is the Python side; ops/diag.run(extra=("handoff",)) runs it next to a
// level's own tests.  The Report, report() and Run are those of common/simd_report.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../common/hip_host.h"
#include "../common/simd_report.h"
#include "handoff_ref.h"

namespace {

constexpr unsigned THREADS = HANDOFF_THREADS;
constexpr unsigned LDS_WORDS = HANDOFF_LDS_BYTES / 4;
constexpr size_t SLAB_BYTES = HANDOFF_SLAB_WORDS * 4;
constexpr size_t PRIVATE_BYTES = HANDOFF_PRIVATE_PASSES * SLAB_BYTES;  // per workgroup
static_assert(HANDOFF_SLAB_WORDS == 4 * HANDOFF_THREADS && HANDOFF_GRANULES == 2 * HANDOFF_THREADS, "16 bytes per thread");
static_assert(HANDOFF_LDS_BYTES > 80 * 1024 && HANDOFF_LDS_BYTES <= 160 * 1024, "more than half of a CU's LDS");

typedef __attribute__((address_space(1))) uint32_t gu32;            // every shared word: a GLOBAL access, never flat
typedef __attribute__((address_space(1))) unsigned long long gu64;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// The first line of the control block.  The block (this line, G flag lines, G ack lines, G slabs) starts at its
// allocation's start, is a multiple of 128 bytes long and is zeroed by a hipMemsetAsync before EVERY launch.
struct Header {
  uint32_t abort;    // set by the first wave that gives up; every spin polls it
  uint32_t claimed;  // 1 once the record below is taken
  uint32_t who, kind, producer, round;  // the first timeout: the workgroup that waited, a HandoffWait, on whom, when
  uint32_t timeouts;                    // waits that ran out
  uint32_t pad;
  unsigned long long rounds_done;       // summed over the workgroups
};
static_assert(sizeof(Header) <= HANDOFF_LINE_BYTES, "one line");

inline size_t ctrl_bytes(unsigned G) { return (1 + 2 * static_cast<size_t>(G)) * HANDOFF_LINE_BYTES + G * SLAB_BYTES; }

struct Args {
  uint8_t* ctrl;      // the control block
  uint8_t* priv;      // G x PRIVATE_BYTES, never read
  uint32_t* slots;    // G: the wave_slot() every workgroup ran on
  Report* rep;
  unsigned long long* map;
  uint64_t seed;
  long long spin_ticks;  // of wall_clock64
  int G, rounds, placement, jitter;
  int hook_block, hook_round;            // -1: no hook
  int hook_flip, hook_stale, hook_mute;  // which one (hook_stale: the word, -1: none)
};

__device__ __forceinline__ gu32* line_word(uint8_t* ctrl, unsigned line) {
  return (gu32*)(ctrl + static_cast<size_t>(line) * HANDOFF_LINE_BYTES);
}

// a wait ran out: count it, take the record if it is free, tell every other spin
__device__ __forceinline__ void give_up(Header* h, uint32_t who, uint32_t kind, uint32_t producer, uint32_t round) {
  __hip_atomic_fetch_add((gu32*)&h->timeouts, 1u, RLX_AGENT);
  if (__hip_atomic_exchange((gu32*)&h->claimed, 1u, RLX_AGENT) == 0u) {
    __hip_atomic_store((gu32*)&h->who, who, RLX_AGENT);
    __hip_atomic_store((gu32*)&h->kind, kind, RLX_AGENT);
    __hip_atomic_store((gu32*)&h->producer, producer, RLX_AGENT);
    __hip_atomic_store((gu32*)&h->round, round, RLX_AGENT);
  }
  __hip_atomic_store((gu32*)&h->abort, 1u, RLX_AGENT);
}

// ONE lane polls ONE word, relaxed at agent scope (global_load_dword sc1), until it equals `want` (AT_LEAST: reaches
// it), with s_sleep between polls.  Bounded: false once the abort word is set or `ticks` have passed.
template <bool AT_LEAST>
__device__ __forceinline__ bool spin(gu32* word, uint32_t want, Header* h, long long ticks, uint32_t who, uint32_t kind,
                                     uint32_t producer, uint32_t round) {
  const long long t0 = wall_clock64();
  for (;;) {
    const uint32_t v = __hip_atomic_load(word, RLX_AGENT);
    if (AT_LEAST ? v >= want : v == want) return true;
    if (__hip_atomic_load((gu32*)&h->abort, RLX_AGENT)) return false;
    if (wall_clock64() - t0 > ticks) {
      give_up(h, who, kind, producer, round);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

__device__ __forceinline__ void store_plain(uint8_t* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %[p], %[v], off" : : [p] "v"(p), [v] "v"(v) : "memory");
}
__device__ __forceinline__ void store_sc1(uint8_t* p, u32x4 v) {  // write-through
  asm volatile("global_store_dwordx4 %[p], %[v], off sc1" : : [p] "v"(p), [v] "v"(v) : "memory");
}
__device__ __forceinline__ u32x4 load_plain(const uint8_t* p) {
  u32x4 d;
  asm volatile("global_load_dwordx4 %[d], %[p], off\ns_waitcnt vmcnt(0)" : [d] "=&v"(d) : [p] "v"(p) : "memory");
  return d;
}
__device__ __forceinline__ u32x4 load_sc1(const uint8_t* p) {  // bypasses the L1
  u32x4 d;
  asm volatile("global_load_dwordx4 %[d], %[p], off sc1\ns_waitcnt vmcnt(0)" : [d] "=&v"(d) : [p] "v"(p) : "memory");
  return d;
}
#define DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

template <int FORM>
__global__ void __launch_bounds__(THREADS) handoff_kernel(Args a) {
  // one array: lds[0] the ack wait's outcome, lds[1] the signal wait's, lds[2 + wave] a wave's sweep
  __shared__ uint32_t lds[LDS_WORDS];
  const long long t0 = wall_clock64();
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t w = blockIdx.x, G = static_cast<uint32_t>(a.G), rounds = static_cast<uint32_t>(a.rounds);
  const uint32_t p = static_cast<uint32_t>(handoff_producer(a.placement, static_cast<int>(w), a.G));
  Header* h = reinterpret_cast<Header*>(a.ctrl);
  gu32 *my_flag = line_word(a.ctrl, 1 + w), *p_flag = line_word(a.ctrl, 1 + p);
  gu32 *my_ack = line_word(a.ctrl, 1 + G + w), *p_ack = line_word(a.ctrl, 1 + G + p);
  uint8_t* slabs = a.ctrl + (1 + 2 * static_cast<size_t>(G)) * HANDOFF_LINE_BYTES;
  uint8_t *my_slab = slabs + w * SLAB_BYTES, *p_slab = slabs + p * SLAB_BYTES;
  uint8_t* mine = my_slab + tid * 16;          // contiguous lanes: 8 lanes write one 128-byte line whole
  const uint8_t* theirs = p_slab + tid * 16;
  uint8_t* priv = a.priv + w * PRIVATE_BYTES + tid * 16;
  lds[LDS_WORDS - THREADS + tid] = w;  // the far end of the allocation
  const bool hooked = static_cast<int>(w) == a.hook_block;
  uint32_t nbad = 0, bad_got = 0, bad_want = 0, done = 0;
  unsigned long long bad_index = 0;

  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t epoch = r + 1;
    const bool hook_now = hooked && static_cast<int>(r) == a.hook_round;
    const bool mute = hook_now && a.hook_mute;
    const int stale = hook_now ? a.hook_stale : -1;
    // what this workgroup writes into word i: the stale hook's one word keeps the round before
    const auto my_word = [&](uint32_t i) { return handoff_word(a.seed, w, static_cast<int>(i) == stale ? r - 1 : r, i); };

    // 1. the slab is free
    if (r) {
      if (tid == 0) lds[0] = spin<true>(my_ack, r, h, a.spin_ticks, w, HANDOFF_WAIT_ACK, w, r);
      __syncthreads();
      if (!lds[0]) break;
    }
    // 2. the consumer's L1 holds the partner's lines of the round before
    {
      const u32x4 warm = load_plain(theirs);
      asm volatile("" : : "v"(warm));
    }
    // 3. uneven arrival, dirty lines in the L2
    if (a.jitter) {
      const uint32_t j = handoff_jitter(a.seed, w, r);
      for (uint32_t s = handoff_sleeps(j); s; --s) __builtin_amdgcn_s_sleep(4);
      for (uint32_t q = 0; q < handoff_passes(j); ++q) store_plain(priv + q * SLAB_BYTES, u32x4{j, q, r, tid});
    }
    // 4. produce
    if constexpr (FORM == HANDOFF_GRANULE) {
      if (!mute) {
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {  // ONE aligned 8-byte store per granule
          const uint32_t g = k * THREADS + tid;
          __hip_atomic_store((gu64*)my_slab + g, (static_cast<unsigned long long>(epoch) << 32) | my_word(g), RLX_AGENT);
        }
      }
    } else {
      const u32x4 v = {my_word(4 * tid), my_word(4 * tid + 1), my_word(4 * tid + 2), my_word(4 * tid + 3)};
      if constexpr (FORM == HANDOFF_FENCE) store_plain(mine, v);
      else store_sc1(mine, v);
      DRAIN();  // EVERY storing wave
      __syncthreads();
      if (tid == 0) {
        if constexpr (FORM == HANDOFF_FENCE) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          DRAIN();  // the compiler can drop the fence's own wait: always, and before the flag
        }
        if (!mute) {
          if constexpr (FORM == HANDOFF_WT_ADD) __hip_atomic_fetch_add(my_flag, 1u, RLX_AGENT);
          else __hip_atomic_store(my_flag, epoch, RLX_AGENT);
        }
      }
    }
    // 5. consume
    uint32_t got[4], want[4], first_word;
    int nwords;
    bool ok;
    if constexpr (FORM == HANDOFF_GRANULE) {
      gu64* g = (gu64*)p_slab + tid;
      const long long s0 = wall_clock64();
      for (;;) {
        bool all = true;
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
          const unsigned long long x = __hip_atomic_load(g + k * THREADS, RLX_AGENT);
          got[k] = static_cast<uint32_t>(x);
          all &= static_cast<uint32_t>(x >> 32) == epoch;
        }
        ok = __all(all);
        if (ok) break;
        if (__any(__hip_atomic_load((gu32*)&h->abort, RLX_AGENT) != 0u)) break;
        if (__any(wall_clock64() - s0 > a.spin_ticks)) {  // wave-uniform
          if (lane == 0) give_up(h, w, HANDOFF_WAIT_GRANULE, p, r);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (lane == 0) lds[2 + wave] = ok;
      __syncthreads();
      ok = lds[2] & lds[3] & lds[4] & lds[5];
      nwords = 2;
      first_word = tid;
      want[0] = handoff_word(a.seed, p, r, tid);
      want[1] = handoff_word(a.seed, p, r, THREADS + tid);
      want[2] = want[3] = got[2] = got[3] = 0;
    } else {
      if (tid == 0) {
        const bool seen = spin<false>(p_flag, epoch, h, a.spin_ticks, w, HANDOFF_WAIT_FLAG, p, r);
        if constexpr (FORM == HANDOFF_FENCE) {
          if (seen) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // ONE buffer_inv sc1, after the match
            DRAIN();  // holds the barrier until the invalidate has completed
          }
        }
        lds[1] = seen;
      }
      __syncthreads();
      ok = lds[1];
      u32x4 d = {0, 0, 0, 0};
      if (ok) {
        if constexpr (FORM == HANDOFF_FENCE) d = load_plain(theirs);
        else d = load_sc1(theirs);  // EVERY load of the handed-off bytes
      }
      got[0] = d.x, got[1] = d.y, got[2] = d.z, got[3] = d.w;
      nwords = 4;
      first_word = 4 * tid;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) want[j] = handoff_word(a.seed, p, r, 4 * tid + j);
    }
    if (!ok) break;  // the same in every lane of the workgroup
    if (hook_now && a.hook_flip && tid == 0) got[0] ^= 0x10u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nwords && got[j] != want[j]) {
        if (!nbad) {
          const uint32_t word = FORM == HANDOFF_GRANULE ? first_word + j * THREADS : first_word + j;
          bad_index = handoff_index(p, r, word), bad_got = got[j], bad_want = want[j];
        }
        ++nbad;
      }
    }
    // 6. ack: this workgroup's loads of the slab have completed
    DRAIN();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(p_ack, epoch, RLX_AGENT);
    ++done;
  }

  const unsigned row = simd_row();
  if (tid == 0) {
    a.slots[w] = row >> 2;
    __hip_atomic_fetch_add((gu64*)&h->rounds_done, static_cast<unsigned long long>(done), RLX_AGENT);
  }
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  // a record's `where`: SIMD map row << 16 | lane; its index: handoff_index(producer, round, word)
  report(a.rep, a.map, row, nbad, (static_cast<unsigned long long>(row) << 16) | lane, bad_index, bad_got, bad_want, dt);
}

template <int FORM>
void launch_form(unsigned grid, const Args& a) {
  hipLaunchKernelGGL(handoff_kernel<FORM>, dim3(grid), dim3(THREADS), 0, nullptr, a);
}
template <int FORM>
hipError_t attributes_form(hipFuncAttributes* attr) {
  return hipFuncGetAttributes(attr, reinterpret_cast<const void*>(handoff_kernel<FORM>));
}
constexpr void (*LAUNCH[HANDOFF_FORMS])(unsigned, const Args&) = {launch_form<HANDOFF_FENCE>, launch_form<HANDOFF_WT>,
                                                                  launch_form<HANDOFF_WT_ADD>, launch_form<HANDOFF_GRANULE>};
constexpr hipError_t (*ATTRIBUTES[HANDOFF_FORMS])(hipFuncAttributes*) = {
    attributes_form<HANDOFF_FENCE>, attributes_form<HANDOFF_WT>, attributes_form<HANDOFF_WT_ADD>,
    attributes_form<HANDOFF_GRANULE>};

std::string row_name(int row) {
  return std::string(HANDOFF_FORM_TABLE[row / HANDOFF_PLACEMENTS].name) + "/" + HANDOFF_PLACEMENT_TABLE[row % HANDOFF_PLACEMENTS];
}

}  // namespace

extern "C" {

const char* handoff_last_error(void) { return g_err.c_str(); }

int handoff_device_count(void) { return device_count(); }

int handoff_slots(void) { return SIMD_ROWS; }  // rows of the simd_map below

int handoff_lds_bytes(void) { return HANDOFF_LDS_BYTES; }  // what every kernel declares, and the only size allowed

// The rows `rows[0..nrows)` (form * 2 + placement, handoff_ref.h), one after the other, on `blocks` workgroups (0: one
// per CU, rounded down to a multiple of 8): a checked warm-up launch, then `reps` timed and checked launches of
// `rounds` hand-offs per workgroup.  Arrays of HANDOFF_ROWS rows, indexed by the row:
//   errors[k]    wrong 32-bit words over all its launches (granule: wrong values)
//   words[k]     words compared over all its launches
//   timeouts[k]  waits that ran out over all its launches
//   first[8 k..] where (SIMD map row << 16 | lane; ~0: none), handoff_index(producer, round, word), got, want, the
//                producer's wave_slot(), the HandoffClass, the age, the launch (0: the warm-up) of one wrong word of the
//                first launch that had any; the host classifies
//   tmo[4 k..]   the first timeout of the first launch that had one: who waited, the HandoffWait (0: none), on which
//                producer, in which round
//   pairs[3 k..] of the row's last launch: consumer/producer pairs on different XCDs, on one XCD, on one CU
//   ms[k]        the mean time of a timed launch
// simd_map: handoff_slots() x 3 (waves run, wrong words, summed wall_clock64 ticks) per physical SIMD, added up over
// every launch of every row.
//
// Refused with -2 and a message: a bad device, blocks other than 0 or a multiple of 8 from 16 to the CU count, rounds
// outside 1..2^15, reps < 1, spin_ms outside 1..1000, no row or an unknown one, a hook outside the rows, the grid or
// the rounds, a stale word outside the slab or in round 0, more than one hook; with -3: a kernel built with scratch
// or another LDS size than HANDOFF_LDS_BYTES, and a complete launch that shows two workgroups of a pair on one CU.
// A timeout is neither: the row is incomplete and says who waited.
//
// Self-check hooks, off by default (inject_row -1), acting in the warm-up launch of row `inject_row` on workgroup
// `inject_block` in round `inject_round`:
//   flip   (neither of the two below) one bit of lane 0's first loaded word is flipped before the compare: 1 wrong
//          word, got = want ^ 0x10
//   stale  (inject_stale_word >= 0) the producer writes that word with its value of the round before: 1 wrong word at
//          its consumer
//   mute   (inject_mute) the producer leaves that round's signal out: its consumer's wait runs out
int handoff_test(int device, int blocks, int rounds, int reps, const int* rows, int nrows, uint64_t seed, int spin_ms,
                 int jitter, int inject_row, int inject_block, int inject_round, int inject_stale_word, int inject_mute,
                 unsigned long long* errors, unsigned long long* words, unsigned long long* timeouts,
                 unsigned long long* first, unsigned long long* tmo, int* pairs, double* ms,
                 unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  bool known = rows != nullptr && nrows >= 1 && nrows <= HANDOFF_ROWS, hook_listed = inject_row < 0;
  for (int i = 0; known && i < nrows; ++i) {
    known = rows[i] >= 0 && rows[i] < HANDOFF_ROWS;
    hook_listed = hook_listed || rows[i] == inject_row;
  }
  if (device < 0 || device >= n || rounds < 1 || rounds > HANDOFF_MAX_ROUNDS || reps < 1 || spin_ms < 1 ||
      spin_ms > HANDOFF_MAX_SPIN_MS || !known) {
    g_err = "handoff: need a valid device, rounds 1..2^15, reps >= 1, spin_ms 1.." + std::to_string(HANDOFF_MAX_SPIN_MS) +
            " and a list of known rows";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const int cus = cu_count(device);
  const int G = blocks ? blocks : cus - cus % HANDOFF_XCD_STRIDE;
  if (G < HANDOFF_MIN_BLOCKS || G > cus || G % HANDOFF_XCD_STRIDE) {
    g_err = "handoff: blocks must be 0 (one per CU) or a multiple of 8 from " + std::to_string(HANDOFF_MIN_BLOCKS) +
            " to the CU count " + std::to_string(cus) + ", not " + std::to_string(G) +
            ": a larger grid is not co-resident, a smaller one pairs a workgroup with itself";
    return -2;
  }
  *blocks_run = G;
  if (!hook_listed) {
    g_err = "handoff: inject_row must be in the list";
    return -2;
  }
  if (inject_row >= 0) {
    const int limit = inject_row / HANDOFF_PLACEMENTS == HANDOFF_GRANULE ? HANDOFF_GRANULES : HANDOFF_SLAB_WORDS;
    if (inject_block < 0 || inject_block >= G || inject_round < 0 || inject_round >= rounds || inject_stale_word >= limit ||
        (inject_stale_word >= 0 && inject_round < 1) || (inject_stale_word >= 0 && inject_mute)) {
      g_err = "handoff: inject_block must lie inside the grid, inject_round inside the rounds, inject_stale_word inside the "
              "slab and in a round >= 1 (round 0 has no round before), and one hook at a time";
      return -2;
    }
  }
  for (int k = 0; k < HANDOFF_ROWS; ++k) {
    errors[k] = words[k] = timeouts[k] = 0;
    for (int j = 0; j < 8; ++j) first[8 * k + j] = 0;
    first[8 * k] = ~0ULL;
    for (int j = 0; j < 4; ++j) tmo[4 * k + j] = 0;
    for (int j = 0; j < 3; ++j) pairs[3 * k + j] = 0;
    ms[k] = 0.0;
  }
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
    (void)hipGetLastError();
    khz = 100000;  // wall_clock64 of gfx9: 100 MHz
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  const size_t cbytes = ctrl_bytes(static_cast<unsigned>(G));
  DevBuf dctrl, dpriv, dslots;
  HIP_CHECK(dctrl.alloc(device, cbytes));
  HIP_CHECK(dpriv.alloc(device, static_cast<size_t>(G) * PRIVATE_BYTES));
  HIP_CHECK(dslots.alloc(device, static_cast<size_t>(G) * sizeof(uint32_t)));
  std::vector<uint32_t> slots(G);
  for (int i = 0; i < nrows; ++i) {
    const int k = rows[i], form = k / HANDOFF_PLACEMENTS, placement = k % HANDOFF_PLACEMENTS;
    hipFuncAttributes attr;
    HIP_CHECK(ATTRIBUTES[form](&attr));
    if (const int rc = refuse_memory("handoff", row_name(k), attr,
                                     ": scratch would add memory traffic of its own, and only " +
                                         std::to_string(HANDOFF_LDS_BYTES) + " bytes of LDS keep one workgroup per CU",
                                     HANDOFF_LDS_BYTES))
      return rc;
    double total_ms = 0.0;
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};
    for (int r = 0; r <= reps; ++r) {  // r == 0: the warm-up, which carries the hooks
      const bool hooked = r == 0 && k == inject_row;
      const Args a = {static_cast<uint8_t*>(dctrl.ptr), static_cast<uint8_t*>(dpriv.ptr), static_cast<uint32_t*>(dslots.ptr),
                      run.rep(), run.map(), seed, static_cast<long long>(spin_ms) * khz, G, rounds, placement, jitter ? 1 : 0,
                      hooked ? inject_block : -1, hooked ? inject_round : -1,
                      hooked && inject_stale_word < 0 && !inject_mute ? 1 : 0, hooked ? inject_stale_word : -1,
                      hooked && inject_mute ? 1 : 0};
      if (const int rc = run.clear()) return rc;
      HIP_CHECK(hipMemsetAsync(dctrl.ptr, 0, cbytes, nullptr));  // every polled word, before EVERY launch
      float t = 0.f;
      if (const int rc = run.launch([&] { LAUNCH[form](static_cast<unsigned>(G), a); }, &t)) return rc;
      const bool had = rec[0] != ~0ULL;
      if (const int rc = run.collect(errors + k, rec)) return rc;
      if (r > 0) total_ms += t;
      Header h;
      HIP_CHECK(hipMemcpy(&h, dctrl.ptr, sizeof h, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(slots.data(), dslots.ptr, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      words[k] += h.rounds_done * (form == HANDOFF_GRANULE ? HANDOFF_GRANULES : HANDOFF_SLAB_WORDS);
      if (h.timeouts && !timeouts[k]) tmo[4 * k] = h.who, tmo[4 * k + 1] = h.kind, tmo[4 * k + 2] = h.producer, tmo[4 * k + 3] = h.round;
      timeouts[k] += h.timeouts;
      int cross = 0, same_xcd = 0, same_cu = 0;
      for (int w = 0; w < G; ++w) {
        const uint32_t mine = slots[w], theirs = slots[handoff_producer(placement, w, G)];
        if (mine == theirs) ++same_cu;
        else if (mine >> 7 == theirs >> 7) ++same_xcd;
        else ++cross;
      }
      pairs[3 * k] = cross, pairs[3 * k + 1] = same_xcd, pairs[3 * k + 2] = same_cu;
      if (same_cu && !h.timeouts) {
        g_err = "handoff " + row_name(k) + ": " + std::to_string(same_cu) + " pairs ran on one CU although a workgroup "
                "takes more than half of its LDS: the hand-off would not leave the CU";
        return -3;
      }
      if (!had && rec[0] != ~0ULL) {  // this launch's record: name the producer's CU and classify the word
        const uint32_t producer = static_cast<uint32_t>(rec[1] >> 32), round = static_cast<uint32_t>(rec[1] >> 16) & 0xffffu;
        const uint32_t word = static_cast<uint32_t>(rec[1]) & 0xffffu;
        int age = 0;
        const int cls = handoff_classify(seed, producer, round, word, static_cast<uint32_t>(rec[2]), &age);
        for (int j = 0; j < 4; ++j) first[8 * k + j] = rec[j];
        first[8 * k + 4] = producer < static_cast<uint32_t>(G) ? slots[producer] : 0;
        first[8 * k + 5] = static_cast<unsigned long long>(cls);
        first[8 * k + 6] = static_cast<unsigned long long>(age);
        first[8 * k + 7] = static_cast<unsigned long long>(r);
      }
    }
    ms[k] = total_ms / reps;
  }
  return run.read_map(simd_map);
}

}  // extern "C"
