// The scratch diagnostic's host models and classifier, shared by csrc/scratch/scratch.hip (device and host)
// and by plain g++ (tests/test_scratch_cpu.py compiles it into an answer program and holds it against an independent
// Python implementation).  Private (scratch) memory is what every other diagnostic here is built NOT to have.
//
// isolate  no two resident waves share a frame: the word a wave writes into cell `word` of lane `lane` in round
//          `round` is scratch_mix(scratch_pack(round, wave, lane, word)) ^ seed, a bijection of the packed tuple, so
//          the host unmixes a wrong word and says whose it is (scratch_classify): `alias` (a valid cell of another
//          wave, lane or word: the writer is named; its round may differ, two waves that share a frame need not be in
//          step), `stale` (the same cell of an earlier round, with its age), `corrupt` (decodes to no cell of this
//          launch).  The tuple fills all 32 bits, so a corrupted word decodes to some cell of the launch with
//          probability rounds / 16 x waves / 16384 and is then called `alias`.
// frames   what the compiler does with locals: scratch_frames_index (a runtime-indexed local array read and written
//          in a data-dependent order) and scratch_frames_calls (four noinline functions, each with a local buffer of
//          its own and the caller's buffer by pointer), run on both sides and compared bit for bit per lane.
//
// Not here: a table of the scratch_* instruction forms (every width in the off / SGPR / VGPR / SGPR+VGPR modes with
// zero, positive and negative immediates, and flat accesses through the private aperture), walked per lane over a
// guarded frame.  It was built; its first run on an MI355X ended in a memory-access fault of the GPU, in one of its 68
// kernels, which one unknown.  Every statement assembled as written and every address lay inside the lane's frame by
// construction, so the cause is an addressing rule of the hardware that the model did not have.  It was not run again
// and is left out whole until the cause is found without a GPU run.
#ifndef K8S_GPU_NODE_CHECKER_AMD_SCRATCH_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_SCRATCH_REF_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCRATCH_HD __host__ __device__ inline
#define SCRATCH_NOINLINE __host__ __device__ __attribute__((noinline))
#else
#define SCRATCH_HD inline
#define SCRATCH_NOINLINE __attribute__((noinline))
#endif

constexpr int SCRATCH_WAVE = 64;
constexpr int SCRATCH_THREADS = 256;          // of a workgroup: 4 waves
constexpr int SCRATCH_ISO_WORDS = 256;        // the isolate frame: 1 KiB per lane
constexpr int SCRATCH_ISO_MAX_ROUNDS = 16;    // the round's field: 4 bits
constexpr int SCRATCH_ISO_MAX_WAVES = 16384;  // the wave's field: 14 bits
constexpr int SCRATCH_ISO_DEFAULT_ROUNDS = 4;
constexpr int SCRATCH_ISO_DWELL = 64;         // s_sleep 16 this many times between a round's writes and its reads
constexpr int SCRATCH_FRAMES_ARRAY = 64;      // the runtime-indexed local array, words
constexpr int SCRATCH_FRAMES_BUF = 16;        // a function's own buffer, words
constexpr int SCRATCH_FRAMES_DEPTH = 4;       // functions in the chain
constexpr int SCRATCH_FRAMES_OUT = 17;        // words a lane hands back
constexpr int SCRATCH_FRAMES_STEPS = 96;
constexpr int SCRATCH_MAX_FRAME_BYTES = 1024; // no kernel's own locals are larger, per lane
constexpr int SCRATCH_MAX_SEGMENT_BYTES = SCRATCH_MAX_FRAME_BYTES + 64;  // ... and the compiler may add this much of its own (it adds 16)

enum ScratchClass { SCRATCH_CLASS_NONE = 0, SCRATCH_CLASS_ALIAS, SCRATCH_CLASS_STALE, SCRATCH_CLASS_CORRUPT };

// the library's rows
constexpr int SCRATCH_ROW_ISOLATE = 0;
constexpr int SCRATCH_ROW_FRAMES_INDEX = 1;
constexpr int SCRATCH_ROW_FRAMES_CALLS = 2;
constexpr int SCRATCH_ROWS = 3;

// ---- the mix: murmur3's 32-bit finalizer, a bijection, and its inverse ---------------------------------------

SCRATCH_HD constexpr uint32_t scratch_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}
SCRATCH_HD constexpr uint32_t scratch_unmix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7ed1b41du;  // the inverse of 0xc2b2ae35 modulo 2^32
  x ^= x >> 13;
  x ^= x >> 26;
  x *= 0xa5cb9243u;  // the inverse of 0x85ebca6b
  x ^= x >> 16;
  return x;
}

// ---- the lanes' start words ------------------------------------------------------------------------------------

SCRATCH_HD constexpr uint32_t scratch_preset(uint32_t seed, uint32_t wave, uint32_t lane, uint32_t walk, uint32_t word) {
  return scratch_mix(scratch_mix(seed ^ (wave * 64u + lane)) + walk * 0x9e3779b9u + word * 0x85ebca77u + 1u);
}
SCRATCH_HD constexpr uint32_t scratch_start(uint32_t seed, uint32_t wave, uint32_t lane, uint32_t walk) {
  return scratch_mix(scratch_preset(seed, wave, lane, walk, 0xffffu) ^ 0x5c4a7c15u);
}

// ---- isolate ---------------------------------------------------------------------------------------------------

// round:4 | wave:14 | lane:6 | word:8
SCRATCH_HD constexpr uint32_t scratch_pack(uint32_t round, uint32_t wave, uint32_t lane, uint32_t word) {
  return ((round & 15u) << 28) | ((wave & 16383u) << 14) | ((lane & 63u) << 8) | (word & 255u);
}
SCRATCH_HD constexpr uint32_t scratch_iso_word(uint32_t seed, uint32_t round, uint32_t wave, uint32_t lane, uint32_t word) {
  return scratch_mix(scratch_pack(round, wave, lane, word)) ^ seed;
}
// the order a lane writes and reads its frame in: a runtime index, a permutation of 0..255 for every odd stride
SCRATCH_HD constexpr uint32_t scratch_iso_index(uint32_t i, uint32_t lane, uint32_t stride) {
  return (i * stride + lane * 5u) & (SCRATCH_ISO_WORDS - 1);
}

struct ScratchVerdict {
  int cls;             // a ScratchClass
  int age;             // rounds between the writer's round and the reader's (stale: >= 1; alias: 0 when the same round)
  uint32_t round, wave, lane, word;  // the cell the word decodes to (the writer, for an alias)
};
// `cell` = scratch_pack(round, wave, lane, word) of the reader's cell; `got` what it read there (not what it should)
inline ScratchVerdict scratch_classify(uint32_t seed, uint32_t cell, uint32_t got, uint32_t waves, uint32_t rounds) {
  const uint32_t t = scratch_unmix(got ^ seed);
  ScratchVerdict v = {SCRATCH_CLASS_CORRUPT, 0, t >> 28, (t >> 14) & 16383u, (t >> 8) & 63u, t & 255u};
  const uint32_t round = cell >> 28;
  if (v.wave >= waves || v.round >= rounds) return v;
  if ((t & 0x0fffffffu) == (cell & 0x0fffffffu)) {  // this very cell
    if (v.round < round) v.cls = SCRATCH_CLASS_STALE, v.age = static_cast<int>(round - v.round);
    return v;  // its own round or a later one: no valid finding
  }
  v.cls = SCRATCH_CLASS_ALIAS;
  v.age = v.round <= round ? static_cast<int>(round - v.round) : 0;
  return v;
}

// The most intervals [after the writes, before the reads] that were open at one time; t = {from, to} per interval.
inline uint32_t scratch_co_resident(const unsigned long long* t, size_t n, unsigned long long* scratchpad /* 2 n */) {
  // events sorted by time, an opening before a closing at the same tick; a small heap-less sort keeps this header bare
  for (size_t i = 0; i < n; ++i) scratchpad[2 * i] = t[2 * i] << 1, scratchpad[2 * i + 1] = (t[2 * i + 1] << 1) | 1;
  const size_t m = 2 * n;
  for (size_t gap = m / 2; gap > 0; gap /= 2)  // Shell sort
    for (size_t i = gap; i < m; ++i) {
      const unsigned long long v = scratchpad[i];
      size_t j = i;
      for (; j >= gap && scratchpad[j - gap] > v; j -= gap) scratchpad[j] = scratchpad[j - gap];
      scratchpad[j] = v;
    }
  uint32_t open = 0, most = 0;
  for (size_t i = 0; i < m; ++i) {
    if (scratchpad[i] & 1) --open;
    else if (++open > most) most = open;
  }
  return most;
}

// ---- frames ----------------------------------------------------------------------------------------------------

// a runtime-indexed local array, read and written in a data-dependent order
SCRATCH_HD void scratch_frames_index(uint32_t seed, uint32_t wave, uint32_t lane, int steps, uint32_t* out) {
  volatile uint32_t a[SCRATCH_FRAMES_ARRAY];  // volatile: stays a memory object on both sides
  uint32_t x = scratch_start(seed, wave, lane, 0x1dec5u);
  for (uint32_t i = 0; i < SCRATCH_FRAMES_ARRAY; ++i) a[(i * 29u + lane) & (SCRATCH_FRAMES_ARRAY - 1)] = scratch_mix(x + i);
  for (int t = 0; t < steps; ++t) {
    const uint32_t j = x & (SCRATCH_FRAMES_ARRAY - 1);
    x = scratch_mix(x ^ a[j]) + static_cast<uint32_t>(t);
    const uint32_t k = (x >> 6) & (SCRATCH_FRAMES_ARRAY - 1);
    a[k] = a[k] + (x | 1u);
    if (x & 0x1000u) a[j] = a[k] ^ (x >> 3);
  }
  for (int k = 0; k < 16; ++k) out[k] = a[k] ^ a[k + 16] ^ a[k + 32] ^ a[k + 48];
  out[16] = x;
}

// a chain of four functions, each with a buffer of its own and the caller's by pointer; no recursion: four
// instantiations, each calling the next
template <int DEPTH>
SCRATCH_NOINLINE uint32_t scratch_chain(uint32_t* up, uint32_t x) {
  uint32_t buf[SCRATCH_FRAMES_BUF];
  for (uint32_t k = 0; k < SCRATCH_FRAMES_BUF; ++k) buf[k] = scratch_mix(x + k * 0x9e3779b9u + DEPTH) ^ up[(k * 7u + DEPTH) & 15u];
  for (uint32_t k = 0; k < SCRATCH_FRAMES_BUF; ++k) {
    const uint32_t j = (x >> (k & 15u)) & 15u;   // runtime indices into both buffers
    buf[j] ^= up[(j * 5u + k) & 15u] + x;
    x = scratch_mix(x + buf[(x >> 4) & 15u]);
    up[x & 15u] += buf[k] | 1u;
  }
  if constexpr (DEPTH + 1 < SCRATCH_FRAMES_DEPTH) x = scratch_chain<DEPTH + 1>(buf, x);
  for (uint32_t k = 0; k < SCRATCH_FRAMES_BUF; ++k) up[k] ^= buf[(k + x) & 15u];  // after the callee wrote into buf
  return scratch_mix(x ^ up[x & 15u]);
}
SCRATCH_HD void scratch_frames_calls(uint32_t seed, uint32_t wave, uint32_t lane, int steps, uint32_t* out) {
  uint32_t top[SCRATCH_FRAMES_BUF];
  uint32_t x = scratch_start(seed, wave, lane, 0xca11u);
  for (uint32_t k = 0; k < SCRATCH_FRAMES_BUF; ++k) top[k] = scratch_mix(x ^ k);
  for (int t = 0; t < steps; t += 32) x = scratch_chain<0>(top, x + static_cast<uint32_t>(t));
  for (int k = 0; k < 16; ++k) out[k] = top[k];
  out[16] = x;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_SCRATCH_REF_H_
