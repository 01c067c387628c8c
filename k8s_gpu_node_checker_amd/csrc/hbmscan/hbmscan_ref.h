// The hbmscan diagnostic's three pure parts (hbmscan.hip): what every 16-byte word of the tested set must hold after
// every step, how the free memory is cut into chunks, and what a set of wrong words is called.  Plain C++ that the
// host compiler takes alone: hbmscan.hip includes it for its kernels and its host side, and tests/test_hbmscan_cpu.py
// compiles it with g++ into a stand-alone program and holds it against an independent Python model.
//
// The tested set is every chunk the scan holds, laid end to end: word g (16 bytes) of it has the global index
// index_base + g, continuous across chunks and 64 bits wide.  The phases, in the order they run:
//   addr    3 steps  the word holds its own global index raw, {lo32(g), hi32(g), ~lo32(g), ~hi32(g)} -- not hashed, so
//                    a word that reads as another word's content names the word it was written as; then the inverse
//   invert  16 steps moving inversions over 0x00000000, 0x55555555, 0x33333333, 0x0F0F0F0F: with their inverses every
//                    bit of the 128-bit word holds 0 and 1 beside equal and beside opposite neighbours
//   random  4 steps per pass: moving inversions over the address hash of the memtest (mix32 of the 32-bit lane's
//                    index plus the seed, csrc/diag/mem_kernels.h pattern()); pass k hashes with seed + k * 2^64/phi
//   fade    3 steps  the hash pattern written, held hold_ms, verified; then the same with its inverse
// A moving inversion over a pattern p is four steps: write p; verify p and write ~p; verify ~p and write p; verify p.
// addr and fade are its first two steps and a last verify.  So a step s of a phase verifies what step s - 1 left
// (s > 0) and, unless it is a phase's or a pattern's last, writes; a step that does both writes the inverse of what it
// verified, from the expected value and never from the word it read.
//
// Every step sweeps all chunks in the same, ascending order.  Between a word's write and its next read lies the whole
// tested set of other traffic, so with more than the caches hold (2 GiB, HBMSCAN_CACHED_BELOW) the read comes from
// HBM, not from the L2s or the 256 MiB Infinity Cache.  There are no descending sweeps, on purpose: order inside a
// launch means nothing on a GPU, and a sweep reversed chunk by chunk would read its most recently written 256 MiB
// and more straight back out of the caches -- it would test less, not more.
#ifndef K8S_GPU_NODE_CHECKER_AMD_HBMSCAN_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_HBMSCAN_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HBMSCAN_HD __host__ __device__ inline
#else
#define HBMSCAN_HD inline
#endif

enum HbmscanPhase { HBMSCAN_ADDR = 0, HBMSCAN_INVERT = 1, HBMSCAN_RANDOM = 2, HBMSCAN_FADE = 3, HBMSCAN_PHASES = 4 };
enum HbmscanStepKind { HBMSCAN_WRITE = 0, HBMSCAN_VERIFY_WRITE = 1, HBMSCAN_VERIFY = 2 };
enum HbmscanFindingKind {
  HBMSCAN_NONE = 0,
  HBMSCAN_STUCK_BIT = 1,
  HBMSCAN_ALIAS = 2,
  HBMSCAN_REGION = 3,
  HBMSCAN_SCATTERED = 4,
};

constexpr int HBMSCAN_INVERT_PATTERNS = 4;
constexpr int HBMSCAN_MAX_RANDOM_PASSES = 64;
constexpr int HBMSCAN_MAX_RECORDS = 64;          // the first wrong words, kept whole
constexpr int HBMSCAN_HIST_WORDS = 4096;         // the first wrong words whose flipped bits are counted
constexpr int HBMSCAN_HIST = 256;                // 128 bit positions x 2 directions: [2 * bit + (0: 1->0, 1: 0->1)]
constexpr int HBMSCAN_MAX_CHUNKS = 4096;
constexpr uint64_t HBMSCAN_WORD = 16;
constexpr uint64_t HBMSCAN_DEFAULT_RESERVE = 2ULL << 30;  // policy, not a measurement: 0.7 % of an MI355X's 288 GB, left
                                                          // to the runtime and to the agent's other libraries
constexpr uint64_t HBMSCAN_DEFAULT_CHUNK = 4ULL << 30;
constexpr uint64_t HBMSCAN_MAX_CHUNK = 16ULL << 30;  // 2^30 words: 2^22 workgroups of 256, far below gridDim.x's 2^31 - 1
constexpr uint64_t HBMSCAN_MIN_CHUNK = 256ULL << 20;  // a chunk that fails to allocate is halved down to here
constexpr uint64_t HBMSCAN_CACHED_BELOW = 2ULL << 30;  // below it the caches may answer a read: csrc/diag's per-XCD HBM
                                                       // test uses the same 2 GiB to get past the L2s and the Infinity Cache
constexpr uint64_t HBMSCAN_REGION_BYTES = 2ULL << 20;  // the aligned span of the `region` finding
constexpr int HBMSCAN_STUCK_PERCENT = 90;  // a classification rule (tested on synthetic input), not a pass threshold

struct HbmscanWord {
  uint32_t w[4];
};

// One wrong word: where it was read and what it held.  `global` is index_base + the word's index in the tested set.
struct HbmscanRecord {
  uint32_t phase, step, chunk, pad;
  uint64_t word;    // in its chunk
  uint64_t global;
  uint32_t got[4], want[4];
};

struct HbmscanFinding {
  int32_t kind;       // HbmscanFindingKind
  int32_t bit;        // stuck_bit: the position in the 128-bit word; alias: the one bit the two indices differ in, or -1
  int32_t direction;  // stuck_bit: 1 = reads 1 where 0 was written (0->1), 0 = 1->0; else -1
  int32_t chunk;      // region: the chunk; else -1
  uint64_t victim;    // alias: the word that read wrong (global index)
  uint64_t source;    // alias: the word whose own-address content it held
  uint64_t span;      // region: byte offset of the aligned 2 MiB span in its chunk
};

HBMSCAN_HD int hbmscan_steps(int phase, int random_passes) {
  switch (phase) {
    case HBMSCAN_ADDR:
    case HBMSCAN_FADE:
      return 3;
    case HBMSCAN_INVERT:
      return 4 * HBMSCAN_INVERT_PATTERNS;
    case HBMSCAN_RANDOM:
      return 4 * random_passes;
    default:
      return 0;
  }
}

HBMSCAN_HD int hbmscan_step_kind(int phase, int step) {
  if (phase == HBMSCAN_ADDR || phase == HBMSCAN_FADE)
    return step == 0 ? HBMSCAN_WRITE : step == 1 ? HBMSCAN_VERIFY_WRITE : HBMSCAN_VERIFY;
  const int sub = step & 3;
  return sub == 0 ? HBMSCAN_WRITE : sub == 3 ? HBMSCAN_VERIFY : HBMSCAN_VERIFY_WRITE;
}

// The 64 -> 32 bit hash of the memtest's pattern (murmur3's finalizer; csrc/common/hip_host.h mix32)
HBMSCAN_HD uint32_t hbmscan_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// What the words hold after a step, without the word index: the kernels take it as one launch argument.
struct HbmscanContent {
  int32_t kind;      // 0 own address, 1 `fixed` in all four lanes, 2 the hash with `seed`
  uint32_t fixed;
  uint32_t invert;   // 0, or ~0: every lane inverted
  uint64_t seed;
};

HBMSCAN_HD HbmscanContent hbmscan_content(int phase, int step, uint64_t seed) {
  HbmscanContent c = {0, 0u, 0u, 0};
  if (phase == HBMSCAN_ADDR || phase == HBMSCAN_FADE) {
    c.kind = phase == HBMSCAN_ADDR ? 0 : 2;
    c.seed = seed ^ 0xFADEFADEFADEFADEULL;  // (fade: another hash than random pass 0's)
    c.invert = step >= 1 ? ~0u : 0u;
    return c;
  }
  const int sub = step & 3, pass = step >> 2;
  c.invert = sub == 1 ? ~0u : 0u;  // after write p / verify-write ~p / verify-write p / verify p
  if (phase == HBMSCAN_INVERT) {
    const int p = pass & (HBMSCAN_INVERT_PATTERNS - 1);
    c.kind = 1;
    c.fixed = p == 0 ? 0x00000000u : p == 1 ? 0x55555555u : p == 2 ? 0x33333333u : 0x0F0F0F0Fu;
  } else {
    c.kind = 2;
    c.seed = seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(pass);
  }
  return c;
}

HBMSCAN_HD HbmscanWord hbmscan_word(const HbmscanContent& c, uint64_t g) {
  HbmscanWord v;
  if (c.kind == 0) {
    v.w[0] = static_cast<uint32_t>(g);
    v.w[1] = static_cast<uint32_t>(g >> 32);
    v.w[2] = ~v.w[0];
    v.w[3] = ~v.w[1];
  } else if (c.kind == 1) {
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = c.fixed;
  } else {
    for (int l = 0; l < 4; ++l) v.w[l] = hbmscan_mix32(4 * g + static_cast<uint64_t>(l) + c.seed);
  }
  for (int l = 0; l < 4; ++l) v.w[l] ^= c.invert;
  return v;
}

// The expected word: what global word g holds once step `step` of `phase` has run (what it wrote, or, for a
// verifying step that writes nothing, what it verified).  A verifying step s compares against step s - 1.
HBMSCAN_HD HbmscanWord hbmscan_ref_want(int phase, int step, uint64_t global_word, uint64_t seed) {
  return hbmscan_word(hbmscan_content(phase, step, seed), global_word);
}

// The plan: the numbers of hipMemGetInfo into chunk sizes.  The target is min(limit, free - reserve) rounded down to
// 16 bytes (limit 0: no limit); every chunk is `chunk` bytes but a ragged last one.  Returns the number of chunks
// written to plan_out (room for HBMSCAN_MAX_CHUNKS), or -2: free above total, a target under one word (free at or
// below the reserve included), a chunk that is no multiple of 16 in 16 .. 16 GiB, or more chunks than fit.
HBMSCAN_HD int hbmscan_ref_plan(uint64_t free_bytes, uint64_t total_bytes, uint64_t reserve, uint64_t limit,
                                uint64_t chunk, uint64_t* plan_out) {
  if (free_bytes > total_bytes || chunk < HBMSCAN_WORD || chunk > HBMSCAN_MAX_CHUNK || chunk % HBMSCAN_WORD) return -2;
  uint64_t target = free_bytes > reserve ? free_bytes - reserve : 0;
  if (limit && limit < target) target = limit;
  target -= target % HBMSCAN_WORD;
  if (target < HBMSCAN_WORD) return -2;
  const uint64_t n = (target + chunk - 1) / chunk;
  if (n > static_cast<uint64_t>(HBMSCAN_MAX_CHUNKS)) return -2;
  for (uint64_t i = 0; i < n; ++i) plan_out[i] = i + 1 < n ? chunk : target - i * chunk;
  return static_cast<int>(n);
}

// The classifier: a name for the wrong words.  `records` are the first n (at most HBMSCAN_MAX_RECORDS) wrong words,
// `hist` the flipped bits of the first HBMSCAN_HIST_WORDS, [index_base, index_base + tested_words) the global indices
// of the tested set.  In this order:
//   none       no record and no flipped bit
//   stuck_bit  at least 90 % of the flipped bits sit at one position of the 128-bit word, in one direction
//   alias      an addr-phase record read the valid own-address content (in the polarity its step expects) of another
//              word of the tested set: an address line, not a cell.  `bit` when the two indices differ in one bit
//   region     every record lies in one aligned 2 MiB span of one chunk
//   scattered  anything else
// A finding is a description for the operator; it never changes pass / fail: any wrong word fails.
inline void hbmscan_ref_classify(const HbmscanRecord* records, int n, const uint64_t* hist, uint64_t index_base,
                                 uint64_t tested_words, HbmscanFinding* out) {
  HbmscanFinding f = {HBMSCAN_NONE, -1, -1, -1, 0, 0, 0};
  uint64_t flipped = 0, top = 0;
  int top_at = 0;
  for (int i = 0; i < HBMSCAN_HIST; ++i) {
    flipped += hist[i];
    if (hist[i] > top) {
      top = hist[i];
      top_at = i;
    }
  }
  if (n <= 0 && !flipped) {
    *out = f;
    return;
  }
  if (flipped && top * 100 >= flipped * static_cast<uint64_t>(HBMSCAN_STUCK_PERCENT)) {
    f.kind = HBMSCAN_STUCK_BIT;
    f.bit = top_at >> 1;
    f.direction = top_at & 1;
    *out = f;
    return;
  }
  for (int i = 0; i < n; ++i) {
    const HbmscanRecord& r = records[i];
    if (r.phase != HBMSCAN_ADDR || r.got[2] != ~r.got[0] || r.got[3] != ~r.got[1]) continue;
    const uint32_t inv = r.want[0] == static_cast<uint32_t>(r.global) ? 0u : ~0u;  // the polarity this step expects
    const uint64_t named = static_cast<uint64_t>(r.got[0] ^ inv) | (static_cast<uint64_t>(r.got[1] ^ inv) << 32);
    if (named == r.global || named < index_base || named - index_base >= tested_words) continue;
    const uint64_t x = named ^ r.global;
    f.kind = HBMSCAN_ALIAS;
    f.victim = r.global;
    f.source = named;
    if (!(x & (x - 1)))
      for (int b = 0; b < 64; ++b)
        if ((x >> b) & 1) f.bit = b;
    *out = f;
    return;
  }
  const uint64_t span_words = HBMSCAN_REGION_BYTES / HBMSCAN_WORD;
  bool one = n > 0;
  for (int i = 1; i < n; ++i)
    one = one && records[i].chunk == records[0].chunk && records[i].word / span_words == records[0].word / span_words;
  if (one) {
    f.kind = HBMSCAN_REGION;
    f.chunk = static_cast<int32_t>(records[0].chunk);
    f.span = records[0].word / span_words * HBMSCAN_REGION_BYTES;
  } else {
    f.kind = HBMSCAN_SCATTERED;
  }
  *out = f;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_HBMSCAN_REF_H_
