// The handoff diagnostic's constants (handoff.hip) and what a correct hand-off must deliver: the word a producer
// writes, who hands to whom, the uneven load of a round, and the classifier of a wrong word.  Plain C++ that the host
// compiler takes alone: handoff.hip includes it for its kernels (every lane computes the expected word in registers)
// and its host side (the classifier), and tests/test_handoff_cpu.py compiles it with g++ into a stand-alone program.
//
// A hand-off only moves bits, so the expected word is a hash and every word compares bit for bit.  Workgroup w of G
// owns one slab of HANDOFF_SLAB_WORDS words; in round r it writes  handoff_word(seed, w, r, i)  into word i and
// consumes the slab of  handoff_producer(placement, w, G):  w + 1 in the `cross` placement (blocks b and b + 1 are
// observed on different XCDs), w + 8 in `same` (b and b + 8 on one).  Nothing is assumed from that: the kernels record
// where they ran.  A wrong word that equals the producer's word of one of the HANDOFF_STALE_ROUNDS rounds before is
// `stale` with that age (the release or the acquire let an old copy through); any other is `corrupt`.
#ifndef K8S_GPU_NODE_CHECKER_AMD_HANDOFF_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_HANDOFF_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HANDOFF_HD __host__ __device__ inline
#else
#define HANDOFF_HD inline
#endif

constexpr int HANDOFF_THREADS = 256;        // of a workgroup: 4 waves
constexpr int HANDOFF_SLAB_WORDS = 1024;    // a slab: 4 KiB, 16 bytes per thread
constexpr int HANDOFF_GRANULES = 512;       // the granule form's slab: 8-byte {tag, value} granules, 2 per thread
constexpr int HANDOFF_LINE_BYTES = 128;     // every flag and every ack sits on a line of its own
constexpr int HANDOFF_MIN_BLOCKS = 16;      // the least grid where w + 8 differs from w, two workgroups per XCD
constexpr int HANDOFF_XCD_STRIDE = 8;       // blocks b and b + 8 are observed on one XCD
constexpr int HANDOFF_STALE_ROUNDS = 8;     // how far back the classifier looks
constexpr int HANDOFF_MAX_ROUNDS = 1 << 15; // Report::index keeps the round in 16 bits
constexpr int HANDOFF_DEFAULT_ROUNDS = 64;
constexpr int HANDOFF_DEFAULT_SPIN_MS = 50; // three orders above the dearest hop measured (44.5 us)
constexpr int HANDOFF_MAX_SPIN_MS = 1000;
constexpr int HANDOFF_SLEEPS = 32;          // a round's delay: handoff_sleeps() < this many s_sleep
constexpr int HANDOFF_PRIVATE_PASSES = 4;   // ... and up to this many 4 KiB passes of private stores (16 KiB)
// more than half of a CU's 160 KiB of LDS: at most one workgroup is resident per CU
constexpr int HANDOFF_LDS_BYTES = 81 * 1024;

enum HandoffForm { HANDOFF_FENCE = 0, HANDOFF_WT, HANDOFF_WT_ADD, HANDOFF_GRANULE, HANDOFF_FORMS };
enum HandoffPlacement { HANDOFF_CROSS = 0, HANDOFF_SAME, HANDOFF_PLACEMENTS };
constexpr int HANDOFF_ROWS = HANDOFF_FORMS * HANDOFF_PLACEMENTS;  // row = form * 2 + placement
enum HandoffWait { HANDOFF_WAIT_NONE = 0, HANDOFF_WAIT_FLAG, HANDOFF_WAIT_ACK, HANDOFF_WAIT_GRANULE };
enum HandoffClass { HANDOFF_CLASS_NONE = 0, HANDOFF_CLASS_STALE, HANDOFF_CLASS_CORRUPT };

struct HandoffFormName {
  const char* name;
  const char* what;
};
constexpr HandoffFormName HANDOFF_FORM_TABLE[HANDOFF_FORMS] = {
    {"fence", "plain stores, agent release fence, flag; poll, agent acquire fence, plain loads"},
    {"wt", "write-through sc1 stores, sc1 flag; sc1 poll, sc1 loads, no fence"},
    {"wt_add", "write-through sc1 stores, agent atomic add; sc1 poll of the counter, sc1 loads"},
    {"granule", "8-byte {tag, value} granules, one agent store each; swept until every tag is the epoch"},
};
constexpr const char* HANDOFF_PLACEMENT_TABLE[HANDOFF_PLACEMENTS] = {"cross", "same"};

// the 64 -> 32 bit hash (murmur3's finalizer)
HANDOFF_HD constexpr uint32_t handoff_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// word i of workgroup w's slab in round r (the granule form: the value of granule i)
HANDOFF_HD constexpr uint32_t handoff_word(uint64_t seed, uint32_t w, uint32_t r, uint32_t i) {
  return handoff_mix32((seed + 0x9E3779B97F4A7C15ULL * (static_cast<uint64_t>(r) + 1)) ^
                       ((static_cast<uint64_t>(w) << 32) | i));
}

// whose slab w consumes, and who consumes w's: permutations of [0, G) without a fixed point for G >= 16
HANDOFF_HD constexpr int handoff_stride(int placement) { return placement == HANDOFF_SAME ? HANDOFF_XCD_STRIDE : 1; }
HANDOFF_HD constexpr int handoff_producer(int placement, int w, int G) { return (w + handoff_stride(placement)) % G; }
HANDOFF_HD constexpr int handoff_consumer(int placement, int w, int G) { return (w + G - handoff_stride(placement)) % G; }

// the uneven load of workgroup w in round r: how many s_sleep it waits, how many 4 KiB passes it stores privately
HANDOFF_HD constexpr uint32_t handoff_jitter(uint64_t seed, uint32_t w, uint32_t r) {
  return handoff_mix32((seed ^ 0x6A09E667F3BCC908ULL) + ((static_cast<uint64_t>(r) << 32) | w));
}
HANDOFF_HD constexpr uint32_t handoff_sleeps(uint32_t jitter) { return jitter % HANDOFF_SLEEPS; }
HANDOFF_HD constexpr uint32_t handoff_passes(uint32_t jitter) {
  return (jitter >> 5) & 1u ? (jitter >> 8) % (HANDOFF_PRIVATE_PASSES + 1) : 0u;
}

// A wrong word `got` read in round `round` for word `word` of `producer`'s slab: the age 1..HANDOFF_STALE_ROUNDS of
// the earlier round whose word it is (stale), or 0 (corrupt).  Round 0 has no earlier round.
HANDOFF_HD constexpr int handoff_stale_age(uint64_t seed, uint32_t producer, uint32_t round, uint32_t word, uint32_t got) {
  for (uint32_t age = 1; age <= static_cast<uint32_t>(HANDOFF_STALE_ROUNDS) && age <= round; ++age)
    if (got == handoff_word(seed, producer, round - age, word)) return static_cast<int>(age);
  return 0;
}
HANDOFF_HD constexpr int handoff_classify(uint64_t seed, uint32_t producer, uint32_t round, uint32_t word, uint32_t got,
                                          int* age) {
  *age = handoff_stale_age(seed, producer, round, word, got);
  return *age ? HANDOFF_CLASS_STALE : HANDOFF_CLASS_CORRUPT;
}

// Report::index of a wrong word: producer << 32 | round << 16 | word
HANDOFF_HD constexpr uint64_t handoff_index(uint32_t producer, uint32_t round, uint32_t word) {
  return (static_cast<uint64_t>(producer) << 32) | (static_cast<uint64_t>(round) << 16) | word;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_HANDOFF_REF_H_
