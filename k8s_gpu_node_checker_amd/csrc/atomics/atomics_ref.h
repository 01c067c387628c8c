// The atomics diagnostic's operands (atomics.hip) and what correct memory-side atomic units must leave behind.
// Plain C++ that the host compiler takes alone: atomics.hip includes it for its kernels and its host side, and
// tests/test_atomics_cpu.py compiles it with g++ into a stand-alone program that applies every element's operands in
// shuffled orders, in the element type's own arithmetic, and holds each order against atomics_expected().
//
// An element i of kind k starts as atomics_init(k, i, seed) and receives one operand atomics_operand(k, i, a, seed)
// from each adder a of 0..adders-1, in whatever order the adders' workgroups arrive.  Every value travels as the 64
// bits of its element (32-bit kinds in the low word), so one verifier compares bits for every kind.  The result does
// not depend on the order:
//   add_u32 / add_u64   modular sums of full-width hash values
//   add_f32             integers: initial value |x| <= 2^15, operands 1 <= |x| <= 2^15; with adders <= 32 every
//                       partial sum is at most 33 * 2^15 < 2^24 in magnitude, so every add is exact in fp32
//   add_f64             integers up to 2^40 likewise: partial sums below 2^46, exact in fp64
//   pk_bf16             two sums per word, integers |x| <= 7 (operands 1..7): partial sums <= 33 * 7 = 231, exact in
//                       bf16's 8 significant bits
//   max_u32             the maximum of the initial value and the operands
//   xor_u32             full-width hash values: every bit position is toggled
// An exact sum that cancels is +0 in round-to-nearest, and no operand is -0, so no result is -0 either.
// Operands of the add and xor kinds are never zero: an adder that was lost always shows.
#ifndef K8S_GPU_NODE_CHECKER_AMD_ATOMICS_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_ATOMICS_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATOMICS_HD __host__ __device__ inline
#else
#define ATOMICS_HD inline
#endif

enum AtomicsKind {
  ATOMICS_ADD_U32 = 0,
  ATOMICS_ADD_U64 = 1,
  ATOMICS_ADD_F32 = 2,
  ATOMICS_ADD_F64 = 3,
  ATOMICS_PK_BF16 = 4,
  ATOMICS_MAX_U32 = 5,
  ATOMICS_XOR_U32 = 6,
  ATOMICS_TICKET = 7,
  ATOMICS_KINDS = 8,
};
constexpr int ATOMICS_MAX_ADDERS = 32;     // the exactness bounds above hold up to here
constexpr int ATOMICS_F32_MAX = 1 << 15;   // |x| of add_f32's integers
constexpr long long ATOMICS_F64_MAX = 1LL << 40;
constexpr int ATOMICS_BF16_MAX = 7;

ATOMICS_HD int atomics_elem_bytes(int kind) { return kind == ATOMICS_ADD_U64 || kind == ATOMICS_ADD_F64 ? 8 : 4; }

// 64 hashed bits of (seed, kind, element, slot); slot 0 is the initial value, slot a + 1 adder a's operand
ATOMICS_HD uint64_t atomics_hash(uint64_t seed, int kind, uint64_t i, int slot) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ULL * (i + 1) + 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(kind * 64 + slot + 1);
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// an integer of -m..m from h; operands (slot > 0) leave out 0
ATOMICS_HD long long atomics_int(uint64_t h, long long m, int slot) {
  if (slot == 0) return static_cast<long long>(h % static_cast<uint64_t>(2 * m + 1)) - m;
  const long long v = static_cast<long long>(h % static_cast<uint64_t>(2 * m)) - m;  // -m .. m - 1
  return v >= 0 ? v + 1 : v;
}

ATOMICS_HD uint32_t atomics_f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof u);
  return u;
}
ATOMICS_HD uint64_t atomics_f64_bits(double f) {
  uint64_t u;
  __builtin_memcpy(&u, &f, sizeof u);
  return u;
}
// bf16 of an integer of at most 8 significant bits: the upper half of its fp32 form, exact
ATOMICS_HD uint32_t atomics_bf16_bits(int v) { return atomics_f32_bits(static_cast<float>(v)) >> 16; }

// the two integers of a pk_bf16 slot: [0] the low half of the word, [1] the high half
ATOMICS_HD int atomics_pk_int(uint64_t h, int half, int slot) {
  return static_cast<int>(atomics_int(half ? h >> 32 : h & 0xffffffffULL, ATOMICS_BF16_MAX, slot));
}

// The element's 64 bits for the integer its slot holds (the float kinds), or the hash itself.
ATOMICS_HD uint64_t atomics_slot_bits(int kind, uint64_t i, int slot, uint64_t seed) {
  const uint64_t h = atomics_hash(seed, kind, i, slot);
  switch (kind) {
    case ATOMICS_ADD_U64:
      return slot && !h ? 1 : h;
    case ATOMICS_ADD_F32:
      return atomics_f32_bits(static_cast<float>(atomics_int(h, ATOMICS_F32_MAX, slot)));
    case ATOMICS_ADD_F64:
      return atomics_f64_bits(static_cast<double>(atomics_int(h, ATOMICS_F64_MAX, slot)));
    case ATOMICS_PK_BF16:
      return atomics_bf16_bits(atomics_pk_int(h, 0, slot)) | (atomics_bf16_bits(atomics_pk_int(h, 1, slot)) << 16);
    case ATOMICS_MAX_U32:
      return h & 0xffffffffULL;
    default: {  // add_u32, xor_u32
      const uint64_t v = h & 0xffffffffULL;
      return slot && !v ? 1 : v;
    }
  }
}

ATOMICS_HD uint64_t atomics_init(int kind, uint64_t i, uint64_t seed) { return atomics_slot_bits(kind, i, 0, seed); }
ATOMICS_HD uint64_t atomics_operand(int kind, uint64_t i, int adder, uint64_t seed) {
  return atomics_slot_bits(kind, i, adder + 1, seed);
}

// What element i holds after adders 0..adders-1 applied their operands, in any order; `without` >= 0 leaves that
// adder's operand out (what a lost add leaves behind).  The float kinds sum their integers exactly and convert once.
ATOMICS_HD uint64_t atomics_expected(int kind, uint64_t i, int adders, uint64_t seed, int without = -1) {
  switch (kind) {
    case ATOMICS_ADD_F32:
    case ATOMICS_ADD_F64: {
      const long long m = kind == ATOMICS_ADD_F32 ? ATOMICS_F32_MAX : ATOMICS_F64_MAX;
      long long sum = atomics_int(atomics_hash(seed, kind, i, 0), m, 0);
      for (int a = 0; a < adders; ++a)
        if (a != without) sum += atomics_int(atomics_hash(seed, kind, i, a + 1), m, a + 1);
      return kind == ATOMICS_ADD_F32 ? atomics_f32_bits(static_cast<float>(sum)) : atomics_f64_bits(static_cast<double>(sum));
    }
    case ATOMICS_PK_BF16: {
      int lo = 0, hi = 0;
      for (int s = 0; s <= adders; ++s) {
        if (s - 1 == without && s > 0) continue;
        const uint64_t h = atomics_hash(seed, kind, i, s);
        lo += atomics_pk_int(h, 0, s);
        hi += atomics_pk_int(h, 1, s);
      }
      return atomics_bf16_bits(lo) | (atomics_bf16_bits(hi) << 16);
    }
    default: {
      uint64_t x = atomics_init(kind, i, seed);
      for (int a = 0; a < adders; ++a) {
        if (a == without) continue;
        const uint64_t v = atomics_operand(kind, i, a, seed);
        if (kind == ATOMICS_MAX_U32)
          x = v > x ? v : x;
        else if (kind == ATOMICS_XOR_U32)
          x ^= v;
        else
          x += v;
      }
      return kind == ATOMICS_ADD_U64 ? x : x & 0xffffffffULL;
    }
  }
}

// The ticket kind.  `words` elements (at most ATOMICS_TICKET_MAX_WORDS take part) draw `adders` tickets each: element
// i draws from counter c = i % counters with a returning add of 1, and marks hits[c * tickets + t] for the value t it
// was handed.  Counter c serves the elements i = c, c + counters, ...: it must end at atomics_ticket_count(c), and
// its hit words below that count must each be exactly 1, the rest of its `tickets` words 0: the returned values were
// then a permutation of 0..count-1.  64 consecutive elements address 64 different counters (counters >= 64, or every
// element has a counter of its own), so a wave's returning add is 64 requests, not one folded add.
constexpr uint64_t ATOMICS_TICKET_MAX_WORDS = 1ULL << 20;
constexpr uint64_t ATOMICS_TICKET_MAX_COUNTERS = 1ULL << 14;
struct AtomicsTicketPlan {
  uint64_t words;     // elements that take part
  uint64_t counters;
  uint64_t tickets;   // hit words per counter: adders * ceil(words / counters)
  ATOMICS_HD uint64_t hits() const { return counters * tickets; }
  ATOMICS_HD uint64_t elements() const { return hits() + counters; }  // what the verifier checks: hits, then counters
};
ATOMICS_HD AtomicsTicketPlan atomics_ticket_plan(uint64_t words, int adders) {
  AtomicsTicketPlan p;
  p.words = words < ATOMICS_TICKET_MAX_WORDS ? words : ATOMICS_TICKET_MAX_WORDS;
  p.counters = p.words < ATOMICS_TICKET_MAX_COUNTERS ? p.words : ATOMICS_TICKET_MAX_COUNTERS;
  p.tickets = static_cast<uint64_t>(adders) * ((p.words + p.counters - 1) / p.counters);
  return p;
}
// tickets drawn from counter c; `without_word` >= 0: one draw of that element was lost
ATOMICS_HD uint64_t atomics_ticket_count(const AtomicsTicketPlan& p, uint64_t c, int adders, long long without_word = -1) {
  const uint64_t served = p.words / p.counters + (c < p.words % p.counters ? 1 : 0);
  const uint64_t lost = without_word >= 0 && static_cast<uint64_t>(without_word) < p.words &&
                                static_cast<uint64_t>(without_word) % p.counters == c ? 1 : 0;
  return served * static_cast<uint64_t>(adders) - lost;
}
// verifier element e of the ticket kind: hit word e, or counter e - hits()
ATOMICS_HD uint64_t atomics_ticket_expected(const AtomicsTicketPlan& p, uint64_t e, int adders, long long without_word = -1) {
  if (e >= p.hits()) return atomics_ticket_count(p, e - p.hits(), adders, without_word);
  return e % p.tickets < atomics_ticket_count(p, e / p.tickets, adders, without_word) ? 1 : 0;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_ATOMICS_REF_H_
