// The vector-ALU burn-in's chains (diag.hip valu_burn_kernel) and what a correct SIMD must leave in them.
// Plain C++: diag.hip includes this inside its anonymous namespace and fills its operand and expectation tables
// from it, and tests/test_simd_diag_cpu.py compiles it with the host compiler against an exact-arithmetic reference.
//
// Every lane runs VALU_CHAINS independent chains of one recurrence, VALU_UNROLL steps per iteration:
//   f64     x = fma(x, a, b) in fp64                                    (v_fma_f64)
//   pk_f32  the same on both halves of a float2                          (v_pk_fma_f32)
//   i32     x = lo32(x) * a + b on a 64-bit x, wrapping mod 2^64         (v_mad_u64_u32)
// Float operands: a = 1 - k / 1024 with k in 16..31 (just below 1), a target t in [0.75, 1.25) on a 2^-11 grid,
// b = (1 - a) * t (exact in either format: 5 x 12 significant bits) and x0 in [1, 2) on a 2^-12 grid.  A step is
// x' = a x + (1 - a) t, which lies between x and t before rounding and, rounding being monotonic, after it: every
// intermediate stays normal and inside [0.75, 2), within the stated [0.5, 2).  A correctly rounded FMA has one
// answer there, so the device must match std::fma bit for bit.
#ifndef K8S_GPU_NODE_CHECKER_AMD_VALU_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_VALU_REF_H_

#include <cmath>
#include <cstdint>

constexpr int VALU_KINDS = 3;    // 0 f64, 1 pk_f32, 2 i32
constexpr int VALU_CHAINS = 8;   // independent chains per lane
constexpr int VALU_UNROLL = 4;   // steps of every chain per iteration
constexpr int VALU_LANES = 64;

inline uint32_t valu_hash(uint32_t lane, uint32_t chain, uint32_t salt) {
  uint64_t x = (static_cast<uint64_t>(lane) * VALU_CHAINS + chain) * 0x9E3779B97F4A7C15ULL + salt * 0xD1B54A32D192ED03ULL;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ULL;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ULL;
  x ^= x >> 32;
  return static_cast<uint32_t>(x);
}

// One float chain's operands as doubles; every one of them is exact in fp32 too.
struct ValuFloatOps {
  double x0, a, b;
};
inline ValuFloatOps valu_float_ops(int lane, int chain, int half) {
  const uint32_t h = valu_hash(lane, chain, 1 + half);
  const double one_minus_a = (16 + (h & 15)) / 1024.0;
  const double t = 0.75 + ((h >> 4) & 1023) / 2048.0;
  return {1.0 + ((h >> 14) & 4095) / 4096.0, 1.0 - one_minus_a, one_minus_a * t};
}

struct ValuIntOps {
  uint64_t x0, b;
  uint32_t a;
};
inline ValuIntOps valu_int_ops(int lane, int chain) {
  const uint64_t h0 = valu_hash(lane, chain, 3), h1 = valu_hash(lane, chain, 4), h2 = valu_hash(lane, chain, 5);
  return {(h0 << 32) | h1, (h2 << 32) | h0, valu_hash(lane, chain, 6) | 1u};  // odd a: the low word never collapses to 0
}

// The value of one chain after `steps` steps; `lo` and `hi` (when given) widen to every intermediate seen.
inline double valu_expect_f64(int lane, int chain, long steps, double* lo = nullptr, double* hi = nullptr) {
  const ValuFloatOps o = valu_float_ops(lane, chain, 0);
  double x = o.x0;
  for (long s = 0; s < steps; ++s) {
    x = std::fma(x, o.a, o.b);
    if (lo && x < *lo) *lo = x;
    if (hi && x > *hi) *hi = x;
  }
  return x;
}
inline float valu_expect_f32(int lane, int chain, int half, long steps, float* lo = nullptr, float* hi = nullptr) {
  const ValuFloatOps o = valu_float_ops(lane, chain, half);
  const float a = static_cast<float>(o.a), b = static_cast<float>(o.b);
  float x = static_cast<float>(o.x0);
  for (long s = 0; s < steps; ++s) {
    x = std::fma(x, a, b);
    if (lo && x < *lo) *lo = x;
    if (hi && x > *hi) *hi = x;
  }
  return x;
}
inline uint64_t valu_expect_i32(int lane, int chain, long steps) {
  const ValuIntOps o = valu_int_ops(lane, chain);
  uint64_t x = o.x0;
  for (long s = 0; s < steps; ++s) x = static_cast<uint64_t>(static_cast<uint32_t>(x)) * o.a + o.b;
  return x;
}

// The tables the kernel reads, lane-major: 8 bytes per word for every kind (a double, a float2's two floats, a u64).
// ops: [lane][chain][x0, a, b] (i32: a in the low word); expect: [lane][chain].
inline void valu_tables(int kind, long steps, uint64_t* ops, uint64_t* expect) {
  auto bits64 = [](double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u; };
  auto bits32 = [](float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return static_cast<uint64_t>(u); };
  for (int l = 0; l < VALU_LANES; ++l)
    for (int c = 0; c < VALU_CHAINS; ++c) {
      uint64_t* o = ops + 3 * (l * VALU_CHAINS + c);
      uint64_t& e = expect[l * VALU_CHAINS + c];
      if (kind == 0) {
        const ValuFloatOps f = valu_float_ops(l, c, 0);
        o[0] = bits64(f.x0), o[1] = bits64(f.a), o[2] = bits64(f.b);
        e = bits64(valu_expect_f64(l, c, steps));
      } else if (kind == 1) {
        const ValuFloatOps f0 = valu_float_ops(l, c, 0), f1 = valu_float_ops(l, c, 1);
        o[0] = bits32(static_cast<float>(f0.x0)) | bits32(static_cast<float>(f1.x0)) << 32;
        o[1] = bits32(static_cast<float>(f0.a)) | bits32(static_cast<float>(f1.a)) << 32;
        o[2] = bits32(static_cast<float>(f0.b)) | bits32(static_cast<float>(f1.b)) << 32;
        e = bits32(valu_expect_f32(l, c, 0, steps)) | bits32(valu_expect_f32(l, c, 1, steps)) << 32;
      } else {
        const ValuIntOps i = valu_int_ops(l, c);
        o[0] = i.x0, o[1] = i.a, o[2] = i.b;
        e = valu_expect_i32(l, c, steps);
      }
    }
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_VALU_REF_H_
