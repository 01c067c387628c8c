// The ifetch diagnostic's constants (ifetch.hip) and what a correct wave must compute: the literal constants of
// every basic block of the walk, a block, a wave's path through the blocks, and the model of every branch op.  Plain
// C++ that the host compiler takes alone: ifetch.hip includes it for its kernels (the constants are literals of the
// instruction stream) and its host side (the expected words), and tests/test_ifetch_cpu.py compiles it with g++ into
// a stand-alone program.
//
// Executing code only computes, so one answer is correct and the host computes it.
//
// walk.  IFETCH_NB basic blocks of IFETCH_ST steps on a per-lane word x; step s of block b is
//     x = ((x rotl ifetch_rot(b, s)) ^ ifetch_xor(b, s)) + ifetch_add(b, s)
// and a block ends with the wave-uniform walker word  p = ifetch_pmix(p ^ ifetch_pk(b)).  The next block is p % nb,
// so the path depends on every block that ran.  A wave's path and its lanes' first words depend on the seed and on
// path = wave_in_grid % IFETCH_PATHS only: the model is IFETCH_PATHS paths by IFETCH_WAVE lanes.
//
// branch.  Every op is one select: taken, the word gets  w + ifetch_branch_lit_t(op);  not taken,
// w ^ ifetch_branch_lit_n(op).  A chain step is  x = ifetch_mix32((x << 32 | op(x, cond(x))) + c[chain]).
#ifndef K8S_GPU_NODE_CHECKER_AMD_IFETCH_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_IFETCH_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IFETCH_HD __host__ __device__ inline
#else
#define IFETCH_HD inline
#endif

constexpr uint32_t IFETCH_NB = 1024;    // basic blocks of the walk kernel
constexpr uint32_t IFETCH_ST = 16;      // steps of a block: a rotate, an xor with a literal, an add of a literal
constexpr int IFETCH_WAVE = 64;
constexpr int IFETCH_PATHS = 64;        // distinct paths of a launch: wave_in_grid % IFETCH_PATHS
constexpr int IFETCH_CHAINS = 4;        // scalar chains of a branch op
constexpr int IFETCH_TABLE_WORDS = IFETCH_PATHS * IFETCH_WAVE + IFETCH_PATHS;  // every final x, then every final p
// a step holds two 32-bit literals, each in an 8-byte instruction: the least a block can span
constexpr uint32_t IFETCH_BLOCK_MIN_BYTES = IFETCH_ST * 8;
constexpr uint32_t IFETCH_FLOOR_BYTES = 256 * 1024;  // the least the NB blocks must span
constexpr int IFETCH_DEFAULT_STEPS = 512;            // 64 paths x 512 steps: 32 draws per block of 1,024

// the 64 -> 32 bit hash (murmur3's finalizer)
IFETCH_HD constexpr uint32_t ifetch_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// Every constant of the instruction stream: row `block` (the branch ops take the rows from IFETCH_NB on), column j.
IFETCH_HD constexpr uint32_t ifetch_k(uint32_t block, uint32_t j) {
  return ifetch_mix32((static_cast<uint64_t>(block + 1) << 32) | (j + 1));
}
// ... as a literal that no inline constant can encode: positive, odd, >= 2^23 (the small integers, the inline floats
// 0.5, 1, 2, 4 and 1 / 2 pi are all excluded), so it takes its own dword after the instruction
IFETCH_HD constexpr uint32_t ifetch_lit(uint32_t block, uint32_t j) {
  return (ifetch_k(block, j) & 0x7fffffffu) | 0x00800001u;
}
IFETCH_HD constexpr uint32_t ifetch_rot(uint32_t block, uint32_t step) { return 1u + ifetch_k(block, 3 * step) % 31u; }
IFETCH_HD constexpr uint32_t ifetch_xor(uint32_t block, uint32_t step) { return ifetch_lit(block, 3 * step + 1); }
IFETCH_HD constexpr uint32_t ifetch_add(uint32_t block, uint32_t step) { return ifetch_lit(block, 3 * step + 2); }
IFETCH_HD constexpr uint32_t ifetch_pk(uint32_t block) { return ifetch_lit(block, 3 * IFETCH_ST); }

IFETCH_HD constexpr uint32_t ifetch_rotl(uint32_t x, uint32_t r) { return (x << r) | (x >> (32u - r)); }  // r in 1..31

IFETCH_HD constexpr uint32_t ifetch_step(uint32_t block, uint32_t step, uint32_t x) {
  return (ifetch_rotl(x, ifetch_rot(block, step)) ^ ifetch_xor(block, step)) + ifetch_add(block, step);
}
IFETCH_HD constexpr uint32_t ifetch_pmix(uint32_t v) {
  v *= 0x9E3779B1u;
  v ^= v >> 15;
  v *= 0x85EBCA6Bu;
  v ^= v >> 13;
  return v;
}
// one block on one lane's word, and on the walker
IFETCH_HD constexpr uint32_t ifetch_block_x(uint32_t block, uint32_t x) {
  for (uint32_t s = 0; s < IFETCH_ST; ++s) x = ifetch_step(block, s, x);
  return x;
}
IFETCH_HD constexpr uint32_t ifetch_block_p(uint32_t block, uint32_t p) { return ifetch_pmix(p ^ ifetch_pk(block)); }

// where a wave starts
IFETCH_HD constexpr uint32_t ifetch_p0(uint64_t seed, uint32_t path) {
  return ifetch_mix32(seed * 0x9E3779B97F4A7C15ULL + 0x1F37ULL + path);
}
IFETCH_HD constexpr uint32_t ifetch_x0(uint64_t seed, uint32_t path, uint32_t lane) {
  return ifetch_mix32((seed ^ 0x5851F42D4C957F2DULL) * 0xD6E8FEB86659FD93ULL + (static_cast<uint64_t>(path) << 8) + lane);
}

// One path: `steps` blocks from (seed, path) over blocks [0, nb), on all 64 lanes.  skip_step >= 0: the block of
// that step is left out (the walker stays, so the next step runs it: the self-check's block that was not executed).
// visited (IFETCH_NB bytes, may be null): set to 1 for every block run.
inline void ifetch_walk(uint64_t seed, uint32_t path, int steps, uint32_t nb, int skip_step, uint32_t* x, uint32_t* p_out,
                        uint8_t* visited) {
  uint32_t p = ifetch_p0(seed, path);
  for (int l = 0; l < IFETCH_WAVE; ++l) x[l] = ifetch_x0(seed, path, static_cast<uint32_t>(l));
  for (int s = 0; s < steps; ++s) {
    if (s == skip_step) continue;
    const uint32_t b = p % nb;
    if (visited) visited[b] = 1;
    for (uint32_t t = 0; t < IFETCH_ST; ++t) {  // the constants once per step, not once per lane
      const uint32_t r = ifetch_rot(b, t), kx = ifetch_xor(b, t), ka = ifetch_add(b, t);
      for (int l = 0; l < IFETCH_WAVE; ++l) x[l] = (ifetch_rotl(x[l], r) ^ kx) + ka;
    }
    p = ifetch_block_p(b, p);
  }
  *p_out = p;
}

// The table every workgroup compares against: table[path * 64 + lane] the final x, table[64 * 64 + path] the final
// p.  Returns the number of distinct blocks of [0, nb) the 64 paths ran.
inline int ifetch_expected(uint64_t seed, int steps, uint32_t nb, uint32_t* table) {
  uint8_t visited[IFETCH_NB] = {};
  for (int q = 0; q < IFETCH_PATHS; ++q)
    ifetch_walk(seed, static_cast<uint32_t>(q), steps, nb, -1, table + q * IFETCH_WAVE,
                table + IFETCH_PATHS * IFETCH_WAVE + q, visited);
  int n = 0;
  for (uint32_t b = 0; b < nb; ++b) n += visited[b];
  return n;
}

// --- branch ----------------------------------------------------------------------------------------------------
enum IfetchBranchOp {
  IFETCH_S_BRANCH = 0,
  IFETCH_S_CBRANCH_SCC0,
  IFETCH_S_CBRANCH_SCC1,
  IFETCH_S_CBRANCH_VCCZ,
  IFETCH_S_CBRANCH_VCCNZ,
  IFETCH_S_CBRANCH_EXECZ,
  IFETCH_S_CBRANCH_EXECNZ,
  IFETCH_S_SETPC_B64,
  IFETCH_S_SWAPPC_B64,
  IFETCH_S_CALL_B64,
  IFETCH_BRANCH_OPS,
};

struct IfetchBranchInfo {
  const char* name;  // the instruction itself
  const char* what;
};
// op k (the index is the enum's).  `cond` is what the op looks at: SCC, VCC != 0, EXEC != 0; for the unconditional
// ops, whether the wave reaches the jump to the taken arm (s_branch, s_call_b64) or which of the two computed
// targets it jumps to (s_setpc_b64, s_swappc_b64).
inline constexpr IfetchBranchInfo IFETCH_BRANCH_TABLE[IFETCH_BRANCH_OPS] = {
    {"s_branch", "reached when cond"},
    {"s_cbranch_scc0", "taken when SCC = cond is 0"},
    {"s_cbranch_scc1", "taken when SCC = cond is 1"},
    {"s_cbranch_vccz", "taken when VCC (one bit set when cond) is 0"},
    {"s_cbranch_vccnz", "taken when VCC (one bit set when cond) is not 0"},
    {"s_cbranch_execz", "taken when EXEC (narrowed to one lane when cond, else to none) is 0"},
    {"s_cbranch_execnz", "taken when EXEC (narrowed to one lane when cond, else to none) is not 0"},
    {"s_setpc_b64", "a computed target: the taken arm when cond"},
    {"s_swappc_b64", "a computed target and a return: the taken arm when cond"},
    {"s_call_b64", "a relative call and a return, reached when cond"},
};

IFETCH_HD constexpr bool ifetch_branch_taken(int op, uint32_t cond) {
  const bool on_zero = op == IFETCH_S_CBRANCH_SCC0 || op == IFETCH_S_CBRANCH_VCCZ || op == IFETCH_S_CBRANCH_EXECZ;
  return on_zero ? cond == 0 : cond != 0;
}
IFETCH_HD constexpr uint32_t ifetch_branch_lit_t(int op) { return ifetch_lit(IFETCH_NB + static_cast<uint32_t>(op), 0); }
IFETCH_HD constexpr uint32_t ifetch_branch_lit_n(int op) { return ifetch_lit(IFETCH_NB + static_cast<uint32_t>(op), 1); }
// one application: a select
IFETCH_HD constexpr uint32_t ifetch_branch_apply(int op, uint32_t w, uint32_t cond) {
  return ifetch_branch_taken(op, cond) ? w + ifetch_branch_lit_t(op) : w ^ ifetch_branch_lit_n(op);
}
// the condition of a step comes from the chain's word, and so does the one bit that VCC / EXEC keep when it holds
IFETCH_HD constexpr uint32_t ifetch_branch_cond(uint32_t x) { return (x >> 13) & 1u; }
IFETCH_HD constexpr uint64_t ifetch_branch_mask(uint32_t x, uint32_t cond) { return cond ? 1ULL << ((x >> 2) & 63u) : 0ULL; }

IFETCH_HD constexpr uint64_t ifetch_op_seed(uint64_t seed, int op) { return seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(op + 1); }
IFETCH_HD constexpr uint32_t ifetch_chain_init(uint64_t seed, int chain) { return ifetch_mix32(seed * 4 + static_cast<uint64_t>(chain)); }
IFETCH_HD constexpr uint32_t ifetch_chain_const(uint64_t seed, int chain) {
  return ifetch_mix32((seed ^ 0xC0DEC0DEULL) * 4 + static_cast<uint64_t>(chain)) | 1u;
}
IFETCH_HD constexpr uint32_t ifetch_chain_step(uint32_t x, uint32_t r, uint32_t c) {
  return ifetch_mix32(((static_cast<uint64_t>(x) << 32) | r) + c);
}

// The IFETCH_CHAINS words every wave must end with after `iters` steps of op `op` under `seed` (already the op's
// own: ifetch_op_seed()).  skip_iter >= 0: the branch of that step did not happen (neither arm ran).
inline void ifetch_branch_expected(int op, uint64_t seed, int iters, int skip_iter, uint32_t* out) {
  for (int ch = 0; ch < IFETCH_CHAINS; ++ch) {
    uint32_t x = ifetch_chain_init(seed, ch);
    const uint32_t c = ifetch_chain_const(seed, ch);
    for (int it = 0; it < iters; ++it)
      x = ifetch_chain_step(x, it == skip_iter ? x : ifetch_branch_apply(op, x, ifetch_branch_cond(x)), c);
    out[ch] = x;
  }
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_IFETCH_REF_H_
