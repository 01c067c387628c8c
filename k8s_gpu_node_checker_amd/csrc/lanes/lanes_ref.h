// The lanes diagnostic's ops (lanes.hip) and what a correct wave must compute: a model of every lane-crossing
// instruction on a 64-lane wave, written from the ISA's definitions.  Plain C++ that the host compiler takes alone:
// lanes.hip includes it for its kernels (the op table, the constants, the hash) and its host side (the expected
// words), and tests/test_lanes_cpu.py compiles it with g++ into a stand-alone program.
//
// A crossing only moves bits, so one answer is correct and the host computes it.  Every op works on two registers of
// a wave, x and y (y = ~x in the chains: the DPP ops' `old`, the swaps' second register); lanes_apply() is one
// application.  A chain step is
//     y = ~x;  (x', y') = op(x, y);  x = lanes_mix32((x << 32 | lanes_fold(op, x', y')) + c[lane][chain])
// so every step's input depends on the previous crossing and a wrong lane propagates.  The lane's own word rides in
// the hash's upper half: under an op that broadcasts (quad_perm:[0,0,0,0], readlane, a gather) a lane would
// otherwise forget its own history at the next step, and a crossing that failed once would be forgotten with it.
#ifndef K8S_GPU_NODE_CHECKER_AMD_LANES_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_LANES_REF_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LANES_HD __host__ __device__ inline
#else
#define LANES_HD inline
#endif

constexpr int LANES_WAVE = 64;
constexpr int LANES_CHAINS = 4;  // independent chains per lane

enum LanesOp {
  // the DPP operand network (v_mov_b32_dpp through __builtin_amdgcn_update_dpp, old = y)
  LANES_DPP_QUAD_1032 = 0,
  LANES_DPP_QUAD_2301,
  LANES_DPP_QUAD_3210,
  LANES_DPP_QUAD_0000,
  LANES_DPP_ROW_SHL1,
  LANES_DPP_ROW_SHR1,
  LANES_DPP_ROW_SHR2,
  LANES_DPP_ROW_SHR3,
  LANES_DPP_ROW_SHR8,
  LANES_DPP_ROW_ROR1,
  LANES_DPP_ROW_ROR4,
  LANES_DPP_WAVE_SHL1,
  LANES_DPP_WAVE_SHR1,
  LANES_DPP_WAVE_ROL1,
  LANES_DPP_WAVE_ROR1,
  LANES_DPP_ROW_MIRROR,
  LANES_DPP_ROW_HALF_MIRROR,
  LANES_DPP_ROW_BCAST15,
  LANES_DPP_ROW_BCAST31,
  LANES_DPP_ROW_SHR1_BC,
  LANES_DPP_ROW_SHR1_MASKED,
  // the LDS crossbar without memory
  LANES_SWZ_XOR1,
  LANES_SWZ_XOR2,
  LANES_SWZ_XOR4,
  LANES_SWZ_XOR8,
  LANES_SWZ_XOR16,
  LANES_SWZ_REV32,
  LANES_SWZ_BCAST0,
  LANES_SWZ_QUAD_2031,
  LANES_BPERM_XOR32,
  LANES_BPERM_ROT1,
  LANES_BPERM_SEEDED,
  LANES_BPERM_GATHER,
  LANES_PERM_ROT17,
  LANES_PERM_SEEDED,
  // the gfx950 half exchanges
  LANES_PERMLANE32_SWAP,
  LANES_PERMLANE16_SWAP,
  // the VGPR <-> SGPR lane port
  LANES_READLANE,
  LANES_READFIRSTLANE,
  LANES_OPS,
};
static_assert(LANES_OPS <= 64, "an op mask is 64 bits");

struct LanesOpInfo {
  const char* name;
  const char* insn;
};
// name and instruction of op k (the index is the enum's)
inline constexpr LanesOpInfo LANES_OP_TABLE[LANES_OPS] = {
    {"dpp_quad_perm_1032", "v_mov_b32_dpp quad_perm:[1,0,3,2]"},
    {"dpp_quad_perm_2301", "v_mov_b32_dpp quad_perm:[2,3,0,1]"},
    {"dpp_quad_perm_3210", "v_mov_b32_dpp quad_perm:[3,2,1,0]"},
    {"dpp_quad_perm_0000", "v_mov_b32_dpp quad_perm:[0,0,0,0]"},
    {"dpp_row_shl1", "v_mov_b32_dpp row_shl:1"},
    {"dpp_row_shr1", "v_mov_b32_dpp row_shr:1"},
    {"dpp_row_shr2", "v_mov_b32_dpp row_shr:2"},
    {"dpp_row_shr3", "v_mov_b32_dpp row_shr:3"},
    {"dpp_row_shr8", "v_mov_b32_dpp row_shr:8"},
    {"dpp_row_ror1", "v_mov_b32_dpp row_ror:1"},
    {"dpp_row_ror4", "v_mov_b32_dpp row_ror:4"},
    {"dpp_wave_shl1", "v_mov_b32_dpp wave_shl:1"},
    {"dpp_wave_shr1", "v_mov_b32_dpp wave_shr:1"},
    {"dpp_wave_rol1", "v_mov_b32_dpp wave_rol:1"},
    {"dpp_wave_ror1", "v_mov_b32_dpp wave_ror:1"},
    {"dpp_row_mirror", "v_mov_b32_dpp row_mirror"},
    {"dpp_row_half_mirror", "v_mov_b32_dpp row_half_mirror"},
    {"dpp_row_bcast15", "v_mov_b32_dpp row_bcast:15 row_mask:0xa"},
    {"dpp_row_bcast31", "v_mov_b32_dpp row_bcast:31 row_mask:0xc"},
    {"dpp_row_shr1_bound_ctrl", "v_mov_b32_dpp row_shr:1 bound_ctrl:1"},
    {"dpp_row_shr1_masked", "v_mov_b32_dpp row_shr:1 row_mask:0x5 bank_mask:0xa"},
    {"swizzle_xor1", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 1"},
    {"swizzle_xor2", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 2"},
    {"swizzle_xor4", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 4"},
    {"swizzle_xor8", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 8"},
    {"swizzle_xor16", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 16"},
    {"swizzle_reverse32", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) xor 0x1f"},
    {"swizzle_bcast0", "ds_swizzle_b32 offset:swizzle(BITMASK_PERM) and 0"},
    {"swizzle_quad_2031", "ds_swizzle_b32 offset:swizzle(QUAD_PERM, 2, 0, 3, 1)"},
    {"bpermute_xor32", "ds_bpermute_b32"},
    {"bpermute_rot1", "ds_bpermute_b32"},
    {"bpermute_seeded", "ds_bpermute_b32"},
    {"bpermute_gather", "ds_bpermute_b32"},
    {"permute_rot17", "ds_permute_b32"},
    {"permute_seeded", "ds_permute_b32"},
    {"permlane32_swap", "v_permlane32_swap_b32"},
    {"permlane16_swap", "v_permlane16_swap_b32"},
    {"readlane", "v_readlane_b32"},
    {"readfirstlane", "v_readfirstlane_b32"},
};

// The 64 -> 32 bit hash of the chains: the project's mix32 (common/hip_host.h; murmur3's finalizer), here for both
// compilers.
LANES_HD uint32_t lanes_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// a lane's starting word and its per-step constant, distinct per (lane, chain) and moved by the seed
LANES_HD uint32_t lanes_init(uint64_t seed, int lane, int chain) {
  return lanes_mix32(seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(lane * LANES_CHAINS + chain + 1));
}
LANES_HD uint32_t lanes_const(uint64_t seed, int lane, int chain) {
  return lanes_mix32(seed + 0xD1B54A32D192ED03ULL * static_cast<uint64_t>(lane * LANES_CHAINS + chain + 1));
}
// the seed of op k's chains
LANES_HD uint64_t lanes_op_seed(uint64_t seed, int op) { return seed + 0x632BE59BD9B4E019ULL * static_cast<uint64_t>(op + 1); }

// --- DPP -------------------------------------------------------------------------------------------------------
// dpp_ctrl encodings (the GFX9 DPP_CTRL field): quad_perm 0x00-0xff (two bits per lane of the quad, lane 0 lowest),
// row_shl:n 0x100+n, row_shr:n 0x110+n, row_ror:n 0x120+n, wave_shl:1 0x130, wave_rol:1 0x134, wave_shr:1 0x138,
// wave_ror:1 0x13c, row_mirror 0x140, row_half_mirror 0x141, row_bcast:15 0x142, row_bcast:31 0x143.
struct LanesDpp {
  int ctrl, row_mask, bank_mask;
  bool bound_ctrl;
};
constexpr int lanes_quad(int a, int b, int c, int d) { return a | (b << 2) | (c << 4) | (d << 6); }
constexpr bool lanes_is_dpp(int op) { return op >= LANES_DPP_QUAD_1032 && op <= LANES_DPP_ROW_SHR1_MASKED; }
constexpr LanesDpp lanes_dpp(int op) {
  switch (op) {
    case LANES_DPP_QUAD_1032: return {lanes_quad(1, 0, 3, 2), 0xf, 0xf, false};
    case LANES_DPP_QUAD_2301: return {lanes_quad(2, 3, 0, 1), 0xf, 0xf, false};
    case LANES_DPP_QUAD_3210: return {lanes_quad(3, 2, 1, 0), 0xf, 0xf, false};
    case LANES_DPP_QUAD_0000: return {lanes_quad(0, 0, 0, 0), 0xf, 0xf, false};
    case LANES_DPP_ROW_SHL1: return {0x101, 0xf, 0xf, false};
    case LANES_DPP_ROW_SHR1: return {0x111, 0xf, 0xf, false};
    case LANES_DPP_ROW_SHR2: return {0x112, 0xf, 0xf, false};
    case LANES_DPP_ROW_SHR3: return {0x113, 0xf, 0xf, false};
    case LANES_DPP_ROW_SHR8: return {0x118, 0xf, 0xf, false};
    case LANES_DPP_ROW_ROR1: return {0x121, 0xf, 0xf, false};
    case LANES_DPP_ROW_ROR4: return {0x124, 0xf, 0xf, false};
    case LANES_DPP_WAVE_SHL1: return {0x130, 0xf, 0xf, false};
    case LANES_DPP_WAVE_SHR1: return {0x138, 0xf, 0xf, false};
    case LANES_DPP_WAVE_ROL1: return {0x134, 0xf, 0xf, false};
    case LANES_DPP_WAVE_ROR1: return {0x13c, 0xf, 0xf, false};
    case LANES_DPP_ROW_MIRROR: return {0x140, 0xf, 0xf, false};
    case LANES_DPP_ROW_HALF_MIRROR: return {0x141, 0xf, 0xf, false};
    case LANES_DPP_ROW_BCAST15: return {0x142, 0xa, 0xf, false};
    case LANES_DPP_ROW_BCAST31: return {0x143, 0xc, 0xf, false};
    case LANES_DPP_ROW_SHR1_BC: return {0x111, 0xf, 0xf, true};
    case LANES_DPP_ROW_SHR1_MASKED: return {0x111, 0x5, 0xa, false};
    default: return {0, 0, 0, false};
  }
}

// The lane that lane i reads under dpp_ctrl `ctrl`, -1 when the ISA calls the source out of range.  A row is 16
// lanes; r is i's place in its row.
constexpr int lanes_dpp_src(int ctrl, int i) {
  const int row = i & ~15, r = i & 15, n = ctrl & 15;
  // quad_perm:[a,b,c,d]: lane q of every group of four reads lane (a,b,c,d)[q] of the same group
  if (ctrl < 0x100) return (i & ~3) | ((ctrl >> (2 * (i & 3))) & 3);
  // row_shl:n: lane i takes lane i+n of its row; past the row's end there is no source
  if (ctrl >= 0x101 && ctrl <= 0x10f) return r + n <= 15 ? i + n : -1;
  // row_shr:n: lane i takes lane i-n of its row; before the row's start there is no source
  if (ctrl >= 0x111 && ctrl <= 0x11f) return r >= n ? i - n : -1;
  // row_ror:n: as row_shr, but the row wraps: lane i takes lane (i-n) mod 16 of its row
  if (ctrl >= 0x121 && ctrl <= 0x12f) return row | ((r - n) & 15);
  switch (ctrl) {
    case 0x130: return i + 1 <= 63 ? i + 1 : -1;  // wave_shl:1: lane i takes lane i+1 of the wave; lane 63 has none
    case 0x134: return (i + 1) & 63;              // wave_rol:1: the same, lane 63 takes lane 0
    case 0x138: return i >= 1 ? i - 1 : -1;       // wave_shr:1: lane i takes lane i-1 of the wave; lane 0 has none
    case 0x13c: return (i - 1) & 63;              // wave_ror:1: the same, lane 0 takes lane 63
    case 0x140: return row | (15 - r);            // row_mirror: the row reversed
    case 0x141: return (i & ~7) | (7 - (i & 7));  // row_half_mirror: each half row (8 lanes) reversed
    case 0x142: return i >= 16 ? row - 1 : -1;    // row_bcast:15: lane 15 of each row feeds every lane of the next row
    case 0x143: return i >= 32 ? 31 : -1;         // row_bcast:31: lane 31 feeds every lane of rows 2 and 3
    default: return -1;
  }
}

// Whether lane i is written at all: bit (i / 16) of row_mask and bit ((i / 4) % 4) of bank_mask (a bank is four
// consecutive lanes of a row) must both be set; a disabled lane keeps `old`.
constexpr bool lanes_dpp_enabled(const LanesDpp& d, int i) {
  return ((d.row_mask >> (i >> 4)) & 1) && ((d.bank_mask >> ((i >> 2) & 3)) & 1);
}

// --- ds_swizzle ------------------------------------------------------------------------------------------------
// The 16-bit offset of a swizzle op.  Bit 15 clear is bitmask mode: and_mask = offset[4:0], or_mask = offset[9:5],
// xor_mask = offset[14:10]; bit 15 set is quad-perm mode with the four selects in offset[7:0], as DPP's quad_perm.
constexpr int lanes_swz_bitmask(int and_mask, int or_mask, int xor_mask) { return and_mask | (or_mask << 5) | (xor_mask << 10); }
constexpr int lanes_swizzle_offset(int op) {
  switch (op) {
    case LANES_SWZ_XOR1: return lanes_swz_bitmask(0x1f, 0, 1);
    case LANES_SWZ_XOR2: return lanes_swz_bitmask(0x1f, 0, 2);
    case LANES_SWZ_XOR4: return lanes_swz_bitmask(0x1f, 0, 4);
    case LANES_SWZ_XOR8: return lanes_swz_bitmask(0x1f, 0, 8);
    case LANES_SWZ_XOR16: return lanes_swz_bitmask(0x1f, 0, 16);
    case LANES_SWZ_REV32: return lanes_swz_bitmask(0x1f, 0, 0x1f);
    case LANES_SWZ_BCAST0: return lanes_swz_bitmask(0, 0, 0);
    case LANES_SWZ_QUAD_2031: return 0x8000 | lanes_quad(2, 0, 3, 1);
    default: return -1;
  }
}
constexpr bool lanes_is_swizzle(int op) { return op >= LANES_SWZ_XOR1 && op <= LANES_SWZ_QUAD_2031; }
// the lane that lane i reads under swizzle offset `off` (every lane of the wave is active, so every source is valid)
constexpr int lanes_swizzle_src(int off, int i) {
  // quad-perm mode: lane q of every group of four reads lane sel[q] of the same group
  if (off & 0x8000) return (i & ~3) | ((off >> (2 * (i & 3))) & 3);
  // bitmask mode works inside groups of 32 lanes: with j = i % 32, the source is ((j & and) | or) ^ xor of the group
  const int j = i & 31;
  return (i & 32) | ((((j & (off & 0x1f)) | ((off >> 5) & 0x1f)) ^ ((off >> 10) & 0x1f)) & 31);
}

// --- ds_bpermute / ds_permute ----------------------------------------------------------------------------------
constexpr uint64_t LANES_PERM_SEED = 0x1A9E5C0DEULL;  // of the two seeded maps and the gather (fixed: not the test's seed)
// a bijection of 0..63 from hash word h: an affine map with an odd multiplier, then an invertible xor-shift
LANES_HD int lanes_bijection(uint32_t h, int i) {
  const int t = (i * static_cast<int>(2 * (h & 31u) + 1) + static_cast<int>((h >> 5) & 63u)) & 63;
  return t ^ (t >> 3);
}
// The lane index op `op` gives lane i: for ds_bpermute the lane i reads, for ds_permute the lane i writes.
// The instruction's address register holds 4 * index.
LANES_HD int lanes_perm_index(int op, int i) {
  switch (op) {
    case LANES_BPERM_XOR32: return i ^ 32;
    case LANES_BPERM_ROT1: return (i + 1) & 63;
    case LANES_BPERM_SEEDED: return lanes_bijection(lanes_mix32(LANES_PERM_SEED), i);
    case LANES_BPERM_GATHER: return static_cast<int>(lanes_mix32(LANES_PERM_SEED + 64 + static_cast<uint64_t>(i)) & 63u);  // not injective
    case LANES_PERM_ROT17: return (i + 17) & 63;
    case LANES_PERM_SEEDED: return lanes_bijection(lanes_mix32(LANES_PERM_SEED + 1), i);
    default: return i;
  }
}

// --- the lane port ---------------------------------------------------------------------------------------------
LANES_HD int lanes_readlane_index(uint32_t iter) { return static_cast<int>((7u * iter + 3u) & 63u); }
LANES_HD int lanes_readfirstlane_floor(uint32_t iter) { return static_cast<int>(iter & 63u); }

// whether the op leaves two registers that a chain folds (the swaps): x' + rotl(y', 16), else x' alone
constexpr bool lanes_two_outputs(int op) { return op == LANES_PERMLANE32_SWAP || op == LANES_PERMLANE16_SWAP; }
LANES_HD uint32_t lanes_fold(int op, uint32_t x, uint32_t y) {
  return lanes_two_outputs(op) ? x + ((y << 16) | (y >> 16)) : x;
}
// the chain step's new word: `own` the lane's word before the op, (x, y) the op's outputs, c the lane's constant
LANES_HD uint32_t lanes_step(int op, uint32_t own, uint32_t x, uint32_t y, uint32_t c) {
  return lanes_mix32(((static_cast<uint64_t>(own) << 32) | lanes_fold(op, x, y)) + c);
}

// One application of op `op` at step `iter` by one wave, in place: x and y are the two registers' 64 lanes.
inline void lanes_apply(int op, uint32_t iter, uint32_t x[LANES_WAVE], uint32_t y[LANES_WAVE]) {
  uint32_t xi[LANES_WAVE], yi[LANES_WAVE];
  for (int i = 0; i < LANES_WAVE; ++i) xi[i] = x[i], yi[i] = y[i];
  if (lanes_is_dpp(op)) {
    // v_mov_b32_dpp vdst, src with vdst preloaded with `old` (= y): an enabled lane with a source in range takes the
    // source lane's src; an enabled lane whose source is out of range keeps old, or takes 0 under bound_ctrl; a
    // lane disabled by row_mask or bank_mask keeps old whatever its source.
    const LanesDpp d = lanes_dpp(op);
    for (int i = 0; i < LANES_WAVE; ++i) {
      const int s = lanes_dpp_src(d.ctrl, i);
      if (!lanes_dpp_enabled(d, i))
        x[i] = yi[i];
      else if (s >= 0)
        x[i] = xi[s];
      else
        x[i] = d.bound_ctrl ? 0u : yi[i];
    }
  } else if (lanes_is_swizzle(op)) {
    // ds_swizzle_b32: every lane reads the lane its offset's pattern names (lanes_swizzle_src)
    const int off = lanes_swizzle_offset(op);
    for (int i = 0; i < LANES_WAVE; ++i) x[i] = xi[lanes_swizzle_src(off, i)];
  } else if (op >= LANES_BPERM_XOR32 && op <= LANES_BPERM_GATHER) {
    // ds_bpermute_b32 (a gather): lane i reads the lane whose index is bits 7:2 of lane i's address
    for (int i = 0; i < LANES_WAVE; ++i) x[i] = xi[((4u * static_cast<uint32_t>(lanes_perm_index(op, i))) >> 2) & 63u];
  } else if (op == LANES_PERM_ROT17 || op == LANES_PERM_SEEDED) {
    // ds_permute_b32 (a scatter): lane i writes the lane whose index is bits 7:2 of lane i's address.  Both maps are
    // bijections, so every lane is written exactly once and no collision is decided.
    for (int i = 0; i < LANES_WAVE; ++i) x[lanes_perm_index(op, i)] = xi[i];
  } else if (op == LANES_PERMLANE32_SWAP) {
    // v_permlane32_swap_b32 vdst (x), src (y): vdst[32..63] and src[0..31] change places; the other halves stay
    for (int i = 0; i < 32; ++i) x[i + 32] = yi[i], y[i] = xi[i + 32];
  } else if (op == LANES_PERMLANE16_SWAP) {
    // v_permlane16_swap_b32 vdst (x), src (y): the odd rows of vdst change places with the even rows of src:
    // vdst row 1 <-> src row 0, vdst row 3 <-> src row 2
    for (int i = 0; i < 16; ++i) {
      x[16 + i] = yi[i], y[i] = xi[16 + i];
      x[48 + i] = yi[32 + i], y[32 + i] = xi[48 + i];
    }
  } else if (op == LANES_READLANE) {
    // v_readlane_b32 with a wave-uniform index: every lane receives that lane's word
    for (int i = 0; i < LANES_WAVE; ++i) x[i] = xi[lanes_readlane_index(iter)];
  } else if (op == LANES_READFIRSTLANE) {
    // v_readfirstlane_b32 under `if (lane >= t)`: the first active lane is t, so the lanes from t up receive lane
    // t's word and the lanes below it, inactive, keep theirs
    const int t = lanes_readfirstlane_floor(iter);
    for (int i = t; i < LANES_WAVE; ++i) x[i] = xi[t];
  }
}

// The words every wave must end with: out[lane * LANES_CHAINS + chain] after `iters` steps of op `op`'s chains under
// `seed` (the test's seed: lanes_op_seed() is applied here).  skip_iter >= 0 leaves the crossing out of that one
// step (the op's outputs are its inputs): what a crossing that did not happen leaves behind.
inline void lanes_expected(int op, uint64_t seed, int iters, int skip_iter, uint32_t out[LANES_WAVE * LANES_CHAINS]) {
  const uint64_t s = lanes_op_seed(seed, op);
  uint32_t x[LANES_CHAINS][LANES_WAVE], y[LANES_WAVE], own[LANES_WAVE];
  for (int c = 0; c < LANES_CHAINS; ++c)
    for (int i = 0; i < LANES_WAVE; ++i) x[c][i] = lanes_init(s, i, c);
  for (int it = 0; it < iters; ++it) {
    for (int c = 0; c < LANES_CHAINS; ++c) {
      for (int i = 0; i < LANES_WAVE; ++i) own[i] = x[c][i], y[i] = ~x[c][i];
      if (it != skip_iter) lanes_apply(op, static_cast<uint32_t>(it), x[c], y);
      for (int i = 0; i < LANES_WAVE; ++i)
        x[c][i] = it != skip_iter ? lanes_step(op, own[i], x[c][i], y[i], lanes_const(s, i, c))
                                  : lanes_step(-1, own[i], own[i], 0, lanes_const(s, i, c));
    }
  }
  for (int i = 0; i < LANES_WAVE; ++i)
    for (int c = 0; c < LANES_CHAINS; ++c) out[i * LANES_CHAINS + c] = x[c][i];
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_LANES_REF_H_
