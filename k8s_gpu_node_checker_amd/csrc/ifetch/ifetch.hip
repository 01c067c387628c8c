// libmi355x_ifetch.so: the ifetch diagnostic (HIP, gfx950).
//
// Every other diagnostic runs a few hundred bytes to a few KiB of code in a tight loop: it is fetched once and then
// served from the instruction buffer or a handful of I-cache lines.  This one tests the front end of a CU, in two
// parts:
//   walk    one kernel of IFETCH_NB straight-line basic blocks (ifetch_ref.h), each IFETCH_ST steps of a rotate, an
//           xor with a 32-bit literal and an add of a 32-bit literal on a per-lane word x, ended by an update of the
//           wave-uniform walker word p; the next block is p % nb, reached through a compile-time binary tree of
//           scalar compare-branches.  All constants are literals of the instruction stream, so a wrongly fetched
//           dword changes x or p, and a wrongly resolved branch derails the rest of the walk.  `nb` is a launch
//           argument: one kernel serves every code footprint from a few KiB to all of it, which is larger than the
//           instruction cache.  A wave's path depends on the seed and wave_in_grid % 64 only, so every workgroup
//           compares against one table of 64 x 64 final words (and 64 final walker words), fetched with vector loads.
//   branch  the branch unit, one native instruction per op of IFETCH_BRANCH_TABLE in one asm statement: both arms
//           inside the statement, the taken one applying one literal operation and the other one another.  Every wave
//           runs IFETCH_CHAINS scalar chains whose every step's condition comes from the previous word.  Targets are
//           assembler-local labels only; the computed ones are s_getpc_b64 plus a label difference.
// Under a wave-uniform flag every block of the walk kernel records its own address (s_getpc_b64), so the host knows
// the code span of blocks [0, nb) from the kernel as loaded, and refuses a build whose blocks were merged or shrunk.
// No LDS allocation, no scratch: every entry point refuses to run a build that has either.  ops/ifetch.py is its
// Python side; ops/diag.run(extra=("ifetch",)) runs it next to a level's own tests.
//
// Wrong words are located to the SIMD that executed (simd_row() of common/hip_host.h).  The instruction cache is
// shared between CUs and the project has no map of which CUs share one: a wrong word names the CU that executed,
// not the cache that served it.  The Report, report() and Run are those of common/simd_report.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "ifetch_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int BLOCKS_PER_CU = 4;  // the default grid
constexpr int MAX_STEPS = 1 << 16;
constexpr int MAX_ITERS = 1 << 20;
constexpr int RAW_WORDS = IFETCH_WAVE + 1;  // a raw application: 64 x, then p

// --- walk ------------------------------------------------------------------------------------------------------
template <uint32_t B, uint32_t S>
__device__ __forceinline__ uint32_t step_of(uint32_t x) {
  constexpr uint32_t r = ifetch_rot(B, S), kx = ifetch_xor(B, S), ka = ifetch_add(B, S);  // literals
  return (__builtin_rotateleft32(x, r) ^ kx) + ka;
}
template <uint32_t B, uint32_t... S>
__device__ __forceinline__ uint32_t steps_of(uint32_t x, std::integer_sequence<uint32_t, S...>) {
  ((x = step_of<B, S>(x)), ...);
  return x;
}

// Block B.  slot (wave-uniform; null in every launch but the map's): the block records its own address there.  The
// caller passes the map's entry of the block it dispatches to: an address that each block computed for itself
// would be hoisted out of the walk, IFETCH_NB of them.
template <uint32_t B>
__device__ __forceinline__ void block(uint32_t& x, uint32_t& p, unsigned long long* slot) {
  if (slot) {
    uint64_t pc;
    asm volatile("s_getpc_b64 %0" : "=s"(pc));
    if ((threadIdx.x & 63u) == 0) *slot = pc;  // a vector store from lane 0
  }
  x = steps_of<B>(x, std::make_integer_sequence<uint32_t, IFETCH_ST>());
  constexpr uint32_t k = ifetch_pk(B);
  p = ifetch_pmix(p ^ k);
}

// the way to block b: `if (b < mid)` over templates, log2(NB) scalar compare-branches
template <uint32_t LO, uint32_t N>
__device__ __forceinline__ void dispatch(uint32_t b, uint32_t& x, uint32_t& p, unsigned long long* slot) {
  if constexpr (N == 1) {
    block<LO>(x, p, slot);
  } else {
    if (b < LO + N / 2) dispatch<LO, N / 2>(b, x, p, slot);
    else dispatch<LO + N / 2, N - N / 2>(b, x, p, slot);
  }
}

// The one kernel that holds the blocks; dispatch() is instantiated once.
//   the walk (list == null): every wave runs `steps` blocks of [0, nb) from (seed, wave_in_grid % 64) and compares
//     every lane's x, and on lane 0 p, with expect[].  (skip_block, skip_step): wave 0 of that workgroup leaves the
//     block of that step out (-1: none); flip_block: one bit of lane 0's final x of that workgroup's wave 0 is
//     flipped (-1: none).
//   raw applications (list != null): wave w runs block list[i], i = w, w + waves, ..., once each, every time from
//     raw_in (64 x, then p), and stores what it leaves to raw_out[65 i ..]; no compare.  With pcs the blocks record
//     their addresses: the map launch.
__global__ void __launch_bounds__(THREADS) walk_kernel(const uint32_t* __restrict__ expect, const int* __restrict__ list,
                                                       int nlist, const uint32_t* __restrict__ raw_in, uint32_t* raw_out,
                                                       unsigned long long* pcs, uint64_t seed, int steps, uint32_t nb,
                                                       int flip_block, int skip_block, int skip_step, Report* rep,
                                                       unsigned long long* simd_map) {
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wave_in_grid = blockIdx.x * (THREADS / 64) + wave, waves = gridDim.x * (THREADS / 64);
  const uint32_t path = wave_in_grid % IFETCH_PATHS;
  const bool hooked_wave = wave == 0;
  const int skip_at = hooked_wave && static_cast<int>(blockIdx.x) == skip_block ? skip_step : -1;  // wave-uniform
  uint32_t x = ifetch_x0(seed, path, lane), p = ifetch_p0(seed, path);
  for (int s = 0; s < steps; ++s) {
    uint32_t b, i = 0;
    if (list) {
      i = wave_in_grid + static_cast<uint32_t>(s) * waves;
      if (i >= static_cast<uint32_t>(nlist)) break;
      b = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(list[i]));
      x = raw_in[lane];
      p = raw_in[IFETCH_WAVE];
    } else {
      b = __builtin_amdgcn_readfirstlane(p) % nb;
    }
    p = __builtin_amdgcn_readfirstlane(p);  // the walker lives in SGPRs
    if (s != skip_at) dispatch<0, IFETCH_NB>(b, x, p, pcs ? pcs + b : nullptr);  // b < IFETCH_NB: the host checks a list
    if (list) {
      raw_out[RAW_WORDS * i + lane] = x;
      if (lane == 0) raw_out[RAW_WORDS * i + IFETCH_WAVE] = p;
    }
  }
  if (list) return;
  if (hooked_wave && static_cast<int>(blockIdx.x) == flip_block && lane == 0) x ^= 0x10u;
  const uint32_t want_x = expect[path * IFETCH_WAVE + lane];
  const uint32_t want_p = expect[IFETCH_PATHS * IFETCH_WAVE + path];
  const bool bad_x = x != want_x, bad_p = lane == 0 && p != want_p;
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  // a record's `where`: SIMD map row << 16 | lane << 8 | which word (0: x, 1: the walker p)
  const unsigned long long where = (static_cast<unsigned long long>(row) << 16) | (lane << 8) | (bad_x ? 0u : 1u);
  report(rep, simd_map, row, (bad_x ? 1u : 0u) + (bad_p ? 1u : 0u), where, path, bad_x ? x : p, bad_x ? want_x : want_p, dt);
}

// --- branch ----------------------------------------------------------------------------------------------------
// One application of op OP on the wave-uniform word w: the instruction, both arms and the merge point in one
// statement.  Labels: 1 the taken arm, 2 the other arm where it is a target, 3 the merge point, 0 what s_getpc_b64
// returns.  The computed targets live in the named pair s[40:41], return addresses in s[42:43].
#define BR_NOT_TAKEN "s_xor_b32 %[w], %[w], %[ln]\n"
#define BR_TAKEN "s_add_u32 %[w], %[w], %[lt]\n"
#define BR_ARMS BR_NOT_TAKEN "s_branch 3f\n1:\n" BR_TAKEN "3:\n"
// s[40:41] = the address of label 1 when cond, of label 2 otherwise
#define BR_TARGET                                                                                            \
  "s_getpc_b64 s[40:41]\n0:\ns_mov_b32 %[t], 2f-0b\ns_cmp_lg_u32 %[c], 0\ns_cmov_b32 %[t], 1f-0b\n"            \
  "s_add_u32 s40, s40, %[t]\ns_addc_u32 s41, s41, 0\n"
#define BR_OPERANDS(...)                                                                                     \
  : [w] "+s"(w), [t] "=&s"(t), [sv] "=&s"(sv)                                                                \
  : [c] "s"(cond), [m] "s"(mask), [lt] "n"(ifetch_branch_lit_t(OP)), [ln] "n"(ifetch_branch_lit_n(OP))       \
  : "scc", "vcc", "s40", "s41", "s42", "s43"

template <int OP>
__device__ __forceinline__ uint32_t branch(uint32_t w, uint32_t cond) {
  const uint64_t mask = ifetch_branch_mask(w, cond);  // what VCC keeps, and what EXEC is narrowed to
  uint32_t t;
  uint64_t sv;
  if constexpr (OP == IFETCH_S_BRANCH) {
    asm volatile("s_cmp_lg_u32 %[c], 0\ns_cbranch_scc0 2f\ns_branch 1f\n2:\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_SCC0) {
    asm volatile("s_cmp_lg_u32 %[c], 0\ns_cbranch_scc0 1f\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_SCC1) {
    asm volatile("s_cmp_lg_u32 %[c], 0\ns_cbranch_scc1 1f\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_VCCZ) {  // a write of all 64 bits: VCCZ follows it
    asm volatile("s_mov_b64 vcc, %[m]\ns_cbranch_vccz 1f\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_VCCNZ) {
    asm volatile("s_mov_b64 vcc, %[m]\ns_cbranch_vccnz 1f\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_EXECZ) {  // exec saved, narrowed and restored; the arms are scalar
    asm volatile("s_mov_b64 %[sv], exec\ns_and_b64 exec, %[sv], %[m]\ns_cbranch_execz 1f\n" BR_ARMS
                 "s_mov_b64 exec, %[sv]\n" BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_CBRANCH_EXECNZ) {
    asm volatile("s_mov_b64 %[sv], exec\ns_and_b64 exec, %[sv], %[m]\ns_cbranch_execnz 1f\n" BR_ARMS
                 "s_mov_b64 exec, %[sv]\n" BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_SETPC_B64) {
    asm volatile(BR_TARGET "s_setpc_b64 s[40:41]\n2:\n" BR_ARMS BR_OPERANDS());
  } else if constexpr (OP == IFETCH_S_SWAPPC_B64) {  // both arms return to the instruction after the swap
    asm volatile(BR_TARGET "s_swappc_b64 s[42:43], s[40:41]\ns_branch 3f\n2:\n" BR_NOT_TAKEN "s_setpc_b64 s[42:43]\n1:\n"
                 BR_TAKEN "s_setpc_b64 s[42:43]\n3:\n" BR_OPERANDS());
  } else {
    static_assert(OP == IFETCH_S_CALL_B64, "an op without an instruction");
    asm volatile("s_cmp_lg_u32 %[c], 0\ns_cbranch_scc0 2f\ns_call_b64 s[42:43], 1f\ns_branch 3f\n2:\n" BR_NOT_TAKEN
                 "s_branch 3f\n1:\n" BR_TAKEN "s_setpc_b64 s[42:43]\n3:\n" BR_OPERANDS());
  }
  (void)t, (void)sv;
  return w;
}

// (skip_block, skip_iter): the self-check's branch that did not happen, on wave 0 of that workgroup at that step
// (-1: none); flip_block: one bit of the final chain-0 word of that workgroup's wave 0 is flipped (-1: none).
// expect: this op's IFETCH_CHAINS words.
template <int OP>
__global__ void __launch_bounds__(THREADS) branch_kernel(const uint32_t* expect, uint64_t seed, int iters, int flip_block,
                                                         int skip_block, int skip_iter, Report* rep,
                                                         unsigned long long* simd_map) {
  static_assert(IFETCH_CHAINS == 4, "lanes 0..3 compare one chain each");
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const bool hooked_wave = wave == 0;
  const int skip_at = hooked_wave && static_cast<int>(blockIdx.x) == skip_block ? skip_iter : -1;  // wave-uniform
  uint32_t x[IFETCH_CHAINS], c[IFETCH_CHAINS];
#pragma unroll
  for (int ch = 0; ch < IFETCH_CHAINS; ++ch) {
    x[ch] = ifetch_chain_init(seed, ch);
    c[ch] = ifetch_chain_const(seed, ch);
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int ch = 0; ch < IFETCH_CHAINS; ++ch) {
      const uint32_t w = __builtin_amdgcn_readfirstlane(x[ch]);
      x[ch] = ifetch_chain_step(w, it != skip_at ? branch<OP>(w, ifetch_branch_cond(w)) : w, c[ch]);
    }
  }
  if (hooked_wave && static_cast<int>(blockIdx.x) == flip_block) x[0] ^= 0x10u;
  // lane ch < 4 holds chain ch's word against the expected one, which it loads itself: a vector load
  const uint32_t ch = lane & 3u;
  const uint32_t want = expect[ch];
  const uint32_t got = ch == 0 ? x[0] : ch == 1 ? x[1] : ch == 2 ? x[2] : x[3];
  const unsigned long long wrong = __ballot(lane < IFETCH_CHAINS && got != want);
  const unsigned first = wrong ? static_cast<unsigned>(__ffsll(static_cast<long long>(wrong)) - 1) : 0u;
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  const uint32_t first_got = __builtin_amdgcn_readlane(got, static_cast<int>(first));
  const uint32_t first_want = __builtin_amdgcn_readlane(want, static_cast<int>(first));
  // a count of the wave's, so lane 0 alone reports; `where`: SIMD map row << 16 | chain
  if (lane == 0)
    report(rep, simd_map, row, __popcll(wrong), (static_cast<unsigned long long>(row) << 16) | first, 0, first_got,
           first_want, dt);
}

// one wave, `n` applications one after the other, returned raw: in[2 i ..] = w, cond -> out[i]
template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(const uint32_t* in, uint32_t* out, int n) {
  for (int i = 0; i < n; ++i) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(in[2 * i]), cond = __builtin_amdgcn_readfirstlane(in[2 * i + 1]);
    const uint32_t r = branch<OP>(w, cond);
    if (threadIdx.x == 0) out[i] = r;
  }
}

struct BranchLaunch {
  const uint32_t* expect;
  uint64_t seed;
  int iters, flip_block, skip_block, skip_iter;
  Report* rep;
  unsigned long long* map;
  unsigned blocks;
};

template <int OP>
void launch_op(const BranchLaunch& l) {
  hipLaunchKernelGGL(branch_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.expect, l.seed, l.iters, l.flip_block,
                     l.skip_block, l.skip_iter, l.rep, l.map);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(branch_kernel<OP>));
}
template <int OP>
void launch_apply(const uint32_t* in, uint32_t* out, int n) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, in, out, n);
}

// the tables from op index to instantiation
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const BranchLaunch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(const uint32_t*, uint32_t*, int) = {launch_apply<OP>...};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, IFETCH_BRANCH_OPS>()));

// --- host ------------------------------------------------------------------------------------------------------
int refuse(const char* who, const hipFuncAttributes& attr, const std::string& what) {
  return refuse_memory(who, what, attr, ": it would test memory, not the front end");
}

int walk_attributes(const char* who) {
  hipFuncAttributes attr;
  HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(walk_kernel)));
  return refuse(who, attr, "the walk");
}

// `n` raw applications (list[i] < IFETCH_NB, checked by the caller) from `in` (64 x, then p) by a few waves of
// `device` (current); out: 65 words each.  pcs (device memory, IFETCH_NB addresses, or null): the map launch.
int run_raw(int device, const std::vector<int>& list, const uint32_t* in, uint32_t* out, unsigned long long* pcs) {
  const size_t n = list.size();
  DevBuf dlist, din, dout;
  HIP_CHECK(dlist.alloc(device, n * sizeof(int)));
  HIP_CHECK(din.alloc(device, RAW_WORDS * sizeof(uint32_t)));
  HIP_CHECK(dout.alloc(device, n * RAW_WORDS * sizeof(uint32_t)));
  HIP_CHECK(hipMemcpy(dlist.ptr, list.data(), n * sizeof(int), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(din.ptr, in, RAW_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
  const unsigned grid = pcs ? 1u : 2u;  // a few waves share the list; the map is one workgroup's
  const int steps = static_cast<int>((n + grid * (THREADS / 64) - 1) / (grid * (THREADS / 64)));
  hipLaunchKernelGGL(walk_kernel, dim3(grid), dim3(THREADS), 0, nullptr, nullptr, static_cast<const int*>(dlist.ptr),
                     static_cast<int>(n), static_cast<const uint32_t*>(din.ptr), static_cast<uint32_t*>(dout.ptr), pcs,
                     0ULL, steps, 1u, -1, -1, -1, nullptr, nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out, dout.ptr, n * RAW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

// The map launch on `device` (current): every block once, each recording its address.  What the blocks computed on
// the way is held against the model, so the map is that of blocks that work.
int read_block_map(int device, std::vector<unsigned long long>& addrs) {
  addrs.assign(IFETCH_NB, 0ULL);
  DevBuf dpcs;
  HIP_CHECK(dpcs.alloc(device, IFETCH_NB * sizeof(unsigned long long)));
  HIP_CHECK(hipMemset(dpcs.ptr, 0, IFETCH_NB * sizeof(unsigned long long)));
  std::vector<int> list(IFETCH_NB);
  for (uint32_t b = 0; b < IFETCH_NB; ++b) list[b] = static_cast<int>(b);
  uint32_t in[RAW_WORDS];
  for (int l = 0; l < IFETCH_WAVE; ++l) in[l] = ifetch_x0(0, 0, static_cast<uint32_t>(l));
  in[IFETCH_WAVE] = ifetch_p0(0, 0);
  std::vector<uint32_t> out(static_cast<size_t>(IFETCH_NB) * RAW_WORDS);
  if (const int rc = run_raw(device, list, in, out.data(), static_cast<unsigned long long*>(dpcs.ptr))) return rc;
  HIP_CHECK(hipMemcpy(addrs.data(), dpcs.ptr, IFETCH_NB * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

// The code span in bytes of blocks [0, nb) for every nb (span[nb - 1]), from the map: a block reaches from its
// address to the next recorded address above it (the last block of the kernel: as far as the shortest other block).
// -3 with a message when two blocks share an address, two lie closer together than a block's literal instructions,
// or all of them span less than the floor.
int spans_of(const std::vector<unsigned long long>& addrs, std::vector<unsigned long long>& span) {
  std::vector<std::pair<unsigned long long, uint32_t>> order(IFETCH_NB);
  for (uint32_t b = 0; b < IFETCH_NB; ++b) order[b] = {addrs[b], b};
  std::sort(order.begin(), order.end());
  unsigned long long least = ~0ULL;
  for (uint32_t k = 1; k < IFETCH_NB; ++k) {
    const unsigned long long gap = order[k].first - order[k - 1].first;
    if (gap < IFETCH_BLOCK_MIN_BYTES) {
      g_err = "ifetch walk: the map shows blocks " + std::to_string(order[k - 1].second) + " and " +
              std::to_string(order[k].second) + " " + std::to_string(gap) + " bytes apart, less than the " +
              std::to_string(IFETCH_BLOCK_MIN_BYTES) + " bytes of a block's literal instructions: the compiler merged or shrank them";
      return -3;
    }
    least = std::min(least, gap);
  }
  std::vector<unsigned long long> end(IFETCH_NB);
  for (uint32_t k = 0; k < IFETCH_NB; ++k)
    end[order[k].second] = k + 1 < IFETCH_NB ? order[k + 1].first : order[k].first + least;
  span.assign(IFETCH_NB, 0ULL);
  unsigned long long lo = ~0ULL, hi = 0;
  for (uint32_t b = 0; b < IFETCH_NB; ++b) {
    lo = std::min(lo, addrs[b]);
    hi = std::max(hi, end[b]);
    span[b] = hi - lo;
  }
  if (span[IFETCH_NB - 1] < IFETCH_FLOOR_BYTES) {
    g_err = "ifetch walk: the map shows all " + std::to_string(IFETCH_NB) + " blocks in " + std::to_string(span[IFETCH_NB - 1]) +
            " bytes of code, under the floor of " + std::to_string(IFETCH_FLOOR_BYTES);
    return -3;
  }
  return 0;
}

}  // namespace

extern "C" {

const char* ifetch_last_error(void) { return g_err.c_str(); }

int ifetch_device_count(void) { return device_count(); }

int ifetch_slots(void) { return SIMD_ROWS; }  // rows of every simd_map below

int ifetch_blocks(void) { return static_cast<int>(IFETCH_NB); }  // blocks of the walk kernel: the length of a map

// The address every block of the walk kernel recorded for itself on `device` (s_getpc_b64 inside the block):
// addrs[IFETCH_NB].  Returned as read; ifetch_walk_test judges it.
int ifetch_block_map(int device, unsigned long long* addrs) {
  const int n = device_count();
  if (device < 0 || device >= n) {
    g_err = "ifetch block_map: need a valid device";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  if (const int rc = walk_attributes("ifetch block_map")) return rc;
  std::vector<unsigned long long> map;
  if (const int rc = read_block_map(device, map)) return rc;
  std::copy(map.begin(), map.end(), addrs);
  return 0;
}

// The walk.  For every footprint nbs[0..nrows) (blocks [0, nb) of the kernel, 1..IFETCH_NB), one after the other, on
// `blocks` workgroups of 4 waves (0: 4 per CU): a checked warm-up launch, then `reps` timed and checked launches of
// `steps` blocks per wave.  Per row k: errors[k] = wrong words over all its launches (a lane's x; on lane 0 also
// the walker p); first[4 k ..] = where (SIMD map row << 16 | lane << 8 | 0: x, 1: p; ~0: none), the path, got, want
// of one wrong word of the first launch that had any; ms[k] the mean time of a timed launch; footprint[k] the code
// span of the row's blocks in bytes, from the map launch that precedes the rows; visited[k] the distinct blocks the
// model's 64 paths run.  simd_map: ifetch_slots() x 3 (waves run, wrong words, summed wall_clock64 ticks) per
// physical SIMD, added up over every launch of every row.
//
// Refused with -2 and a message: a bad device, blocks < 0, steps outside 1..2^16, reps < 1, no row or an nb outside
// 1..IFETCH_NB, a hook outside the rows, the grid or the steps, and a (seed, steps, nb) whose 64 paths leave a block
// of [0, nb) unvisited; with -3: a kernel built with a scratch segment or an LDS allocation, and a map that shows
// two blocks at one address or closer together than a block's literal instructions, or all blocks in less than
// IFETCH_FLOOR_BYTES.
//
// Self-check hooks, off by default (inject_row -1), both acting in the warm-up launch of row `inject_row`, on wave 0
// of workgroup `inject_block`:
//   flip  (inject_skip_step < 0): one bit of lane 0's final x is flipped before the compare: 1 wrong word,
//         got = want ^ 0x10
//   skip  (inject_skip_step >= 0): the wave leaves the block of that one step out; wrong words > 0
int ifetch_walk_test(int device, int blocks, int steps, int reps, const int* nbs, int nrows, uint64_t seed, int inject_row,
                     int inject_block, int inject_skip_step, unsigned long long* errors, unsigned long long* first,
                     double* ms, unsigned long long* footprint, int* visited, unsigned long long* simd_map,
                     int* blocks_run) {
  const int n = device_count();
  bool known = nbs != nullptr && nrows >= 1 && nrows <= 64;
  for (int k = 0; known && k < nrows; ++k) known = nbs[k] >= 1 && nbs[k] <= static_cast<int>(IFETCH_NB);
  if (device < 0 || device >= n || blocks < 0 || steps < 1 || steps > MAX_STEPS || reps < 1 || !known) {
    g_err = "ifetch walk: need a valid device, blocks >= 0 (0: 4 per CU), steps 1..2^16, reps >= 1 and 1..64 rows of nb 1.." +
            std::to_string(IFETCH_NB);
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (inject_row >= 0 && (inject_row >= nrows || !hook_in_range(inject_block, grid, inject_skip_step, steps))) {
    g_err = "ifetch walk: inject_row must be one of the rows, inject_block inside the grid and inject_skip_step below steps";
    return -2;
  }
  for (int k = 0; k < nrows; ++k) {
    errors[k] = footprint[k] = 0;
    no_record(first + 4 * k);
    ms[k] = 0.0;
    visited[k] = 0;
  }
  // the model first: a walk that cannot cover its blocks is refused before anything is launched
  std::vector<std::vector<uint32_t>> tables(nrows, std::vector<uint32_t>(IFETCH_TABLE_WORDS));
  for (int k = 0; k < nrows; ++k) {
    visited[k] = ifetch_expected(seed, steps, static_cast<uint32_t>(nbs[k]), tables[k].data());
    if (visited[k] != nbs[k]) {
      g_err = "ifetch walk: the 64 paths of seed " + std::to_string(seed) + " visit " + std::to_string(visited[k]) + " of " +
              std::to_string(nbs[k]) + " blocks in " + std::to_string(steps) + " steps: more steps or another seed";
      return -2;
    }
  }
  if (const int rc = walk_attributes("ifetch walk")) return rc;
  std::vector<unsigned long long> addrs, span;
  if (const int rc = read_block_map(device, addrs)) return rc;
  if (const int rc = spans_of(addrs, span)) return rc;
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf dexp;
  HIP_CHECK(dexp.alloc(device, IFETCH_TABLE_WORDS * sizeof(uint32_t)));
  for (int k = 0; k < nrows; ++k) {
    footprint[k] = span[nbs[k] - 1];
    HIP_CHECK(hipMemcpy(dexp.ptr, tables[k].data(), IFETCH_TABLE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_row, inject_block, inject_skip_step);
      hipLaunchKernelGGL(walk_kernel, dim3(grid), dim3(THREADS), 0, nullptr, static_cast<const uint32_t*>(dexp.ptr),
                         nullptr, 0, nullptr, nullptr, nullptr, seed, steps, static_cast<uint32_t>(nbs[k]), h.flip_block,
                         h.skip_block, h.skip_at, run.rep(), run.map());
    };
    if (const int rc = run.series(reps, enqueue, errors + k, first + 4 * k, ms + k)) return rc;
  }
  return run.read_map(simd_map);
}

// The branch unit.  Every op of `ops[0..nops)` (IfetchBranchOp of ifetch_ref.h), one after the other, on `blocks`
// workgroups of 4 waves (0: 4 per CU), `iters` steps of 4 chains per wave: a checked warm-up launch, then `reps`
// timed and checked launches.  Per op k (arrays of the table's length): errors[k] = wrong wave-words over all its
// launches; first[4 k ..] = where (SIMD map row << 16 | chain; ~0: none), 0, got, want of one wrong word of the
// first launch that had any; ms[k] the mean time of a timed launch.  simd_map as ifetch_walk_test's.
//
// Refused with -2 and a message: a bad device, blocks < 0, iters outside 1..2^20, reps < 1, no op or an unknown one,
// a hook outside the list or the grid; with -3: a kernel built with a scratch segment or an LDS allocation.
//
// Self-check hooks, off by default (inject_op -1), both acting in the warm-up launch of op `inject_op`, on wave 0 of
// workgroup `inject_block`:
//   flip  (inject_skip_iter < 0): one bit of the final chain-0 word is flipped before the compare: 1 wrong word,
//         got = want ^ 0x10
//   skip  (inject_skip_iter >= 0): the wave leaves the branch out of that one step (neither arm runs); wrong words > 0
int ifetch_branch_test(int device, int blocks, int iters, int reps, const int* ops, int nops, uint64_t seed, int inject_op,
                       int inject_block, int inject_skip_iter, unsigned long long* errors, unsigned long long* first,
                       double* ms, unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || iters < 1 || iters > MAX_ITERS || reps < 1 ||
      !op_list_known(ops, nops, IFETCH_BRANCH_OPS, false)) {
    g_err = "ifetch branch: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a list of known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (!op_list_has_hook(ops, nops, inject_op) || (inject_op >= 0 && !hook_in_range(inject_block, grid, inject_skip_iter, iters))) {
    g_err = "ifetch branch: inject_op must be in the list, inject_block inside the grid and inject_skip_iter below iters";
    return -2;
  }
  for (int k = 0; k < IFETCH_BRANCH_OPS; ++k) {
    errors[k] = 0;
    no_record(first + 4 * k);
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf dexp;
  HIP_CHECK(dexp.alloc(device, IFETCH_CHAINS * sizeof(uint32_t)));
  uint32_t expect[IFETCH_CHAINS];
  for (int i = 0; i < nops; ++i) {
    const int k = ops[i];
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse("ifetch branch", attr, IFETCH_BRANCH_TABLE[k].name)) return rc;
    ifetch_branch_expected(k, ifetch_op_seed(seed, k), iters, -1, expect);
    HIP_CHECK(hipMemcpy(dexp.ptr, expect, sizeof expect, hipMemcpyHostToDevice));
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};  // of this series: an op listed twice reports its last one's
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_iter);
      AllOps::launch[k]({static_cast<const uint32_t*>(dexp.ptr), ifetch_op_seed(seed, k), iters, h.flip_block, h.skip_block,
                         h.skip_at, run.rep(), run.map(), grid});
    };
    if (const int rc = run.series(reps, enqueue, errors + k, rec, ms + k)) return rc;
    for (int j = 0; j < 4; ++j) first[4 * k + j] = rec[j];
  }
  return run.read_map(simd_map);
}

// Each block of `blocks[0..n)` (0..IFETCH_NB-1, n up to 2^16) run once by one wave of `device` from x[64] and p,
// returned raw: x_out[64 i ..] the lanes' words and p_out[i] the walker after block blocks[i].
int ifetch_apply_blocks(int device, const int* blocks, int n, const uint32_t* x, uint32_t p, uint32_t* x_out,
                        uint32_t* p_out) {
  const int ndev = device_count();
  bool known = blocks != nullptr && n >= 1 && n <= MAX_STEPS;
  for (int i = 0; known && i < n; ++i) known = blocks[i] >= 0 && blocks[i] < static_cast<int>(IFETCH_NB);
  if (device < 0 || device >= ndev || !known) {
    g_err = "ifetch apply_blocks: need a valid device and 1..2^16 blocks of 0.." + std::to_string(IFETCH_NB - 1);
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  if (const int rc = walk_attributes("ifetch apply_blocks")) return rc;
  uint32_t in[RAW_WORDS];
  std::copy(x, x + IFETCH_WAVE, in);
  in[IFETCH_WAVE] = p;
  std::vector<uint32_t> out(static_cast<size_t>(n) * RAW_WORDS);
  if (const int rc = run_raw(device, std::vector<int>(blocks, blocks + n), in, out.data(), nullptr)) return rc;
  for (int i = 0; i < n; ++i) {
    std::copy(out.begin() + static_cast<size_t>(i) * RAW_WORDS, out.begin() + static_cast<size_t>(i) * RAW_WORDS + IFETCH_WAVE,
              x_out + static_cast<size_t>(i) * IFETCH_WAVE);
    p_out[i] = out[static_cast<size_t>(i) * RAW_WORDS + IFETCH_WAVE];
  }
  return 0;
}

// `n` applications of branch op `op` by one wave of `device`, one after the other, returned raw: out[i] the word
// after the statement on w[i] under cond[i] (0 or 1).
int ifetch_apply(int device, int op, int n, const uint32_t* w, const uint32_t* cond, uint32_t* out) {
  const int ndev = device_count();
  bool flags = n >= 1 && n <= MAX_ITERS;
  for (int i = 0; flags && i < n; ++i) flags = cond[i] <= 1;
  if (device < 0 || device >= ndev || op < 0 || op >= IFETCH_BRANCH_OPS || !flags) {
    g_err = "ifetch apply: need a valid device, an op of the table, 1..2^20 rows and cond 0 or 1";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  std::vector<uint32_t> in(2 * static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) in[2 * i] = w[i], in[2 * i + 1] = cond[i];
  DevBuf din, dout;
  HIP_CHECK(din.alloc(device, in.size() * sizeof(uint32_t)));
  HIP_CHECK(dout.alloc(device, static_cast<size_t>(n) * sizeof(uint32_t)));
  HIP_CHECK(hipMemcpy(din.ptr, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  AllOps::apply[op](static_cast<const uint32_t*>(din.ptr), static_cast<uint32_t*>(dout.ptr), n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out, dout.ptr, static_cast<size_t>(n) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
