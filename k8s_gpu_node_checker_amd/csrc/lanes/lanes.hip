// libmi355x_lanes.so: the lanes diagnostic (HIP, gfx950).
//
// Every other compute diagnostic keeps each lane's data in its own lane.  This one tests the hardware that moves a
// value from one lane of a wave to another: the DPP operand network of each SIMD, the gfx950 half exchanges
// v_permlane16_swap / v_permlane32_swap, the LDS crossbar used without memory (ds_bpermute, ds_permute, ds_swizzle)
// and the VGPR <-> SGPR lane port (v_readlane, v_readfirstlane).  ops/lanes.py is its Python side;
// ops/diag.run(extra=("lanes",)) runs it next to a level's own tests.
//
// One template instantiation per op of lanes_ref.h, one native instruction each.  Every lane runs LANES_CHAINS
// independent chains of  y = ~x; (x', y') = op(x, y); x = mix32((x << 32 | fold(x', y')) + c[lane][chain]),  so each
// step's input depends on the previous crossing and a wrong lane propagates.  All waves run the same chains; the 64 x 4 words a
// wave must end with come from the host's model of the op (lanes_expected() of lanes_ref.h), and every lane compares
// bit for bit.  No LDS allocation, no scratch: lanes_test refuses to run a build that has either.
//
// Wrong lanes are located to their SIMD as the register-file test's are: the SIMD map row is simd_row() of
// common/hip_host.h.  The Report a launch leaves, the report() that ends the kernel and the host's Run are those of
// common/simd_report.h.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "lanes_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int BLOCKS_PER_CU = 4;        // the default grid
constexpr int MAX_ITERS = 1 << 20;
constexpr int LANES_APPLY_BPERMUTE_Y = LANES_OPS;  // lanes_apply only: ds_bpermute with y_in as the address register

struct Pair {
  uint32_t x, y;
};

// One application of op OP: the instruction itself, on this lane's x and y.  `addr` is the ds_(b)permute address
// register (4 * lanes_perm_index(), loaded once per kernel), `it` the step (wave-uniform).
template <int OP>
__device__ __forceinline__ Pair cross(uint32_t x, uint32_t y, uint32_t it, uint32_t lane, uint32_t addr) {
  if constexpr (lanes_is_dpp(OP)) {
    constexpr LanesDpp d = lanes_dpp(OP);
    x = __builtin_amdgcn_update_dpp(y, x, d.ctrl, d.row_mask, d.bank_mask, d.bound_ctrl);
  } else if constexpr (lanes_is_swizzle(OP)) {
    x = __builtin_amdgcn_ds_swizzle(x, lanes_swizzle_offset(OP));
  } else if constexpr ((OP >= LANES_BPERM_XOR32 && OP <= LANES_BPERM_GATHER) || OP == LANES_APPLY_BPERMUTE_Y) {
    x = __builtin_amdgcn_ds_bpermute(addr, x);
  } else if constexpr (OP == LANES_PERM_ROT17 || OP == LANES_PERM_SEEDED) {
    x = __builtin_amdgcn_ds_permute(addr, x);
  } else if constexpr (OP == LANES_PERMLANE32_SWAP) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);  // the builtin: the compiler pads the hazard
    x = r[0], y = r[1];
  } else if constexpr (OP == LANES_PERMLANE16_SWAP) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    x = r[0], y = r[1];
  } else if constexpr (OP == LANES_READLANE) {
    x = __builtin_amdgcn_readlane(x, lanes_readlane_index(it));
  } else {
    static_assert(OP == LANES_READFIRSTLANE, "an op without an instruction");
    if (lane >= static_cast<uint32_t>(lanes_readfirstlane_floor(it))) x = __builtin_amdgcn_readfirstlane(x);
  }
  return {x, y};
}

// (skip_block, skip_iter): the self-check's crossing that did not happen, on wave 0 of that workgroup at that step
// (-1: none); flip_block: one bit of lane 0's final chain-0 word of that workgroup's wave 0 is flipped (-1: none).
template <int OP>
__global__ void __launch_bounds__(THREADS) lanes_kernel(const uint32_t* __restrict__ expect, uint64_t seed, int iters,
                                                        int flip_block, int skip_block, int skip_iter, Report* rep,
                                                        unsigned long long* simd_map) {
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int skip_at = wave == 0 && static_cast<int>(blockIdx.x) == skip_block ? skip_iter : -1;  // wave-uniform
  const uint32_t addr = 4u * static_cast<uint32_t>(lanes_perm_index(OP, static_cast<int>(lane)));
  uint32_t x[LANES_CHAINS], c[LANES_CHAINS];
#pragma unroll
  for (int ch = 0; ch < LANES_CHAINS; ++ch) {
    x[ch] = lanes_init(seed, static_cast<int>(lane), ch);
    c[ch] = lanes_const(seed, static_cast<int>(lane), ch);
  }
  for (int it = 0; it < iters; ++it) {
    if (it != skip_at) {
#pragma unroll
      for (int ch = 0; ch < LANES_CHAINS; ++ch) {
        const Pair p = cross<OP>(x[ch], ~x[ch], static_cast<uint32_t>(it), lane, addr);
        x[ch] = lanes_step(OP, x[ch], p.x, p.y, c[ch]);
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < LANES_CHAINS; ++ch) x[ch] = lanes_step(-1, x[ch], x[ch], 0, c[ch]);
    }
  }
  if (static_cast<int>(blockIdx.x) == flip_block && threadIdx.x == 0) x[0] ^= 0x10u;
  int bad_chain = -1;
  uint32_t got = 0, want = 0;
#pragma unroll
  for (int ch = LANES_CHAINS - 1; ch >= 0; --ch) {  // ends at the first wrong chain
    const uint32_t w = expect[lane * LANES_CHAINS + ch];
    if (x[ch] != w) bad_chain = ch, got = x[ch], want = w;
  }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  // a wrong lane counts once; its record's `where`: SIMD map row << 16 | lane << 8 | its first wrong chain
  const unsigned long long where =
      (static_cast<unsigned long long>(row) << 16) | (lane << 8) | static_cast<unsigned>(bad_chain);
  report(rep, simd_map, row, bad_chain >= 0 ? 1u : 0u, where, 0, got, want, dt);
}

// one wave, one application, returned raw: io[0..63] x, io[64..127] y, in place
template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(uint32_t* io, uint32_t it) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t addr = OP == LANES_APPLY_BPERMUTE_Y ? io[64 + lane]
                                                     : 4u * static_cast<uint32_t>(lanes_perm_index(OP, static_cast<int>(lane)));
  const Pair p = cross<OP>(io[lane], io[64 + lane], it, lane, addr);
  io[lane] = p.x;
  io[64 + lane] = p.y;
}

struct Launch {
  const uint32_t* expect;
  uint64_t seed;
  int iters, flip_block, skip_block, skip_iter;
  Report* rep;
  unsigned long long* map;
  unsigned blocks;
};

template <int OP>
void launch_op(const Launch& l) {
  hipLaunchKernelGGL(lanes_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.expect, l.seed, l.iters, l.flip_block,
                     l.skip_block, l.skip_iter, l.rep, l.map);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(lanes_kernel<OP>));
}
template <int OP>
void launch_apply(uint32_t* io, uint32_t it) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, io, it);
}

// the tables from op index to instantiation
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const Launch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(uint32_t*, uint32_t) = {launch_apply<OP>..., launch_apply<LANES_APPLY_BPERMUTE_Y>};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, LANES_OPS>()));

}  // namespace

extern "C" {

const char* lanes_last_error(void) { return g_err.c_str(); }

int lanes_device_count(void) { return device_count(); }

int lanes_slots(void) { return SIMD_ROWS; }  // rows of lanes_test's simd_map

// Every op whose bit is set in `op_mask` (bit k: LanesOp k of lanes_ref.h), one after the other, on `blocks`
// workgroups of 4 waves (0: 4 per CU), `iters` steps of 4 chains per lane: a checked warm-up launch, then `reps`
// timed and checked launches.  Per op k: errors[k] = wrong lanes over all its launches; first_where[k] = SIMD map
// row << 16 | lane << 8 | chain of one wrong lane of the first launch that had any (~0: none), got[k] / want[k] that
// chain's word and the model's; ms[k] the mean time of a timed launch.  simd_map: lanes_slots() x 3 (waves run, wrong lanes,
// summed wall_clock64 ticks) per physical SIMD (simd_row()), added up over every launch of every op.
//
// Refused with -2 and a message: a bad device, blocks < 0, iters outside 1..2^20, reps < 1, an empty mask or unknown
// op, a hook outside the mask or the grid; with -3: a kernel built with a scratch segment or an LDS allocation (it
// would test memory, not the crossing).
//
// Self-check hooks, off by default (inject_op -1), both acting in the warm-up launch of op `inject_op`, on wave 0 of
// workgroup `inject_block`:
//   flip  (inject_skip_iter < 0): one bit of lane 0's final chain-0 word is flipped before the compare: 1 wrong lane,
//         got = want ^ 0x10
//   skip  (inject_skip_iter >= 0): the wave leaves the crossing out of that one step (the op's outputs are its
//         inputs): a crossing that did not happen; wrong lanes > 0
int lanes_test(int device, int blocks, int iters, int reps, unsigned long long op_mask, uint64_t seed, int inject_op,
               int inject_block, int inject_skip_iter, unsigned long long* errors, unsigned long long* first_where,
               unsigned long long* got, unsigned long long* want, double* ms, unsigned long long* simd_map,
               int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || iters < 1 || iters > MAX_ITERS || reps < 1 || !op_mask ||
      (LANES_OPS < 64 && (op_mask >> LANES_OPS))) {
    g_err = "lanes test: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a mask of known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (inject_op >= 0 && (inject_op >= LANES_OPS || !((op_mask >> inject_op) & 1ULL) ||
                         !hook_in_range(inject_block, grid, inject_skip_iter, iters))) {
    g_err = "lanes test: inject_op must be in the mask, inject_block inside the grid and inject_skip_iter below iters";
    return -2;
  }
  for (int k = 0; k < LANES_OPS; ++k) {
    errors[k] = got[k] = want[k] = 0;
    first_where[k] = ~0ULL;
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  DevBuf dexp;
  HIP_CHECK(dexp.alloc(device, LANES_WAVE * LANES_CHAINS * sizeof(uint32_t)));
  std::vector<uint32_t> expect(LANES_WAVE * LANES_CHAINS);
  for (int k = 0; k < LANES_OPS; ++k) {
    if (!((op_mask >> k) & 1ULL)) continue;
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse_memory("lanes test", LANES_OP_TABLE[k].name, attr, ": it would test memory, not the crossing"))
      return rc;
    lanes_expected(k, seed, iters, -1, expect.data());
    HIP_CHECK(hipMemcpy(dexp.ptr, expect.data(), expect.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    unsigned long long rec[4] = {~0ULL, 0, 0, 0};
    const auto enqueue = [&](int r) {
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_iter);
      AllOps::launch[k]({static_cast<const uint32_t*>(dexp.ptr), lanes_op_seed(seed, k), iters, h.flip_block, h.skip_block,
                         h.skip_at, run.rep(), run.map(), grid});
    };
    if (const int rc = run.series(reps, enqueue, errors + k, rec, ms + k)) return rc;
    first_where[k] = rec[0], got[k] = rec[2], want[k] = rec[3];
  }
  return run.read_map(simd_map);
}

// One application of op `op` at step `iter` by one wave of `device`, returned raw: x_out / y_out = the two registers
// after the instruction on x_in / y_in (64 words each).  op == the number of ops (one past the table) is ds_bpermute
// with y_in as the address register, so a test can hold any lane map against the crossbar.
int lanes_apply(int device, int op, unsigned int iter, const uint32_t* x_in, const uint32_t* y_in, uint32_t* x_out,
                uint32_t* y_out) {
  const int n = device_count();
  if (device < 0 || device >= n || op < 0 || op > LANES_APPLY_BPERMUTE_Y) {
    g_err = "lanes apply: need a valid device and an op of the table (or one past it: ds_bpermute by y_in)";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  DevBuf io;
  HIP_CHECK(io.alloc(device, 2 * LANES_WAVE * sizeof(uint32_t)));
  uint32_t* p = static_cast<uint32_t*>(io.ptr);
  HIP_CHECK(hipMemcpy(p, x_in, LANES_WAVE * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(p + LANES_WAVE, y_in, LANES_WAVE * sizeof(uint32_t), hipMemcpyHostToDevice));
  AllOps::apply[op](p, iter);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(x_out, p, LANES_WAVE * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(y_out, p + LANES_WAVE, LANES_WAVE * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
