// libmi355x_vmem.so: the vector-memory diagnostic (HIP, gfx950).
//
// Every byte a kernel reads or writes goes through the vector memory path of its CU: the address adders, the texture
// addresser's range check, the 32 KiB vector L1, the byte enables of the store path.  The other diagnostics load and
// store with 16-byte global accesses only.  This one has four parts, reported in one result:
//   loads   every load form as one native instruction (VMEM_LOAD_LIST of vmem_ref.h: global, saddr with immediates,
//           the sc0 / sc1 / nt policies, flat, buffer with offen / idxen / soffset), one template instantiation per op,
//           an asm statement that holds the instruction and its own s_waitcnt.  Every lane runs VMEM_CHAINS chains
//           over a 64 KiB table; every step's address depends on the previous step's data.  All waves run the same
//           chains; the host's model of one wave (vmem_expected()) supplies the final words.
//   stores  every store form the same way (VMEM_STORE_LIST): a lane stores into its own 64-byte cell of its wave's
//           region, waits, reloads the 16 bytes the store began in with global_load_dwordx4 sc1 and folds them into the
//           chain.  After the walk every wave's whole region, a guard cell on either side included, is compared with
//           the model's image of one wave -- by a plain kernel on the device: copying every region to the host
//           after every launch would cost more than the whole test.
//   bounds  the buffer descriptor's range check: a raw and a structured descriptor whose num_records covers the first
//           half of a buffer; a rejected load must return 0, a rejected store must be dropped (the host checks all
//           bytes).  Every address formed lies inside the buffer: a leak reads or writes our own bytes.
//   l1      the vector L1 of every CU: co-resident workgroups walk a small slice each, again and again, every word
//           compared in registers; timed a second time with sc1 loads, which bypass the L1.  Nothing proves that a
//           read was served by the L1: the test reads data that should be held there, and reports both times.
//           ldsdma: the LDS-DMA forms (global_load_lds_dword / x4, buffer_load_dword / x4 ... lds), read back from
//           the LDS by other lanes.
// Results leave the waves through vector stores and vector atomics only: the Report, report() and the host's Run of
// common/simd_report.h, on the SIMD map rows of simd_row() (common/hip_host.h).  Only the LDS-DMA kernel has an LDS
// allocation, no kernel has scratch: every entry point refuses a build that differs (-3).  ops/vmem.py is its Python
// side; ops/diag.run(extra=("vmem",)) runs it next to a level's own tests.
//
// Left out: see the head of vmem_ref.h (typed buffer formats, misaligned accesses, straddling accesses, an soffset
// that crosses num_records, the LDS-DMA sub-dword forms), and what was removed after the device disagreed with the
// model (the D16 loads, the LDS-DMA dwordx3 forms).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../common/hip_host.h"
#include "../common/op_list.h"
#include "../common/simd_report.h"
#include "vmem_ref.h"

namespace {

constexpr unsigned THREADS = 256;
constexpr int BLOCKS_PER_CU = 2;       // the default grid of every part
constexpr int MAX_ITERS = 1 << 16;
constexpr int MAX_BLOCKS = 8192;       // the store regions of the largest grid: 138 MB
constexpr int DMA_FORMS = 4;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// a record's `where`: SIMD map row << 32 | lane << 8 | chain  (walks; the lane alone elsewhere; 0xffff: no lane)
__device__ __forceinline__ unsigned long long where_of(unsigned row, unsigned low) {
  return (static_cast<unsigned long long>(row) << 32) | low;
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the buffer descriptor of `bytes`-long memory at `base`: stride 0 (raw, num_records in bytes) or a stride with
// num_records in elements; every word wave-uniform, word 3 the gfx9 raw-buffer word
__device__ __forceinline__ u32x4 descriptor(const void* base, uint32_t stride, uint32_t num_records) {
  const uint64_t b = reinterpret_cast<uint64_t>(base);
  return {uniform(static_cast<uint32_t>(b)), uniform((static_cast<uint32_t>(b >> 32) & 0xffffu) | (stride << 16)),
          uniform(num_records), uniform(0x00020000u)};
}

// --- one access ---------------------------------------------------------------------------------------------------
// What an op gets: the wave-uniform base, the raw and the structured descriptor over the same memory, the byte
// offset `off` the lane accesses (the op splits it over its own address parts) and the wave-uniform soffset.
struct Addr {
  const uint8_t* base;
  u32x4 raw, strided;
  uint32_t off, soff;
};

template <int N>
struct Regs {
  typedef uint32_t type __attribute__((ext_vector_type(N)));
};
template <>
struct Regs<1> {
  typedef uint32_t type;
};
template <int N>
__device__ __forceinline__ typename Regs<N>::type pack(u32x4 v) {
  if constexpr (N == 1) return v.x;
  else if constexpr (N == 2) return u32x2{v.x, v.y};
  else if constexpr (N == 3) return u32x3{v.x, v.y, v.z};
  else return v;
}
__device__ __forceinline__ u32x4 unpack(uint32_t d) { return {d, 0, 0, 0}; }
__device__ __forceinline__ u32x4 unpack(u32x2 d) { return {d.x, d.y, 0, 0}; }
__device__ __forceinline__ u32x4 unpack(u32x3 d) { return {d.x, d.y, d.z, 0}; }
__device__ __forceinline__ u32x4 unpack(u32x4 d) { return d; }

#define VM_STR_(x) #x
#define VM_STR(x) VM_STR_(x)
// Every statement opens with s_nop 4 (an SGPR operand may come fresh from v_readfirstlane) and ends with its own
// wait: the destination is valid, and a store has left the data registers, when the statement ends.
#define VM_HEAD "s_nop 4\n"
#define VM_WAIT "\ns_waitcnt vmcnt(0)"
#define VM_WAIT_FLAT "\ns_waitcnt vmcnt(0) lgkmcnt(0)"
// loads: the destination is read-write: a skipped load and a load see the same registers before it
#define VM_L_GLOBAL(M, MODS, IMM)                                                                             \
  const uint8_t* p = a.base + a.off;                                                                          \
  asm volatile(VM_HEAD M " %[d], %[p], off" MODS VM_WAIT : [d] "+v"(d) : [p] "v"(p) : "memory");
#define VM_L_SADDR(M, MODS, IMM)                                                                              \
  const uint32_t o = a.off - static_cast<uint32_t>(IMM);                                                      \
  asm volatile(VM_HEAD M " %[d], %[o], %[b] offset:" VM_STR(IMM) MODS VM_WAIT : [d] "+v"(d) : [o] "v"(o), [b] "s"(a.base) : "memory");
#define VM_L_FLAT(M, MODS, IMM)                                                                               \
  const uint8_t* p = a.base + a.off - (IMM);                                                                  \
  asm volatile(VM_HEAD M " %[d], %[p] offset:" VM_STR(IMM) MODS VM_WAIT_FLAT : [d] "+v"(d) : [p] "v"(p) : "memory");
#define VM_L_OFFEN(M, MODS, IMM)                                                                              \
  asm volatile(VM_HEAD M " %[d], %[o], %[r], 0 offen" MODS VM_WAIT : [d] "+v"(d) : [o] "v"(a.off), [r] "s"(a.raw) : "memory");
#define VM_L_IDXEN(M, MODS, IMM)                                                                              \
  const uint32_t i = a.off / VMEM_STRIDE;                                                                     \
  asm volatile(VM_HEAD M " %[d], %[i], %[r], 0 idxen" MODS VM_WAIT : [d] "+v"(d) : [i] "v"(i), [r] "s"(a.strided) : "memory");
#define VM_L_IDXEN_OFFEN(M, MODS, IMM)                                                                        \
  const u32x2 io = {a.off / VMEM_STRIDE, a.off % VMEM_STRIDE};                                                \
  asm volatile(VM_HEAD M " %[d], %[io], %[r], 0 idxen offen" MODS VM_WAIT : [d] "+v"(d) : [io] "v"(io), [r] "s"(a.strided) : "memory");
#define VM_L_OFF_SOFF(M, MODS, IMM)                                                                           \
  asm volatile(VM_HEAD M " %[d], off, %[r], %[so]" MODS VM_WAIT : [d] "+v"(d) : [r] "s"(a.raw), [so] "s"(a.soff) : "memory");
#define VM_L_OFFEN_SOFF(M, MODS, IMM)                                                                         \
  const uint32_t o = a.off - static_cast<uint32_t>(IMM) - a.soff;                                             \
  asm volatile(VM_HEAD M " %[d], %[o], %[r], %[so] offen offset:" VM_STR(IMM) MODS VM_WAIT                    \
               : [d] "+v"(d) : [o] "v"(o), [r] "s"(a.raw), [so] "s"(a.soff) : "memory");
// stores
#define VM_S_GLOBAL(M, MODS, IMM)                                                                             \
  const uint8_t* p = a.base + a.off;                                                                          \
  asm volatile(VM_HEAD M " %[p], %[d], off" MODS VM_WAIT : : [d] "v"(d), [p] "v"(p) : "memory");
#define VM_S_SADDR(M, MODS, IMM)                                                                              \
  const uint32_t o = a.off - static_cast<uint32_t>(IMM);                                                      \
  asm volatile(VM_HEAD M " %[o], %[d], %[b] offset:" VM_STR(IMM) MODS VM_WAIT : : [d] "v"(d), [o] "v"(o), [b] "s"(a.base) : "memory");
#define VM_S_FLAT(M, MODS, IMM)                                                                               \
  const uint8_t* p = a.base + a.off;                                                                          \
  asm volatile(VM_HEAD M " %[p], %[d]" MODS VM_WAIT_FLAT : : [d] "v"(d), [p] "v"(p) : "memory");
#define VM_S_OFFEN(M, MODS, IMM)                                                                              \
  asm volatile(VM_HEAD M " %[d], %[o], %[r], 0 offen" MODS VM_WAIT : : [d] "v"(d), [o] "v"(a.off), [r] "s"(a.raw) : "memory");
#define VM_S_IDXEN(M, MODS, IMM)                                                                              \
  const uint32_t i = a.off / VMEM_STRIDE;                                                                     \
  asm volatile(VM_HEAD M " %[d], %[i], %[r], 0 idxen" MODS VM_WAIT : : [d] "v"(d), [i] "v"(i), [r] "s"(a.strided) : "memory");

// One application of op OP at `a` on the registers v (a load's preset destination; a store's data): a load returns the
// registers it wrote (the rest 0), a store returns v.
template <int OP>
__device__ __forceinline__ u32x4 access(const Addr& a, u32x4 v);

#define VMEM_X_LOAD(NAME, W, F, IMM, M, MODS)                                   \
  template <>                                                                   \
  __device__ __forceinline__ u32x4 access<VO_##NAME>(const Addr& a, u32x4 v) {  \
    auto d = pack<vmem_regs(W)>(v);                                             \
    VM_L_##F(M, MODS, IMM)                                                      \
    return unpack(d);                                                           \
  }
#define VMEM_X_STORE(NAME, W, F, IMM, M, MODS)                                  \
  template <>                                                                   \
  __device__ __forceinline__ u32x4 access<VO_##NAME>(const Addr& a, u32x4 v) {  \
    const auto d = pack<vmem_regs(W)>(v);                                       \
    VM_S_##F(M, MODS, IMM)                                                      \
    return v;                                                                   \
  }
VMEM_LOAD_LIST(VMEM_X_LOAD)
VMEM_STORE_LIST(VMEM_X_STORE)
#undef VMEM_X_LOAD
#undef VMEM_X_STORE

// the reload of the stores' walk, and the plain load of the L1 test
template <bool SC1>
__device__ __forceinline__ u32x4 load_x4(const void* p) {
  u32x4 d;
  if constexpr (SC1) asm volatile("global_load_dwordx4 %[d], %[p], off sc1" VM_WAIT : [d] "=&v"(d) : [p] "v"(p) : "memory");
  else asm volatile("global_load_dwordx4 %[d], %[p], off" VM_WAIT : [d] "=&v"(d) : [p] "v"(p) : "memory");
  return d;
}

// --- loads and stores: the walks ----------------------------------------------------------------------------------
// mem: the table (loads) or the store regions of the whole grid (stores), `mem_bytes` long.  expect: the
// VMEM_WAVE * VMEM_CHAINS words a wave must end with.  (skip_block, skip_iter): wave 0 of that workgroup leaves chain
// 0's access out of that step (-1: none); flip_block: one bit of lane 0's final chain-0 word of that workgroup's
// wave 0 is flipped before the compare (-1: none).  wave_row (stores): the SIMD map row each wave ran on.
template <int OP>
__global__ void __launch_bounds__(THREADS) walk_kernel(uint8_t* mem, uint32_t mem_bytes, const uint32_t* expect, uint32_t seed,
                                                       int iters, int flip_block, int skip_block, int skip_iter, Report* rep,
                                                       unsigned long long* simd_map, uint32_t* wave_row) {
  constexpr bool STORE = vmem_is_store(OP);
  constexpr int W = VMEM_OP_TABLE[OP].width, FORM = VMEM_OP_TABLE[OP].form, IMM = VMEM_OP_TABLE[OP].imm, REGS = vmem_regs(W);
  const long long t0 = wall_clock64();
  const int lane = static_cast<int>(threadIdx.x & 63u);
  const uint32_t wave = uniform(blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6));
  const bool hooked_wave = (wave & 3u) == 0;
  const int skip_at = hooked_wave && static_cast<int>(blockIdx.x) == skip_block ? skip_iter : -1;  // wave-uniform
  Addr a;
  a.base = mem;
  a.raw = descriptor(mem, 0, mem_bytes);
  a.strided = descriptor(mem, VMEM_STRIDE, mem_bytes / VMEM_STRIDE);
  a.soff = 0;
  // a store's lane owns cell lane + 1 of its wave's region; a load's lane the whole table
  const uint32_t home = STORE ? wave * VMEM_REGION + VMEM_CELL * static_cast<uint32_t>(lane + 1) : 0u;
  uint32_t x[VMEM_CHAINS], c[VMEM_CHAINS];
#pragma unroll
  for (int ch = 0; ch < VMEM_CHAINS; ++ch) {
    x[ch] = vmem_init(seed, lane, ch);
    c[ch] = vmem_const(seed, lane, ch);
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int ch = 0; ch < VMEM_CHAINS; ++ch) {
      const bool skipped = ch == 0 && it == skip_at;
      const uint32_t x0 = uniform(x[ch]);
      const u32x4 pre = {vmem_preset(x[ch], 0), vmem_preset(x[ch], 1), vmem_preset(x[ch], 2), vmem_preset(x[ch], 3)};
      uint32_t r[4];
      if constexpr (!STORE) {
        a.off = vmem_off_of(W, FORM, IMM, FORM == VF_OFF_SOFF ? x0 : x[ch], VMEM_TABLE_BYTES);
        if constexpr (FORM == VF_OFF_SOFF) a.soff = uniform(a.off);
        if constexpr (FORM == VF_OFFEN_SOFF) a.soff = vmem_soff(x0);
        const u32x4 got = skipped ? pre : access<OP>(a, pre);
        r[0] = got.x, r[1] = got.y, r[2] = got.z, r[3] = got.w;
        x[ch] = vmem_step(x[ch], vmem_fold(r, REGS), c[ch]);
      } else {
        const uint32_t off = vmem_off_of(W, FORM, IMM, x[ch], VMEM_CELL);
        a.off = home + off;
        if (!skipped) access<OP>(a, pre);
        const u32x4 got = load_x4<true>(mem + home + (off & ~15u));
        r[0] = got.x, r[1] = got.y, r[2] = got.z, r[3] = got.w;
        x[ch] = vmem_step(x[ch], vmem_fold(r, 4), c[ch]);
      }
    }
  }
  if (hooked_wave && static_cast<int>(blockIdx.x) == flip_block && lane == 0) x[0] ^= 0x10u;
  unsigned nbad = 0, first_chain = 0;
  uint32_t got = 0, want = 0;
#pragma unroll
  for (int ch = VMEM_CHAINS - 1; ch >= 0; --ch) {
    const uint32_t w = expect[lane * VMEM_CHAINS + ch];
    if (x[ch] != w) ++nbad, first_chain = ch, got = x[ch], want = w;
  }
  const unsigned row = simd_row();
  if (STORE && lane == 0) wave_row[wave] = row;
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  report(rep, simd_map, row, nbad, where_of(row, (static_cast<unsigned>(lane) << 8) | first_chain), wave, got, want, dt);
}

// the stores' regions before a walk: every wave's gets the background image
__global__ void __launch_bounds__(THREADS) fill_regions_kernel(uint32_t* regions, const uint32_t* background, uint32_t words) {
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < words; i += gridDim.x * THREADS)
    regions[i] = background[i % (VMEM_REGION / 4)];
}

// ... and after it: every byte of every region against the model's image of one wave, guard cells included.  Plain
// loads: nothing of the op under test.  Wrong bytes go to the row of the SIMD that ran the region's wave.
__global__ void __launch_bounds__(THREADS) check_regions_kernel(const uint32_t* regions, const uint32_t* image, uint32_t words,
                                                                const uint32_t* wave_row, Report* rep,
                                                                unsigned long long* simd_map) {
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < words; i += gridDim.x * THREADS) {
    const uint32_t g = regions[i], w = image[i % (VMEM_REGION / 4)], diff = g ^ w;
    if (!diff) continue;
    const unsigned nbad = !!(diff & 0xffu) + !!(diff & 0xff00u) + !!(diff & 0xff0000u) + !!(diff & 0xff000000u);
    const uint32_t wave = i / (VMEM_REGION / 4);
    const unsigned row = wave_row[wave];
    const unsigned long long index = (static_cast<unsigned long long>(wave) << 32) | (4u * (i % (VMEM_REGION / 4)));
    report_wrong(rep, simd_map, row, nbad, where_of(row, 0xffffu), index, g, w);  // no lane: a byte of the image
  }
}

// one wave, `n` applications one after the other, returned raw.  Loads: out[(i * 64 + lane) * 4 + j] = register j.
// Stores: the target memory itself is the result.
template <int OP>
__global__ void __launch_bounds__(64) apply_kernel(uint8_t* mem, uint32_t stride, uint32_t num_records, const uint32_t* offsets,
                                                   const uint32_t* preset, uint32_t* out, int n) {
  constexpr int FORM = VMEM_OP_TABLE[OP].form, REGS = vmem_regs(VMEM_OP_TABLE[OP].width);
  Addr a;
  a.base = mem;
  a.raw = a.strided = descriptor(mem, stride, num_records);
  for (int i = 0; i < n; ++i) {
    const uint32_t k = static_cast<uint32_t>(i) * 64u + threadIdx.x;
    a.off = offsets[k];
    a.soff = FORM == VF_OFF_SOFF ? uniform(a.off) : FORM == VF_OFFEN_SOFF ? 1u : 0u;
    const u32x4 v = {preset[4 * k], preset[4 * k + 1], preset[4 * k + 2], preset[4 * k + 3]};
    const u32x4 r = access<OP>(a, v);
    if constexpr (!vmem_is_store(OP)) {
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < REGS; ++j) out[4 * k + j] = w[j];
    }
  }
}

struct WalkLaunch {
  uint8_t* mem;
  uint32_t mem_bytes;
  const uint32_t* expect;
  uint32_t seed;
  int iters, flip_block, skip_block, skip_iter;
  Report* rep;
  unsigned long long* map;
  uint32_t* wave_row;
  unsigned blocks;
};
struct ApplyLaunch {
  uint8_t* mem;
  uint32_t stride, num_records;
  const uint32_t *offsets, *preset;
  uint32_t* out;
  int n;
};

template <int OP>
void launch_op(const WalkLaunch& l) {
  hipLaunchKernelGGL(walk_kernel<OP>, dim3(l.blocks), dim3(THREADS), 0, nullptr, l.mem, l.mem_bytes, l.expect, l.seed, l.iters,
                     l.flip_block, l.skip_block, l.skip_iter, l.rep, l.map, l.wave_row);
}
template <int OP>
hipError_t attributes_op(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(walk_kernel<OP>));
}
template <int OP>
void launch_apply(const ApplyLaunch& l) {
  hipLaunchKernelGGL(apply_kernel<OP>, dim3(1), dim3(64), 0, nullptr, l.mem, l.stride, l.num_records, l.offsets, l.preset, l.out,
                     l.n);
}
template <int OP>
hipError_t attributes_apply(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(apply_kernel<OP>));
}
template <int... OP>
struct Ops {
  static constexpr void (*launch[])(const WalkLaunch&) = {launch_op<OP>...};
  static constexpr hipError_t (*attributes[])(hipFuncAttributes*) = {attributes_op<OP>...};
  static constexpr void (*apply[])(const ApplyLaunch&) = {launch_apply<OP>...};
  static constexpr hipError_t (*apply_attributes[])(hipFuncAttributes*) = {attributes_apply<OP>...};
};
template <int... I>
Ops<I...> ops_of(std::integer_sequence<int, I...>);
using AllOps = decltype(ops_of(std::make_integer_sequence<int, VMEM_OPS>()));

// --- bounds -------------------------------------------------------------------------------------------------------
// the four rows of loads and of stores: raw dword, raw dwordx4, structured dword, structured dwordx4
constexpr int BOUNDS_ROWS = 4;
#define BND_LOAD(M, MODE) asm volatile(VM_HEAD M " %[d], %[o], %[r], 0 " MODE VM_WAIT : [d] "+v"(d) : [o] "v"(o), [r] "s"(rsrc) : "memory")
#define BND_STORE(M, MODE) asm volatile(VM_HEAD M " %[d], %[o], %[r], 0 " MODE VM_WAIT : : [d] "v"(d), [o] "v"(o), [r] "s"(rsrc) : "memory")

// buf: 2 n bytes of vmem_bounds_word(); the descriptor covers `num_records` (what the host passes: n, or n / 16
// elements; the self-check passes twice that) while the expected values are those of n.  Every lane's address lies
// inside buf whatever the descriptor says.  STORE: the lanes store vmem_bounds_data() and the host checks buf.
template <int ROW, bool STORE>
__global__ void __launch_bounds__(THREADS) bounds_kernel(uint32_t* buf, uint32_t n, uint32_t num_records, uint32_t seed, Report* rep,
                                                         unsigned long long* simd_map) {
  constexpr bool STRUCT = ROW >= 2, X4 = ROW & 1;
  constexpr int REGS = X4 ? 4 : 1;
  const long long t0 = wall_clock64();
  const int lane = static_cast<int>(threadIdx.x & 63u);
  const uint32_t wave = uniform(blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6));
  // a store kernel's wave owns 2 n bytes of its own; the loads all read the same 2 n
  uint32_t* mine = STORE ? buf + static_cast<size_t>(wave) * (n / 2) : buf;
  const u32x4 rsrc = descriptor(mine, STRUCT ? VMEM_STRIDE : 0u, num_records);
  unsigned nbad = 0;
  uint32_t first = 0, got = 0, want = 0;
  for (uint32_t k = 0; k < vmem_bounds_rounds(n); ++k)
    for (uint32_t sub = 0; sub < (X4 || STRUCT ? 1u : 4u); ++sub) {  // a raw dword row visits all four dwords of a slot
      const uint32_t slot = vmem_bounds_slot(n, lane, k), byte = slot * 16u + 4u * sub;
      const uint32_t o = STRUCT ? slot : byte;
      typename Regs<REGS>::type d;
      if constexpr (STORE) {
        const u32x4 v = {vmem_bounds_data(seed, lane, k * 4 + sub, 0), vmem_bounds_data(seed, lane, k * 4 + sub, 1),
                         vmem_bounds_data(seed, lane, k * 4 + sub, 2), vmem_bounds_data(seed, lane, k * 4 + sub, 3)};
        d = pack<REGS>(v);
        if constexpr (ROW == 0) BND_STORE("buffer_store_dword", "offen");
        else if constexpr (ROW == 1) BND_STORE("buffer_store_dwordx4", "offen");
        else if constexpr (ROW == 2) BND_STORE("buffer_store_dword", "idxen");
        else BND_STORE("buffer_store_dwordx4", "idxen");
      } else {
        d = pack<REGS>(u32x4{0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu});
        if constexpr (ROW == 0) BND_LOAD("buffer_load_dword", "offen");
        else if constexpr (ROW == 1) BND_LOAD("buffer_load_dwordx4", "offen");
        else if constexpr (ROW == 2) BND_LOAD("buffer_load_dword", "idxen");
        else BND_LOAD("buffer_load_dwordx4", "idxen");
        const u32x4 r = unpack(d);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < REGS; ++j) {
          const uint32_t e = byte < n ? vmem_bounds_word(seed, byte / 4 + j) : 0u;
          if (w[j] != e) {
            if (!nbad) first = byte + 4 * j, got = w[j], want = e;
            ++nbad;
          }
        }
      }
    }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  report(rep, simd_map, row, nbad, where_of(row, lane << 8), first, got, want, dt);
}

template <int ROW, bool STORE>
void launch_bounds_row(unsigned grid, uint32_t* buf, uint32_t n, uint32_t num_records, uint32_t seed, Report* rep,
                       unsigned long long* map) {
  hipLaunchKernelGGL((bounds_kernel<ROW, STORE>), dim3(grid), dim3(THREADS), 0, nullptr, buf, n, num_records, seed, rep, map);
}
template <int ROW, bool STORE>
hipError_t attributes_bounds_row(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(bounds_kernel<ROW, STORE>));
}
using BoundsLaunch = void (*)(unsigned, uint32_t*, uint32_t, uint32_t, uint32_t, Report*, unsigned long long*);
constexpr BoundsLaunch BOUNDS_LAUNCH[2][BOUNDS_ROWS] = {
    {launch_bounds_row<0, false>, launch_bounds_row<1, false>, launch_bounds_row<2, false>, launch_bounds_row<3, false>},
    {launch_bounds_row<0, true>, launch_bounds_row<1, true>, launch_bounds_row<2, true>, launch_bounds_row<3, true>}};
constexpr hipError_t (*BOUNDS_ATTRIBUTES[2][BOUNDS_ROWS])(hipFuncAttributes*) = {
    {attributes_bounds_row<0, false>, attributes_bounds_row<1, false>, attributes_bounds_row<2, false>, attributes_bounds_row<3, false>},
    {attributes_bounds_row<0, true>, attributes_bounds_row<1, true>, attributes_bounds_row<2, true>, attributes_bounds_row<3, true>}};

// --- l1 -----------------------------------------------------------------------------------------------------------
// Workgroup b walks slice b (slice_words words of vmem_l1_word()) `passes` times per wave, 1 KiB per wave-instruction,
// wave w starting a quarter of the slice further on; every word of every pass is compared in registers.
template <bool SC1>
__global__ void __launch_bounds__(THREADS) l1_kernel(const uint32_t* slices, uint32_t slice_words, uint32_t seed, int passes,
                                                     Report* rep, unsigned long long* simd_map) {
  const long long t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6), slice = blockIdx.x;
  const uint32_t* base = slices + static_cast<size_t>(slice) * slice_words;
  const uint32_t chunks = slice_words / 256u, start = wave * chunks / 4u;  // chunks: a power of two
  unsigned nbad = 0;
  uint32_t first = 0, got = 0, want = 0;
  for (int p = 0; p < passes; ++p)
    for (uint32_t c = 0; c < chunks; ++c) {
      const uint32_t word = ((start + c) & (chunks - 1)) * 256u + lane * 4u;
      const u32x4 v = load_x4<SC1>(base + word);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t e = vmem_l1_word(seed, slice, word + j);
        if (w[j] != e) {
          if (!nbad) first = word + j, got = w[j], want = e;
          ++nbad;
        }
      }
    }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  report(rep, simd_map, row, nbad, where_of(row, lane << 8), (static_cast<unsigned long long>(slice) << 32) | first, got, want,
         dt);
}

__global__ void __launch_bounds__(THREADS) fill_slices_kernel(uint32_t* slices, uint32_t slice_words, uint32_t seed) {
  uint32_t* base = slices + static_cast<size_t>(blockIdx.x) * slice_words;
  for (uint32_t i = threadIdx.x; i < slice_words; i += THREADS) base[i] = vmem_l1_word(seed, blockIdx.x, i);
}

// --- ldsdma -------------------------------------------------------------------------------------------------------
// One LDS-DMA load per step: lane l's SIZE bytes from its own slot of the table land at M0 + l * SIZE of the wave's
// 1 KiB of LDS.  M0 is saved and restored inside the statement that writes it.
#define DMA_GLOBAL(M)                                                                                         \
  asm volatile("s_mov_b32 %[k], m0\ns_mov_b32 m0, %[l]\ns_nop 0\n" M " %[p], off\ns_mov_b32 m0, %[k]" VM_WAIT   \
               : [k] "=&s"(keep) : [p] "v"(src), [l] "s"(dst) : "memory")
#define DMA_BUFFER(M)                                                                                         \
  asm volatile("s_nop 4\ns_mov_b32 %[k], m0\ns_mov_b32 m0, %[l]\ns_nop 0\n" M " %[o], %[r], 0 offen lds\ns_mov_b32 m0, %[k]" VM_WAIT \
               : [k] "=&s"(keep) : [o] "v"(off), [r] "s"(rsrc), [l] "s"(dst) : "memory")

constexpr int dma_bytes(int form) { return form % 2 == 0 ? 4 : 16; }
constexpr const char* DMA_NAMES[DMA_FORMS] = {"global_load_lds_dword", "global_load_lds_dwordx4", "buffer_load_dword_lds",
                                              "buffer_load_dwordx4_lds"};

template <int FORM>
__global__ void __launch_bounds__(THREADS) ldsdma_kernel(const uint8_t* table, uint32_t table_seed, uint32_t seed, int iters,
                                                         Report* rep, unsigned long long* simd_map) {
  constexpr int SIZE = dma_bytes(FORM), WORDS = SIZE / 4;
  __shared__ uint32_t lds[(THREADS / 64) * 256];  // 1 KiB per wave: 64 lanes x 16 bytes
  const long long t0 = wall_clock64();
  const int lane = static_cast<int>(threadIdx.x & 63u);
  const uint32_t wave = uniform(threadIdx.x >> 6);
  uint32_t* area = lds + wave * 256u;
  // the LDS byte address of the wave's area: the low half of its flat address
  const uint32_t dst = uniform(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(area)));
  const u32x4 rsrc = descriptor(table, 0, VMEM_TABLE_BYTES);
  const int partner = vmem_dma_partner(lane);
  unsigned nbad = 0;
  uint32_t first = 0, got = 0, want = 0;
  for (int it = 0; it < iters; ++it) {
    const uint32_t off = vmem_dma_slot(seed, lane, static_cast<uint32_t>(it)) * 16u;
    const uint8_t* src = table + off;
    uint32_t keep;
    if constexpr (FORM == 0) DMA_GLOBAL("global_load_lds_dword");
    else if constexpr (FORM == 1) DMA_GLOBAL("global_load_lds_dwordx4");
    else if constexpr (FORM == 2) DMA_BUFFER("buffer_load_dword");
    else DMA_BUFFER("buffer_load_dwordx4");
    (void)src, (void)off;
    __syncthreads();
    const uint32_t theirs = vmem_dma_slot(seed, partner, static_cast<uint32_t>(it)) * 4u;  // the partner's first table word
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      const uint32_t g = area[partner * WORDS + j], e = vmem_word(theirs + j, table_seed);
      if (g != e) {
        if (!nbad) first = (static_cast<uint32_t>(it) << 8) | (partner * WORDS + j), got = g, want = e;
        ++nbad;
      }
    }
    __syncthreads();
  }
  const unsigned row = simd_row();
  const unsigned long long dt = static_cast<unsigned long long>(wall_clock64() - t0);
  report(rep, simd_map, row, nbad, where_of(row, lane << 8), first, got, want, dt);
}

template <int FORM>
void launch_dma(unsigned grid, const uint8_t* table, uint32_t table_seed, uint32_t seed, int iters, Report* rep,
                unsigned long long* map) {
  hipLaunchKernelGGL(ldsdma_kernel<FORM>, dim3(grid), dim3(THREADS), 0, nullptr, table, table_seed, seed, iters, rep, map);
}
template <int FORM>
hipError_t attributes_dma(hipFuncAttributes* a) {
  return hipFuncGetAttributes(a, reinterpret_cast<const void*>(ldsdma_kernel<FORM>));
}
using DmaLaunch = void (*)(unsigned, const uint8_t*, uint32_t, uint32_t, int, Report*, unsigned long long*);
constexpr DmaLaunch DMA_LAUNCH[DMA_FORMS] = {launch_dma<0>, launch_dma<1>, launch_dma<2>, launch_dma<3>};
constexpr hipError_t (*DMA_ATTRIBUTES[DMA_FORMS])(hipFuncAttributes*) = {attributes_dma<0>, attributes_dma<1>, attributes_dma<2>,
                                                                        attributes_dma<3>};

// --- host ------------------------------------------------------------------------------------------------------
// -3 with a message when a kernel was built with scratch, or with another LDS allocation than it may have
int refuse(const hipFuncAttributes& attr, const std::string& what, size_t lds_allowed = 0) {
  return refuse_memory("vmem test", what, attr,
                       " (allowed: 0 and " + std::to_string(lds_allowed) + "): it would test another memory than the one it names",
                       lds_allowed);
}

void fill_table(std::vector<uint32_t>* t, uint32_t seed) {
  t->resize(VMEM_TABLE_BYTES / 4);
  for (uint32_t i = 0; i < VMEM_TABLE_BYTES / 4; ++i) (*t)[i] = vmem_word(i, seed);
}

}  // namespace

extern "C" {

const char* vmem_last_error(void) { return g_err.c_str(); }

int vmem_device_count(void) { return device_count(); }

int vmem_slots(void) { return SIMD_ROWS; }  // rows of every simd_map below

int vmem_ops(void) { return VMEM_OPS; }  // the op table's length; the first vmem_loads() of them are loads

int vmem_loads(void) { return VMEM_LOADS; }

// 1 when the walk of load op `op` under `seed` for `iters` steps reads byte 0 of table word `word` (where the
// self-check flips a bit), 0 when not, -2 for an op that is no load or a word outside the table.  Host only.
int vmem_walk_reads(int op, uint64_t seed, int iters, unsigned int word) {
  if (op < 0 || op >= VMEM_LOADS || iters < 1 || iters > MAX_ITERS || word >= VMEM_TABLE_BYTES / 4) {
    g_err = "vmem walk_reads: need a load op, iters 1..2^16 and a word of the table";
    return -2;
  }
  std::vector<uint32_t> table;
  fill_table(&table, vmem_mix32(seed));
  std::vector<uint8_t> touched(VMEM_TABLE_BYTES, 0);
  uint32_t words[VMEM_WAVE * VMEM_CHAINS];
  vmem_expected(op, vmem_op_seed(seed, op), iters, -1, reinterpret_cast<const uint8_t*>(table.data()), words, nullptr, touched.data());
  return touched[4 * word];
}

// The walks.  Every op of `ops[0..nops)` (VmemOp of vmem_ref.h: loads and stores), one after the other, on `blocks`
// workgroups of 4 waves (0: 2 per CU), `iters` steps of 4 chains per lane: a checked warm-up launch, then `reps`
// timed and checked launches.  Per op k (arrays of the table's length): errors[k] = wrong chain words (and, for a
// store, wrong bytes of the regions) over all its launches; first[4 k ..] = where (SIMD map row << 32 | lane << 8 |
// chain; lane 0xff: a byte of a region), index (the wave; wave << 32 | byte of its region), got, want of one wrong
// word of the first launch that had any (where ~0: none); ms[k] the mean time of a timed launch (a store's: the walk
// alone, without the fill and the check of the regions).  simd_map: vmem_slots() x 3 (waves run, wrong words,
// summed wall_clock64 ticks) per physical SIMD, added up over every launch of every op.
//
// Refused with -2 and a message: a bad device, blocks outside 0..8192, iters outside 1..2^16, reps < 1, no op, an
// unknown or repeated one, a hook outside the list, the grid or the table; with -3: a kernel built with a scratch
// segment or an LDS allocation.
//
// Self-check hooks, off by default (-1), all acting in the warm-up launch:
//   flip   (inject_op, inject_block; inject_skip_iter < 0): one bit of lane 0's final chain-0 word of wave 0 of that
//          workgroup is flipped before the compare: 1 wrong word, got = want ^ 0x10
//   skip   (inject_skip_iter >= 0): that wave leaves chain 0's load or store out of that step; wrong words > 0
//   table  (inject_table_word >= 0): the host flips one bit of that table word for every load op's warm-up launch and
//          restores it after; every op whose walk reads the word's byte 0 (vmem_walk_reads) reports it
int vmem_walks(int device, int blocks, int iters, int reps, const int* ops, int nops, uint64_t seed, int inject_op,
               int inject_block, int inject_skip_iter, long long inject_table_word, unsigned long long* errors,
               unsigned long long* first, double* ms, unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || blocks > MAX_BLOCKS || iters < 1 || iters > MAX_ITERS || reps < 1 ||
      !op_list_known(ops, nops, VMEM_OPS, true)) {
    g_err = "vmem walks: need a valid device, blocks 0..8192 (0: 2 per CU), iters 1..2^16, reps >= 1 and a list of distinct known ops";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (!op_list_has_hook(ops, nops, inject_op) || grid > static_cast<unsigned>(MAX_BLOCKS) ||
      (inject_op >= 0 && !hook_in_range(inject_block, grid, inject_skip_iter, iters)) ||
      inject_table_word >= static_cast<long long>(VMEM_TABLE_BYTES / 4)) {
    g_err = "vmem walks: inject_op must be in the list, inject_block inside the grid (at most 8192 workgroups), "
            "inject_skip_iter below iters and inject_table_word inside the table";
    return -2;
  }
  for (int k = 0; k < VMEM_OPS; ++k) {
    errors[k] = 0;
    no_record(first + 4 * k);
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  std::vector<uint32_t> table;
  fill_table(&table, vmem_mix32(seed));
  const uint32_t waves = grid * (THREADS / 64), region_words = waves * (VMEM_REGION / 4);
  DevBuf dtable, dexp, dregions, dbg, dimg, drow;
  HIP_CHECK(dtable.alloc(device, VMEM_TABLE_BYTES));
  HIP_CHECK(hipMemcpy(dtable.ptr, table.data(), VMEM_TABLE_BYTES, hipMemcpyHostToDevice));
  HIP_CHECK(dexp.alloc(device, VMEM_WAVE * VMEM_CHAINS * sizeof(uint32_t)));
  HIP_CHECK(dregions.alloc(device, static_cast<size_t>(region_words) * 4));
  HIP_CHECK(dbg.alloc(device, VMEM_REGION));
  HIP_CHECK(dimg.alloc(device, VMEM_REGION));
  HIP_CHECK(drow.alloc(device, static_cast<size_t>(waves) * 4));
  HIP_CHECK(hipMemset(drow.ptr, 0, static_cast<size_t>(waves) * 4));
  std::vector<uint32_t> expect(VMEM_WAVE * VMEM_CHAINS);
  std::vector<uint8_t> image(VMEM_REGION), background(VMEM_REGION);
  const unsigned sweep_grid = (region_words + THREADS - 1) / THREADS < 2048 ? (region_words + THREADS - 1) / THREADS : 2048;
  for (int i = 0; i < nops; ++i) {
    const int k = ops[i];
    const bool store = vmem_is_store(k);
    hipFuncAttributes attr;
    HIP_CHECK(AllOps::attributes[k](&attr));
    if (const int rc = refuse(attr, VMEM_OP_TABLE[k].name)) return rc;
    const uint32_t op_seed = vmem_op_seed(seed, k);
    vmem_expected(k, op_seed, iters, -1, reinterpret_cast<const uint8_t*>(table.data()), expect.data(), image.data(), nullptr);
    HIP_CHECK(hipMemcpy(dexp.ptr, expect.data(), expect.size() * 4, hipMemcpyHostToDevice));
    if (store) {
      for (uint32_t b = 0; b < VMEM_REGION; ++b) background[b] = vmem_background(op_seed, b);
      HIP_CHECK(hipMemcpy(dbg.ptr, background.data(), VMEM_REGION, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dimg.ptr, image.data(), VMEM_REGION, hipMemcpyHostToDevice));
    }
    double total_ms = 0.0;
    for (int r = 0; r <= reps; ++r) {  // r == 0: the warm-up, which carries the hooks
      const HookTrio h = hook_trio(r == 0 && k == inject_op, inject_block, inject_skip_iter);
      const bool table_hook = r == 0 && !store && inject_table_word >= 0;
      if (table_hook)
        if (const int rc = flip_word_bit(static_cast<uint32_t*>(dtable.ptr) + inject_table_word)) return rc;
      if (const int rc = run.clear()) return rc;
      if (store) {
        hipLaunchKernelGGL(fill_regions_kernel, dim3(sweep_grid), dim3(THREADS), 0, nullptr, static_cast<uint32_t*>(dregions.ptr),
                           static_cast<const uint32_t*>(dbg.ptr), region_words);
        HIP_CHECK(hipGetLastError());
      }
      const WalkLaunch l = {static_cast<uint8_t*>(store ? dregions.ptr : dtable.ptr), store ? region_words * 4u : VMEM_TABLE_BYTES,
                            static_cast<const uint32_t*>(dexp.ptr), op_seed, iters, h.flip_block, h.skip_block, h.skip_at,
                            run.rep(), run.map(), static_cast<uint32_t*>(drow.ptr), grid};
      float t = 0.f;
      if (const int rc = run.launch([&] { AllOps::launch[k](l); }, &t)) return rc;
      if (store) {
        hipLaunchKernelGGL(check_regions_kernel, dim3(sweep_grid), dim3(THREADS), 0, nullptr,
                           static_cast<const uint32_t*>(dregions.ptr), static_cast<const uint32_t*>(dimg.ptr), region_words,
                           static_cast<const uint32_t*>(drow.ptr), run.rep(), run.map());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
      }
      if (const int rc = run.collect(errors + k, first + 4 * k)) return rc;
      if (table_hook)
        if (const int rc = flip_word_bit(static_cast<uint32_t*>(dtable.ptr) + inject_table_word)) return rc;
      if (r > 0) total_ms += t;
    }
    ms[k] = total_ms / reps;
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// The descriptor's range check.  `blocks` workgroups of 4 waves (0: 2 per CU) run four rows of loads (raw dword, raw
// dwordx4, structured dword, structured dwordx4) over one buffer of 2 n bytes whose descriptor covers n (n / 16
// elements of stride 16), then the same four rows of stores, every wave over 2 n bytes of its own: a warm-up launch
// and one timed launch per row.  n: a power of two from 1 KiB to 64 KiB.  errors[0..4) = wrong words per load row
// (an in-range lane must read the buffer, a lane at or past num_records 0); errors[4..8) = wrong bytes per store row
// (the host compares all 2 n bytes of every wave with the model's image).  first[4 row ..] = where (SIMD map row
// << 32 | lane << 8; ~0: none; a store row's where is 0: the host found it), index (the byte offset; a store's: wave
// << 32 | byte), got, want.  ms[row] the timed launch.  simd_map as vmem_walks' (the load rows only add wrong words).
//
// Self-check hook: leak != 0 passes a descriptor of twice the num_records in the warm-up launches while the expected
// values stay those of n: the lanes out of range are served, and every row must report them.  All addresses stay
// inside the 2 n bytes.
int vmem_bounds(int device, int blocks, unsigned int n, uint64_t seed, int leak, unsigned long long* errors,
                unsigned long long* first, double* ms, unsigned long long* simd_map, int* blocks_run) {
  const int ndev = device_count();
  if (device < 0 || device >= ndev || blocks < 0 || blocks > MAX_BLOCKS || n < 1024 || n > 65536 || (n & (n - 1))) {
    g_err = "vmem bounds: need a valid device, blocks 0..8192 (0: 2 per CU) and n a power of two from 1 KiB to 64 KiB";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  if (grid > static_cast<unsigned>(MAX_BLOCKS)) {
    g_err = "vmem bounds: at most 8192 workgroups";
    return -2;
  }
  for (int k = 0; k < 2 * BOUNDS_ROWS; ++k) {
    errors[k] = 0;
    no_record(first + 4 * k);
    ms[k] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  const uint32_t seed32 = vmem_mix32(seed), words = n / 2;  // of 2 n bytes
  const uint32_t waves = grid * (THREADS / 64);
  std::vector<uint32_t> fill(words), back(static_cast<size_t>(waves) * words), image(words);
  for (uint32_t i = 0; i < words; ++i) fill[i] = vmem_bounds_word(seed32, i);
  DevBuf dload, dstore;
  HIP_CHECK(dload.alloc(device, static_cast<size_t>(words) * 4));
  HIP_CHECK(dstore.alloc(device, back.size() * 4));
  HIP_CHECK(hipMemcpy(dload.ptr, fill.data(), fill.size() * 4, hipMemcpyHostToDevice));
  for (int store = 0; store < 2; ++store)
    for (int row = 0; row < BOUNDS_ROWS; ++row) {
      const int k = store * BOUNDS_ROWS + row;
      const bool structured = row >= 2, x4 = row & 1;
      hipFuncAttributes attr;
      HIP_CHECK(BOUNDS_ATTRIBUTES[store][row](&attr));
      if (const int rc = refuse(attr, "a bounds row")) return rc;
      if (store) {  // the model's image of one wave: the background, then the in-range lanes' words
        image = fill;
        for (uint32_t kk = 0; kk < vmem_bounds_rounds(n); ++kk)
          for (uint32_t sub = 0; sub < (x4 || structured ? 1u : 4u); ++sub)
            for (int lane = 0; lane < VMEM_WAVE; ++lane) {
              const uint32_t byte = vmem_bounds_slot(n, lane, kk) * 16u + 4u * sub;
              if (byte >= n) continue;
              for (int j = 0; j < (x4 ? 4 : 1); ++j) image[byte / 4 + j] = vmem_bounds_data(seed32, lane, kk * 4 + sub, j);
            }
      }
      for (int r = 0; r < 2; ++r) {  // r == 0: the warm-up, which carries the hook
        const uint32_t covered = (structured ? n / VMEM_STRIDE : n) * (r == 0 && leak ? 2u : 1u);
        if (store)
          for (uint32_t w = 0; w < waves; ++w)
            HIP_CHECK(hipMemcpyAsync(static_cast<uint32_t*>(dstore.ptr) + static_cast<size_t>(w) * words, fill.data(),
                                     static_cast<size_t>(words) * 4, hipMemcpyHostToDevice, nullptr));
        float t = 0.f;
        uint32_t* buf = static_cast<uint32_t*>(store ? dstore.ptr : dload.ptr);
        const auto enqueue = [&] { BOUNDS_LAUNCH[store][row](grid, buf, n, covered, seed32, run.rep(), run.map()); };
        if (const int rc = run.checked(enqueue, &t, errors + k, first + 4 * k)) return rc;
        if (store) {
          HIP_CHECK(hipMemcpy(back.data(), dstore.ptr, back.size() * 4, hipMemcpyDeviceToHost));
          for (uint32_t w = 0; w < waves; ++w)
            for (uint32_t i = 0; i < words; ++i) {
              const uint32_t g = back[static_cast<size_t>(w) * words + i], diff = g ^ image[i];
              if (!diff) continue;
              errors[k] += !!(diff & 0xffu) + !!(diff & 0xff00u) + !!(diff & 0xff0000u) + !!(diff & 0xff000000u);
              if (first[4 * k] == ~0ULL)
                first[4 * k] = 0, first[4 * k + 1] = (static_cast<unsigned long long>(w) << 32) | (4u * i), first[4 * k + 2] = g,
                          first[4 * k + 3] = image[i];
            }
        }
        if (r > 0) ms[k] = t;
      }
    }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// The vector L1.  `blocks` workgroups of 4 waves (0: 2 per CU), each over its own slice of `slice_bytes` (a power of
// two from 1 KiB to 1 MiB) filled with vmem_l1_word(); every wave reads the whole slice `passes` times (1..65536) with
// global_load_dwordx4, 1 KiB per wave-instruction, and compares every word: a warm-up launch and `reps` timed
// launches with plain loads, then `reps` timed launches with sc1 loads, which bypass the L1; all checked.  *errors =
// wrong reads; first[0..4) = where (SIMD map row << 32 | lane << 8; ~0: none), index (slice << 32 | word), got, want;
// *ms_plain / *ms_sc1 the mean times.  Nothing here proves a read was served by the L1.
//
// Self-check hook: inject_block >= 0 has the host flip one bit of word `inject_word` of that workgroup's slice for the
// warm-up launch and restore it: passes x 4 wrong reads, all of that word, on one CU.
int vmem_l1(int device, int blocks, int reps, unsigned int slice_bytes, int passes, uint64_t seed, int inject_block,
            long long inject_word, unsigned long long* errors, unsigned long long* first, double* ms_plain, double* ms_sc1,
            unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || blocks > MAX_BLOCKS || reps < 1 || slice_bytes < 1024 || slice_bytes > (1u << 20) ||
      (slice_bytes & (slice_bytes - 1)) || passes < 1 || passes > 65536) {
    g_err = "vmem l1: need a valid device, blocks 0..8192 (0: 2 per CU), reps >= 1, slice_bytes a power of two from 1 KiB to "
            "1 MiB and passes 1..65536";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  const uint32_t slice_words = slice_bytes / 4;
  if (grid > static_cast<unsigned>(MAX_BLOCKS) ||
      (inject_block >= 0 && (static_cast<unsigned>(inject_block) >= grid || inject_word < 0 || inject_word >= slice_words))) {
    g_err = "vmem l1: at most 8192 workgroups, inject_block inside the grid and inject_word inside the slice";
    return -2;
  }
  *errors = 0;
  no_record(first);
  *ms_plain = *ms_sc1 = 0.0;
  hipFuncAttributes attr;
  HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(l1_kernel<false>)));
  if (const int rc = refuse(attr, "the L1 walk")) return rc;
  HIP_CHECK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(l1_kernel<true>)));
  if (const int rc = refuse(attr, "the L1 walk with sc1")) return rc;
  Run run;
  if (const int rc = run.open(device)) return rc;
  const uint32_t seed32 = vmem_mix32(seed);
  DevBuf dslices;
  HIP_CHECK(dslices.alloc(device, static_cast<size_t>(grid) * slice_bytes));
  uint32_t* slices = static_cast<uint32_t*>(dslices.ptr);
  hipLaunchKernelGGL(fill_slices_kernel, dim3(grid), dim3(THREADS), 0, nullptr, slices, slice_words, seed32);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  uint32_t* hooked_word = inject_block >= 0 ? slices + static_cast<size_t>(inject_block) * slice_words + inject_word : nullptr;
  for (int sc1 = 0; sc1 < 2; ++sc1) {
    double total_ms = 0.0;
    for (int r = sc1 ? 1 : 0; r <= reps; ++r) {
      const bool hooked = r == 0 && hooked_word;
      if (hooked)
        if (const int rc = flip_word_bit(hooked_word)) return rc;
      float t = 0.f;
      const auto enqueue = [&] {
        if (sc1) hipLaunchKernelGGL(l1_kernel<true>, dim3(grid), dim3(THREADS), 0, nullptr, slices, slice_words, seed32, passes, run.rep(), run.map());
        else hipLaunchKernelGGL(l1_kernel<false>, dim3(grid), dim3(THREADS), 0, nullptr, slices, slice_words, seed32, passes, run.rep(), run.map());
      };
      if (const int rc = run.checked(enqueue, &t, errors, first)) return rc;
      if (hooked)
        if (const int rc = flip_word_bit(hooked_word)) return rc;
      if (r > 0) total_ms += t;
    }
    *(sc1 ? ms_sc1 : ms_plain) = total_ms / reps;
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

int vmem_ldsdma_forms(void) { return DMA_FORMS; }

const char* vmem_ldsdma_name(int form) { return form >= 0 && form < DMA_FORMS ? DMA_NAMES[form] : ""; }

// The LDS-DMA loads.  Every form (vmem_ldsdma_name) on `blocks` workgroups of 4 waves (0: 2 per CU), `iters` steps
// (1..2^16) each: a lane's bytes come from its own slot of the 64 KiB table and land at M0 + lane x size of its wave's
// 1 KiB of LDS; after the wait and a barrier every lane reads back what another lane's load brought and compares: a
// warm-up and `reps` timed launches.  Per form: errors[f] = wrong words, first[4 f ..] = where (row << 32 | lane <<
// 8; ~0: none), index (step << 8 | LDS word), got, want; ms[f].
int vmem_ldsdma(int device, int blocks, int iters, int reps, uint64_t seed, unsigned long long* errors, unsigned long long* first,
                double* ms, unsigned long long* simd_map, int* blocks_run) {
  const int n = device_count();
  if (device < 0 || device >= n || blocks < 0 || blocks > MAX_BLOCKS || iters < 1 || iters > MAX_ITERS || reps < 1) {
    g_err = "vmem ldsdma: need a valid device, blocks 0..8192 (0: 2 per CU), iters 1..2^16 and reps >= 1";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  const unsigned grid = default_grid(device, blocks, BLOCKS_PER_CU);
  *blocks_run = static_cast<int>(grid);
  for (int f = 0; f < DMA_FORMS; ++f) {
    errors[f] = 0;
    no_record(first + 4 * f);
    ms[f] = 0.0;
  }
  Run run;
  if (const int rc = run.open(device)) return rc;
  const uint32_t table_seed = vmem_mix32(seed);
  std::vector<uint32_t> table;
  fill_table(&table, table_seed);
  DevBuf dtable;
  HIP_CHECK(dtable.alloc(device, VMEM_TABLE_BYTES));
  HIP_CHECK(hipMemcpy(dtable.ptr, table.data(), VMEM_TABLE_BYTES, hipMemcpyHostToDevice));
  for (int f = 0; f < DMA_FORMS; ++f) {
    hipFuncAttributes attr;
    HIP_CHECK(DMA_ATTRIBUTES[f](&attr));
    if (const int rc = refuse(attr, DMA_NAMES[f], (THREADS / 64) * 1024)) return rc;
    const auto enqueue = [&](int r) {
      DMA_LAUNCH[f](grid, static_cast<const uint8_t*>(dtable.ptr), table_seed, vmem_op_seed(seed, 1000 + f + 16 * r), iters,
                    run.rep(), run.map());
    };
    if (const int rc = run.series(reps, enqueue, errors + f, first + 4 * f, ms + f)) return rc;
  }
  if (const int rc = run.read_map(simd_map)) return rc;
  return 0;
}

// `n` applications of op `op` by one wave of `device`, one after the other, returned raw.  mem_words[0..nwords): the
// memory the op works on (a load's table; a store's target before).  offsets[i * 64 + lane]: the byte offset the lane
// accesses (VF_OFF_SOFF: lane 0's, for the whole wave); regs[(i * 64 + lane) * 4 ..]: a load's preset destination
// registers, a store's data.  The buffer forms use a descriptor of `stride` (0, or 16 for the idxen forms) and
// `num_records` (bytes; elements with a stride), which may cover less than the memory: that is how the range check
// is probed, straddling accesses included.  A load: out[(i * 64 + lane) * 4 + j] = register j (registers the op does
// not write: 0).  A store: out[0..nwords) = the memory after.
//
// Refused with -2: a bad device or op, n outside 1..4096, memory outside 64 B..1 MiB, an access that does not lie
// whole and aligned inside the memory (with the room its immediate needs below it), a stride the form cannot take or a
// descriptor that covers more than the memory.
int vmem_apply(int device, int op, int n, const unsigned int* mem_words, unsigned int nwords, const unsigned int* offsets,
               const unsigned int* regs, unsigned int stride, unsigned int num_records, unsigned int* out) {
  const int ndev = device_count();
  bool ok = device >= 0 && device < ndev && op >= 0 && op < VMEM_OPS && n >= 1 && n <= 4096 && nwords >= 16 && nwords <= (1u << 18);
  if (ok) {
    const VmemOpInfo& t = VMEM_OP_TABLE[op];
    const uint32_t bytes = nwords * 4u, size = static_cast<uint32_t>(vmem_bytes(t.width)), al = size < 4 ? size : 4;
    const bool indexed = t.form == VF_IDXEN || t.form == VF_IDXEN_OFFEN;
    ok = stride == (indexed ? VMEM_STRIDE : 0u) && static_cast<uint64_t>(num_records) * (stride ? stride : 1u) <= bytes;
    const uint32_t low = t.form == VF_OFFEN_SOFF ? 4096u : t.imm > 0 ? static_cast<uint32_t>(t.imm) : 0u;
    for (int i = 0; ok && i < n * VMEM_WAVE; ++i)
      ok = offsets[i] % (t.form == VF_IDXEN ? VMEM_STRIDE : al) == 0 && offsets[i] >= low && offsets[i] <= bytes - size &&
           (t.imm >= 0 || offsets[i] + static_cast<uint32_t>(-t.imm) <= bytes);
  }
  if (!ok) {
    g_err = "vmem apply: need a valid device, an op of the table, 1..4096 rows, 64 B..1 MiB of memory, accesses aligned and whole "
            "inside it (at or above the op's positive immediate, 4096 for offen + soffset), stride 16 for the idxen forms and 0 "
            "otherwise, and a descriptor inside the memory";
    return -2;
  }
  DeviceScope scope;
  if (const int rc = scope.enter(device)) return rc;
  hipFuncAttributes attr;
  HIP_CHECK(AllOps::apply_attributes[op](&attr));
  if (const int rc = refuse(attr, std::string("apply of ") + VMEM_OP_TABLE[op].name)) return rc;
  const size_t rows = static_cast<size_t>(n) * VMEM_WAVE;
  DevBuf dmem, doff, dregs, dout;
  HIP_CHECK(dmem.alloc(device, static_cast<size_t>(nwords) * 4));
  HIP_CHECK(doff.alloc(device, rows * 4));
  HIP_CHECK(dregs.alloc(device, rows * 16));
  HIP_CHECK(dout.alloc(device, rows * 16));
  HIP_CHECK(hipMemcpy(dmem.ptr, mem_words, static_cast<size_t>(nwords) * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(doff.ptr, offsets, rows * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dregs.ptr, regs, rows * 16, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(dout.ptr, 0, rows * 16));
  AllOps::apply[op]({static_cast<uint8_t*>(dmem.ptr), stride, num_records, static_cast<const uint32_t*>(doff.ptr),
                     static_cast<const uint32_t*>(dregs.ptr), static_cast<uint32_t*>(dout.ptr), n});
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  if (vmem_is_store(op)) HIP_CHECK(hipMemcpy(out, dmem.ptr, static_cast<size_t>(nwords) * 4, hipMemcpyDeviceToHost));
  else HIP_CHECK(hipMemcpy(out, dout.ptr, rows * 16, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
