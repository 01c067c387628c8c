// The vmem diagnostic's op table and host model, shared by csrc/vmem/vmem.hip (device and host) and by plain g++
// (tests/test_vmem_cpu.py compiles it into an answer program and holds it against an independent implementation).
//
// A vector memory instruction only moves bytes, so every op has one correct answer:
//   loads   the bytes at the lane's address, zero- or sign-extended; 1-4 registers
//   stores  the low / high byte or half of the data register, or 1-4 registers, at the lane's address; every other
//           byte of memory keeps its value
// The walks (vmem_expected) chain them: every step's address is chosen from the previous step's data.
//
// Not covered, on purpose: the typed buffer_load_format_* / tbuffer_* instructions (their format converter is a
// model of its own); misaligned accesses, an soffset that moves an access across num_records and a multi-dword
// access that straddles num_records (their rules are unmeasured here; vmem_apply() of vmem.hip exposes the last for
// probing); the LDS-DMA sub-dword forms (global_load_lds_ubyte / sbyte / ushort / sshort): no document at hand states
// how their destination is laid out, and no probe of them was run, so they are left out of the library entirely;
// scratch and LDS-aperture flat accesses.
//
// Removed after one application on an MI355X disagreed with the model, the cause unsettled: the twelve D16 loads
// (global_load_ / buffer_load_ ubyte_d16, ubyte_d16_hi, sbyte_d16, sbyte_d16_hi, short_d16, short_d16_hi).  The model
// kept the other half of the preset destination register, as the ISA text reads; the device returned it as 0
// (global_load_ubyte_d16 of byte 0x67 into 0xa5a5xxxx gave 0x00000067).  The D16 *stores* are in the list.
// Removed likewise: the LDS-DMA dwordx3 forms (global_load_lds_dwordx3, buffer_load_dwordx3 ... lds).  The model put
// lane l's 12 bytes at M0 + 12 l; 3,024 of the 3,072 words one workgroup read back over 2 launches of 2 steps differed,
// for both forms alike.  The dword and dwordx4 forms agree with M0 + lane x size and are in the test.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VMEM_HD __host__ __device__ inline
#else
#define VMEM_HD inline
#endif

constexpr int VMEM_WAVE = 64;
constexpr int VMEM_CHAINS = 4;                     // independent chains per lane
constexpr uint32_t VMEM_TABLE_BYTES = 64 * 1024;   // the loads' table
constexpr uint32_t VMEM_CELL = 64;                 // bytes a lane owns in its wave's store region
constexpr uint32_t VMEM_REGION = (VMEM_WAVE + 2) * VMEM_CELL;  // a wave's cells between two guard cells
constexpr uint32_t VMEM_STRIDE = 16;               // of the structured descriptors

enum VmemWidth {
  VW_UBYTE, VW_SBYTE, VW_USHORT, VW_SSHORT, VW_DWORD, VW_X2, VW_X3, VW_X4,
  VW_UBYTE_D16, VW_UBYTE_D16_HI, VW_SBYTE_D16, VW_SBYTE_D16_HI, VW_SHORT_D16, VW_SHORT_D16_HI,
  VMEM_WIDTHS
};
// stores: byte = VW_UBYTE, byte_d16_hi = VW_UBYTE_D16_HI, short = VW_USHORT, short_d16_hi = VW_SHORT_D16_HI

enum VmemForm {
  VF_GLOBAL,       // v[a:a+1], off
  VF_SADDR,        // v_off, s[b:b+1] offset:IMM
  VF_FLAT,         // v[a:a+1] offset:IMM
  VF_OFFEN,        // buffer: v_off, s[r:r+3], 0 offen
  VF_IDXEN,        // buffer: v_idx, structured descriptor, 0 idxen
  VF_IDXEN_OFFEN,  // buffer: v[idx, off], structured descriptor, 0 idxen offen
  VF_OFF_SOFF,     // buffer: off, s[r:r+3], s_soffset: one address for the whole wave, lane 0's
  VF_OFFEN_SOFF    // buffer: v_off, s[r:r+3], s_soffset offen offset:IMM
};

VMEM_HD constexpr int vmem_bytes(int w) {
  return w == VW_UBYTE || w == VW_SBYTE || (w >= VW_UBYTE_D16 && w <= VW_SBYTE_D16_HI) ? 1
         : w == VW_USHORT || w == VW_SSHORT || w == VW_SHORT_D16 || w == VW_SHORT_D16_HI ? 2
         : w == VW_DWORD ? 4 : w == VW_X2 ? 8 : w == VW_X3 ? 12 : 16;
}
VMEM_HD constexpr int vmem_regs(int w) { return w == VW_X2 ? 2 : w == VW_X3 ? 3 : w == VW_X4 ? 4 : 1; }

// X(name, width, form macro suffix, immediate offset, mnemonic, modifiers)
#define VMEM_LOAD_LIST(X)                                                                         \
  X(global_load_ubyte, VW_UBYTE, GLOBAL, 0, "global_load_ubyte", "")                              \
  X(global_load_sbyte, VW_SBYTE, GLOBAL, 0, "global_load_sbyte", "")                              \
  X(global_load_ushort, VW_USHORT, GLOBAL, 0, "global_load_ushort", "")                           \
  X(global_load_sshort, VW_SSHORT, GLOBAL, 0, "global_load_sshort", "")                           \
  X(global_load_dword, VW_DWORD, GLOBAL, 0, "global_load_dword", "")                              \
  X(global_load_dwordx2, VW_X2, GLOBAL, 0, "global_load_dwordx2", "")                             \
  X(global_load_dwordx3, VW_X3, GLOBAL, 0, "global_load_dwordx3", "")                             \
  X(global_load_dwordx4, VW_X4, GLOBAL, 0, "global_load_dwordx4", "")                             \
  X(global_load_dword_saddr, VW_DWORD, SADDR, 0, "global_load_dword", "")                         \
  X(global_load_dword_saddr_p4092, VW_DWORD, SADDR, 4092, "global_load_dword", "")                \
  X(global_load_dword_saddr_m4096, VW_DWORD, SADDR, -4096, "global_load_dword", "")               \
  X(global_load_dwordx4_saddr, VW_X4, SADDR, 0, "global_load_dwordx4", "")                        \
  X(global_load_dwordx4_saddr_p4092, VW_X4, SADDR, 4092, "global_load_dwordx4", "")               \
  X(global_load_dwordx4_saddr_m4096, VW_X4, SADDR, -4096, "global_load_dwordx4", "")              \
  X(global_load_dword_sc0, VW_DWORD, GLOBAL, 0, "global_load_dword", " sc0")                      \
  X(global_load_dword_sc1, VW_DWORD, GLOBAL, 0, "global_load_dword", " sc1")                      \
  X(global_load_dword_sc0_sc1, VW_DWORD, GLOBAL, 0, "global_load_dword", " sc0 sc1")              \
  X(global_load_dword_nt, VW_DWORD, GLOBAL, 0, "global_load_dword", " nt")                        \
  X(global_load_dwordx4_sc0, VW_X4, GLOBAL, 0, "global_load_dwordx4", " sc0")                     \
  X(global_load_dwordx4_sc1, VW_X4, GLOBAL, 0, "global_load_dwordx4", " sc1")                     \
  X(global_load_dwordx4_sc0_sc1, VW_X4, GLOBAL, 0, "global_load_dwordx4", " sc0 sc1")             \
  X(global_load_dwordx4_nt, VW_X4, GLOBAL, 0, "global_load_dwordx4", " nt")                       \
  X(flat_load_dword, VW_DWORD, FLAT, 0, "flat_load_dword", "")                                    \
  X(flat_load_dwordx4_p4095, VW_X4, FLAT, 4095, "flat_load_dwordx4", "")                          \
  X(buffer_load_ubyte, VW_UBYTE, OFFEN, 0, "buffer_load_ubyte", "")                               \
  X(buffer_load_sbyte, VW_SBYTE, OFFEN, 0, "buffer_load_sbyte", "")                               \
  X(buffer_load_ushort, VW_USHORT, OFFEN, 0, "buffer_load_ushort", "")                            \
  X(buffer_load_sshort, VW_SSHORT, OFFEN, 0, "buffer_load_sshort", "")                            \
  X(buffer_load_dword, VW_DWORD, OFFEN, 0, "buffer_load_dword", "")                               \
  X(buffer_load_dwordx2, VW_X2, OFFEN, 0, "buffer_load_dwordx2", "")                              \
  X(buffer_load_dwordx3, VW_X3, OFFEN, 0, "buffer_load_dwordx3", "")                              \
  X(buffer_load_dwordx4, VW_X4, OFFEN, 0, "buffer_load_dwordx4", "")                              \
  X(buffer_load_dword_idxen, VW_DWORD, IDXEN, 0, "buffer_load_dword", "")                         \
  X(buffer_load_dword_idxen_offen, VW_DWORD, IDXEN_OFFEN, 0, "buffer_load_dword", "")             \
  X(buffer_load_dword_soffset, VW_DWORD, OFF_SOFF, 0, "buffer_load_dword", "")                    \
  X(buffer_load_dword_offen_soffset_p4095, VW_DWORD, OFFEN_SOFF, 4095, "buffer_load_dword", "")

#define VMEM_STORE_LIST(X)                                                                        \
  X(global_store_byte, VW_UBYTE, GLOBAL, 0, "global_store_byte", "")                              \
  X(global_store_byte_d16_hi, VW_UBYTE_D16_HI, GLOBAL, 0, "global_store_byte_d16_hi", "")         \
  X(global_store_short, VW_USHORT, GLOBAL, 0, "global_store_short", "")                           \
  X(global_store_short_d16_hi, VW_SHORT_D16_HI, GLOBAL, 0, "global_store_short_d16_hi", "")       \
  X(global_store_dword, VW_DWORD, GLOBAL, 0, "global_store_dword", "")                            \
  X(global_store_dwordx2, VW_X2, GLOBAL, 0, "global_store_dwordx2", "")                           \
  X(global_store_dwordx3, VW_X3, GLOBAL, 0, "global_store_dwordx3", "")                           \
  X(global_store_dwordx4, VW_X4, GLOBAL, 0, "global_store_dwordx4", "")                           \
  X(global_store_dword_saddr_m8, VW_DWORD, SADDR, -8, "global_store_dword", "")                   \
  X(global_store_dword_nt, VW_DWORD, GLOBAL, 0, "global_store_dword", " nt")                      \
  X(global_store_dword_sc0_sc1, VW_DWORD, GLOBAL, 0, "global_store_dword", " sc0 sc1")            \
  X(global_store_dwordx4_nt, VW_X4, GLOBAL, 0, "global_store_dwordx4", " nt")                     \
  X(global_store_dwordx4_sc0_sc1, VW_X4, GLOBAL, 0, "global_store_dwordx4", " sc0 sc1")           \
  X(flat_store_dword, VW_DWORD, FLAT, 0, "flat_store_dword", "")                                  \
  X(buffer_store_byte, VW_UBYTE, OFFEN, 0, "buffer_store_byte", "")                               \
  X(buffer_store_byte_d16_hi, VW_UBYTE_D16_HI, OFFEN, 0, "buffer_store_byte_d16_hi", "")          \
  X(buffer_store_short, VW_USHORT, OFFEN, 0, "buffer_store_short", "")                            \
  X(buffer_store_short_d16_hi, VW_SHORT_D16_HI, OFFEN, 0, "buffer_store_short_d16_hi", "")        \
  X(buffer_store_dword, VW_DWORD, OFFEN, 0, "buffer_store_dword", "")                             \
  X(buffer_store_dwordx2, VW_X2, OFFEN, 0, "buffer_store_dwordx2", "")                            \
  X(buffer_store_dwordx3, VW_X3, OFFEN, 0, "buffer_store_dwordx3", "")                            \
  X(buffer_store_dwordx4, VW_X4, OFFEN, 0, "buffer_store_dwordx4", "")                            \
  X(buffer_store_dword_idxen, VW_DWORD, IDXEN, 0, "buffer_store_dword", "")

#define VMEM_X_ENUM(NAME, W, F, IMM, M, MODS) VO_##NAME,
enum VmemOp { VMEM_LOAD_LIST(VMEM_X_ENUM) VMEM_LOADS, VMEM_STORES_AT = VMEM_LOADS - 1, VMEM_STORE_LIST(VMEM_X_ENUM) VMEM_OPS };
#undef VMEM_X_ENUM

struct VmemOpInfo {
  const char* name;
  int width, form, imm;
  const char* insn;
  const char* mods;
};
#define VMEM_X_ROW(NAME, W, F, IMM, M, MODS) \
    {#NAME, W, VF_##F, IMM, M, MODS},
constexpr VmemOpInfo VMEM_OP_TABLE[VMEM_OPS] = {
VMEM_LOAD_LIST(VMEM_X_ROW)
VMEM_STORE_LIST(VMEM_X_ROW)
};
#undef VMEM_X_ROW

VMEM_HD constexpr bool vmem_is_store(int op) { return op >= VMEM_LOADS; }

// the 64 -> 32 bit hash of every pattern here (murmur3's finalizer)
VMEM_HD uint32_t vmem_mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return static_cast<uint32_t>(x);
}

// word `index` of a table filled under `seed`
VMEM_HD uint32_t vmem_word(uint32_t index, uint32_t seed) { return vmem_mix32((static_cast<uint64_t>(seed) << 32) | index); }
// word `index` of slice `slice` of the L1 test
VMEM_HD uint32_t vmem_l1_word(uint32_t seed, uint32_t slice, uint32_t index) {
  return vmem_mix32((static_cast<uint64_t>(seed ^ (slice * 0x9E3779B1u)) << 32) | index);
}
VMEM_HD uint32_t vmem_op_seed(uint64_t seed, int op) { return vmem_mix32(seed + 0x9E3779B97F4A7C15ULL * static_cast<uint64_t>(op + 1)); }
VMEM_HD uint32_t vmem_init(uint32_t seed, int lane, int chain) { return vmem_mix32((static_cast<uint64_t>(seed) << 32) | static_cast<uint32_t>(0x100 + lane * VMEM_CHAINS + chain)); }
VMEM_HD uint32_t vmem_const(uint32_t seed, int lane, int chain) { return vmem_mix32((static_cast<uint64_t>(seed) << 32) | static_cast<uint32_t>(0x10000 + lane * VMEM_CHAINS + chain)); }
// register j of a load's preset destination / of a store's data, chosen from the chain word
VMEM_HD uint32_t vmem_preset(uint32_t x, int j) { return x * 0x9E3779B1u + 0x7F4A7C15u * static_cast<uint32_t>(j + 1); }
VMEM_HD uint32_t vmem_step(uint32_t x, uint32_t loaded, uint32_t c) { return vmem_mix32(((static_cast<uint64_t>(x) << 32) | loaded) + c); }
VMEM_HD uint32_t vmem_fold(const uint32_t* r, int n) {
  uint32_t h = r[0];
  for (int j = 1; j < n; ++j) h = h * 0x01000193u ^ r[j];
  return h;
}

// The byte offset op `op` accesses for chain word x inside `span` bytes (the table; a lane's cell): aligned to the
// element (4 bytes for the multi-dword forms, the stride for idxen), the whole access inside the span, and far enough
// from its ends that the address parts the instruction adds up (saddr + voffset, voffset alone) lie inside it too.
VMEM_HD uint32_t vmem_off_of(int width, int form, int imm, uint32_t x, uint32_t span) {
  const uint32_t bytes = static_cast<uint32_t>(vmem_bytes(width));
  const uint32_t al = form == VF_IDXEN ? VMEM_STRIDE : bytes < 4 ? bytes : 4;
  uint32_t lo = 0, hi = span;
  if (span > VMEM_CELL) {  // the table: room for the immediates
    if (form == VF_OFFEN_SOFF) lo = 8192;
    else if (imm > 0) lo = 4096;
    else if (imm < 0) hi = span - 4096;
  }
  return lo + ((x >> 7) % ((hi - lo - bytes) / al + 1)) * al;
}
inline uint32_t vmem_off(int op, uint32_t x, uint32_t span) {  // the host's: by op index
  return vmem_off_of(VMEM_OP_TABLE[op].width, VMEM_OP_TABLE[op].form, VMEM_OP_TABLE[op].imm, x, span);
}
// the soffset of VF_OFFEN_SOFF, from lane 0's chain word: 4 k + 1, so that voffset + soffset + 4095 is aligned
VMEM_HD uint32_t vmem_soff(uint32_t x0) { return 4u * ((x0 >> 3) & 255u) + 1u; }

// One load: `mem` + off -> out[0..regs); `pre`, the registers before it, is what a skipped load leaves.
VMEM_HD void vmem_load(int width, const uint8_t* mem, uint32_t off, const uint32_t* pre, uint32_t* out) {
  (void)pre;  // no op of the list keeps a part of its destination
  const uint8_t* p = mem + off;
  const uint32_t b = p[0];
  const uint32_t h = vmem_bytes(width) >= 2 ? b | (static_cast<uint32_t>(p[1]) << 8) : 0;
  switch (width) {
    case VW_UBYTE: out[0] = b; break;
    case VW_SBYTE: out[0] = (b & 0x80u ? 0xffffff00u : 0u) | b; break;
    case VW_USHORT: out[0] = h; break;
    case VW_SSHORT: out[0] = (h & 0x8000u ? 0xffff0000u : 0u) | h; break;
    default:
      for (int j = 0; j < vmem_regs(width); ++j)
        out[j] = p[4 * j] | (static_cast<uint32_t>(p[4 * j + 1]) << 8) | (static_cast<uint32_t>(p[4 * j + 2]) << 16) |
                 (static_cast<uint32_t>(p[4 * j + 3]) << 24);
  }
}

// One store of the data registers `d` to `mem` + off: exactly vmem_bytes(width) bytes change.
VMEM_HD void vmem_store(int width, uint8_t* mem, uint32_t off, const uint32_t* d) {
  uint8_t* p = mem + off;
  switch (width) {
    case VW_UBYTE: p[0] = static_cast<uint8_t>(d[0]); break;
    case VW_UBYTE_D16_HI: p[0] = static_cast<uint8_t>(d[0] >> 16); break;
    case VW_USHORT: p[0] = static_cast<uint8_t>(d[0]), p[1] = static_cast<uint8_t>(d[0] >> 8); break;
    case VW_SHORT_D16_HI: p[0] = static_cast<uint8_t>(d[0] >> 16), p[1] = static_cast<uint8_t>(d[0] >> 24); break;
    default:
      for (int j = 0; j < vmem_regs(width); ++j)
        for (int k = 0; k < 4; ++k) p[4 * j + k] = static_cast<uint8_t>(d[j] >> (8 * k));
  }
}

// byte i of a wave's store region before the walk
VMEM_HD uint8_t vmem_background(uint32_t seed, uint32_t i) { return static_cast<uint8_t>(vmem_word(i >> 2, seed ^ 0xB6B6B6B6u) >> (8 * (i & 3))); }

// --- bounds ------------------------------------------------------------------------------------------------------
// The 16-byte slot lane `lane` accesses in round k of the bounds rows over a buffer of 2 N bytes (N a power of two
// >= 1024): even lanes walk the first half (in range), odd lanes the second (out of range), so one wave-instruction
// holds both kinds, and rounds 0..N/512-1 cover every slot of both halves once -- the last slot in range and the
// first out of range included.
VMEM_HD uint32_t vmem_bounds_rounds(uint32_t n) { return n / 512; }
VMEM_HD uint32_t vmem_bounds_slot(uint32_t n, int lane, uint32_t k) {
  const uint32_t half = n / 16;
  return static_cast<uint32_t>(lane & 1) * half + ((static_cast<uint32_t>(lane >> 1) * (half / 32) + k) % half);
}
// word i of the bounds buffer: never 0, so a wrongly served load differs from the 0 a rejected one returns
VMEM_HD uint32_t vmem_bounds_word(uint32_t seed, uint32_t i) { return vmem_word(i, seed ^ 0x0B0B0B0Bu) | 0x100u; }
// the word lane `lane` stores in round k, register j
VMEM_HD uint32_t vmem_bounds_data(uint32_t seed, int lane, uint32_t k, int j) {
  return vmem_word((k << 10) | (static_cast<uint32_t>(lane) << 2) | static_cast<uint32_t>(j), seed ^ 0x57575757u) | 0x1u;
}

// --- LDS DMA -----------------------------------------------------------------------------------------------------
// the 16-byte slot of the table lane `lane` loads from in step `it`: a per-lane permutation
VMEM_HD uint32_t vmem_dma_slot(uint32_t seed, int lane, uint32_t it) {
  return (vmem_mix32((static_cast<uint64_t>(seed) << 32) | it) + static_cast<uint32_t>(lane) * 97u) & (VMEM_TABLE_BYTES / 16 - 1);
}
// the lane whose landed bytes lane `lane` reads back
VMEM_HD int vmem_dma_partner(int lane) { return (lane + 17) & 63; }

// --- the walks, on the host ---------------------------------------------------------------------------------------
// What one wave of op `op` must end with after `iters` steps under op seed `seed` (vmem_op_seed()): words[lane * 4 +
// chain].  Loads walk `table` (VMEM_TABLE_BYTES; `touched`, when given, gets 1 in every byte a load read).  Stores
// walk a region of VMEM_REGION bytes, left in `image`.  skip_iter >= 0: the wave leaves chain 0's access out of that
// step (a load then leaves the preset registers as they were).
inline void vmem_expected(int op, uint32_t seed, int iters, int skip_iter, const uint8_t* table, uint32_t* words,
                          uint8_t* image, uint8_t* touched) {
  const VmemOpInfo& t = VMEM_OP_TABLE[op];
  const bool store = vmem_is_store(op);
  const int regs = vmem_regs(t.width);
  if (store)
    for (uint32_t i = 0; i < VMEM_REGION; ++i) image[i] = vmem_background(seed, i);
  uint32_t x[VMEM_WAVE][VMEM_CHAINS];
  for (int l = 0; l < VMEM_WAVE; ++l)
    for (int ch = 0; ch < VMEM_CHAINS; ++ch) x[l][ch] = vmem_init(seed, l, ch);
  for (int it = 0; it < iters; ++it)
    for (int ch = 0; ch < VMEM_CHAINS; ++ch) {
      const bool skipped = it == skip_iter && ch == 0;
      const uint32_t x0 = x[0][ch];  // lane 0's, for the wave-uniform address parts
      for (int l = 0; l < VMEM_WAVE; ++l) {
        const uint32_t xv = x[l][ch];
        uint32_t pre[4], r[4] = {0, 0, 0, 0};
        for (int j = 0; j < 4; ++j) pre[j] = vmem_preset(xv, j);
        uint32_t loaded;
        if (!store) {
          const uint32_t off = vmem_off(op, t.form == VF_OFF_SOFF ? x0 : xv, VMEM_TABLE_BYTES);
          if (skipped) {
            for (int j = 0; j < regs; ++j) r[j] = pre[j];
          } else {
            vmem_load(t.width, table, off, pre, r);
            if (touched) memset(touched + off, 1, static_cast<size_t>(vmem_bytes(t.width)));
          }
          loaded = vmem_fold(r, regs);
        } else {
          uint8_t* cell = image + VMEM_CELL * static_cast<uint32_t>(l + 1);
          const uint32_t off = vmem_off(op, xv, VMEM_CELL);
          if (!skipped) vmem_store(t.width, cell, off, pre);
          vmem_load(VW_X4, cell, off & ~15u, pre, r);  // the reload of the quad the store began in
          loaded = vmem_fold(r, 4);
        }
        x[l][ch] = vmem_step(xv, loaded, vmem_const(seed, l, ch));
      }
    }
  for (int l = 0; l < VMEM_WAVE; ++l)
    for (int ch = 0; ch < VMEM_CHAINS; ++ch) words[l * VMEM_CHAINS + ch] = x[l][ch];
}
