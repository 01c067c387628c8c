// The matrix diagnostic's ops (matrix.hip) and what a correct matrix core must compute: a model of every MFMA /
// SMFMAC instruction of the table on one 64-lane wave, on raw per-lane register words.  Plain C++ that the host
// compiler takes alone: matrix.hip includes it for its kernels (the op table) and its host side (operands and
// expectation), and tests/test_matrix_cpu.py compiles it with g++ into a stand-alone program.
//
// Bit for bit without knowing the instruction's internal accumulation order or width (the exactness rule): every
// operand is an integer number of a per-format quantum, and the operands are kept so small that the sum of the
// magnitudes of every product and of C stays below 2^24 quanta (fp32 out), 2^53 (fp64 out) or 2^31 (int32 out).
// Every partial sum in any order is then an integer below that bound, exactly representable, and the result has
// one value.  matrix_apply() computes it in __int128 and refuses (-2) operands that break the bound, so the rule is
// enforced and not assumed.
//
// The operand widths at 4 chained steps per round (matrix_budget(); `units` is the largest operand magnitude in
// quanta, mbits x espan its split into significand bits and a power-of-two span for the formats whose operands are
// drawn as m << e; the sub-byte and 8-bit formats draw from every finite code of at most `units` quanta):
//
//   format        ops (K per instruction)            quantum  units            drawn as
//   fp32          32x32x2 / 16x16x4                  1        1023 / 511       mbits 10 / 9, espan 0
//   fp16          K = 8 / 16 / 32                    1        511 / 255 / 255  mbits 9 / 8 / 8, espan 0
//   fp16 sparse   16x16x32 / 32x32x16 (half kept)    1        255 / 511        as the dense op of the kept K
//   bf16          K = 8 / 16 / 32                    1        510 / 255 / 255  mbits 8 (every significand), espan 1 / 0 / 0
//   bf16 sparse   16x16x32 / 32x32x16                1        255 / 510        mbits 8, espan 0 / 1
//   int8          every K                            1        128              every code, -128 included
//   fp64          16x16x4                            1        2^24 - 1         mbits 24, espan 0
//   bf8 E5M2      every K                            2^-16    4 .. 64          every significand of the normal codes, span 16
//   bf6 E3M2      K = 64 / 128                       2^-4     4 .. 64          every significand of the normal codes, span 16
//   fp6 E2M3      K = 64 / 128                       2^-3     60               every finite code
//   fp4 E2M1      K = 64 / 128                       2^-1     12               every finite code
//   scaled ops    E8M0 scales of {2^0, 2^1} per lane, counted as a factor 4 in the bound; fp6 and fp4 keep every code
//   C             any nonzero integer of up to half the bound, in product quanta
//
// Not in the table, because one application on the device disagreed with this model and the cause was not settled:
// every op with an E4M3 (fp8) operand (sums a quantum or two off in a few elements), the 32x32 int8 ops dense and
// sparse (a few elements read exactly twice the model's), the f8f6f4 ops with two different formats and the scaled
// fp8 ones (the k order of an fp8 lane and the reach of its scale are not what the fp6 / fp4 lanes show), and the
// gfx950 sparse ops 16x16x64 / 32x32x32 (16-bit) and 16x16x128 / 32x32x64 (8-bit), whose B order or index bits differ
// from the gfx94x-era ones'.
#ifndef K8S_GPU_NODE_CHECKER_AMD_MATRIX_REF_H_
#define K8S_GPU_NODE_CHECKER_AMD_MATRIX_REF_H_

#include <cstdint>
#include <vector>

constexpr int MATRIX_WAVE = 64;
constexpr int MATRIX_STEPS = 4;   // dependent instructions per round
constexpr int MATRIX_AW = 8;      // words per lane of the A and B register blocks (the widest operand: 8 VGPRs)
constexpr int MATRIX_CW = 16;     // words per lane of the C / D register block (the 32x32 ops: 16 VGPRs)

enum MatrixFmt { MF_F32 = 0, MF_F16, MF_BF16, MF_I8, MF_F64, MF_FP8, MF_BF8, MF_FP6, MF_BF6, MF_FP4, MF_I32 };

struct MatrixFmtInfo {
  int bits, ebits, mbits, bias;  // ebits 0: a two's complement integer
};
constexpr MatrixFmtInfo matrix_fmt(int f) {
  switch (f) {
    case MF_F32: return {32, 8, 23, 127};
    case MF_F16: return {16, 5, 10, 15};
    case MF_BF16: return {16, 8, 7, 127};
    case MF_I8: return {8, 0, 0, 0};
    case MF_F64: return {64, 11, 52, 1023};
    case MF_FP8: return {8, 4, 3, 7};    // OCP E4M3: no infinity, one NaN (S.1111.111)
    case MF_BF8: return {8, 5, 2, 15};   // OCP E5M2: IEEE-like, exponent 31 is Inf / NaN
    case MF_FP6: return {6, 2, 3, 1};    // OCP E2M3: every code finite
    case MF_BF6: return {6, 3, 2, 3};    // OCP E3M2: every code finite
    case MF_FP4: return {4, 2, 1, 1};    // OCP E2M1: every code finite
    default: return {32, 0, 0, 0};       // MF_I32
  }
}

struct MatrixOpInfo {
  const char* name;
  const char* insn;  // the mnemonic the kernel must compile to
  int M, N, K;       // K: the dense K, for the sparse ops too
  int afmt, bfmt, cfmt;
  int sparse;        // 1: v_smfmac, A holds K/2 values per row and an index register names their places
  int f8f6f4;        // 1: the gfx950 f8f6f4 instruction; cbsz / blgp are its format codes of A / B
  int cbsz, blgp;
  int scaled;        // 1: v_mfma_scale_*, one E8M0 scale per lane for A and for B
};

// name and shape of op k (the index is the native op index; ops/matrix.py's OPS mirrors the names in order)
inline constexpr MatrixOpInfo MATRIX_OP_TABLE[] = {
    {"f32_32x32x2_f32", "v_mfma_f32_32x32x2_f32", 32, 32, 2, MF_F32, MF_F32, MF_F32, 0, 0, 0, 0, 0},
    {"f32_16x16x4_f32", "v_mfma_f32_16x16x4_f32", 16, 16, 4, MF_F32, MF_F32, MF_F32, 0, 0, 0, 0, 0},
    {"f32_32x32x8_f16", "v_mfma_f32_32x32x8_f16", 32, 32, 8, MF_F16, MF_F16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_16x16x16_f16", "v_mfma_f32_16x16x16_f16", 16, 16, 16, MF_F16, MF_F16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_32x32x16_f16", "v_mfma_f32_32x32x16_f16", 32, 32, 16, MF_F16, MF_F16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_16x16x32_f16", "v_mfma_f32_16x16x32_f16", 16, 16, 32, MF_F16, MF_F16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_32x32x8_bf16_1k", "v_mfma_f32_32x32x8_bf16", 32, 32, 8, MF_BF16, MF_BF16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_16x16x16_bf16_1k", "v_mfma_f32_16x16x16_bf16", 16, 16, 16, MF_BF16, MF_BF16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_32x32x16_bf16", "v_mfma_f32_32x32x16_bf16", 32, 32, 16, MF_BF16, MF_BF16, MF_F32, 0, 0, 0, 0, 0},
    {"f32_16x16x32_bf16", "v_mfma_f32_16x16x32_bf16", 16, 16, 32, MF_BF16, MF_BF16, MF_F32, 0, 0, 0, 0, 0},
    {"i32_16x16x32_i8", "v_mfma_i32_16x16x32_i8", 16, 16, 32, MF_I8, MF_I8, MF_I32, 0, 0, 0, 0, 0},
    {"i32_16x16x64_i8", "v_mfma_i32_16x16x64_i8", 16, 16, 64, MF_I8, MF_I8, MF_I32, 0, 0, 0, 0, 0},
    {"f64_16x16x4_f64", "v_mfma_f64_16x16x4_f64", 16, 16, 4, MF_F64, MF_F64, MF_F64, 0, 0, 0, 0, 0},
    {"f32_16x16x32_bf8_bf8", "v_mfma_f32_16x16x32_bf8_bf8", 16, 16, 32, MF_BF8, MF_BF8, MF_F32, 0, 0, 0, 0, 0},
    {"f32_32x32x16_bf8_bf8", "v_mfma_f32_32x32x16_bf8_bf8", 32, 32, 16, MF_BF8, MF_BF8, MF_F32, 0, 0, 0, 0, 0},
    {"f8f6f4_16x16x128_bf8", "v_mfma_f32_16x16x128_f8f6f4", 16, 16, 128, MF_BF8, MF_BF8, MF_F32, 0, 1, 1, 1, 0},
    {"f8f6f4_16x16x128_fp6", "v_mfma_f32_16x16x128_f8f6f4", 16, 16, 128, MF_FP6, MF_FP6, MF_F32, 0, 1, 2, 2, 0},
    {"f8f6f4_16x16x128_bf6", "v_mfma_f32_16x16x128_f8f6f4", 16, 16, 128, MF_BF6, MF_BF6, MF_F32, 0, 1, 3, 3, 0},
    {"f8f6f4_16x16x128_fp4", "v_mfma_f32_16x16x128_f8f6f4", 16, 16, 128, MF_FP4, MF_FP4, MF_F32, 0, 1, 4, 4, 0},
    {"f8f6f4_16x16x128_scale_fp6", "v_mfma_scale_f32_16x16x128_f8f6f4", 16, 16, 128, MF_FP6, MF_FP6, MF_F32, 0, 1, 2, 2, 1},
    {"f8f6f4_16x16x128_scale_fp4", "v_mfma_scale_f32_16x16x128_f8f6f4", 16, 16, 128, MF_FP4, MF_FP4, MF_F32, 0, 1, 4, 4, 1},
    {"f8f6f4_32x32x64_bf8", "v_mfma_f32_32x32x64_f8f6f4", 32, 32, 64, MF_BF8, MF_BF8, MF_F32, 0, 1, 1, 1, 0},
    {"f8f6f4_32x32x64_fp6", "v_mfma_f32_32x32x64_f8f6f4", 32, 32, 64, MF_FP6, MF_FP6, MF_F32, 0, 1, 2, 2, 0},
    {"f8f6f4_32x32x64_bf6", "v_mfma_f32_32x32x64_f8f6f4", 32, 32, 64, MF_BF6, MF_BF6, MF_F32, 0, 1, 3, 3, 0},
    {"f8f6f4_32x32x64_fp4", "v_mfma_f32_32x32x64_f8f6f4", 32, 32, 64, MF_FP4, MF_FP4, MF_F32, 0, 1, 4, 4, 0},
    {"f8f6f4_32x32x64_scale_fp6", "v_mfma_scale_f32_32x32x64_f8f6f4", 32, 32, 64, MF_FP6, MF_FP6, MF_F32, 0, 1, 2, 2, 1},
    {"f8f6f4_32x32x64_scale_fp4", "v_mfma_scale_f32_32x32x64_f8f6f4", 32, 32, 64, MF_FP4, MF_FP4, MF_F32, 0, 1, 4, 4, 1},
    {"smfmac_f32_16x16x32_f16", "v_smfmac_f32_16x16x32_f16", 16, 16, 32, MF_F16, MF_F16, MF_F32, 1, 0, 0, 0, 0},
    {"smfmac_f32_32x32x16_f16", "v_smfmac_f32_32x32x16_f16", 32, 32, 16, MF_F16, MF_F16, MF_F32, 1, 0, 0, 0, 0},
    {"smfmac_f32_16x16x32_bf16", "v_smfmac_f32_16x16x32_bf16", 16, 16, 32, MF_BF16, MF_BF16, MF_F32, 1, 0, 0, 0, 0},
    {"smfmac_f32_32x32x16_bf16", "v_smfmac_f32_32x32x16_bf16", 32, 32, 16, MF_BF16, MF_BF16, MF_F32, 1, 0, 0, 0, 0},
    {"smfmac_i32_16x16x64_i8", "v_smfmac_i32_16x16x64_i8", 16, 16, 64, MF_I8, MF_I8, MF_I32, 1, 0, 0, 0, 0},
    {"smfmac_f32_16x16x64_bf8_bf8", "v_smfmac_f32_16x16x64_bf8_bf8", 16, 16, 64, MF_BF8, MF_BF8, MF_F32, 1, 0, 0, 0, 0},
    {"smfmac_f32_32x32x32_bf8_bf8", "v_smfmac_f32_32x32x32_bf8_bf8", 32, 32, 32, MF_BF8, MF_BF8, MF_F32, 1, 0, 0, 0, 0},
};
constexpr int MATRIX_OPS = static_cast<int>(sizeof(MATRIX_OP_TABLE) / sizeof(MATRIX_OP_TABLE[0]));

// --- the lane maps ---------------------------------------------------------------------------------------------
// elements a lane holds of A (the kept K/2 of a sparse op), B and C/D
constexpr int matrix_a_elems(const MatrixOpInfo& o) { return o.M * o.K / MATRIX_WAVE / (o.sparse ? 2 : 1); }
constexpr int matrix_b_elems(const MatrixOpInfo& o) { return o.N * o.K / MATRIX_WAVE; }
constexpr int matrix_cd_elems(const MatrixOpInfo& o) { return o.M * o.N / MATRIX_WAVE; }
// registers (32-bit words) a lane's elements occupy: element e sits at bit e * bits of the lane's block
constexpr int matrix_a_words(const MatrixOpInfo& o) { return (matrix_a_elems(o) * matrix_fmt(o.afmt).bits + 31) / 32; }
constexpr int matrix_b_words(const MatrixOpInfo& o) { return (matrix_b_elems(o) * matrix_fmt(o.bfmt).bits + 31) / 32; }
constexpr int matrix_cd_words(const MatrixOpInfo& o) { return matrix_cd_elems(o) * matrix_fmt(o.cfmt).bits / 32; }

struct MatrixCoord {
  int row, col;  // of A: (row i, k); of B: (k, column j); of C/D: (row i, column j)
};
// A: lane l holds row l % M, and the K (sparse: K/2 kept) values of a row are dealt to the 64/M lanes of that row in
// consecutive runs: k = (l / M) * elems + e.  For a sparse op `col` is the index into the compressed row.
constexpr MatrixCoord matrix_a_coord(const MatrixOpInfo& o, int lane, int e) {
  return {lane % o.M, (lane / o.M) * matrix_a_elems(o) + e};
}
// B: the same with the column in the lane: lane l holds column l % N, k = (l / N) * elems + e
constexpr MatrixCoord matrix_b_coord(const MatrixOpInfo& o, int lane, int e) {
  return {(lane / o.N) * matrix_b_elems(o) + e, lane % o.N};
}
// C/D: the column in the lane; the rows by shape (fp64 has its own)
constexpr MatrixCoord matrix_cd_coord(const MatrixOpInfo& o, int lane, int reg) {
  if (o.cfmt == MF_F64) return {(lane >> 4) + 4 * reg, lane & 15};
  if (o.M == 16) return {4 * (lane >> 4) + reg, lane & 15};
  return {(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31};
}
// Sparse: compressed element c of a row (0 .. K/2-1) belongs to the group of four consecutive k  4 * (c / 2) .. +3,
// at the position its 2-bit field names.  A lane's index register carries one field per element it holds, element e
// in bits 2e+1:2e (cbsz = abid = 0: the low 8, 16 or 32 bits are used).
constexpr int matrix_sparse_k(int c, uint32_t idx_word, int e) { return 4 * (c / 2) + static_cast<int>((idx_word >> (2 * e)) & 3u); }

// --- decoders --------------------------------------------------------------------------------------------------
struct MatrixVal {
  int64_t m;  // the value is m * 2^e exactly
  int e;
};
// bits [off, off + n) of a lane's register block
inline uint64_t matrix_bits(const uint32_t* w, int off, int n) {
  uint64_t v = 0;
  for (int b = 0; b < n; ++b) v |= static_cast<uint64_t>((w[(off + b) >> 5] >> ((off + b) & 31)) & 1u) << b;
  return v;
}
// code -> value; false for NaN / Inf
inline bool matrix_decode(int fmt, uint64_t code, MatrixVal* v) {
  const MatrixFmtInfo f = matrix_fmt(fmt);
  if (f.ebits == 0) {  // two's complement
    const int sh = 64 - f.bits;
    v->m = static_cast<int64_t>(code << sh) >> sh;
    v->e = 0;
    return true;
  }
  const uint64_t frac = code & ((1ULL << f.mbits) - 1);
  const int ex = static_cast<int>((code >> f.mbits) & ((1ULL << f.ebits) - 1));
  const bool neg = (code >> (f.bits - 1)) & 1;
  const int top = (1 << f.ebits) - 1;
  if (fmt == MF_FP8) {
    if (ex == top && frac == 7) return false;
  } else if (fmt != MF_FP6 && fmt != MF_BF6 && fmt != MF_FP4) {
    if (ex == top) return false;
  }
  // subnormal: frac * 2^(1 - bias - mbits); normal: (1.frac) * 2^(ex - bias)
  const int64_t mag = static_cast<int64_t>(ex == 0 ? frac : frac | (1ULL << f.mbits));
  v->m = neg ? -mag : mag;
  v->e = (ex == 0 ? 1 : ex) - f.bias - f.mbits;
  while (v->m && !(v->m & 1)) v->m /= 2, ++v->e;  // the odd significand: products of two stay far inside 64 bits
  return true;
}
// the E8M0 block scale: 2^(code - 127); 255 is NaN
inline bool matrix_decode_e8m0(uint32_t code, int* e) {
  *e = static_cast<int>(code & 0xffu) - 127;
  return (code & 0xffu) != 0xffu;
}
// mag * 2^e (mag != 0) as a normal number of a float format, exactly; false where it has no such encoding
inline bool matrix_encode(int fmt, bool neg, unsigned __int128 mag, int e, uint64_t* code) {
  const MatrixFmtInfo f = matrix_fmt(fmt);
  int p = 127;
  while (p > 0 && !((mag >> p) & 1)) --p;
  if (p > f.mbits) {
    const int s = p - f.mbits;
    if (mag & ((static_cast<unsigned __int128>(1) << s) - 1)) return false;  // more significant bits than the format has
    mag >>= s, e += s;
  } else {
    mag <<= f.mbits - p, e -= f.mbits - p;
  }
  const int ex = e + f.mbits + f.bias;
  if (ex < 1 || ex >= (1 << f.ebits) - 1) return false;
  *code = (static_cast<uint64_t>(neg) << (f.bits - 1)) | (static_cast<uint64_t>(ex) << f.mbits) |
          (static_cast<uint64_t>(mag) & ((1ULL << f.mbits) - 1));
  return true;
}

// the bound of the exactness rule, in quanta
constexpr int64_t matrix_limit(const MatrixOpInfo& o) {
  return o.cfmt == MF_F64 ? (1LL << 53) : o.cfmt == MF_I32 ? (1LL << 31) : (1LL << 24);
}

// --- one instruction -------------------------------------------------------------------------------------------
// One wave's instruction on raw per-lane register words: A and B hold MATRIX_AW words per lane (lane l's block at
// l * MATRIX_AW), C and D MATRIX_CW words per lane; idx (sparse ops) and scale_a / scale_b (scaled ops: byte 0 is the
// E8M0 code) one word per lane, ignored (may be null) otherwise.  0, or: -1 an operand is NaN / Inf, -2 the sum of
// magnitudes breaks the exactness bound (the result would depend on the hardware's order), -3 the exponents span
// too far for the exact sum, -4 the result has no exact encoding.
inline int matrix_apply(int op, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* idx,
                        const uint32_t* scale_a, const uint32_t* scale_b, uint32_t* D) {
  const MatrixOpInfo& o = MATRIX_OP_TABLE[op];
  const int ea = matrix_a_elems(o), eb = matrix_b_elems(o), ec = matrix_cd_elems(o);
  const int ka = o.sparse ? o.K / 2 : o.K;  // products per output element
  const int abits = matrix_fmt(o.afmt).bits, bbits = matrix_fmt(o.bfmt).bits;
  std::vector<MatrixVal> a(o.M * ka), b(o.K * o.N);  // a[i * ka + c], b[k * N + j]
  std::vector<int> ak(o.M * ka);                      // the dense k of a[i * ka + c]
  for (int l = 0; l < MATRIX_WAVE; ++l) {
    int sa = 0, sb = 0;
    if (o.scaled && (!matrix_decode_e8m0(scale_a[l], &sa) || !matrix_decode_e8m0(scale_b[l], &sb))) return -1;
    for (int e = 0; e < ea; ++e) {
      const MatrixCoord c = matrix_a_coord(o, l, e);
      MatrixVal v;
      if (!matrix_decode(o.afmt, matrix_bits(A + l * MATRIX_AW, e * abits, abits), &v)) return -1;
      v.e += sa;  // a lane's scale covers the elements that lane holds
      a[c.row * ka + c.col] = v;
      ak[c.row * ka + c.col] = o.sparse ? matrix_sparse_k(c.col, idx[l], e) : c.col;
    }
    for (int e = 0; e < eb; ++e) {
      const MatrixCoord c = matrix_b_coord(o, l, e);
      MatrixVal v;
      if (!matrix_decode(o.bfmt, matrix_bits(B + l * MATRIX_AW, e * bbits, bbits), &v)) return -1;
      v.e += sb;
      b[c.row * o.N + c.col] = v;
    }
  }
  const int cbits = matrix_fmt(o.cfmt).bits, cw = cbits / 32;
  const int64_t limit = matrix_limit(o);
  for (int l = 0; l < MATRIX_WAVE; ++l) {
    for (int r = 0; r < ec; ++r) {
      const MatrixCoord rc = matrix_cd_coord(o, l, r);
      MatrixVal t[129];
      int n = 0;
      if (!matrix_decode(o.cfmt, matrix_bits(C + l * MATRIX_CW, r * cbits, cbits), &t[n])) return -1;
      n += t[n].m != 0;
      for (int c = 0; c < ka; ++c) {
        const MatrixVal& x = a[rc.row * ka + c];
        const MatrixVal& y = b[ak[rc.row * ka + c] * o.N + rc.col];
        const __int128 wide = static_cast<__int128>(x.m) * y.m;
        if (wide != static_cast<int64_t>(wide)) return -3;
        t[n] = {static_cast<int64_t>(wide), x.e + y.e};
        n += t[n].m != 0;
      }
      // the quantum of this element: the largest power of two that divides every term
      int emin = 0;
      for (int i = 0; i < n; ++i) {
        while (!(t[i].m & 1)) t[i].m /= 2, ++t[i].e;
        emin = i == 0 || t[i].e < emin ? t[i].e : emin;
      }
      __int128 sum = 0;
      unsigned __int128 mags = 0;
      for (int i = 0; i < n; ++i) {
        if (t[i].e - emin > 60) return -3;
        const __int128 term = static_cast<__int128>(t[i].m) * (static_cast<__int128>(1) << (t[i].e - emin));
        sum += term;
        mags += static_cast<unsigned __int128>(term < 0 ? -term : term);
      }
      if (mags >= static_cast<unsigned __int128>(limit)) return -2;
      uint64_t code = 0;
      if (o.cfmt == MF_I32) {
        code = static_cast<uint32_t>(static_cast<int64_t>(sum));
      } else if (sum != 0 && !matrix_encode(o.cfmt, sum < 0, static_cast<unsigned __int128>(sum < 0 ? -sum : sum), emin, &code)) {
        return -4;
      }
      D[l * MATRIX_CW + r * cw] = static_cast<uint32_t>(code);
      if (cw == 2) D[l * MATRIX_CW + r * cw + 1] = static_cast<uint32_t>(code >> 32);
    }
  }
  return 0;
}

// --- operands and expectation ----------------------------------------------------------------------------------
inline uint64_t matrix_hash(uint64_t seed, uint64_t op, uint64_t stream, uint64_t i) {  // splitmix64 of a counter
  uint64_t x = seed + 0x9E3779B97F4A7C15ULL * (1 + i + (stream << 24) + (op << 40));
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

// the smallest magnitude step of a format's operands: 2^qexp (the sub-byte and 8-bit floats: their subnormal step)
constexpr int matrix_qexp(int fmt) {
  const MatrixFmtInfo f = matrix_fmt(fmt);
  return (fmt == MF_FP8 || fmt == MF_BF8 || fmt == MF_FP6 || fmt == MF_BF6 || fmt == MF_FP4) ? 1 - f.bias - f.mbits : 0;
}
// The 8-bit floats and bf6 reach further down than the matrix cores keep apart inside one instruction: with their
// subnormals next to their large codes the device's sums came out a quantum or two off the exact ones (measured).
// Their operands are therefore normal codes only, over a span of 16: lo = the smallest normal's units, hi = 16 lo.
constexpr bool matrix_wide_exp(int fmt) { return fmt == MF_FP8 || fmt == MF_BF8 || fmt == MF_BF6; }
constexpr int64_t matrix_lo_units(int fmt) { return matrix_wide_exp(fmt) ? 1LL << matrix_fmt(fmt).mbits : 0; }
constexpr bool matrix_by_code(int fmt) { return matrix_fmt(fmt).bits <= 8; }  // operands drawn from the codes themselves
// the largest finite magnitude of a by-code format, in quanta
inline int64_t matrix_full_units(int fmt) {
  int64_t best = 0;
  for (uint64_t c = 0; c < (1ULL << matrix_fmt(fmt).bits); ++c) {
    MatrixVal v;
    if (!matrix_decode(fmt, c, &v)) continue;
    const int64_t u = (v.m < 0 ? -v.m : v.m) << (v.e - matrix_qexp(fmt));
    best = u > best ? u : best;
  }
  return best;
}

struct MatrixBudget {
  int64_t units_a, units_b;  // the largest operand magnitude, in quanta of its format
  int mbits_a, espan_a, mbits_b, espan_b;  // m << e with m < 2^mbits, e <= espan (by-code formats: of the units)
  int64_t cmax;              // |C| <= cmax product quanta
  int qexp;                  // a product quantum is 2^qexp
  int scale_span;            // the scales are 2^0 .. 2^scale_span
};
inline int64_t matrix_isqrt(int64_t x) {
  int64_t r = 0;
  for (int64_t bit = 1LL << 31; bit; bit >>= 1)
    if ((r + bit) * (r + bit) <= x) r += bit;
  return r;
}
inline void matrix_split(int fmt, int64_t units, int* mbits, int* espan) {
  const int sig = matrix_fmt(fmt).ebits ? matrix_fmt(fmt).mbits + 1 : 8;
  int mb = 0;
  while (mb < sig && (1LL << (mb + 1)) - 1 <= units) ++mb;
  int es = 0;
  while (es < 8 && (((1LL << mb) - 1) << (es + 1)) <= units) ++es;
  *mbits = mb, *espan = es;
}
// The widest operands that fit the bound at MATRIX_STEPS chained steps: half the bound is C's, the other half is
// shared by steps x products-per-element x the scales' largest factor, and what is left is units_a * units_b.
// `widen` doubles the operands that many times (the tests' deliberately too-wide set): -2 when they no longer fit.
inline int matrix_budget(int op, int widen, MatrixBudget* g) {
  const MatrixOpInfo& o = MATRIX_OP_TABLE[op];
  const int64_t limit = matrix_limit(o);
  const int ka = o.sparse ? o.K / 2 : o.K;
  g->scale_span = o.scaled ? 1 : 0;
  const int64_t scale = 1LL << (2 * g->scale_span);
  g->cmax = limit / 2 - 1;
  const int64_t p = (limit / 2) / (MATRIX_STEPS * ka * scale);
  const int64_t big = 1LL << 40;
  const int64_t full_a = matrix_by_code(o.afmt) ? matrix_full_units(o.afmt) : big;
  const int64_t full_b = matrix_by_code(o.bfmt) ? matrix_full_units(o.bfmt) : big;
  const int64_t root = matrix_isqrt(p);
  const int64_t cap_a = matrix_wide_exp(o.afmt) ? 16 * matrix_lo_units(o.afmt) : big;
  const int64_t cap_b = matrix_wide_exp(o.bfmt) ? 16 * matrix_lo_units(o.bfmt) : big;
  int64_t ua = full_a < root ? full_a : root;
  int64_t ub = full_b < p / ua ? full_b : p / ua;
  ua = full_a < p / ub ? full_a : p / ub;
  ua = ua < cap_a ? ua : cap_a, ub = ub < cap_b ? ub : cap_b;
  matrix_split(o.afmt, ua, &g->mbits_a, &g->espan_a);
  matrix_split(o.bfmt, ub, &g->mbits_b, &g->espan_b);
  if (!matrix_by_code(o.afmt)) ua = ((1LL << g->mbits_a) - 1) << g->espan_a;
  if (!matrix_by_code(o.bfmt)) ub = ((1LL << g->mbits_b) - 1) << g->espan_b;
  g->units_a = ua << widen, g->units_b = ub << widen;
  g->espan_a += widen, g->espan_b += widen;
  g->qexp = matrix_qexp(o.afmt) + matrix_qexp(o.bfmt);
  const __int128 worst = static_cast<__int128>(MATRIX_STEPS) * ka * scale * g->units_a * g->units_b + g->cmax;
  return worst < limit ? 0 : -2;
}

struct MatrixOperands {
  uint32_t A[MATRIX_STEPS][MATRIX_WAVE * MATRIX_AW], B[MATRIX_STEPS][MATRIX_WAVE * MATRIX_AW];
  uint32_t idx[MATRIX_STEPS][MATRIX_WAVE], scale_a[MATRIX_STEPS][MATRIX_WAVE], scale_b[MATRIX_STEPS][MATRIX_WAVE];
  uint32_t C[MATRIX_WAVE * MATRIX_CW];
  uint32_t D[MATRIX_WAVE * MATRIX_CW];  // matrix_expect(): the accumulator after the round
};

// One operand's draws: by-code formats draw among the finite codes of at most `units` quanta, the others encode
// (m << e) with m of mbits bits and e <= espan.
struct MatrixDraw {
  int fmt, mbits, espan, n = 0;
  uint64_t ok[256];
  MatrixDraw(int fmt_, int64_t units, int mbits_, int espan_) : fmt(fmt_), mbits(mbits_), espan(espan_) {
    if (!matrix_by_code(fmt)) return;
    for (uint64_t c = 0; c < (1ULL << matrix_fmt(fmt).bits); ++c) {
      MatrixVal v;
      if (!matrix_decode(fmt, c, &v)) continue;
      const int64_t u = (v.m < 0 ? -v.m : v.m) << (v.e - matrix_qexp(fmt));
      if (u <= units && u >= matrix_lo_units(fmt)) ok[n++] = c;
    }
  }
  uint64_t operator()(uint64_t h) const {
    if (n) return ok[h % static_cast<uint64_t>(n)];
    const uint64_t m = 1 + (h >> 8) % ((1ULL << mbits) - 1);
    uint64_t code = 0;
    matrix_encode(fmt, h & 1, m, static_cast<int>((h >> 1) % static_cast<uint64_t>(espan + 1)), &code);
    return code;
  }
};
inline void matrix_put(uint32_t* w, int off, int n, uint64_t code) {
  for (int b = 0; b < n; ++b)
    if ((code >> b) & 1) w[(off + b) >> 5] |= 1u << ((off + b) & 31);
}

// The operands of the chained test, op `op` under `seed`: MATRIX_STEPS sets of A, B (and idx, scales) and one C.
// `attempt` moves every draw (matrix_expect()'s redraw).  0, or matrix_budget()'s -2.
inline int matrix_operands(int op, uint64_t seed, int widen, int attempt, MatrixOperands* out) {
  const MatrixOpInfo& o = MATRIX_OP_TABLE[op];
  MatrixBudget g;
  if (const int rc = matrix_budget(op, widen, &g)) return rc;
  const uint64_t s = seed + 0x632BE59BD9B4E019ULL * static_cast<uint64_t>(attempt);
  const int ea = matrix_a_elems(o), eb = matrix_b_elems(o), ec = matrix_cd_elems(o);
  const int abits = matrix_fmt(o.afmt).bits, bbits = matrix_fmt(o.bfmt).bits, cbits = matrix_fmt(o.cfmt).bits;
  *out = MatrixOperands();
  const MatrixDraw draw_a(o.afmt, g.units_a, g.mbits_a, g.espan_a), draw_b(o.bfmt, g.units_b, g.mbits_b, g.espan_b);
  static const uint32_t pairs[6] = {0 | 1 << 2, 0 | 2 << 2, 0 | 3 << 2, 1 | 2 << 2, 1 | 3 << 2, 2 | 3 << 2};  // low < high
  for (int st = 0; st < MATRIX_STEPS; ++st) {
    for (int l = 0; l < MATRIX_WAVE; ++l) {
      for (int e = 0; e < ea; ++e)
        matrix_put(out->A[st] + l * MATRIX_AW, e * abits, abits,
                   draw_a(matrix_hash(s, op, st, l * 64 + e)));
      for (int e = 0; e < eb; ++e)
        matrix_put(out->B[st] + l * MATRIX_AW, e * bbits, bbits,
                   draw_b(matrix_hash(s, op, 8 + st, l * 64 + e)));
      if (o.sparse) {
        // two kept values per group of four, the lower position first; the bits the lane does not use carry noise
        uint32_t w = static_cast<uint32_t>(matrix_hash(s, op, 16 + st, l * 64 + 63));
        for (int pr = 0; pr < ea / 2; ++pr) {
          w &= ~(0xfu << (4 * pr));
          w |= pairs[matrix_hash(s, op, 16 + st, l * 64 + pr) % 6] << (4 * pr);
        }
        out->idx[st][l] = w;
      }
      if (o.scaled) {
        // byte 0 is the scale (op_sel 0); the other bytes carry noise
        const uint64_t h = matrix_hash(s, op, 24 + st, l);
        out->scale_a[st][l] = (static_cast<uint32_t>(h) & ~0xffu) | (127u + ((h >> 32) % (g.scale_span + 1)));
        out->scale_b[st][l] = (static_cast<uint32_t>(h >> 8) & ~0xffu) | (127u + ((h >> 40) % (g.scale_span + 1)));
      }
    }
  }
  for (int l = 0; l < MATRIX_WAVE; ++l) {
    for (int r = 0; r < ec; ++r) {
      const uint64_t h = matrix_hash(s, op, 32, l * 64 + r);
      const uint64_t c = 1 + (h >> 1) % static_cast<uint64_t>(g.cmax);
      uint64_t code = 0;
      if (o.cfmt == MF_I32)
        code = static_cast<uint32_t>((h & 1) ? -static_cast<int64_t>(c) : static_cast<int64_t>(c));
      else
        matrix_encode(o.cfmt, h & 1, c, g.qexp, &code);
      matrix_put(out->C + l * MATRIX_CW, r * cbits, cbits, code);
    }
  }
  return 0;
}

// The operands and the accumulator a correct SIMD holds after one round (out->D): acc = C; for s: acc = op(A_s, B_s,
// acc).  An operand set that leaves a zero anywhere in D is drawn again, so the sign of zero never decides a compare.
// skip_step >= 0 leaves that step out (what the self-test's skipped MFMA leaves behind).  The number of draws (>= 1),
// or a negative code of matrix_budget() / matrix_apply().
inline int matrix_expect(int op, uint64_t seed, int widen, int skip_step, MatrixOperands* out) {
  const MatrixOpInfo& o = MATRIX_OP_TABLE[op];
  for (int attempt = 0; attempt < 16; ++attempt) {
    if (const int rc = matrix_operands(op, seed, widen, attempt, out)) return rc;
    uint32_t acc[MATRIX_WAVE * MATRIX_CW], next[MATRIX_WAVE * MATRIX_CW] = {};
    for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) acc[i] = out->C[i];
    for (int st = 0; st < MATRIX_STEPS; ++st) {
      if (st == skip_step) continue;
      if (const int rc = matrix_apply(op, out->A[st], out->B[st], acc, out->idx[st], out->scale_a[st], out->scale_b[st], next))
        return rc;
      for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) acc[i] = next[i];
    }
    bool zero = false;
    const int cw = matrix_fmt(o.cfmt).bits / 32;
    for (int l = 0; l < MATRIX_WAVE; ++l)
      for (int r = 0; r < matrix_cd_elems(o); ++r) {
        uint32_t any = 0;  // the element's words without a float's sign bit
        for (int w = 0; w < cw; ++w)
          any |= acc[l * MATRIX_CW + r * cw + w] & (w == cw - 1 && o.cfmt != MF_I32 ? 0x7fffffffu : ~0u);
        zero |= any == 0;
      }
    if (zero) continue;
    for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) out->D[i] = acc[i];
    return attempt + 1;
  }
  return -5;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_MATRIX_REF_H_
