"""The cvt diagnostic on CPU: the model of csrc/cvt/cvt_ref.h (decode, scale, round) against an exact referee written
here with fractions.Fraction from the formats' definitions, hand-worked rows, the operand domain and what the shapes
reach, the C ABI of csrc/cvt/cvt.hip against ops/cvt.py and its fake, the instructions the kernels compile to, the
opt-in wiring on the fakes and the build target.  The kernels themselves run on an MI355X in tests/test_gpu_cvt.py."""
import ctypes
import functools
import inspect
import json
import math
import os
import re
import shutil
import struct
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, cvt, diag, fabric
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeCvtLib, FakeDiagLib, FakeFabricLib, c_exports, cvt_c_ops

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "cvt")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
SEEDS = (cvt.DEFAULT_SEED, 7, 0xFEEDFACE12345)
ROWS_PER_SEED = 192
DRAWS = 1 << 16

# Modes: `table` prints the op table; `shaped SEED N` per op N shaped rows with the model's answer; `eval` the model's
# answer for the rows on stdin (op a b c s); `steer` per op, over 2^16 draws, how many left the domain and how many
# results were ties (the source exactly between two neighbours of the destination's grid), subnormal, the largest
# finite number, zero, and how many packed pairs had equal halves.
REF_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "cvt_ref.h"
static void answer(int op, const CvtArgs& a) {
  CvtOut o = {{0, 0}};
  const bool ok = cvt_convert(op, a, &o);
  if (ok != cvt_in_domain(op, a)) abort();
  printf("row %d %x %x %x %x %d %x %x\n", op, a.a, a.b, a.c, a.s, ok ? 1 : 0, o.r[0], o.r[1]);
}
static void answer_wide(int op, const CvtWideArgs& a) {
  CvtWideOut o;
  for (int j = 0; j < CVT_WIDE; ++j) o.r[j] = 0;
  const bool ok = cvt_convert_wide(op, a, &o);
  if (ok != cvt_in_domain_wide(op, a)) abort();
  printf("row %d", op);
  for (int j = 0; j < CVT_WIDE; ++j) printf(" %x", a.v[j]);
  printf(" %x %d", a.s, ok ? 1 : 0);
  for (int j = 0; j < CVT_WIDE; ++j) printf(" %x", o.r[j]);
  printf("\n");
}
// one narrowing conversion of `src` (format S) over 2^k to D: a tie, a subnormal, the largest or a zero result?
static void classify(const CvtFmt& S, const CvtFmt& D, CvtRound mode, uint64_t src, int k, long* ties, long* sub, long* top,
                     long* zero) {
  CvtVal v = {false, 0, 0};
  cvt_decode(S, src, &v);
  v.e -= k;
  // a tie: exact on the grid of half units, at an odd half unit
  const CvtFmt half = {D.ebits, D.mbits + 1, D.bias, 2};
  uint64_t hc = 0, dc = 0;
  CvtVal back = {false, 0, 0};
  if (v.m && cvt_encode(half, v, CVT_RTZ, &hc) && (hc & 1)) {
    const uint64_t E = (hc >> half.mbits) & ((1ULL << half.ebits) - 1), M = hc & ((1ULL << half.mbits) - 1);
    back.m = E ? (M | (1ULL << half.mbits)) : M, back.e = static_cast<int>(E ? E : 1) - half.bias - half.mbits;
    // the same value: compare after removing trailing zeros
    uint64_t m1 = v.m, m2 = back.m;
    int e1 = v.e, e2 = back.e;
    while (m1 && !(m1 & 1)) m1 >>= 1, ++e1;
    while (m2 && !(m2 & 1)) m2 >>= 1, ++e2;
    if (m1 == m2 && e1 == e2) ++*ties;
  }
  cvt_encode(D, v, mode, &dc);
  const uint64_t mag = dc & (cvt_sign_bit(D) - 1);
  if (mag == 0) ++*zero;
  else if (mag < (1ULL << D.mbits)) ++*sub;
  if (mag == cvt_max_code(D)) ++*top;
}
// the narrowing float ops: source format, destination format, whether a scale applies; false for the others
static bool narrowing(int kind, CvtFmt* S, CvtFmt* D, bool* scaled, CvtRound* mode) {
  *scaled = false, *mode = CVT_RNE, *S = CVT_F32;
  switch (kind) {
    case CK_F16_F32: *D = CVT_F16; return true;
    case CK_PKRTZ: *D = CVT_F16, *mode = CVT_RTZ; return true;
    case CK_F32_F64: *S = CVT_F64, *D = CVT_F32; return true;
    case CK_PK_BF16_F32: *D = CVT_BF16; return true;
    case CK_PK_FP8_F32: *D = CVT_FP8; return true;
    case CK_PK_BF8_F32: *D = CVT_BF8; return true;
    case CK_S_PK_FP8_F32: *D = CVT_FP8, *scaled = true; return true;
    case CK_S_PK_BF8_F32: *D = CVT_BF8, *scaled = true; return true;
    case CK_S_PK_FP4_F32: *D = CVT_FP4, *scaled = true; return true;
    case CK_S_PK_FP8_F16: *S = CVT_F16, *D = CVT_FP8, *scaled = true; return true;
    case CK_S_PK_FP8_BF16: *S = CVT_BF16, *D = CVT_FP8, *scaled = true; return true;
    case CK_S_PK_BF8_F16: *S = CVT_F16, *D = CVT_BF8, *scaled = true; return true;
    case CK_S_PK_BF8_BF16: *S = CVT_BF16, *D = CVT_BF8, *scaled = true; return true;
    case CK_S_PK_FP4_F16: *S = CVT_F16, *D = CVT_FP4, *scaled = true; return true;
    case CK_S_PK_FP4_BF16: *S = CVT_BF16, *D = CVT_FP4, *scaled = true; return true;
    default: return false;
  }
}
int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "table")) {
    for (int op = 0; op < CVT_OPS; ++op) {
      const CvtOpInfo& t = CVT_OP_TABLE[op];
      if (t.kind != cvt_kind(op) || t.sel != cvt_sel(op)) return 3;
      printf("op %d %s %s %d %d %d\n", op, t.name, t.insn, t.group, t.kind, t.sel);
    }
  } else if (argc >= 4 && !strcmp(argv[1], "shaped")) {
    const uint64_t seed = strtoull(argv[2], nullptr, 0);
    const int n = atoi(argv[3]);
    uint32_t words[CVT_WAVE * CVT_CHAINS];
    for (int op = 0; op < CVT_OPS; ++op) {
      for (int i = 0; i < n; ++i) {
        const uint32_t w = cvt_mix32(seed + 0x9E3779B97F4A7C15ULL * (op + 1) + i);
        if (cvt_is_wide(op)) answer_wide(op, cvt_shape_wide(op, w));
        else answer(op, cvt_shape(op, w));
      }
      const bool ok = cvt_expected(op, seed, 3, words);
      uint32_t sum = 0;
      for (uint32_t w : words) sum = sum * 31u + w;
      printf("expect %d %d %x\n", op, ok ? 1 : 0, sum);
    }
  } else if (argc >= 2 && !strcmp(argv[1], "eval")) {
    int op;
    CvtArgs a;
    while (scanf("%d", &op) == 1) {
      if (op >= 0 && op < CVT_OPS && cvt_is_wide(op)) {
        CvtWideArgs wa;
        for (int j = 0; j < CVT_WIDE; ++j)
          if (scanf("%x", &wa.v[j]) != 1) return 4;
        if (scanf("%x", &wa.s) != 1) return 4;
        answer_wide(op, wa);
      } else {
        if (scanf("%x %x %x %x", &a.a, &a.b, &a.c, &a.s) != 4) return 4;
        answer(op, a);
      }
    }
  } else if (argc >= 2 && !strcmp(argv[1], "steer")) {
    for (int op = 0; op < CVT_OPS; ++op) {
      long out = 0, ties = 0, sub = 0, top = 0, zero = 0, same = 0;
      bool other = false;
      CvtFmt S = CVT_F32, D = CVT_F32;
      bool scaled;
      CvtRound mode;
      const bool nar = narrowing(cvt_kind(op), &S, &D, &scaled, &mode);
      for (int i = 0; i < (1 << 16) && cvt_is_wide(op); ++i) {  // a wide form: every one of its 32 values
        const CvtWideArgs a = cvt_shape_wide(op, cvt_mix32(0x51EE7ULL * (op + 1) + i));
        if (!cvt_in_domain_wide(op, a)) {
          ++out;
          continue;
        }
        const int kind = cvt_kind(op);
        if (!cvt_wide_narrows(kind)) continue;
        other = true;
        int k = 0;
        cvt_scale_exp(a.s, &k);
        for (int j = 0; j < CVT_WIDE; ++j)
          classify(cvt_wide_big_fmt(kind), cvt_wide_small_fmt(kind), CVT_RNE,
                   cvt_wide_big(kind) == 0 ? a.v[j] : (a.v[j / 2] >> (16 * (j & 1))) & 0xffffu, k, &ties, &sub, &top, &zero);
      }
      for (int i = 0; i < (1 << 16) && !cvt_is_wide(op); ++i) {
        const CvtArgs a = cvt_shape(op, cvt_mix32(0x51EE7ULL * (op + 1) + i));
        if (!cvt_in_domain(op, a)) {
          ++out;
          continue;
        }
        if (!nar) {
          // the conversions between floats and integers: a tie is a source exactly between two results; `top` the
          // result at a bound of the destination's range; `sub` a subnormal source; `zero` a zero result
          const int kind = cvt_kind(op);
          CvtFmt F = CVT_F32;
          CvtRound md = CVT_RTZ;
          int64_t lo = INT32_MIN, hi = INT32_MAX;
          bool to_int = true, is_signed = false;
          int ibits = 32;
          switch (kind) {
            case CK_I32_F32: break;
            case CK_FLR: md = CVT_FLOOR; break;
            case CK_RPI: md = CVT_RPI; break;
            case CK_U32_F32: lo = 0, hi = UINT32_MAX; break;
            case CK_I32_F64: F = CVT_F64; break;
            case CK_U32_F64: F = CVT_F64, lo = 0, hi = UINT32_MAX; break;
            case CK_U16_F16: F = CVT_F16, lo = 0, hi = 65535; break;
            case CK_I16_F16: F = CVT_F16, lo = -32768, hi = 32767; break;
            case CK_PK_U8: md = CVT_RNE, lo = 0, hi = 255; break;
            case CK_F32_I32: to_int = false, is_signed = true; break;
            case CK_F32_U32: to_int = false; break;
            case CK_F16_I16: to_int = false, is_signed = true, ibits = 16, F = CVT_F16; break;
            case CK_F16_U16: to_int = false, ibits = 16, F = CVT_F16; break;
            default: continue;
          }
          CvtVal v = {false, 0, 0};
          if (to_int) {
            const uint64_t src = F.mbits == 52 ? (static_cast<uint64_t>(a.b) << 32) | a.a : F.mbits == 10 ? (a.a & 0xffffu) : a.a;
            cvt_decode(F, src, &v);
            if (v.m && v.e < 0 && -v.e < 64 && (v.m & ((1ULL << -v.e) - 1)) == (1ULL << (-v.e - 1))) ++ties;
            if (v.m && (src & (cvt_sign_bit(F) - 1)) < (1ULL << F.mbits)) ++sub;
            const int64_t r = cvt_to_int(v, md, lo, hi);
            if (r == 0) ++zero;
            if (r == hi || (lo < 0 && r == lo)) ++top;
          } else {
            const uint32_t word = ibits == 16 ? (a.a & 0xffffu) : a.a;
            const int64_t i = is_signed ? (ibits == 16 ? static_cast<int16_t>(word) : static_cast<int32_t>(word)) : word;
            v.neg = i < 0, v.m = static_cast<uint64_t>(i < 0 ? -i : i), v.e = 0;
            const int sig = cvt_sig_bits(v.m);
            if (sig == F.mbits + 2) ++ties;  // one bit more than the format holds: exactly between two neighbours
            if (i == 0) ++zero;
            const int64_t most = is_signed ? (1LL << (ibits - 1)) - 1 : (1LL << ibits) - 1;
            if (i == (F.mbits == 10 && most > 65519 ? 65519 : most) || (is_signed && i == -most - 1)) ++top;
          }
          other = true;
          continue;
        }
        int k = 0;
        if (scaled) cvt_scale_exp(a.s, &k);
        const bool src16 = S.ebits + S.mbits == 15;
        const uint64_t src = S.mbits == 52 ? (static_cast<uint64_t>(a.b) << 32) | a.a : src16 ? (a.a & 0xffffu) : a.a;
        classify(S, D, mode, src, k, &ties, &sub, &top, &zero);
        if (src16 ? (a.a & 0xffffu) == (a.a >> 16) : cvt_kind(op) != CK_F16_F32 && cvt_kind(op) != CK_F32_F64 && a.a == a.b) ++same;
      }
      printf("steer %d %d %ld %ld %ld %ld %ld %ld\n", op, nar ? 1 : !other ? 0 : cvt_is_wide(op) ? 3 : 2, out, ties, sub, top, zero, same);
    }
  }
  printf("ok %d\n", CVT_OPS);
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _ref_exe(sanitize):
    """cvt_ref.h compiled with the host compiler alone into a stand-alone program: (directory object, path) or the
    compiler's complaint."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    tmp = tempfile.TemporaryDirectory()
    src, exe = os.path.join(tmp.name, "cvt_ref.cpp"), os.path.join(tmp.name, "cvt_ref")
    with open(src, "w") as f:
        f.write(REF_CPP)
    c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    if c.returncode != 0:
        return None, c.stderr
    return tmp, exe


def _run(*args, sanitize=False, stdin=None):
    tmp, exe = _ref_exe(sanitize)
    assert tmp is not None, exe
    p = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _rows(out):
    """(op, (a, b, c, s), ok, (r0, r1)) per `row` line."""
    res = []
    for ln in out.splitlines():
        f = ln.split()
        if f[0] == "row":
            n = len(f) - 3 - (32 if len(f) > 9 else 2)  # operand words: 4, or a wide form's 33
            res.append((int(f[1]), tuple(int(x, 16) for x in f[2:2 + n]), f[2 + n] == "1", tuple(int(x, 16) for x in f[3 + n:])))
    return res


def _eval(rows):
    """The C model's answer for [(op name, a, b, c, s)]: (r0, r1), or None outside the domain."""
    text = "".join(f"{cvt.OPS.index(op)} " + " ".join(f"{v:x}" for v in words) + "\n" for op, *words in rows)
    return [r if ok else None for _, _, ok, r in _rows(_run("eval", stdin=text))]


# --- the referee ---------------------------------------------------------------------------------------------------
# Written from the formats' definitions, with exact rationals: decode exactly, scale exactly, round to the
# destination's grid by the stated rule.  (ebits, mbits, bias, kind): kind 0 IEEE, 1 OCP E4M3 (only S.1111.111 is a
# NaN), 2 no special codes.
F64, F32, F16, BF16 = (11, 52, 1023, 0), (8, 23, 127, 0), (5, 10, 15, 0), (8, 7, 127, 0)
BF8, FP8, FP4, FP6, BF6 = (5, 2, 15, 0), (4, 3, 7, 1), (2, 1, 1, 2), (2, 3, 1, 2), (3, 2, 3, 2)
ONE = 0x3f800000


def _max_code(fmt):
    e, m, _, kind = fmt
    top = (1 << e) - 1
    return ((top - 1) << m | ((1 << m) - 1)) if kind == 0 else (top << m | ((1 << m) - 2)) if kind == 1 else (top << m | ((1 << m) - 1))


def dec(fmt, code):
    """(sign, exact value) of a code; None for an Inf or a NaN."""
    e, m, bias, _ = fmt
    sign, mag = code >> (e + m) & 1, code & ((1 << (e + m)) - 1)
    if mag > _max_code(fmt):
        return None
    E, M = mag >> m, mag & ((1 << m) - 1)
    v = Fraction(M, 1 << m) * Fraction(2) ** (1 - bias) if E == 0 else (1 + Fraction(M, 1 << m)) * Fraction(2) ** (E - bias)
    return sign, -v if sign else v


def enc(fmt, sign, x, mode="rne"):
    """The code of x rounded to fmt's grid (ties to even, or towards zero); None beyond the largest finite number."""
    e, m, bias, _ = fmt
    a = abs(x)
    if a == 0:
        return sign << (e + m)
    binade = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** binade > a:
        binade -= 1
    assert Fraction(2) ** binade <= a < Fraction(2) ** (binade + 1)
    q = max(binade, 1 - bias) - m  # the exponent of one unit in the last place
    scaled = a / Fraction(2) ** q
    n = math.floor(scaled)
    rest = scaled - n
    if mode == "rne" and (rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2)):
        n += 1
    if n == 1 << (m + 1):
        n, q = n >> 1, q + 1
    mag = n if n < (1 << m) else ((q + m + bias) << m) | (n - (1 << m))
    return None if mag > _max_code(fmt) else (sign << (e + m)) | mag


def _scale(s):
    if s >> 31 or s & 0x7fffff or not -8 <= (s >> 23) - 127 <= 8:
        return None
    return Fraction(2) ** ((s >> 23) - 127)


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _narrow(S, D, code, scale=Fraction(1), mode="rne"):
    d = dec(S, code)
    return None if d is None else enc(D, d[0], d[1] / scale, mode)


def _widen(S, code, scale=Fraction(1), D=F32):
    d = dec(S, code)
    return None if d is None else enc(D, d[0], d[1] * scale)


def _codes6(words):
    bits = sum(w << 32 * i for i, w in enumerate(words[:6]))
    return [bits >> 6 * j & 63 for j in range(32)]


def referee_wide(op, *words):
    """A wide form: 32 values and the scale in, 32 result words out (ops/cvt.row_words has the layout)."""
    v, scale = words[:32], _scale(words[32])
    m = re.fullmatch(r"scalef32_(2xpk16|pk32)_(\w+)_(\w+)", op)
    dst, src = m[2], m[3]
    big = {"f32": F32, "f16": F16, "bf16": BF16}
    six = {"fp6": FP6, "bf6": BF6}
    if scale is None:
        return None
    out = [0] * 32
    if src in big:  # 32 values to 32 six-bit codes in 192 bits; 2xpk16 takes them from its two blocks in turn
        vals = [v[16 * (j % 2) + j // 2] for j in range(32)] if src == "f32" else [v[j // 2] >> 16 * (j % 2) & 0xffff for j in range(32)]
        codes = [_narrow(big[src], six[dst], x, scale) for x in vals]
        if None in codes:
            return None
        bits = sum(c << 6 * j for j, c in enumerate(codes))
        out[:6] = [bits >> 32 * i & 0xffffffff for i in range(6)]
    else:
        res = [_widen(six[src], c, scale, big[dst]) for c in _codes6(v)]
        if dst == "f32":
            out = res
        else:
            out[:16] = [res[2 * i] | res[2 * i + 1] << 16 for i in range(16)]
    return tuple(out)


def referee(op, a, b, c, s, *more):
    if more:
        return referee_wide(op, a, b, c, s, *more)
    """What op must leave in its two result words, or None outside the domain (cvt_ref.h's head comment)."""
    a64 = b << 32 | a
    pair = lambda lo, hi: None if lo is None or hi is None else (lo | hi << 16, 0)
    one = lambda r: None if r is None else (r & 0xffffffff, r >> 32)
    m = re.fullmatch(r"(scalef32_)?(pk_)?(\w+?)_(\w+?)_(?:b(\d)|(lo|hi))", op)
    if op == "f16_f32":
        return one(_narrow(F32, F16, a))
    if op == "f32_f16":
        return one(_widen(F16, a & 0xffff))
    if op == "f32_bf16":
        return one(_widen(BF16, a & 0xffff))
    if op == "f32_f64":
        return one(_narrow(F64, F32, a64))
    if op == "f64_f32":
        return one(_widen(F32, a, D=F64))
    if op in ("i32_f32", "u32_f32", "i32_f64", "u32_f64", "flr_i32_f32", "u16_f16", "i16_f16"):
        d = dec({"f32": F32, "f64": F64, "f16": F16}[op[-3:]], a64 if op.endswith("f64") else a & 0xffff if op.endswith("f16") else a)
        if d is None:
            return None
        lo, hi = {"i32": (-2 ** 31, 2 ** 31 - 1), "u32": (0, 2 ** 32 - 1), "flr": (-2 ** 31, 2 ** 31 - 1), "u16": (0, 65535),
                  "i16": (-32768, 32767)}[op[:3]]
        v = _clamp(math.floor(d[1]) if op.startswith("flr") else math.trunc(d[1]), lo, hi)
        return (v & (0xffff if "16_" in op else 0xffffffff), 0)
    if op == "rpi_i32_f32":
        d = dec(F32, a)
        y = None if d is None else d[1] + Fraction(1, 2)
        if d is None or (d[1] != 0 and dec(F32, enc(F32, int(y < 0), y))[1] != y):
            return None  # x + 0.5 must be exact in fp32
        return (_clamp(math.floor(d[1] + Fraction(1, 2)), -2 ** 31, 2 ** 31 - 1) & 0xffffffff, 0)
    if op in ("f32_i32", "f32_u32", "f64_i32", "f64_u32"):
        v = a - (1 << 32) if op.endswith("i32") and a >> 31 else a
        return one(enc(F32 if op.startswith("f32") else F64, int(v < 0), Fraction(v)))
    if op in ("f16_u16", "f16_i16"):
        v = a & 0xffff
        v = v - 65536 if op.endswith("i16") and v >> 15 else v
        return one(enc(F16, int(v < 0), Fraction(v)))
    if op.startswith("f32_ubyte"):
        return one(enc(F32, 0, Fraction(a >> 8 * int(op[-1]) & 0xff)))
    if op == "off_f32_i4":
        v = a & 0xf
        return one(enc(F32, int(v >= 8), Fraction(v - 16 if v >= 8 else v, 16)))
    if op == "pkrtz_f16_f32":
        return pair(_narrow(F32, F16, a, mode="rtz"), _narrow(F32, F16, b, mode="rtz"))
    if op == "pk_bf16_f32":
        return pair(_narrow(F32, BF16, a), _narrow(F32, BF16, b))
    if op in ("pknorm_i16_f32", "pknorm_u16_f32"):
        unit, low = (32767, -1) if "i16" in op else (65535, 0)
        halves = []
        for src in (a, b):
            d = dec(F32, src)
            if d is None:
                return None
            x = d[1]
            if abs(x) < 1 and (abs(x).numerator.bit_length() > 9):  # the product must be exact in fp32
                return None
            halves.append(round(_clamp(x, low, 1) * unit) & 0xffff)  # round(): ties to even
        return pair(*halves)
    if op == "pk_u8_f32":
        d = dec(F32, a)
        if d is None or d[1] < 0 or round(d[1]) > 255:
            return None
        sh = 8 * (b & 3)
        return ((c & ~(0xff << sh) | round(d[1]) << sh) & 0xffffffff, 0)
    small = {"fp8": FP8, "bf8": BF8, "fp4": FP4}
    wide = {"f32": F32, "f16": F16, "bf16": BF16}
    half = re.fullmatch(r"scalef32_f16_(fp8|bf8)_b(\d)_(lo|hi)", op)
    if half:  # one byte of a, times the scale, into one half of c; the other half kept
        scale = _scale(s)
        r = None if scale is None else _widen(small[half[1]], a >> 8 * int(half[2]) & 0xff, scale, D=F16)
        sh = 16 * (half[3] == "hi")
        return None if r is None else ((c & ~(0xffff << sh) | r << sh) & 0xffffffff, 0)
    assert m, op
    scaled, packed, dst, src, byte, word = m.groups()
    scale = _scale(s) if scaled else Fraction(1)
    if scale is None:
        return None
    if src in wide:  # narrowing: into the low part of the selected byte / word of c, the rest of c kept
        D = small[dst]
        if src == "f32":
            lo, hi = _narrow(F32, D, a, scale), _narrow(F32, D, b, scale)
        else:  # both 16-bit sources in a
            lo, hi = _narrow(wide[src], D, a & 0xffff, scale), _narrow(wide[src], D, a >> 16, scale)
        if lo is None or hi is None:
            return None
        if D is FP4:
            sh = 8 * int(byte)
            return ((c & ~(0xff << sh) | (lo | hi << 4) << sh) & 0xffffffff, 0)
        sh = 16 * (word == "hi")
        return ((c & ~(0xffff << sh) | (lo | hi << 8) << sh) & 0xffffffff, 0)
    S, D = small[src], wide[dst]
    if not packed:
        return one(_widen(S, a >> 8 * int(byte) & 0xff, scale))
    if S is FP4:
        w = a >> 8 * int(byte) & 0xff
        lo, hi = _widen(S, w & 0xf, scale, D), _widen(S, w >> 4, scale, D)
    else:
        w = a >> 16 * (word == "hi") & 0xffff
        lo, hi = _widen(S, w & 0xff, scale, D), _widen(S, w >> 8, scale, D)
    if lo is None or hi is None:
        return None
    return (lo, hi) if D is F32 else (lo | hi << 16, 0)  # two registers of fp32, or one of two halves


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# --- the model -----------------------------------------------------------------------------------------------------

def test_the_op_table_is_the_python_one():
    table = [ln.split() for ln in _run("table").splitlines() if ln.startswith("op ")]
    assert [t[2] for t in table] == list(cvt.OPS) == cvt_c_ops() and len(set(cvt.OPS)) == len(cvt.OPS)
    groups = {name: g for g, names in enumerate(cvt.GROUPS.values()) for name in names}
    for _, k, name, insn, group, _kind, _sel in table:
        assert insn.startswith("v_cvt_") and int(group) == groups[name], name
        assert insn[6:] == re.sub(r"(_b\d)?(_lo|_hi)?$", "", name), (name, insn)  # an op is named after its instruction
    assert FakeCvtLib.OPS == len(cvt.OPS)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_model_is_the_referee_over_the_shaped_domain(seed):
    out = _run("shaped", seed, ROWS_PER_SEED)
    rows = _rows(out)
    assert len(rows) == ROWS_PER_SEED * len(cvt.OPS)
    for k, args, ok, got in rows:
        assert ok, (cvt.OPS[k], args)  # the shapes stay inside the domain
        assert referee(cvt.OPS[k], *args) == got, (cvt.OPS[k], [hex(v) for v in args], [hex(v) for v in got])
    assert len(re.findall(r"^expect \d+ 1 ", out, re.M)) == len(cvt.OPS)  # and so the chains' words exist


def _exhaustive():
    """Every source code of every op whose source has 16 bits or fewer."""
    rows = []
    for op in cvt.OPS:
        if op in ("f32_f16", "f32_bf16", "f16_u16", "f16_i16", "u16_f16", "i16_f16"):
            rows += [(op, code | 0xabcd0000, 0, 0, ONE) for code in range(1 << 16)]
        elif op.startswith("f32_ubyte") or op == "off_f32_i4":
            rows += [(op, code * 0x01010101 ^ 0x5a000000 if op != "f32_ubyte3" else code << 24 | 0x123456, 0, 0, ONE)
                     for code in range(256)]
        elif re.match(r"(scalef32_)?(pk_)?(f32|f16|bf16)_(fp8|bf8|fp4)_", op):
            for s in ((ONE,) if not op.startswith("scalef32") else (ONE, 0x3b800000, 0x43800000, 0x40000000)):
                rows += [(op, (code | (code * 7 + 3 & 0xff) << 8) * 0x00010001, 0, 0, s) for code in range(256)]
        elif re.match(r"scalef32_pk32_(f32|f16|bf16)_(fp6|bf6)", op):  # every code in every one of the 32 positions
            for sc in (ONE, 0x3b800000, 0x43800000, 0x40000000):
                for r in range(64):
                    bits = sum(((j + r) % 64) << 6 * j for j in range(32))
                    rows.append((op, *[bits >> 32 * i & 0xffffffff for i in range(6)], *[0] * 26, sc))
        elif re.match(r"scalef32_pk32_(fp6|bf6)_(f16|bf16)", op):  # the 16-bit sources, a stride of them, in every position
            for base in range(0, 1 << 16, 32 * 3):
                halves = [(base + 3 * j) & 0xffff for j in range(32)]
                rows.append((op, *[halves[2 * i] | halves[2 * i + 1] << 16 for i in range(16)], *[0] * 16, 0x40800000))
        elif re.match(r"scalef32_pk_(fp8|bf8|fp4)_(f16|bf16)_(lo|b0)", op):  # one select of each: the selects share the model's path
            rows += [(op, code | 0x3c000000, 0, 0x12345678, sc) for sc in (ONE, 0x40800000) for code in range(0, 1 << 16, 3)]
    return rows


def test_the_model_is_the_referee_on_every_code_of_the_narrow_sources():
    rows = _exhaustive()
    got = _eval(rows)
    assert len(got) == len(rows) > 6 * 65536
    nan = 0
    for row, g in zip(rows, got):
        want = referee(*row)
        assert g == want, (row[0], [hex(v) for v in row[1:]], g, want)
        nan += want is None
    assert nan > 0  # the Inf and NaN codes of f16, bf16, fp8 and bf8 are refused, by both


def test_the_model_is_numpys_cast_where_numpy_has_the_format():
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    floats = words.view(np.float32)
    keep = np.isfinite(floats)
    with np.errstate(over="ignore"):
        h = floats.astype(np.float16)
    ok16 = keep & np.isfinite(h)
    got = _eval([("f16_f32", int(w), 0, 0, ONE) for w in words[ok16]])
    assert [g[0] for g in got] == [int(v) for v in h[ok16].view(np.uint16)]
    halves = rng.integers(0, 1 << 16, 4000, dtype=np.uint32).astype(np.uint16)
    fin = np.isfinite(halves.view(np.float16))
    got = _eval([("f32_f16", int(w), 0, 0, ONE) for w in halves[fin]])
    assert [g[0] for g in got] == [int(v) for v in halves[fin].view(np.float16).astype(np.float32).view(np.uint32)]
    doubles = (rng.standard_normal(4000) * 10.0 ** rng.integers(-44, 38, 4000)).astype(np.float64)
    with np.errstate(over="ignore"):
        singles = doubles.astype(np.float32)
    fin = np.isfinite(singles)
    bits = doubles.view(np.uint64)
    got = _eval([("f32_f64", int(w) & 0xffffffff, int(w) >> 32, 0, ONE) for w in bits[fin]])
    assert [g[0] for g in got] == [int(v) for v in singles[fin].view(np.uint32)]
    got = _eval([("f64_f32", int(w), 0, 0, ONE) for w in words[keep]])
    assert [g[0] | g[1] << 32 for g in got] == [int(v) for v in floats[keep].astype(np.float64).view(np.uint64)]
    ints = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    got = _eval([("f32_i32", int(w), 0, 0, ONE) for w in ints] + [("f32_u32", int(w), 0, 0, ONE) for w in ints])
    assert [g[0] for g in got] == [int(v) for v in ints.view(np.int32).astype(np.float32).view(np.uint32)] + \
        [int(v) for v in ints.astype(np.float32).view(np.uint32)]


def test_hand_worked_rows():
    e = lambda op, a, b=0, c=0, s=ONE, *more: _eval([(op, a, b, c, s, *more)])[0]
    # f16: 11 significant bits.  2049 lies between 2048 (even) and 2050: down; 2051 between 2050 and 2052 (even): up
    assert e("f16_f32", f32(2049.0))[0] == 0x6800 and e("f16_f32", f32(2051.0))[0] == 0x6802
    assert e("f16_f32", f32(65504.0))[0] == 0x7bff and e("f16_f32", f32(65519.0))[0] == 0x7bff  # the largest; below the half unit
    assert e("f16_f32", f32(65520.0)) is None                                                  # the half unit above it: Inf
    assert e("f16_f32", f32(2.0 ** -24))[0] == 0x0001 and e("f16_f32", f32(2.0 ** -25))[0] == 0x0000  # tie to the even 0
    assert e("f16_f32", f32(1.5 * 2.0 ** -24))[0] == 0x0002                                    # tie to the even 2
    assert e("f16_f32", 0x80000000)[0] == 0x8000 and e("f16_f32", 0)[0] == 0
    assert e("pkrtz_f16_f32", f32(2051.0), f32(-2049.9))[0] == 0xe800_6801                     # both cut towards zero
    # bf16: the upper half of an fp32, ties to even
    assert e("pk_bf16_f32", 0x3f808000, 0x3f818000)[0] == 0x3f82_3f80                          # down to even, up to even
    assert e("pk_bf16_f32", 0x3f808001, 0x7f7f7fff)[0] == 0x7f7f_3f81                          # one ulp above; the largest
    assert e("pk_bf16_f32", 0x00008000, 0x80000000)[0] == 0x8000_0000                          # half the smallest subnormal
    assert e("pk_bf16_f32", 0x00018000, 0x00010000)[0] == 0x0001_0002
    assert e("f32_bf16", 0xffff0001)[0] == 0x00010000                                          # a subnormal stays one
    # f32 from f64
    d = struct.unpack("<Q", struct.pack("<d", 1.0 + 2.0 ** -24))[0]
    assert e("f32_f64", d & 0xffffffff, d >> 32)[0] == 0x3f800000                              # tie down to even
    d = struct.unpack("<Q", struct.pack("<d", 1.0 + 3 * 2.0 ** -24))[0]
    assert e("f32_f64", d & 0xffffffff, d >> 32)[0] == 0x3f800002                              # tie up to even
    d = struct.unpack("<Q", struct.pack("<d", 2.0 ** -149))[0]
    assert e("f32_f64", d & 0xffffffff, d >> 32)[0] == 1
    d = struct.unpack("<Q", struct.pack("<d", 3.4028234663852886e38))[0]                      # the largest fp32, exactly
    assert e("f32_f64", d & 0xffffffff, d >> 32)[0] == 0x7f7fffff
    assert e("f32_f64", 0, 0x80000000)[0] == 0x80000000 and e("f32_f64", 0, 0)[0] == 0     # -0, +0
    assert e("f32_f64", 0, 0x47f00000) is None                                                # 2^128: beyond the largest
    # an f64 destination holds every source exactly: the largest and the smallest fp32, +-0, the integers' extremes
    assert e("f64_f32", 0x7f7fffff) == (0xe0000000, 0x47efffff) and e("f64_f32", 0x00000001) == (0, 0x36a00000)
    assert e("f64_f32", 0x80000000) == (0, 0x80000000) and e("f64_f32", 0) == (0, 0)
    assert e("f64_i32", 0x80000000) == (0, 0xc1e00000) and e("f64_u32", 0xffffffff) == (0xffe00000, 0x41efffff)
    assert e("f64_i32", 0) == (0, 0) and e("i32_f64", 0, 0xc1e00000)[0] == 0x80000000
    # the 16-bit scalef32 forms: both sources in one register; an f16 result in the chosen half, the other kept
    assert e("scalef32_pk_fp8_f16_hi", 0x4c40_4c80, 0, 0x1111_2222)[0] == 0x5859_2222   # 18 is a number of the grid, 17 -> 16 (tie, even)
    assert e("scalef32_pk_bf8_bf16_lo", 0x40b0_4090, 0, 0x1111_2222)[0] == 0x1111_4644  # 4.5 -> 4, 5.5 -> 6 (ties to even)
    assert e("scalef32_pk_f16_fp8_lo", 0x7e38, 0, 0, f32(0.5)) == (0x5b00_3800, 0)        # 1 * 0.5, 448 * 0.5
    assert e("scalef32_pk_bf16_bf8_hi", 0x7b01_0000, 0, 0, f32(2.0)) == (0x47e0_3800, 0)  # 2^-16 * 2, 57344 * 2
    assert e("scalef32_f16_fp8_b2_hi", 0x00c00000, 0, 0xaaaa_bbbb, f32(4.0))[0] == 0xc800_bbbb   # -2 * 4 into the high half
    assert e("scalef32_f16_bf8_b1_lo", 0x7b00, 0, 0xaaaa_bbbb, f32(1.0))[0] == 0xaaaa_7b00 and \
        e("scalef32_f16_bf8_b1_lo", 0x7b00, 0, 0, f32(2.0)) is None                      # 57344 * 2 is no f16
    assert e("scalef32_pk_fp4_f16_b3", 0xc300_4100, 0, 0x00ffffff)[0] == 0xe4ff_ffff         # 2.5 -> 2, -3.5 -> -4
    assert e("scalef32_pk_bf16_fp4_b1", 0xf700, 0, 0, f32(2.0)) == (0xc140_4140, 0)       # 6 * 2, -6 * 2
    # fp6 (E2M3): 0, 0.125 .. 0.875 subnormal, 1 .. 7.5; bf6 (E3M2): 2^-4 the smallest subnormal, 28 the largest.
    # 2xpk16 takes its codes from its two blocks of 16 sources in turn
    six = lambda *codes: tuple(sum(c << 6 * j for j, c in enumerate(codes)) >> 32 * i & 0xffffffff for i in range(6))
    src = [f32(x) for x in (7.5, 0.0625, -0.0, 2.375)] + [0] * 12 + [f32(x) for x in (7.74, 0.1875, 2.125, 1.0)] + [0] * 12
    assert e("scalef32_2xpk16_fp6_f32", *src, ONE)[:6] == six(0x1f, 0x1f, 0x00, 0x02, 0x20, 0x10, 0x12, 0x08)  # 2.125 and 2.375: ties to even
    assert e("scalef32_2xpk16_fp6_f32", f32(7.75), *[0] * 31, ONE) is None               # the tie with 8: beyond 7.5
    got = e("scalef32_2xpk16_bf6_f32", *[f32(x) for x in (28.0, 2.0 ** -5, 5.5)], *[0] * 13, *[f32(x) for x in (2.0 ** -4, 4.5, -29.0)],
            *[0] * 13, ONE)
    assert got[:6] == six(0x1f, 0x01, 0x00, 0x14, 0x16, 0x3f)  # 4.5 -> 4, 5.5 -> 6, -29 -> -28
    assert e("scalef32_pk32_f32_fp6", *six(0x1f, 0x01, 0x20, 0x29), *[0] * 26, f32(2.0))[:4] == (f32(15.0), f32(0.25), 0x80000000, f32(-2.25))
    assert e("scalef32_pk32_f16_bf6", *six(0x1f, 0x01, 0x3f), *[0] * 26, f32(0.5))[:2] == (0x2800_4b00, 0x0000_cb00)   # 14, 2^-5; -14
    assert e("scalef32_pk32_fp6_bf16", 0x4010_40f0, *[0] * 31, f32(2.0))[0] == six(0x17, 0x09)[0]                      # 7.5 / 2 -> 3.75; 2.25 / 2 -> 1.125
    # fp8 (E4M3): 448 the largest, 2^-9 the smallest subnormal; bf8 (E5M2): 57344 and 2^-16
    assert e("pk_fp8_f32_lo", f32(448.0), f32(-464.0 + 2.0 ** -15), 0xaaaa5555)[0] == 0xaaaa_fe7e
    assert e("pk_fp8_f32_lo", f32(464.0))[0] == 0x007e            # the tie with 480, which E4M3 lacks: to the even 448
    assert e("pk_fp8_f32_lo", f32(464.0 + 2.0 ** -15)) is None    # above it: beyond the largest finite number
    assert e("pk_fp8_f32_hi", f32(17.0), f32(19.0), 0xaaaa5555)[0] == 0x5a58_5555               # 17 -> 16, 19 -> 20; low half kept
    assert e("pk_fp8_f32_lo", f32(2.0 ** -9), f32(2.0 ** -10))[0] == 0x0001 and e("pk_fp8_f32_lo", 0x80000000, 0)[0] == 0x0080
    assert e("pk_bf8_f32_lo", f32(57344.0), f32(2.0 ** -16))[0] == 0x017b
    assert e("pk_bf8_f32_lo", f32(4.5), f32(5.5))[0] == 0x4644 and e("pk_bf8_f32_lo", f32(2.0 ** -17), 0x80000000)[0] == 0x8000
    assert e("f32_fp8_b2", 0x007e0000)[0] == f32(448.0) and e("f32_fp8_b0", 0x7f) is None and e("f32_fp8_b0", 0x01)[0] == f32(2.0 ** -9)
    assert e("f32_bf8_b3", 0x7b000000)[0] == f32(57344.0) and e("f32_bf8_b3", 0x7c000000) is None
    assert e("pk_f32_fp8_hi", 0xc0380000) == (f32(1.0), f32(-2.0))
    # scalef32: a narrowing op divides by the scale, a widening op multiplies
    assert e("scalef32_pk_fp8_f32_hi", f32(896.0), f32(34.0), 0x1234ffff, f32(2.0))[0] == 0x587e_ffff
    assert e("scalef32_pk_f32_fp8_lo", 0x7e38, 0, 0, f32(0.5)) == (f32(0.5), f32(224.0))
    assert e("scalef32_f32_bf8_b1", 0x7b00, 0, 0, f32(256.0))[0] == f32(57344.0 * 256)
    # fp4 (E2M1): 0, 0.5, 1, 1.5, 2, 3, 4, 6.  2.5 between 2 (even code 4) and 3: down; 5 between 4 (even) and 6: down; 3.5: up
    assert e("scalef32_pk_fp4_f32_b1", f32(2.5), f32(-3.5), 0xffffffff)[0] == 0xffff_e4ff
    assert e("scalef32_pk_fp4_f32_b0", f32(6.0), f32(0.25))[0] == 0x07 and e("scalef32_pk_fp4_f32_b0", f32(7.0), 0) is None
    assert e("scalef32_pk_fp4_f32_b3", f32(0.75), 0x80000000, 0, f32(1.0))[0] == 0x8200_0000    # 0.75: tie up to the even 1.0
    assert e("scalef32_pk_f32_fp4_b2", 0x00f10000, 0, 0, f32(4.0)) == (f32(2.0), f32(-24.0))
    # integers
    assert e("i32_f32", f32(-2.9))[0] == 0xfffffffe and e("i32_f32", f32(3e9))[0] == 0x7fffffff and e("u32_f32", f32(-1.0))[0] == 0
    assert e("flr_i32_f32", f32(-2.1))[0] == 0xfffffffd and e("rpi_i32_f32", f32(2.5))[0] == 3 and e("rpi_i32_f32", f32(-2.5))[0] == 0xfffffffe
    assert e("rpi_i32_f32", f32(0.49999997)) is None                                           # x + 0.5 is not exact
    assert e("f32_i32", 0x01000001)[0] == 0x4b800000 and e("f32_i32", 0x01000003)[0] == 0x4b800002  # 2^24 + 1 down, + 3 up
    assert e("f32_u32", 0xffffffff)[0] == 0x4f800000 and e("f32_ubyte2", 0x00c80000)[0] == f32(200.0)
    assert e("off_f32_i4", 0xfff8)[0] == f32(-0.5) and e("off_f32_i4", 7)[0] == f32(0.4375)
    assert e("f16_u16", 2049)[0] == 0x6800 and e("f16_u16", 2051)[0] == 0x6802 and e("f16_i16", 0x8000)[0] == 0xf800
    assert e("f16_u16", 65520) is None and e("u16_f16", 0xbc00)[0] == 0 and e("i16_f16", 0x7bff)[0] == 0x7fff
    assert e("pknorm_i16_f32", f32(1.0), f32(-7.0))[0] == 0x8001_7fff and e("pknorm_u16_f32", f32(0.5), f32(-0.5))[0] == 0x0000_8000
    assert e("pk_u8_f32", f32(2.5), 1, 0x11223344)[0] == 0x11220244 and e("pk_u8_f32", f32(3.5), 3, 0x11223344)[0] == 0x04223344


def test_the_domain_is_refused_when_broken():
    e = lambda op, a, b=0, c=0, s=ONE: _eval([(op, a, b, c, s)])[0]
    assert e("f16_f32", f32(1e6)) is None and e("pk_bf16_f32", 0x7f7fffff, 0) is None      # overflow
    assert e("pk_fp8_f32_lo", f32(1.0), f32(500.0)) is None and e("pk_bf8_f32_hi", f32(61440.0), 0) is None
    assert e("f16_f32", 0x7fc00000) is None and e("f32_f16", 0x7e00) is None and e("i32_f32", 0x7f800000) is None  # NaN, Inf
    assert e("f32_fp8_b1", 0xff00) is None and e("scalef32_pk_f32_bf8_lo", 0x007d) is None
    ok = ("scalef32_pk_fp8_f32_lo", f32(1.0), f32(1.0), 0)
    assert e(*ok, f32(2.0)) is not None and e(*ok, f32(256.0)) is not None and e(*ok, f32(2.0 ** -8)) is not None
    for bad in (f32(3.0), f32(512.0), f32(2.0 ** -9), f32(-2.0), 0, 0x7fc00000):               # not 2^-8 .. 2^8 exactly
        assert e(*ok, bad) is None, hex(bad)
    assert e("pk_u8_f32", f32(256.0)) is None and e("pk_u8_f32", f32(-1.0)) is None
    assert e("pknorm_i16_f32", f32(0.3), 0) is None                                            # too many significant bits


def test_the_shapes_reach_the_steered_cases():
    steer = [list(map(int, ln.split()[1:])) for ln in _run("steer").splitlines() if ln.startswith("steer ")]
    assert [s[0] for s in steer] == list(range(len(cvt.OPS)))
    narrowing = converted = 0
    for k, nar, out, ties, sub, top, zero, same in steer:
        assert out == 0, cvt.OPS[k]  # over 2^16 draws no operand leaves the domain
        if nar == 1:
            narrowing += 1
            assert min(ties, sub, top, zero) > DRAWS // 64 and same == 0, (cvt.OPS[k], ties, sub, top, zero, same)
        elif nar == 3:  # a wide form that narrows: over its 32 values a draw
            narrowing += 1
            assert min(ties, sub, top, zero) > DRAWS // 64, (cvt.OPS[k], ties, sub, top, zero)
        elif nar == 2:  # between floats and integers: an integer source has no subnormal; pk_u8 and rpi are kept below
            name = cvt.OPS[k]  # their bounds (cvt_ref.h's domain), so no draw of theirs sits at one
            converted += 1
            assert ties > DRAWS // 64 and zero > 0, (name, ties, zero)
            # (u16_f16: the largest f16, 65504, lies below the destination's 65535)
            assert top > 0 or name in ("pk_u8_f32", "rpi_i32_f32", "u16_f16"), (name, top)
            assert sub > 0 or re.match(r"f(16|32)_[iu]", name) or name in ("pk_u8_f32", "rpi_i32_f32"), (name, sub)
    assert narrowing == sum(bool(re.fullmatch(r"f16_f32|f32_f64|pkrtz_f16_f32|pk_bf16_f32|(scalef32_)?pk_(fp8|bf8|fp4)_(f32|f16|bf16)_\w+|scalef32_(2xpk16|pk32)_(fp6|bf6)_\w+",
                                              k)) for k in cvt.OPS)
    assert converted == 13


def test_the_reference_is_clean_under_the_host_sanitizers():
    tmp, exe = _ref_exe(True)
    if tmp is None and re.search(r"cannot find|asan|ubsan|unrecognized", exe):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert tmp is not None, exe
    for args in (("table",), ("shaped", 7, 64), ("steer",)):
        assert _run(*args, sanitize=True).strip().endswith(f"ok {len(cvt.OPS)}")
    rows = _exhaustive()[::37] + [("pk_fp8_f32_lo", 0x7fc00000, 0x7f800000, 0, 0), ("f32_f64", 0xffffffff, 0xffffffff, 0, 0)]
    text = "".join(f"{cvt.OPS.index(op)} " + " ".join(f"{v:x}" for v in words) + "\n" for op, *words in rows)
    assert len(_rows(_run("eval", sanitize=True, stdin=text))) == len(rows)


# --- ABI -------------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("cvt"), cvt._signatures()
    assert set(exports) == set(sig) == {"cvt_last_error", "cvt_device_count", "cvt_slots", "cvt_ops", "cvt_row_words", "cvt_shape_rows",
                                        "cvt_model_rows", "cvt_test", "cvt_apply_many"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeCvtLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["cvt_test"]) == 16 and len(exports["cvt_apply_many"]) == 5


# --- instructions ----------------------------------------------------------------------------------------------

def test_every_op_compiles_to_its_native_instruction_without_scratch_or_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-save-temps",
                        os.path.join(CSRC, "cvt.hip"), "-o", os.path.join(tmp, "cvt.o")], check=True,
                       capture_output=True, text=True, cwd=tmp)
        asm = [f for f in os.listdir(tmp) if f.endswith(".s")]
        assert len(asm) == 1, os.listdir(tmp)
        with open(os.path.join(tmp, asm[0])) as f:
            text = f.read()
    chained = {int(k): body for k, body in re.findall(r"^_ZN\w*10cvt_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text, re.M | re.S)}
    applied = {int(k): body for k, body in re.findall(r"^_ZN\w*12apply_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text, re.M | re.S)}
    assert sorted(chained) == sorted(applied) == list(range(len(cvt.OPS)))
    insn = {int(t[1]): t[3] for t in (ln.split() for ln in _run("table").splitlines()) if t[0] == "op"}
    mnemonic = r"\b(v_cvt_\w+?)(?:_e32|_e64|_sdwa|_dpp)?\b"  # the compiler prints a builtin's encoding behind its name
    for k, name in enumerate(cvt.OPS):
        # its own conversion and no other: once per chain in the test's kernel, once in the one-application kernel
        found = re.findall(mnemonic, chained[k])
        if cvt.row_words_of(name) == (4, 2):
            assert found == [insn[k]] * cvt.CHAINS, (name, found)
        else:  # a form of 32 values per lane: the compiler may keep the loop over the chains rolled, whole or in halves
            assert set(found) == {insn[k]} and len(found) in (1, 2, cvt.CHAINS), (name, found)
        assert re.findall(mnemonic, applied[k]) == [insn[k]], (name, re.findall(mnemonic, applied[k]))
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {"0"}    # nor an LDS allocation


# --- wiring on the fakes ---------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, cvt_kw, **FakeDiagLib kwargs)`` -> FakeCvtLib for an n x MI355X node."""
    def install(n=1, cvt_kw=None, **kw):
        lib, clib = FakeDiagLib(n=n, **kw), FakeCvtLib(n=n, **(cvt_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(cvt, "lib", lambda: clib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return clib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}


def test_off_by_default_and_on_when_asked(node):
    clib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and clib.calls == []
    res = diag.run(1, 0, extra=("cvt",))
    assert list(res)[-1] == "cvt" and set(res) == LEVEL1 | {"cvt"} and clib.calls == ["cvt0"]
    r = res["cvt"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["iters"] == cvt.DEFAULT_ITERS
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "iters", "ops", "mode", "ms", "wall_s", "detail"}
    assert r["blocks"] == 1024 and r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["ops"]) == cvt.OPS
    assert r["mode"] == {"round": 0, "denorm": 15, "nearest_even": True, "denormals_kept": True}
    for row in r["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "gops"}
        assert row["errors"] == 0 and row["first_bad"] is None and row["gops"] > 0
    json.dumps(r)
    assert diag.run(0, 0, extra=("cvt",)).keys() == {"cvt"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("cvt" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["cvt"] and "cvt" not in diag.REFERENCE_RATES
    assert f"{len(cvt.OPS)} ops x {cvt.DEFAULT_ITERS} steps on 1024 SIMDs of 8 XCDs, round 0 denorm 15, 0 wrong words" \
        in diag._summary("cvt", r)


def test_a_wrong_word_fails_the_gpu_and_names_the_simd(node):
    op = "scalef32_pk_fp8_f32_hi"
    node(4, {"bad": {(2, cvt.OPS.index(op)): 3}})
    r = diag.run(1, 2, extra=("cvt",))["cvt"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == f"3 wrong words in {op} on xcd5/se1/cu7/simd2"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    assert r["ops"][op]["first_bad"] == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "chain": 1, "got": "0x5eedc1a7",
                                         "want": "0x5eedc0a7"}
    assert r["ops"]["f16_f32"]["errors"] == 0 and r["ops"]["f16_f32"]["first_bad"] is None
    assert diag.run(1, 1, extra=("cvt",))["cvt"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_cvt=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag cvt failed ("))
    assert f"3 wrong words in {op} on xcd5/se1/cu7/simd2" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["cvt"])
    assert "FAIL" in line and "3 wrong words" in line


def test_refused_calls_the_mode_and_the_injection_knob_of_the_fake(node):
    node(1)
    with pytest.raises(ValueError):
        cvt.cvt_test(0, ops=("f16_f32",), inject_op="f32_f16")
    with pytest.raises(ValueError):
        cvt.cvt_test(0, ops=("no_such_op",))
    with pytest.raises(ValueError):
        cvt.cvt_test(0, ops=("f16_f32", "f16_f32"))
    with pytest.raises(ValueError):
        cvt.apply_many("no_such_op", [(0, 0, 0, 0)])
    with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
        cvt.cvt_test(0, iters=0)
    with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
        cvt.cvt_test(0, ops=("f16_f32",), inject_op="f16_f32", inject_block=5000)
    r = cvt.cvt_test(0, ops=("f16_f32", "pk_bf16_f32"), inject_op="pk_bf16_f32", inject_block=0)
    assert r["errors"] == 1 and list(r["ops"]) == ["f16_f32", "pk_bf16_f32"] and r["ops"]["f16_f32"]["errors"] == 0
    node(1, {"mode": 0xf1})  # another rounding mode: the library refuses to judge, naming the field
    with pytest.raises(RuntimeError, match=r"cvt failed \(-3\).*FP_ROUND"):
        cvt.cvt_test(0)
    node(1, {"mode": 0x30})  # fp32 denormals flushed
    with pytest.raises(RuntimeError, match=r"cvt failed \(-3\).*FP_DENORM"):
        cvt.cvt_test(0)
    r = diag.run(0, 0, extra=("cvt",))["cvt"]  # ... which diag.run reports as a failed test
    assert r["pass"] is False and "FP_DENORM" in r["detail"]


def test_an_agent_cycle_publishes_it_only_when_asked(node):
    bad = {"bad": {(1, 0): 1}}
    node(2, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 2, "cvt": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=2, diag_timeout=60, diag_when="always", isolation="process",
              diag_setup=setup)
    rep = A.Agent("n2", diag_cvt=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"cvt"} and g["diag"]["cvt"]["pass"] is (d != 1), (d, g["diag"].keys())
    rep = A.Agent("n2", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"]) and rep["state"] == H.HEALTHY


def test_the_flags(node, capsys):
    clib = node(2)
    assert diag.main(["--level", "1", "--cvt", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["cvt", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(clib.calls) == ["cvt0", "cvt1"]
    assert diag.main(["--level", "1"]) == 0
    assert "cvt" not in capsys.readouterr().out and len(clib.calls) == 2
    clib = node(1)
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--cvt"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and clib.calls == ["cvt0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(clib.calls) == 1
    assert A.build_parser().parse_args(["--node", "n", "--diag-cvt"]).diag_cvt is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_cvt is False
    for main, flag in ((diag.main, "--cvt"), (node_cycle.main, "--cvt"), (A.main, "--diag-cvt")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- build -----------------------------------------------------------------------------------------------------

def test_the_build_has_a_cvt_target():
    t = B._targets()
    assert "cvt" in t and t["cvt"]["out"].endswith("libmi355x_cvt.so")
    assert t["cvt"]["cmd"] == t["xgmi"]["cmd"] and t["cvt"]["headers"][0].endswith("cvt_ref.h")
    assert [os.path.basename(h) for h in t["cvt"]["headers"]] == ["cvt_ref.h", "hip_host.h", "simd_report.h", "op_list.h"]
    assert "libmi355x_cvt.so" in B.__doc__ and "vmem,cvt" in B.__doc__
