"""The scalar diagnostic on CPU: the model of csrc/scalar/scalar_ref.h against an independent big-integer
implementation written here and against rows worked by hand from the ISA's rules, the condition that no op's chain
hides a step that did not happen, the patterns of the SGPR and scalar-load parts, the C ABI of csrc/scalar/scalar.hip
against ops/scalar.py and its fake, the opt-in wiring (ops/diag.run(extra=...), the CLIs, whole agent cycles) and the
build target.  The kernels themselves run on an MI355X in tests/test_gpu_scalar.py."""
import ctypes
import functools
import inspect
import json
import os
import random
import re
import shutil
import subprocess
import tempfile

import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, atomics, diag, fabric, lanes, scalar
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeAtomicsLib, FakeDiagLib, FakeFabricLib, FakeLanesLib,
                                                          FakeScalarLib, c_exports, scalar_model)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "scalar")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
M32, M64 = 0xffffffff, (1 << 64) - 1
SEED = 0x5CA1A


# --- 1. the reference header, alone under the host compiler ----------------------------------------------------

# Prints the op table, whether a skipped step shows for every op (iters 8, skip 0 / 1 / 7), a checksum of the expected
# words, samples of the two patterns, then answers "op a b scc" lines from stdin with "r result scc".
REF_CPP = r"""
#include <cinttypes>
#include <cstdio>
#include "scalar_ref.h"

int main() {
  for (int op = 0; op < SCALAR_OPS; ++op) {
    printf("op %d %s\n", op, SCALAR_OP_TABLE[op].name);
    const int iters = 8, skips[3] = {0, 1, iters - 1};
    uint32_t want[SCALAR_CHAINS], got[SCALAR_CHAINS];
    scalar_expected(op, 0x5CA1A, iters, -1, want);
    for (int s : skips) {
      scalar_expected(op, 0x5CA1A, iters, s, got);
      int differ = 0;
      for (int i = 0; i < SCALAR_CHAINS; ++i) differ += got[i] != want[i];
      printf("skip %d %d %d\n", op, s, differ);
    }
    printf("expect %d %u %u %u %u\n", op, want[0], want[1], want[2], want[3]);
  }
  for (int k = 0; k < SCALAR_SMEM_KINDS; ++k) printf("kind %d %s %d\n", k, SCALAR_SMEM_TABLE[k].name, SCALAR_SMEM_TABLE[k].words);
  for (uint64_t seed = 1; seed <= 2; ++seed)
    for (uint32_t wave = 0; wave < 64; ++wave)
      for (int reg = 0; reg < 128; ++reg)
        printf("sgpr %" PRIu64 " %u %d %u\n", seed, wave, reg, scalar_sgpr_word(scalar_sgpr_key(seed, wave), reg));
  for (uint32_t i = 0; i < 1024; ++i) printf("smem %u %u\n", i, scalar_smem_word(7u, i));
  for (uint32_t wave = 0; wave < 8; ++wave)
    for (uint32_t k = 0; k < 64; ++k)
      printf("index %u %u %u %u\n", wave, k, scalar_smem_index(k, 0, 0, 4, 256),
             scalar_smem_index(k, scalar_mix32(wave), scalar_smem_stride(wave), 16, 1024));
  printf("ok %d\n", SCALAR_OPS);
  fflush(stdout);
  int op, scc;
  unsigned long long a, b;
  while (scanf("%d %llx %llx %d", &op, &a, &b, &scc) == 4) {
    const ScalarOut o = scalar_apply(op, a, b, static_cast<uint32_t>(scc));
    printf("r %" PRIx64 " %u\n", o.result, o.scc);
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _ref_program(sanitize, stdin=""):
    """scalar_ref.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "scalar_ref.cpp"), os.path.join(tmp, "scalar_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


# the operand set: the edge values, the shift and field operands, and 64 seeded random pairs; both values of SCC
EDGES32 = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)
EDGES_A = EDGES32 + (0x7fffffffffffffff, 0x8000000000000000, M64, 0x100000000, 0xffffffff00000000)
SHIFTS = (0, 31, 32, 63, 64)
FIELDS = tuple(off | (w << 16) for off in SHIFTS for w in (0, 1, 32, 64))
EDGES_B = EDGES_A + SHIFTS + FIELDS + (0x00050003, 0x0008001c, 0x00100038)


@functools.lru_cache(maxsize=None)
def operands():
    rng = random.Random(SEED)
    rows = [(a, b, scc) for a in EDGES_A for b in EDGES_B for scc in (0, 1)]
    rows += [(rng.getrandbits(64), rng.getrandbits(64), i & 1) for i in range(64)]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _model():
    """The driver's output parsed: names, {(op, skip): differing words}, {op: expected words}, load kinds, the
    pattern samples, and {(op index, row index): (result, scc)} for every op on operands()."""
    stdin = "".join(f"{k} {a:x} {b:x} {scc}\n" for k in range(len(scalar.OPS)) for a, b, scc in operands())
    rc, out = _ref_program(False, stdin)
    assert rc == 0 and f"\nok {len(scalar.OPS)}\n" in out, out[-2000:]
    names, skips, expect, kinds, sgpr, smem, index, answers = {}, {}, {}, [], {}, {}, [], []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "op":
            names[int(f[1])] = f[2]
        elif f[0] == "skip":
            skips[(names[int(f[1])], int(f[2]))] = int(f[3])
        elif f[0] == "expect":
            expect[names[int(f[1])]] = [int(v) for v in f[2:]]
        elif f[0] == "kind":
            kinds.append((f[2], int(f[3])))
        elif f[0] == "sgpr":
            sgpr[(int(f[1]), int(f[2]), int(f[3]))] = int(f[4])
        elif f[0] == "smem":
            smem[int(f[1])] = int(f[2])
        elif f[0] == "index":
            index.append(tuple(int(v) for v in f[1:]))
        elif f[0] == "r":
            answers.append((int(f[1], 16), int(f[2])))
    n = len(operands())
    assert len(answers) == n * len(scalar.OPS)
    applied = {(k, i): answers[k * n + i] for k in range(len(scalar.OPS)) for i in range(n)}
    return names, skips, expect, kinds, sgpr, smem, index, applied


def test_the_op_table_is_the_python_one_and_every_name_is_distinct():
    names = _model()[0]
    assert tuple(names[k] for k in range(len(names))) == scalar.OPS
    assert len(set(scalar.OPS)) == len(scalar.OPS) == FakeScalarLib.OPS >= 48
    assert _model()[3] == list(zip(scalar.SMEM_KINDS, scalar.SMEM_WORDS)) and len(scalar.SMEM_KINDS) == FakeScalarLib.KINDS
    with open(os.path.join(CSRC, "scalar_ref.h")) as f:
        ref = f.read()
    assert re.findall(r"^  X\(SCALAR_\w+, (\w+), \w+\)", ref, re.M) == list(scalar.OPS)  # the C op list, in order
    # every group the diagnostic promises is there
    for must in ("s_addc_u32", "s_subb_u32", "s_absdiff_i32", "s_lshl4_add_u32", "s_addk_i32", "s_mul_hi_i32",
                 "s_mulk_i32", "s_xnor_b64", "s_not_b32", "s_ashr_i64", "s_bfm_b64", "s_bfe_i64", "s_bcnt1_i32_b64",
                 "s_ff1_i32_b64", "s_flbit_i32_i64", "s_brev_b64", "s_bitset1_b32", "s_wqm_b64", "s_quadmask_b64",
                 "s_bitreplicate_b64_b32", "s_max_u32", "s_cselect_b64", "s_cmov_b32", "s_sext_i32_i16", "s_abs_i32",
                 "s_pack_hh_b32_b16", "s_cmp_eq_u64", "s_bitcmp1_b32"):
        assert must in scalar.OPS, must


# --- an independent implementation, on Python's unbounded integers ---------------------------------------------

def signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def big_int_model(op, a, b, scc):
    """(result, scc_out) of one scalar instruction by the ISA's rules: a = S0, b = S1, 64 bits each."""
    name = op[2:]  # without "s_"
    lo_a, lo_b = a & M32, b & M32
    sa, sb = signed(a, 32), signed(b, 32)

    def out(value, bits, flag):
        value &= (1 << bits) - 1
        return value, (scc if flag is None else int(value != 0) if flag == "nonzero" else int(bool(flag)))

    logic = re.fullmatch(r"(and|or|xor|andn2|orn2|nand|nor|xnor|not)_b(32|64)", name)
    if logic:
        bits = int(logic.group(2))
        x, y = a & ((1 << bits) - 1), b & ((1 << bits) - 1)
        ones = (1 << bits) - 1
        value = {"and": x & y, "or": x | y, "xor": x ^ y, "andn2": x & (y ^ ones), "orn2": x | (y ^ ones),
                 "nand": (x & y) ^ ones, "nor": (x | y) ^ ones, "xnor": x ^ y ^ ones, "not": x ^ ones}[logic.group(1)]
        return out(value, bits, "nonzero")
    shift = re.fullmatch(r"(lshl|lshr|ashr)_[bi](32|64)", name)
    if shift:
        bits = int(shift.group(2))
        n = lo_b % bits  # the low 5 or 6 bits of the count
        x = a & ((1 << bits) - 1)
        value = {"lshl": x << n, "lshr": x >> n, "ashr": signed(x, bits) >> n}[shift.group(1)]
        return out(value, bits, "nonzero")
    bfe = re.fullmatch(r"bfe_([ui])(32|64)", name)
    if bfe:
        bits = int(bfe.group(2))
        offset, width = lo_b % bits, (lo_b >> 16) % 128
        x = a & ((1 << bits) - 1)
        field = (signed(x, bits) if bfe.group(1) == "i" else x) >> offset  # an arithmetic shift brings the sign along
        if width == 0:
            field = 0
        elif width < bits:
            field = signed(field, width) if bfe.group(1) == "i" else field % (1 << width)
        return out(field, bits, "nonzero")
    lshl_add = re.fullmatch(r"lshl([1-4])_add_u32", name)
    if lshl_add:
        total = lo_a * 2 ** int(lshl_add.group(1)) + lo_b
        return out(total, 32, total >= 2 ** 32)
    cmp = re.fullmatch(r"cmp_(eq|lg|gt|ge|lt|le)_([iu])(32|64)", name)
    if cmp:
        bits = int(cmp.group(3))
        x, y = (signed(a, bits), signed(b, bits)) if cmp.group(2) == "i" else (a % 2 ** bits, b % 2 ** bits)
        return 0, int({"eq": x == y, "lg": x != y, "gt": x > y, "ge": x >= y, "lt": x < y, "le": x <= y}[cmp.group(1)])
    if name in ("bitcmp0_b32", "bitcmp1_b32"):
        return 0, int((lo_a >> (lo_b % 32)) % 2 == int(name[6]))
    fits = lambda v: -2 ** 31 <= v < 2 ** 31  # noqa: E731
    if name == "add_u32":
        return out(lo_a + lo_b, 32, lo_a + lo_b >= 2 ** 32)
    if name == "addc_u32":
        return out(lo_a + lo_b + scc, 32, lo_a + lo_b + scc >= 2 ** 32)
    if name == "sub_u32":
        return out(lo_a - lo_b, 32, lo_a - lo_b < 0)
    if name == "subb_u32":
        return out(lo_a - lo_b - scc, 32, lo_a - lo_b - scc < 0)
    if name == "add_i32":
        return out(sa + sb, 32, not fits(sa + sb))
    if name == "sub_i32":
        return out(sa - sb, 32, not fits(sa - sb))
    if name == "addk_i32":
        return out(sa + 0x6b35, 32, not fits(sa + 0x6b35))
    if name == "absdiff_i32":
        return out(abs(signed(sa - sb, 32)), 32, "nonzero")  # the difference wraps to 32 bits before the sign test
    if name == "mul_i32":
        return out(sa * sb, 32, None)
    if name == "mulk_i32":
        return out(sa * -0x2c4b, 32, None)
    if name == "mul_hi_u32":
        return out(lo_a * lo_b // 2 ** 32, 32, None)
    if name == "mul_hi_i32":
        return out(sa * sb // 2 ** 32, 32, None)  # floor division: the high word of the two's-complement product
    if name == "bfm_b32":
        return out((2 ** (lo_a % 32) - 1) * 2 ** (lo_b % 32), 32, None)
    if name == "bfm_b64":
        return out((2 ** (lo_a % 64) - 1) * 2 ** (lo_b % 64), 64, None)
    if name == "bcnt0_i32_b32":
        return out(f"{lo_a:032b}".count("0"), 32, "nonzero")
    if name == "bcnt1_i32_b64":
        return out(f"{a:064b}".count("1"), 32, "nonzero")
    if name == "ff0_i32_b32":
        return out(f"{lo_a:032b}"[::-1].find("0"), 32, None)  # str.find gives -1 when there is none
    if name == "ff1_i32_b64":
        return out(f"{a:064b}"[::-1].find("1"), 32, None)
    if name == "flbit_i32_b32":
        return out(f"{lo_a:032b}".find("1"), 32, None)
    if name == "flbit_i32":
        text = f"{lo_a:032b}"
        return out(text.find("1" if text[0] == "0" else "0"), 32, None)  # the first bit unlike the sign bit
    if name == "flbit_i32_i64":
        text = f"{a:064b}"
        return out(text.find("1" if text[0] == "0" else "0"), 32, None)
    if name == "brev_b32":
        return out(int(f"{lo_a:032b}"[::-1], 2), 32, None)
    if name == "brev_b64":
        return out(int(f"{a:064b}"[::-1], 2), 64, None)
    if name == "bitset0_b32":
        return out(lo_b - (lo_b & 2 ** (lo_a % 32)), 32, None)
    if name == "bitset1_b32":
        return out(lo_b | 2 ** (lo_a % 32), 32, None)
    quads = [(a >> (4 * q)) % 16 for q in range(16)]
    if name == "wqm_b64":
        return out(sum(15 * 16 ** q for q, v in enumerate(quads) if v), 64, "nonzero")
    if name == "quadmask_b64":
        return out(sum(2 ** q for q, v in enumerate(quads) if v), 64, "nonzero")
    if name == "bitreplicate_b64_b32":
        return out(int("".join(c + c for c in f"{lo_a:032b}"), 2), 64, None)
    if name in ("min_i32", "max_i32", "min_u32", "max_u32"):
        x, y = (sa, sb) if name.endswith("i32") else (lo_a, lo_b)
        first = x < y if name.startswith("min") else x > y
        return out(lo_a if first else lo_b, 32, first)
    if name in ("cselect_b32", "cmov_b32"):
        return out(lo_a if scc else lo_b, 32, None)
    if name == "cselect_b64":
        return out(a if scc else b, 64, None)
    if name == "sext_i32_i8":
        return out(signed(a, 8), 32, None)
    if name == "sext_i32_i16":
        return out(signed(a, 16), 32, None)
    if name == "abs_i32":
        return out(abs(sa), 32, "nonzero")
    if name == "pack_ll_b32_b16":
        return out(lo_a % 65536 + lo_b % 65536 * 65536, 32, None)
    if name == "pack_lh_b32_b16":
        return out(lo_a % 65536 + lo_b // 65536 * 65536, 32, None)
    if name == "pack_hh_b32_b16":
        return out(lo_a // 65536 + lo_b // 65536 * 65536, 32, None)
    raise AssertionError(f"no independent model of {op}")


@pytest.mark.parametrize("op", scalar.OPS)
def test_the_model_equals_an_independent_big_int_implementation(op):
    applied, k = _model()[7], scalar.OPS.index(op)
    for i, (a, b, scc) in enumerate(operands()):
        assert applied[(k, i)] == big_int_model(op, a, b, scc), (op, hex(a), hex(b), scc)
        assert scalar_model(op, a, b, scc) == applied[(k, i)], ("the fake's model", op, hex(a), hex(b), scc)


def field(offset, width):
    return offset | (width << 16)


# Rows worked by hand from the ISA's rules (not from the header): (op, S0, S1, SCC in) -> (result, SCC out).
HAND = [
    # shift counts use the low 5 (32 bit) or 6 (64 bit) bits
    ("s_lshl_b32", 1, 33, 0, 2, 1), ("s_lshl_b32", 1, 32, 0, 1, 1), ("s_lshr_b32", 0x80000000, 63, 0, 1, 1),
    ("s_lshl_b64", 1, 64, 0, 1, 1), ("s_lshl_b64", 1, 63, 0, 1 << 63, 1), ("s_lshr_b64", 1 << 63, 127, 0, 1, 1),
    ("s_ashr_i32", 0x80000000, 31, 0, 0xffffffff, 1), ("s_ashr_i64", 1 << 63, 32, 0, 0xffffffff80000000, 1),
    ("s_lshr_b32", 1, 1, 1, 0, 0),  # SCC = result != 0
    # bfe: offset S1[4:0] / S1[5:0], width S1[22:16]; width 0 gives 0; the signed form extends from the field's top
    ("s_bfe_u32", 0xdeadbeef, field(8, 8), 0, 0xbe, 1), ("s_bfe_u32", 0xdeadbeef, field(8, 0), 1, 0, 0),
    ("s_bfe_u32", 0xdeadbeef, field(40, 4), 0, 0xe, 1),  # offset 40 & 31 = 8
    ("s_bfe_u32", 0xdeadbeef, field(4, 32), 0, 0x0deadbee, 1), ("s_bfe_u32", 0xdeadbeef, field(0, 64), 0, 0xdeadbeef, 1),
    ("s_bfe_i32", 0xdeadbeef, field(8, 8), 0, 0xffffffbe, 1), ("s_bfe_i32", 0xdeadbeef, field(0, 7), 0, 0xffffffef, 1),
    ("s_bfe_i32", 0xdeadbeef, field(8, 7), 0, 0x3e, 1), ("s_bfe_i32", 0xdeadbeef, field(28, 32), 0, 0xfffffffd, 1),
    ("s_bfe_u64", 0xfeedfacedeadbeef, field(32, 16), 0, 0xface, 1), ("s_bfe_u64", 0xfeedfacedeadbeef, field(64, 8), 0, 0xef, 1),
    ("s_bfe_i64", 0xfeedfacedeadbeef, field(32, 16), 0, 0xffffffffffffface, 1),
    ("s_bfe_i64", 0xfeedfacedeadbeef, field(60, 64), 0, M64, 1), ("s_bfe_u64", 0xfeedfacedeadbeef, field(60, 64), 0, 0xf, 1),
    # SCC = result != 0: logic, not, bcnt, wqm, quadmask, abs, absdiff
    ("s_and_b32", 0xf0, 0x0f, 1, 0, 0), ("s_or_b32", 0, 0, 1, 0, 0), ("s_xnor_b32", 0xf0f0f0f0, 0x0f0f0f0f, 1, 0, 0),
    ("s_andn2_b32", 0xff, 0x0f, 0, 0xf0, 1), ("s_orn2_b32", 0, 0xffffffff, 1, 0, 0), ("s_nand_b64", M64, M64, 1, 0, 0),
    ("s_nor_b64", 0, 0, 0, M64, 1), ("s_not_b32", 0xffffffff, 0, 1, 0, 0), ("s_not_b64", 0, 0, 0, M64, 1),
    ("s_bcnt0_i32_b32", 0xffffffff, 0, 1, 0, 0), ("s_bcnt0_i32_b32", 0xff, 0, 0, 24, 1),
    ("s_bcnt1_i32_b64", 0xff000000000000ff, 0, 0, 16, 1), ("s_bcnt1_i32_b64", 0, 0, 1, 0, 0),
    ("s_wqm_b64", 0x0000000100000020, 0, 0, 0x0000000f000000f0, 1), ("s_wqm_b64", 0, 0, 1, 0, 0),
    ("s_quadmask_b64", 0x0000000100000020, 0, 0, 0x0102, 1), ("s_quadmask_b64", 0xf000000000000000, 0, 0, 0x8000, 1),
    ("s_abs_i32", 0xffffffff, 0, 0, 1, 1), ("s_abs_i32", 0x80000000, 0, 0, 0x80000000, 1), ("s_abs_i32", 0, 0, 1, 0, 0),
    ("s_absdiff_i32", 2, 5, 0, 3, 1), ("s_absdiff_i32", 0x80000000, 1, 0, 0x7fffffff, 1),
    ("s_absdiff_i32", 0x80000000, 0, 0, 0x80000000, 1), ("s_absdiff_i32", 7, 7, 1, 0, 0),
    # SCC = unsigned carry or borrow
    ("s_add_u32", 0xffffffff, 1, 0, 0, 1), ("s_add_u32", 0x7fffffff, 1, 1, 0x80000000, 0),
    ("s_addc_u32", 0xffffffff, 0, 1, 0, 1), ("s_addc_u32", 1, 2, 1, 4, 0), ("s_addc_u32", 0xffffffff, 0xffffffff, 1, 0xffffffff, 1),
    ("s_sub_u32", 0, 1, 0, 0xffffffff, 1), ("s_sub_u32", 5, 5, 1, 0, 0),
    ("s_subb_u32", 5, 5, 1, 0xffffffff, 1), ("s_subb_u32", 0, 0xffffffff, 1, 0, 1), ("s_subb_u32", 9, 4, 1, 4, 0),
    ("s_lshl1_add_u32", 0x80000000, 0, 0, 0, 1), ("s_lshl2_add_u32", 3, 1, 1, 13, 0),
    ("s_lshl3_add_u32", 0x1fffffff, 8, 0, 0, 1), ("s_lshl4_add_u32", 0x10000000, 5, 0, 5, 1),
    # SCC = signed overflow
    ("s_add_i32", 0x7fffffff, 1, 0, 0x80000000, 1), ("s_add_i32", 0xffffffff, 1, 1, 0, 0),
    ("s_sub_i32", 0x80000000, 1, 0, 0x7fffffff, 1), ("s_sub_i32", 0, 1, 1, 0xffffffff, 0),
    ("s_addk_i32", 0x7fffffff, 0, 0, 0x80006b34, 1), ("s_addk_i32", 1, 0, 1, 0x6b36, 0),
    # SCC = the first operand was chosen; a tie takes the second
    ("s_min_i32", 0xffffffff, 1, 0, 0xffffffff, 1), ("s_min_u32", 0xffffffff, 1, 1, 1, 0), ("s_min_u32", 4, 4, 1, 4, 0),
    ("s_max_i32", 0xffffffff, 1, 1, 1, 0), ("s_max_u32", 0xffffffff, 1, 0, 0xffffffff, 1), ("s_max_i32", 4, 4, 1, 4, 0),
    # SCC untouched: mul*, bfm, brev, ff*, flbit*, sext, pack, bitset, cselect, cmov
    ("s_mul_i32", 0x10000, 0x10000, 1, 0, 1), ("s_mul_hi_u32", 0xffffffff, 0xffffffff, 0, 0xfffffffe, 0),
    ("s_mul_hi_i32", 0xffffffff, 0xffffffff, 1, 0, 1), ("s_mul_hi_i32", 0x80000000, 2, 0, 0xffffffff, 0),
    ("s_mulk_i32", 2, 0, 1, (-2 * 0x2c4b) & M32, 1),
    ("s_bfm_b32", 4, 8, 1, 0xf00, 1), ("s_bfm_b32", 36, 40, 0, 0xf00, 0), ("s_bfm_b32", 0, 5, 1, 0, 1),
    ("s_bfm_b64", 36, 8, 0, 0xfffffffff00, 0), ("s_bfm_b64", 1, 63, 1, 1 << 63, 1),
    ("s_brev_b32", 1, 0, 1, 0x80000000, 1), ("s_brev_b64", 1, 0, 0, 1 << 63, 0), ("s_brev_b32", 0, 0, 1, 0, 1),
    # ff0 / ff1 / flbit_b32 return -1 when the bit does not occur; flbit_i32(_i64) -1 for 0 and for -1
    ("s_ff0_i32_b32", 0xffffffff, 0, 1, 0xffffffff, 1), ("s_ff0_i32_b32", 0x0000ffff, 0, 0, 16, 0),
    ("s_ff1_i32_b64", 0, 0, 0, 0xffffffff, 0), ("s_ff1_i32_b64", 1 << 40, 0, 1, 40, 1),
    ("s_flbit_i32_b32", 0, 0, 1, 0xffffffff, 1), ("s_flbit_i32_b32", 1, 0, 0, 31, 0), ("s_flbit_i32_b32", 0x80000000, 0, 0, 0, 0),
    ("s_flbit_i32", 0, 0, 0, 0xffffffff, 0), ("s_flbit_i32", 0xffffffff, 0, 1, 0xffffffff, 1),
    ("s_flbit_i32", 0x0000cccc, 0, 0, 16, 0), ("s_flbit_i32", 0xffff3333, 0, 0, 16, 0), ("s_flbit_i32", 0x7fffffff, 0, 0, 1, 0),
    ("s_flbit_i32", 0x80000000, 0, 0, 1, 0),
    ("s_flbit_i32_i64", 0, 0, 1, 0xffffffff, 1), ("s_flbit_i32_i64", M64, 0, 0, 0xffffffff, 0),
    ("s_flbit_i32_i64", 1, 0, 0, 63, 0), ("s_flbit_i32_i64", M64 - 1, 0, 0, 63, 0),
    ("s_sext_i32_i8", 0x1280, 0, 1, 0xffffff80, 1), ("s_sext_i32_i16", 0x12348000, 0, 0, 0xffff8000, 0),
    ("s_sext_i32_i8", 0x7f, 0, 0, 0x7f, 0),
    ("s_pack_ll_b32_b16", 0x11112222, 0x33334444, 1, 0x44442222, 1), ("s_pack_lh_b32_b16", 0x11112222, 0x33334444, 0, 0x33332222, 0),
    ("s_pack_hh_b32_b16", 0x11112222, 0x33334444, 0, 0x33331111, 0),
    # bitset takes the index from S0[4:0] and modifies the destination's old value (S1 here)
    ("s_bitset0_b32", 35, 0xffffffff, 1, 0xfffffff7, 1), ("s_bitset1_b32", 35, 0, 0, 8, 0), ("s_bitset1_b32", 31, 1, 0, 0x80000001, 0),
    # cselect and cmov read SCC and leave it
    ("s_cselect_b32", 7, 9, 1, 7, 1), ("s_cselect_b32", 7, 9, 0, 9, 0), ("s_cselect_b64", M64, 5, 0, 5, 0),
    ("s_cselect_b64", M64, 5, 1, M64, 1), ("s_cmov_b32", 7, 9, 1, 7, 1), ("s_cmov_b32", 7, 9, 0, 9, 0),
    ("s_bitreplicate_b64_b32", 0x80000005, 0, 1, 0xc000000000000033, 1),
    # compares: SCC only
    ("s_cmp_eq_i32", 5, 5, 0, 0, 1), ("s_cmp_lg_u32", 5, 5, 1, 0, 0), ("s_cmp_gt_i32", 0xffffffff, 0, 1, 0, 0),
    ("s_cmp_ge_u32", 0xffffffff, 0, 0, 0, 1), ("s_cmp_lt_u32", 0, 0xffffffff, 0, 0, 1), ("s_cmp_lt_i32", 0, 0xffffffff, 1, 0, 0),
    ("s_cmp_le_i32", 0x80000000, 0x80000000, 0, 0, 1), ("s_cmp_eq_u64", 1 << 32, 0, 1, 0, 0), ("s_cmp_eq_u64", M64, M64, 0, 0, 1),
    ("s_bitcmp0_b32", 4, 34, 1, 0, 0), ("s_bitcmp1_b32", 4, 34, 0, 0, 1), ("s_bitcmp0_b32", 4, 1, 0, 0, 1),
]


def test_the_model_gives_the_hand_worked_rows():
    stdin = "".join(f"{scalar.OPS.index(op)} {a:x} {b:x} {scc}\n" for op, a, b, scc, _, _ in HAND)
    rc, out = _ref_program(False, stdin)
    assert rc == 0
    got = [(int(f[1], 16), int(f[2])) for f in (ln.split() for ln in out.splitlines()) if f[0] == "r"]
    assert len(got) == len(HAND)
    for row, g in zip(HAND, got):
        assert g == (row[4], row[5]), (row, hex(g[0]), g[1])
        assert big_int_model(*row[:4]) == (row[4], row[5]), row  # the independent implementation agrees too
    # every op outside the plain logic, shift and compare families has a row of its own
    family = re.compile(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|lshl|lshr|ashr|cmp_\w+)_[biu](32|64)")
    assert {row[0] for row in HAND} >= {op for op in scalar.OPS if not family.fullmatch(op)}


@pytest.mark.parametrize("op", scalar.OPS)
def test_no_op_hides_a_skipped_step(op):
    """A chain whose instruction was left out once (at its first, second or last step of 8) must end different from
    the expected words: otherwise the test could not see that step fail.  The chain's own word rides in the hash, so
    this holds for the ops that collapse their inputs too (min, bcnt, the compares)."""
    skips = _model()[1]
    for s in (0, 1, 7):
        assert skips[(op, s)] == scalar.CHAINS, (op, s)


def test_the_sgpr_pattern_is_distinct_per_register_wave_and_seed():
    sgpr = _model()[4]
    one = {k: v for k, v in sgpr.items() if k[0] == 1}
    assert len(one) == 64 * 128 and len(set(one.values())) == len(one)  # no two registers of a launch hold one word
    assert all(sgpr[(1, w, r)] != sgpr[(2, w, r)] for w in range(64) for r in range(128))
    g = 0x9E3779B1
    assert sgpr[(1, 3, 21)] == (sgpr[(1, 3, 20)] + g) & M32 and sgpr[(1, 4, 0)] == (sgpr[(1, 3, 0)] + 128 * g) & M32


def test_the_smem_pattern_and_walk():
    smem, index = _model()[5], _model()[6]
    assert len(set(smem.values())) > 1000  # an index hash: (nearly) every word differs
    assert all(smem[i] == (((i ^ 7) * 0x9E3779B1) & M32) ^ (i >> 3) for i in range(1024))
    for wave, k, ordered, scattered in index:
        assert ordered == (4 * k) % 256                      # in order, wrapping: the later passes hit
        assert scattered % 16 == 0 and scattered <= 1024 - 16  # a whole load always lies inside the table
    starts = {w: [s for ww, _, _, s in index if ww == w] for w in range(8)}
    assert len({tuple(v) for v in starts.values()}) == 8  # every wave its own walk


def test_the_reference_is_clean_under_the_host_sanitizers():
    stdin = "".join(f"{k} {a:x} {b:x} {scc}\n" for k in range(len(scalar.OPS)) for a, b, scc in operands()[::7])
    rc, out = _ref_program(True, stdin)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and f"\nok {len(scalar.OPS)}\n" in out, out[-2000:]
    assert len(re.findall(r"^expect ", out, re.M)) == len(scalar.OPS)


# --- 2. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("scalar"), scalar._signatures()
    assert set(exports) == set(sig) == {"scalar_last_error", "scalar_device_count", "scalar_slots", "scalar_sgpr_lo",
                                        "scalar_sgpr_hi", "scalar_sgpr_regs", "scalar_salu", "scalar_sgpr",
                                        "scalar_smem", "scalar_apply"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeScalarLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    with open(os.path.join(CSRC, "scalar.hip")) as f:
        src = f.read()
    lo, hi, skip = (int(v) for v in re.search(r"SG_LO = (\d+), SG_HI = (\d+), SG_SKIP = (\d+)", src).groups())
    assert (lo, hi, hi - lo) == (FakeScalarLib.SGPR_LO, FakeScalarLib.SGPR_HI, FakeScalarLib.SGPR_REGS) and lo < skip < hi
    assert f"s{lo}-" in diag.KERNEL_REVISION["scalar"] and f"-{hi}" in diag.KERNEL_REVISION["scalar"]
    assert f"{len(scalar.OPS)}ops" in diag.KERNEL_REVISION["scalar"]


# --- 3. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, scalar_kw, **FakeDiagLib kwargs)`` -> (FakeScalarLib, FakeLanesLib, FakeAtomicsLib)."""
    def install(n=1, scalar_kw=None, **kw):
        lib, slib = FakeDiagLib(n=n, **kw), FakeScalarLib(n=n, **(scalar_kw or {}))
        llib, alib = FakeLanesLib(n=n), FakeAtomicsLib(n=n)
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(scalar, "lib", lambda: slib)
        monkeypatch.setattr(lanes, "lib", lambda: llib)
        monkeypatch.setattr(atomics, "lib", lambda: alib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return slib, llib, alib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}
CALLS = ["salu0", "sgpr0", "smem0"]


def test_off_by_default_and_on_when_asked(node):
    slib, llib, alib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and slib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and slib.calls == []
    res = diag.run(1, 0, extra=("scalar",))
    assert list(res)[-1] == "scalar" and set(res) == LEVEL1 | {"scalar"} and slib.calls == CALLS
    r = res["scalar"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == ""
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "parts", "ms", "wall_s", "detail"}
    assert r["simds"] == 1024 and r["xcds"] == 8 and r["blocks"] == {"salu": 1024, "sgpr": 1792, "smem": 1024}
    assert tuple(r["parts"]) == scalar.PARTS and all({"errors", "ms"} <= set(p) for p in r["parts"].values())
    salu, sgpr, smem = (r["parts"][k] for k in scalar.PARTS)
    assert tuple(salu["ops"]) == scalar.OPS and salu["iters"] == scalar.DEFAULT_ITERS
    for row in salu["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "gops"}
        assert row["errors"] == 0 and row["first_bad"] is None and row["gops"] > 0
    assert sgpr["regs_per_wave"] == 75 and sgpr["range"] == "s20-s95 without s32" and sgpr["first_bad"] is None
    assert sgpr["waves_per_simd"] == {"min": 7, "max": 7} and sgpr["bytes_per_simd"]["max"] == 7 * 75 * 4
    assert tuple(smem["kinds"]) == scalar.SMEM_KINDS
    for row in smem["kinds"].values():
        assert set(row) == {"errors", "first_bad", "ms", "ms_hit", "ms_miss", "gwords_hit", "gwords_miss"}
        assert row["errors"] == 0 and row["gwords_hit"] > 0 and row["gwords_miss"] > 0
    json.dumps(r)
    assert alib.calls == [] and llib.calls == []
    every = diag.run(1, 0, extra=("atomics", "lanes", "scalar"))  # the three opt-in tests combine, in order
    assert list(every)[-3:] == ["atomics", "lanes", "scalar"]
    assert alib.calls == ["atomics0"] and llib.calls == ["lanes0"] and slib.calls == CALLS * 2
    assert diag.run(0, 0, extra=("scalar",)).keys() == {"scalar"}
    assert scalar.scalar_test(0, parts=("sgpr",))["parts"].keys() == {"sgpr"} and slib.calls[-1] == "sgpr0"
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("scalar" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["scalar"] and "scalar" not in diag.REFERENCE_RATES
    assert "scalar" not in diag.DMA_TESTS | diag.SHARED_TESTS
    line = diag._summary("scalar", r)
    assert f"83 ops x {scalar.DEFAULT_ITERS} steps 0 wrong; 75 SGPRs x 7 waves per SIMD 0 wrong; 7 load kinds 0 wrong; 1024 SIMDs of 8 XCDs" in line


def test_the_fake_answers_apply_from_the_model(node):
    node(1)
    assert scalar.apply("s_add_u32", 0xffffffff, 1) == (0, 1)
    for op, a, b, scc, want, want_scc in HAND:
        assert scalar.apply(op, a, b, scc) == (want, want_scc), op
    with pytest.raises(ValueError):
        scalar.apply("s_nop", 0, 0)


def test_a_wrong_word_fails_the_gpu_and_names_the_simd(node):
    k = scalar.OPS.index("s_mul_hi_u32")
    slib, _, _ = node(4, {"bad": {(2, "salu", k): 3, (2, "smem", 3): 2}})
    r = diag.run(1, 2, extra=("scalar",))["scalar"]
    assert r["pass"] is False and r["errors"] == 5
    assert r["detail"] == ("3 wrong words in s_mul_hi_u32 on xcd5/se1/cu7/simd2; "
                           "2 wrong words from s_load_dwordx8, first word 105 on xcd5/se1/cu7/simd2")
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (5)"]
    bad = r["parts"]["salu"]["ops"]["s_mul_hi_u32"]["first_bad"]
    assert bad == {"where": "xcd5/se1/cu7/simd2", "chain": 1, "got": "0x5ca1a39e", "want": "0x5ca1a29e"}
    assert r["parts"]["salu"]["errors"] == 3 and r["parts"]["sgpr"]["errors"] == 0 and r["parts"]["smem"]["errors"] == 2
    assert r["parts"]["salu"]["ops"]["s_mul_i32"]["errors"] == 0
    assert diag.run(1, 1, extra=("scalar",))["scalar"]["pass"]
    slib.bad = {(2, "sgpr", 0): 1}
    r = diag.run(1, 2, extra=("scalar",))["scalar"]
    assert r["detail"] == "1 wrong SGPRs, first s41 under inverse on xcd5/se1/cu7/simd2"
    assert r["parts"]["sgpr"]["first_bad"]["reg"] == "s41"
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_scalar=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag scalar failed ("))
    assert "1 wrong SGPRs, first s41" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["scalar"])
    assert "FAIL" in line and "1 wrong" in line and "xcd5/se1/cu7/simd2" in text


def test_the_hooks_reach_the_library_and_bad_arguments_are_refused(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    r = scalar.scalar_test(0, parts=("salu",), ops=("s_add_u32", "s_sub_u32"), inject_op="s_sub_u32", inject_block=0)
    assert r["errors"] == 1 and r["parts"]["salu"]["ops"]["s_sub_u32"]["errors"] == 1
    r = scalar.scalar_test(0, parts=("sgpr",), inject_reg="hi", inject_block=0)
    assert r["errors"] == 1 and r["parts"]["sgpr"]["first_bad"]["reg"] == "s95"
    r = scalar.scalar_test(0, parts=("smem",), inject_word=77)
    assert all(row["errors"] > 0 and row["first_bad"]["word"] == 77 for row in r["parts"]["smem"]["kinds"].values())
    monkeypatch.setitem(diag._TESTS, "scalar", ("scalar_test", {"iters": 0}))
    r = diag.run(1, 0, extra=("scalar",))["scalar"]
    assert r["pass"] is False and "scalar failed (-2)" in r["detail"] and "iters 1..2^20" in r["detail"]
    for kw in ({"ops": ("s_add_u32",), "inject_op": "s_sub_u32"}, {"ops": ("no_such_op",)}, {"parts": ("valu",)},
               {"kinds": ("s_load_dwordx3",)}, {"inject_reg": "middle"}):
        with pytest.raises(ValueError):
            scalar.scalar_test(0, **kw)
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(scalar, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("scalar",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, isolation):
    bad = {"bad": {(5, "salu", 0): 1}}
    node(8, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "scalar": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_scalar=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"scalar"}, (d, g["diag"].keys())
        assert g["diag"]["scalar"]["pass"] is (d != 5), (d, g["diag"]["scalar"])
    assert "1 wrong words in s_add_u32" in rep["gpus"][5]["diag"]["scalar"]["detail"]  # each child its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", diag_scalar=True, diag_lanes=True, diag_atomics=True, **kw).probe_once()
    assert all(list(g["diag"])[-3:] == ["atomics", "lanes", "scalar"] for g in rep["gpus"])
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    slib, llib, alib = node(2)
    assert diag.main(["--level", "1", "--scalar", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["scalar", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(slib.calls) == sorted(CALLS + ["salu1", "sgpr1", "smem1"]) and alib.calls == [] and llib.calls == []
    assert diag.main(["--level", "1"]) == 0
    assert "scalar" not in capsys.readouterr().out and len(slib.calls) == 6
    assert diag.main(["--level", "1", "--lanes"]) == 0
    assert "scalar" not in capsys.readouterr().out and len(slib.calls) == 6 and len(llib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--scalar", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--scalar", "--atomics", "--lanes", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [("scalar",), ("atomics", "lanes", "scalar"), None]
    capsys.readouterr()
    monkeypatch.undo()
    slib, llib, alib = node(1)
    b = diag.burn_in(1, [0], 0.0, extra=("scalar",))
    assert b["pass"] and b["rounds"] == 1 and slib.calls == CALLS
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--scalar"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and slib.calls == CALLS * 2
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(slib.calls) == 6 and alib.calls == [] and llib.calls == []
    assert A.build_parser().parse_args(["--node", "n", "--diag-scalar"]).diag_scalar is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_scalar is False
    for main, flag in ((diag.main, "--scalar"), (node_cycle.main, "--scalar"), (A.main, "--diag-scalar")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 4. build --------------------------------------------------------------------------------------------------

def test_the_build_has_a_scalar_target(tmp_path, monkeypatch):
    t = B._targets()
    assert "scalar" in t and t["scalar"]["out"].endswith("libmi355x_scalar.so")
    assert t["scalar"]["cmd"] == t["lanes"]["cmd"]
    assert [os.path.basename(h) for h in t["scalar"]["headers"]] == ["scalar_ref.h", "hip_host.h", "simd_report.h", "op_list.h"]
    assert "libmi355x_scalar.so" in B.__doc__ and "scalar" in B.__doc__.splitlines()[2]
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    monkeypatch.setattr(B, "OUT", str(tmp_path))  # a fresh output directory: the tree's own library stays as it is
    msgs = B.build(only=["scalar"])
    assert msgs == [f"scalar: built {os.path.relpath(os.path.join(str(tmp_path), 'libmi355x_scalar.so'), os.path.dirname(B.PKG))}"]
    L = ctypes.CDLL(os.path.join(str(tmp_path), "libmi355x_scalar.so"))
    for name in scalar._signatures():
        getattr(L, name)  # AttributeError: not exported
    assert B.build(only=["scalar"]) == []  # up to date
    asm = os.path.join(str(tmp_path), "scalar.s")
    subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "scalar.hip"), "-o", asm], check=True, capture_output=True, text=True)
    with open(asm) as f:
        text = f.read()
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {"0"}    # nor an LDS allocation
    assert set(re.findall(r"\.sgpr_spill_count: (\d+)", text)) == {"0"} == set(re.findall(r"\.vgpr_spill_count: (\d+)", text))
    bodies = {int(k): body for k, body in re.findall(r"^_ZN\w*11salu_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                     re.M | re.S)}
    assert sorted(bodies) == list(range(len(scalar.OPS)))
    for k, name in enumerate(scalar.OPS):  # one native instruction per chain, each between its SCC set and read
        found = re.findall(r"s_cmp_lg_u32 s\d+, 0\n\s*" + name + r" [^\n]*\n\s*s_cselect_b32 s\d+, 1, 0", bodies[k])
        assert len(found) == scalar.CHAINS, (name, len(found))
    kinds = {int(k): body for k, body in re.findall(r"^_ZN\w*11smem_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                    re.M | re.S)}
    for k, name in enumerate(scalar.SMEM_KINDS):  # the load and its wait in one statement
        assert re.search(r"^\s*" + name + r" [^\n]*\n\s*s_waitcnt lgkmcnt\(0\)", kinds[k], re.M), name
