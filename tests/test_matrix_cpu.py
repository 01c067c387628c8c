"""The matrix diagnostic on CPU: the model of csrc/matrix/matrix_ref.h (lane maps, decoders, one instruction, the
operand generator and its exactness bound) against an exact matmul written here from the formats' definitions, the C
ABI of csrc/matrix/matrix.hip against ops/matrix.py and its fake, the instructions the kernels compile to, the opt-in
wiring on the fakes and the build target.  The kernels themselves run on an MI355X in tests/test_gpu_matrix.py."""
import ctypes
import functools
import inspect
import json
import os
import re
import shutil
import struct
import subprocess
import tempfile
from fractions import Fraction

import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, matrix
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeDiagLib, FakeFabricLib, FakeMatrixLib, c_exports

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "matrix")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
SEEDS = (matrix.DEFAULT_SEED, 7, 0xFEEDFACE12345)

# Prints the op table, every lane map, a few decoded codes, the budget and expectation status of every op at three
# seeds and with a deliberately too-wide operand set, and per op and seed the first step's operands with the D
# registers matrix_apply() gives for them.
REF_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "matrix_ref.h"
static void row(const char* tag, const uint32_t* w, int n) {
  printf("%s", tag);
  for (int i = 0; i < n; ++i) printf(" %x", w[i]);
  printf("\n");
}
int main(int argc, char** argv) {
  MatrixOperands* o = new MatrixOperands;
  uint32_t* d = new uint32_t[MATRIX_WAVE * MATRIX_CW]();
  const int fmts[9] = {MF_F16, MF_BF16, MF_FP8, MF_BF8, MF_FP6, MF_BF6, MF_FP4, MF_I8, MF_F32};
  for (int f : fmts)
    for (uint64_t c = 0; c < (matrix_fmt(f).bits <= 8 ? 1ULL << matrix_fmt(f).bits : 0x10000ULL); c += matrix_fmt(f).bits <= 8 ? 1 : 257) {
      const uint64_t code = f == MF_F32 ? c << 16 : c;
      MatrixVal v = {0, 0};
      const bool ok = matrix_decode(f, code, &v);
      printf("dec %d %llu %d %lld %d\n", f, static_cast<unsigned long long>(code), ok, static_cast<long long>(v.m), v.e);
    }
  for (uint32_t c = 0; c < 256; ++c) {
    int e = 0;
    const bool ok = matrix_decode_e8m0(c | 0xabcd00u, &e);
    printf("e8m0 %u %d %d\n", c, ok, e);
  }
  for (int e = 0; e < 4; ++e) printf("sparsek %d\n", matrix_sparse_k(2 * 3 + (e & 1), 0x000000e4u, e));
  for (int op = 0; op < MATRIX_OPS; ++op) {
    const MatrixOpInfo& t = MATRIX_OP_TABLE[op];
    printf("op %d %s %s %d %d %d %d %d %d %d %d %d\n", op, t.name, t.insn, t.M, t.N, t.K, t.afmt, t.bfmt, t.cfmt, t.sparse,
           t.f8f6f4, t.scaled);
    printf("amap %d", op);
    for (int l = 0; l < MATRIX_WAVE; ++l)
      for (int e = 0; e < matrix_a_elems(t); ++e) printf(" %d %d", matrix_a_coord(t, l, e).row, matrix_a_coord(t, l, e).col);
    printf("\nbmap %d", op);
    for (int l = 0; l < MATRIX_WAVE; ++l)
      for (int e = 0; e < matrix_b_elems(t); ++e) printf(" %d %d", matrix_b_coord(t, l, e).row, matrix_b_coord(t, l, e).col);
    printf("\ncmap %d", op);
    for (int l = 0; l < MATRIX_WAVE; ++l)
      for (int e = 0; e < matrix_cd_elems(t); ++e) printf(" %d %d", matrix_cd_coord(t, l, e).row, matrix_cd_coord(t, l, e).col);
    MatrixBudget g;
    const int rb = matrix_budget(op, 0, &g);
    printf("\nbudget %d %d %lld %lld %d %d %d %d %d\n", op, rb, static_cast<long long>(g.units_a),
           static_cast<long long>(g.units_b), g.mbits_a, g.espan_a, g.mbits_b, g.espan_b, g.qexp);
    printf("wide %d %d %d\n", op, matrix_expect(op, 1, 8, -1, o), matrix_operands(op, 1, 8, 0, o));
    for (int s = 1; s < argc; ++s) {
      const uint64_t seed = strtoull(argv[s], nullptr, 0);
      const int re = matrix_expect(op, seed, 0, -1, o);
      uint32_t sum = 0;
      for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) sum = sum * 31u + o->D[i];
      const int rs = matrix_expect(op, seed, 0, 2, o);
      int differ = 0;
      uint32_t sum2 = 0;
      for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) sum2 = sum2 * 31u + o->D[i];
      differ = sum2 != sum;
      printf("expect %d %llu %d %u %d %d\n", op, static_cast<unsigned long long>(seed), re, sum, rs, differ);
      if (matrix_operands(op, seed, 0, 0, o)) return 2;
      for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) d[i] = 0;
      const int ra = matrix_apply(op, o->A[0], o->B[0], o->C, o->idx[0], o->scale_a[0], o->scale_b[0], d);
      printf("case %d %llu %d\n", op, static_cast<unsigned long long>(seed), ra);
      row("A", o->A[0], MATRIX_WAVE * MATRIX_AW);
      row("B", o->B[0], MATRIX_WAVE * MATRIX_AW);
      row("C", o->C, MATRIX_WAVE * MATRIX_CW);
      row("idx", o->idx[0], MATRIX_WAVE);
      row("sa", o->scale_a[0], MATRIX_WAVE);
      row("sb", o->scale_b[0], MATRIX_WAVE);
      row("D", d, MATRIX_WAVE * MATRIX_CW);
    }
  }
  printf("ok %d\n", MATRIX_OPS);
  delete o;
  delete[] d;
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _ref_program(sanitize):
    """matrix_ref.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "matrix_ref.cpp"), os.path.join(tmp, "matrix_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe, *[str(s) for s in SEEDS]], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


@functools.lru_cache(maxsize=None)
def _model():
    rc, out = _ref_program(False)
    assert rc == 0 and out.strip().endswith(f"ok {len(matrix.OPS)}"), out[-2000:]
    m = {"ops": {}, "amap": {}, "bmap": {}, "cmap": {}, "dec": {}, "e8m0": {}, "sparsek": [], "budget": {}, "wide": {},
         "expect": {}, "case": {}}
    cur = None
    for line in out.splitlines():
        f = line.split()
        if f[0] == "op":
            m["ops"][int(f[1])] = dict(name=f[2], insn=f[3], M=int(f[4]), N=int(f[5]), K=int(f[6]), afmt=int(f[7]),
                                       bfmt=int(f[8]), cfmt=int(f[9]), sparse=int(f[10]), f8f6f4=int(f[11]),
                                       scaled=int(f[12]))
        elif f[0] in ("amap", "bmap", "cmap"):
            v = [int(x) for x in f[2:]]
            m[f[0]][int(f[1])] = list(zip(v[0::2], v[1::2]))
        elif f[0] == "dec":
            m["dec"][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]), int(f[5]))
        elif f[0] == "e8m0":
            m["e8m0"][int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "sparsek":
            m["sparsek"].append(int(f[1]))
        elif f[0] in ("budget", "wide"):
            m[f[0]][int(f[1])] = [int(x) for x in f[2:]]
        elif f[0] == "expect":
            m["expect"][(int(f[1]), int(f[2]))] = [int(x) for x in f[3:]]
        elif f[0] == "case":
            cur = m["case"].setdefault((int(f[1]), int(f[2])), {"rc": int(f[3])})
        elif f[0] in ("A", "B", "C", "idx", "sa", "sb", "D"):
            cur[f[0]] = [int(x, 16) for x in f[1:]]
    return m


F32, F16, BF16, I8, F64, FP8, BF8, FP6, BF6, FP4, I32 = range(11)
# (bits, exponent bits, mantissa bits, bias) from the IEEE / OCP definitions
FORMATS = {F32: (32, 8, 23, 127), F16: (16, 5, 10, 15), BF16: (16, 8, 7, 127), F64: (64, 11, 52, 1023),
           FP8: (8, 4, 3, 7), BF8: (8, 5, 2, 15), FP6: (6, 2, 3, 1), BF6: (6, 3, 2, 3), FP4: (4, 2, 1, 1)}


def value(fmt, code):
    """The exact value of a code, from the format's definition (None: NaN / Inf)."""
    if fmt in (I8, I32):
        bits = 8 if fmt == I8 else 32
        return Fraction(code - (1 << bits) if code >> (bits - 1) else code)
    bits, eb, mb, bias = FORMATS[fmt]
    sign = -1 if code >> (bits - 1) else 1
    ex, frac = (code >> mb) & ((1 << eb) - 1), code & ((1 << mb) - 1)
    if fmt == FP8 and ex == 15 and frac == 7:
        return None
    if fmt in (F32, F16, BF16, F64, BF8) and ex == (1 << eb) - 1:
        return None
    if ex == 0:
        return sign * Fraction(frac, 1 << mb) * Fraction(2) ** (1 - bias)
    return sign * (1 + Fraction(frac, 1 << mb)) * Fraction(2) ** (ex - bias)


def test_the_op_table_is_the_python_one():
    ops = _model()["ops"]
    assert tuple(ops[k]["name"] for k in range(len(ops))) == matrix.OPS
    assert len(set(matrix.OPS)) == len(matrix.OPS) == FakeMatrixLib.OPS == 34
    for t in ops.values():
        assert matrix.shape(t["name"]) == (t["M"], t["N"], t["K"]), t
    assert sum(t["sparse"] for t in ops.values()) == 7 and sum(t["scaled"] for t in ops.values()) == 4


@pytest.mark.parametrize("k", range(len(matrix.OPS)))
def test_every_lane_map_is_a_bijection(k):
    m = _model()
    t = m["ops"][k]
    ka = t["K"] // 2 if t["sparse"] else t["K"]  # a sparse op's A map covers the compressed A
    assert sorted(m["amap"][k]) == [(i, c) for i in range(t["M"]) for c in range(ka)]
    assert sorted(m["bmap"][k]) == [(c, j) for c in range(t["K"]) for j in range(t["N"])]
    assert sorted(m["cmap"][k]) == [(i, j) for i in range(t["M"]) for j in range(t["N"])]


def test_the_cd_maps_are_the_documented_ones():
    m = _model()
    for k, t in m["ops"].items():
        per = t["M"] * t["N"] // 64
        for lane in range(64):
            for reg in range(per):
                if t["cfmt"] == F64:
                    want = ((lane >> 4) + 4 * reg, lane & 15)
                elif t["M"] == 16:
                    want = (4 * (lane >> 4) + reg, lane & 15)
                else:
                    want = ((reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31)
                assert m["cmap"][k][lane * per + reg] == want, (t["name"], lane, reg)


def test_the_decoders_give_the_hand_worked_values():
    dec = _model()["dec"]

    def val(fmt, code):
        ok, mant, e = dec[(fmt, code)]
        return Fraction(mant) * Fraction(2) ** e if ok else None
    assert val(FP8, 0x7E) == 448 and val(FP8, 0x01) == Fraction(1, 512) and val(FP8, 0x7F) is None
    assert val(FP8, 0x38) == 1 and val(FP8, 0xC0) == -2
    assert val(BF8, 0x7B) == 57344 and val(BF8, 0x01) == Fraction(1, 65536) and val(BF8, 0x7C) is None
    assert val(FP4, 0x7) == 6 and val(FP4, 0x1) == Fraction(1, 2) and val(FP4, 0x9) == Fraction(-1, 2)
    assert max(val(FP6, c) for c in range(64)) == Fraction(15, 2) and val(FP6, 0x01) == Fraction(1, 8)
    assert max(val(BF6, c) for c in range(64)) == 28 and val(BF6, 0x01) == Fraction(1, 16)
    assert val(I8, 0x80) == -128 and val(I8, 0x7F) == 127 and val(I8, 0xFF) == -1
    e8 = _model()["e8m0"]
    assert e8[127] == (1, 0) and e8[128] == (1, 1) and e8[0] == (1, -127) and e8[255][0] == 0
    # every code of the small formats, and a stride of the 16-bit ones, against the definitions written here
    for (fmt, code), (ok, mant, e) in dec.items():
        want = value(fmt, code)
        assert (want is None) == (not ok), (fmt, code)
        if ok:
            assert Fraction(mant) * Fraction(2) ** e == want, (fmt, code)
    assert value(F16, 0x3C00) == 1 and value(F16, 0xC500) == -5 and value(BF16, 0x3F80) == 1 and value(BF16, 0x42F7) == 123.5


def test_a_sparse_index_word_selects_the_expected_positions():
    # index bits 0xe4 = 11 10 01 00: the four kept values of compressed columns 6, 7, 6, 7 (group 3: k 12..15) sit
    # at positions 0, 1, 2, 3
    assert _model()["sparsek"] == [12, 13, 14, 15]


def _elements(words, lane, stride, bits, count):
    block = 0
    for w in range(stride):
        block |= words[lane * stride + w] << (32 * w)
    return [(block >> (bits * e)) & ((1 << bits) - 1) for e in range(count)]


def _encode(fmt, v):
    if fmt == I32:
        return [int(v) & 0xffffffff]
    if fmt == F32:
        assert Fraction(struct.unpack("<f", struct.pack("<f", float(v)))[0]) == v
        return [struct.unpack("<I", struct.pack("<f", float(v)))[0]]
    assert Fraction(float(v)) == v
    return list(struct.unpack("<II", struct.pack("<d", float(v))))


@pytest.mark.parametrize("k", range(len(matrix.OPS)))
def test_one_instruction_is_an_exact_matmul(k):
    """matrix_apply() on the generator's operands against A x B + C assembled here: own decode tables, the maps
    re-stated below, the sparse A decompressed here, an exact sum in fractions, converted to the output's bits."""
    m = _model()
    t = m["ops"][k]
    M, N, K = t["M"], t["N"], t["K"]
    abits = 8 if t["afmt"] == I8 else FORMATS[t["afmt"]][0]
    bbits = 8 if t["bfmt"] == I8 else FORMATS[t["bfmt"]][0]
    ea, eb, ec = M * K // 64 // (2 if t["sparse"] else 1), N * K // 64, M * N // 64
    cw = 2 if t["cfmt"] == F64 else 1
    for seed in SEEDS:
        c = m["case"][(k, seed)]
        assert c["rc"] == 0
        a = [[Fraction(0)] * K for _ in range(M)]
        b = [[Fraction(0)] * N for _ in range(K)]
        for lane in range(64):
            sa = Fraction(2) ** ((c["sa"][lane] & 0xff) - 127) if t["scaled"] else 1
            sb = Fraction(2) ** ((c["sb"][lane] & 0xff) - 127) if t["scaled"] else 1
            for e, code in enumerate(_elements(c["A"], lane, 8, abits, ea)):
                col = (lane // M) * ea + e  # lane l: row l % M, a run of ea consecutive (kept) k
                if t["sparse"]:             # kept value e: group (col / 2) of four, position = bits 2e+1:2e
                    col = 4 * (col // 2) + ((c["idx"][lane] >> (2 * e)) & 3)
                a[lane % M][col] += value(t["afmt"], code) * sa
            for e, code in enumerate(_elements(c["B"], lane, 8, bbits, eb)):
                b[(lane // N) * eb + e][lane % N] = value(t["bfmt"], code) * sb
        bt = list(zip(*b))
        for lane in range(64):
            for reg in range(ec):
                if t["cfmt"] == F64:
                    i, j = (lane >> 4) + 4 * reg, lane & 15
                elif M == 16:
                    i, j = 4 * (lane >> 4) + reg, lane & 15
                else:
                    i, j = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31
                cin = c["C"][16 * lane + cw * reg] | (c["C"][16 * lane + cw * reg + 1] << 32 if cw == 2 else 0)
                total = value(t["cfmt"], cin) + sum(x * y for x, y in zip(a[i], bt[j]) if x)
                assert c["D"][16 * lane + cw * reg:16 * lane + cw * reg + cw] == _encode(t["cfmt"], total), \
                    (t["name"], seed, lane, reg)


def test_the_budget_holds_and_a_too_wide_set_is_refused():
    m = _model()
    for k, t in m["ops"].items():
        assert m["budget"][k][0] == 0, t["name"]
        assert m["wide"][k] == [-2, -2], t["name"]  # 8 more bits per operand: the generator returns its error
        for seed in SEEDS:
            drawn, _, skipped, differ = m["expect"][(k, seed)]
            assert 1 <= drawn <= 16 and skipped >= 1, (t["name"], seed)  # >= 1: the number of draws; < 0: an error
            assert differ == 1, (t["name"], seed)  # a round without its third instruction ends elsewhere
    # the widths the README states
    by = {t["name"]: m["budget"][k] for k, t in m["ops"].items()}
    assert by["f32_16x16x32_bf16"][3:5] == [8, 0] and by["f32_32x32x8_bf16_1k"][3:5] == [8, 1]  # full 8-bit significands
    assert by["f64_16x16x4_f64"][3] == 24 and by["f32_32x32x2_f32"][3] == 10 and by["f32_16x16x32_f16"][3] == 8
    assert by["i32_16x16x64_i8"][1] == 128 and by["f8f6f4_16x16x128_fp4"][1] == 12 and by["f8f6f4_16x16x128_fp6"][1] == 60
    assert by["f8f6f4_16x16x128_scale_fp6"][1] == 60 and by["f8f6f4_16x16x128_bf8"][1] == 64


def test_the_reference_is_clean_under_the_host_sanitizers():
    rc, out = _ref_program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and out.strip().endswith(f"ok {len(matrix.OPS)}"), out[-3000:]
    assert len(re.findall(r"^case ", out, re.M)) == len(matrix.OPS) * len(SEEDS)  # every op's model ran


# --- ABI -------------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("matrix"), matrix._signatures()
    assert set(exports) == set(sig) == {"matrix_last_error", "matrix_device_count", "matrix_slots", "matrix_test",
                                        "matrix_apply"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeMatrixLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["matrix_test"]) == 17 and len(exports["matrix_apply"]) == 9
    with open(os.path.join(CSRC, "matrix_ref.h")) as f:
        ref = f.read()
    assert re.findall(r'^    \{"(\w+)", "', ref, re.M) == list(matrix.OPS)  # the C op table, in order


# --- instructions ----------------------------------------------------------------------------------------------

def test_every_op_compiles_to_its_native_instruction_without_scratch_or_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-save-temps",
                        os.path.join(CSRC, "matrix.hip"), "-o", os.path.join(tmp, "matrix.o")], check=True,
                       capture_output=True, text=True, cwd=tmp)
        asm = [f for f in os.listdir(tmp) if f.endswith(".s")]
        assert len(asm) == 1, os.listdir(tmp)
        with open(os.path.join(tmp, asm[0])) as f:
            text = f.read()
    chained = {int(k): body for k, body in re.findall(r"^_ZN\w*13matrix_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                      re.M | re.S)}
    applied = {int(k): body for k, body in re.findall(r"^_ZN\w*12apply_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                      re.M | re.S)}
    assert sorted(chained) == sorted(applied) == list(range(len(matrix.OPS)))
    ops = _model()["ops"]
    for k, name in enumerate(matrix.OPS):
        insn = ops[k]["insn"]
        every = re.findall(r"^\s*(v_s?mfmac?_\w+)", chained[k], re.M)
        assert every and set(every) == {insn}, (name, set(every))  # its own instruction and no other
        # behind the round's operand barrier, the four dependent instructions back to back
        straight = re.split(r"^\s*s_cbranch|^\.LBB", chained[k].split(";;#ASMEND", 1)[1], 1, re.M)[0]
        assert len(re.findall(r"^\s*" + insn + r" ", straight, re.M)) == 4, name
        assert re.findall(r"^\s*(v_s?mfmac?_\w+)", applied[k], re.M) == [insn], name
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {"0"}    # nor an LDS allocation
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}


# --- wiring on the fakes ---------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, matrix_kw, **FakeDiagLib kwargs)`` -> FakeMatrixLib for an n x MI355X node."""
    def install(n=1, matrix_kw=None, **kw):
        lib, mlib = FakeDiagLib(n=n, **kw), FakeMatrixLib(n=n, **(matrix_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(matrix, "lib", lambda: mlib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return mlib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}


def test_off_by_default_and_on_when_asked(node):
    mlib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and mlib.calls == []
    res = diag.run(1, 0, extra=("matrix",))
    assert list(res)[-1] == "matrix" and set(res) == LEVEL1 | {"matrix"} and mlib.calls == ["matrix0"]
    r = res["matrix"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["iters"] == matrix.DEFAULT_ITERS
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "iters", "ops", "ms", "wall_s", "detail"}
    assert r["blocks"] == 512 and r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["ops"]) == matrix.OPS
    for row in r["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "tops"}
        assert row["errors"] == 0 and row["first_bad"] is None and row["tops"] > 0
    json.dumps(r)
    assert diag.run(0, 0, extra=("matrix",)).keys() == {"matrix"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("matrix" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["matrix"] and "matrix" not in diag.REFERENCE_RATES
    assert "34 ops x 8000 rounds on 1024 SIMDs of 8 XCDs, 0 wrong elements" in diag._summary("matrix", r)


def test_a_wrong_element_fails_the_gpu_and_names_the_simd(node):
    op = "f8f6f4_32x32x64_fp4"
    node(4, {"bad": {(2, matrix.OPS.index(op)): 3}})
    r = diag.run(1, 2, extra=("matrix",))["matrix"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == f"3 wrong elements in {op} on xcd5/se1/cu7/simd2"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    assert r["ops"][op]["first_bad"] == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "reg": 1, "got": "0x4a82c74e",
                                         "want": "0x4a82c64e"}
    assert r["ops"]["f32_16x16x4_f32"]["errors"] == 0 and r["ops"]["f32_16x16x4_f32"]["first_bad"] is None
    assert diag.run(1, 1, extra=("matrix",))["matrix"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_matrix=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag matrix failed ("))
    assert f"3 wrong elements in {op} on xcd5/se1/cu7/simd2" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["matrix"])
    assert "FAIL" in line and "3 wrong elements" in line


def test_refused_calls_and_the_injection_knob_of_the_fake(node):
    node(1)
    with pytest.raises(ValueError):
        matrix.matrix_test(0, ops=("f32_16x16x4_f32",), inject_op="f64_16x16x4_f64")
    with pytest.raises(ValueError):
        matrix.matrix_test(0, ops=("no_such_op",))
    with pytest.raises(ValueError):
        matrix.matrix_test(0, ops=("f32_16x16x4_f32", "f32_16x16x4_f32"))
    with pytest.raises(RuntimeError, match=r"matrix failed \(-2\)"):
        matrix.matrix_test(0, iters=0)
    r = matrix.matrix_test(0, ops=("f32_16x16x4_f32", "f64_16x16x4_f64"), inject_op="f64_16x16x4_f64", inject_block=0)
    assert r["errors"] == 1 and list(r["ops"]) == ["f32_16x16x4_f32", "f64_16x16x4_f64"]
    assert len(r["ops"]["f64_16x16x4_f64"]["first_bad"]["got"]) == 18  # an fp64 element prints 16 digits


def test_an_agent_cycle_publishes_it_only_when_asked(node):
    bad = {"bad": {(1, 0): 1}}
    node(2, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 2, "matrix": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=2, diag_timeout=60, diag_when="always", isolation="process",
              diag_setup=setup)
    rep = A.Agent("n2", diag_matrix=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"matrix"} and g["diag"]["matrix"]["pass"] is (d != 1), (d, g["diag"].keys())
    rep = A.Agent("n2", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"]) and rep["state"] == H.HEALTHY


def test_the_flags(node, capsys):
    mlib = node(2)
    assert diag.main(["--level", "1", "--matrix", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["matrix", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(mlib.calls) == ["matrix0", "matrix1"]
    assert diag.main(["--level", "1"]) == 0
    assert "matrix" not in capsys.readouterr().out and len(mlib.calls) == 2
    mlib = node(1)
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--matrix"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and mlib.calls == ["matrix0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(mlib.calls) == 1
    assert A.build_parser().parse_args(["--node", "n", "--diag-matrix"]).diag_matrix is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_matrix is False
    for main, flag in ((diag.main, "--matrix"), (node_cycle.main, "--matrix"), (A.main, "--diag-matrix")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- build -----------------------------------------------------------------------------------------------------

def test_the_build_has_a_matrix_target():
    t = B._targets()
    assert "matrix" in t and t["matrix"]["out"].endswith("libmi355x_matrix.so")
    assert t["matrix"]["cmd"] == t["xgmi"]["cmd"] and t["matrix"]["headers"][0].endswith("matrix_ref.h")
    assert "libmi355x_matrix.so" in B.__doc__
