"""libmi355x_matrix.so on an MI355X: one application of every op held against the host's model word for word, a
plain one-hot matmul per C/D map class, the chained test clean at the smallest shape and at the default grid, both
self-check hooks, and the opt-in wiring up to ``mi355x-diag --matrix``.

These tests plant wrong values in data; none provokes a GPU fault.  No rate is asserted: the rates are reported
(profiles/matrix_mi355x.json) and never judged.

The model is csrc/matrix/matrix_ref.h itself, compiled here with the host compiler into a small program that prints
the generator's operands of each op and seed and the D registers matrix_apply() gives for them."""
import functools
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu

SEEDS = (0x3A7121, 1, 0xDEADBEEFCAFE)
# one dense 16x16, one dense 32x32, one f8f6f4 and one sparse op
HOOKED = ("f32_16x16x16_f16", "f32_32x32x8_f16", "f8f6f4_16x16x128_scale_fp6", "smfmac_f32_16x16x32_bf16")

MODEL_CPP = r"""
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
  for (int s = 1; s < argc; ++s) {
    const uint64_t seed = strtoull(argv[s], nullptr, 0);
    for (int op = 0; op < MATRIX_OPS; ++op) {
      if (matrix_operands(op, seed, 0, 0, o)) return 2;
      for (int i = 0; i < MATRIX_WAVE * MATRIX_CW; ++i) d[i] = 0;
      if (matrix_apply(op, o->A[0], o->B[0], o->C, o->idx[0], o->scale_a[0], o->scale_b[0], d)) return 3;
      printf("op %s %llu\n", MATRIX_OP_TABLE[op].name, static_cast<unsigned long long>(seed));
      row("A", o->A[0], MATRIX_WAVE * MATRIX_AW);
      row("B", o->B[0], MATRIX_WAVE * MATRIX_AW);
      row("C", o->C, MATRIX_WAVE * MATRIX_CW);
      row("idx", o->idx[0], MATRIX_WAVE);
      row("sa", o->scale_a[0], MATRIX_WAVE);
      row("sb", o->scale_b[0], MATRIX_WAVE);
      row("D", d, MATRIX_WAVE * MATRIX_CW);
    }
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def model_cases():
    """{(op name, seed): {"A", "B", "C", "idx", "sa", "sb", "D": words}} from matrix_ref.h"""
    from k8s_gpu_node_checker_amd import build as B
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "matrix_model.cpp"), os.path.join(tmp, "matrix_model")
        with open(src, "w") as f:
            f.write(MODEL_CPP)
        subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(B.CSRC, "matrix"), src, "-o", exe], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe, *[str(s) for s in SEEDS]], check=True, capture_output=True, text=True,
                             timeout=120).stdout
    cases, cur = {}, None
    for line in out.splitlines():
        f = line.split()
        if f[0] == "op":
            cur = cases.setdefault((f[1], int(f[2])), {})
        else:
            cur[f[0]] = [int(v, 16) for v in f[1:]]
    return cases


@pytest.fixture(scope="module")
def matrix():
    from k8s_gpu_node_checker_amd.ops import matrix as mx
    assert mx.device_count() >= 1
    return mx


def test_one_application_of_every_op_matches_the_model_word_for_word(matrix):
    cases = model_cases()
    assert len(cases) == len(matrix.OPS) * len(SEEDS)
    wrong = []
    for op in matrix.OPS:
        for seed in SEEDS:
            c = cases[(op, seed)]
            got = matrix.apply(op, c["A"], c["B"], c["C"], c["idx"], c["sa"], c["sb"])
            off = [i for i in range(len(got)) if got[i] != c["D"][i]]
            if off:
                wrong.append((op, seed, len(off), [(i // 16, i % 16, hex(got[i]), hex(c["D"][i])) for i in off[:4]]))
    print("ops x seeds checked:", len(cases), "disagreeing:", wrong)
    assert not wrong, wrong


def _f32(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _f64(v):
    lo, hi = struct.unpack("<II", struct.pack("<d", v))
    return [lo, hi]


@pytest.mark.parametrize("op,m,k", (("f32_16x16x4_f32", 16, 4), ("f32_32x32x2_f32", 32, 2), ("f64_16x16x4_f64", 16, 4)))
def test_a_one_hot_a_returns_the_rows_of_an_asymmetric_b(matrix, op, m, k):
    """A[i][kk] = 1 where kk == i % K, B[kk][j] = 100 (kk + 1) + j: D[i][j] must be B[i % K][j], in the register the
    C/D map of the op's class names.  A row / column swap, which symmetric data would hide, shows here."""
    f64 = op.startswith("f64")
    a, b = [0] * (64 * 8), [0] * (64 * 8)
    for lane in range(64):
        i, kk = lane % m, lane // m  # A: lane l holds A[l % M][l / M]; B: lane l holds B[l / N][l % N]
        av, bv = (1.0 if kk == i % k else 0.0), 100.0 * (lane // m + 1) + lane % m
        if f64:
            a[8 * lane:8 * lane + 2], b[8 * lane:8 * lane + 2] = _f64(av), _f64(bv)
        else:
            a[8 * lane], b[8 * lane] = _f32(av), _f32(bv)
    d = matrix.apply(op, a, b, [0] * (64 * 16))
    for lane in range(64):
        for reg in range(m * m // 64):
            if f64:
                row, col = (lane >> 4) + 4 * reg, lane & 15
                got = struct.unpack("<d", struct.pack("<II", d[16 * lane + 2 * reg], d[16 * lane + 2 * reg + 1]))[0]
            else:
                row, col = ((4 * (lane >> 4) + reg, lane & 15) if m == 16
                            else ((reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31))
                got = struct.unpack("<f", struct.pack("<I", d[16 * lane + reg]))[0]
            assert got == 100.0 * (row % k + 1) + col, (op, lane, reg, row, col, got)


def _clean(matrix, r, ops=None):
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and "bad_simds" not in r, r
    assert tuple(r["ops"]) == tuple(ops or matrix.OPS)
    for op, row in r["ops"].items():
        assert row["errors"] == 0 and row["first_bad"] is None and row["ms"] > 0 and row["tops"] > 0, (op, row)
    for slot in r["slots"]:
        assert re.fullmatch(r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]", matrix.simd_name(slot)), slot
    assert r["simds"] == len(r["slots"]) >= 1


def test_one_workgroup_one_round_is_clean(matrix):
    r = matrix.matrix_test(0, blocks=1, iters=1, reps=1, slots=True)
    print({k: v for k, v in r.items() if k != "ops"})
    _clean(matrix, r)
    assert r["blocks"] == 1 and r["iters"] == 1 and r["xcds"] >= 1


def test_the_default_grid_is_clean_on_every_xcd(matrix):
    from k8s_gpu_node_checker_amd.ops import diag
    r = matrix.matrix_test(0, iters=4, reps=1, slots=True)
    print(json.dumps({k: v for k, v in r.items() if k not in ("ops", "slots")}))
    _clean(matrix, r)
    cus = diag.device_info(0)["cus"]
    assert r["blocks"] == 2 * cus and r["simds"] == 4 * cus
    if cus == 256:
        assert r["simds"] == 1024 and r["xcds"] == 8


@pytest.mark.parametrize("op", HOOKED)
def test_an_injected_flip_is_one_wrong_element_in_that_op_only(matrix, op):
    r = matrix.matrix_test(0, ops=HOOKED, blocks=8, iters=4, reps=1, inject_op=op, inject_block=5)
    print(op, r["detail"], r["ops"][op])
    assert r["pass"] is False and r["errors"] == 1
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    bad = r["ops"][op]["first_bad"]
    assert bad["lane"] == 0 and bad["reg"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert re.fullmatch(r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]", bad["where"]), bad
    assert r["detail"] == f"1 wrong elements in {op} on {bad['where']}" and r["bad_simds"] == [f"{bad['where']} (1)"]


@pytest.mark.parametrize("op", HOOKED)
def test_a_skipped_instruction_shows_in_that_op_only(matrix, op):
    r = matrix.matrix_test(0, ops=HOOKED, blocks=8, iters=4, reps=1, inject_op=op, inject_block=5, inject_skip_step=2)
    print(op, r["detail"], r["ops"][op])
    m, n, _ = matrix.shape(op)
    assert r["pass"] is False and 0 < r["errors"] <= m * n  # one wave's accumulator at the most
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    assert r["ops"][op]["first_bad"]["got"] != r["ops"][op]["first_bad"]["want"]


def test_refused_calls(matrix):
    for kw in (dict(iters=0), dict(reps=0), dict(blocks=4, inject_op="f32_16x16x4_f32", inject_block=4),
               dict(iters=4, inject_op="f32_16x16x4_f32", inject_block=0, inject_skip_step=4)):
        with pytest.raises(RuntimeError, match=r"matrix failed \(-2\)"):
            matrix.matrix_test(0, **kw)


def test_diag_run_carries_a_passing_matrix_result(matrix):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(0, 0, extra=("matrix",))
    assert list(res) == ["matrix"] and res["matrix"]["pass"] and res["matrix"]["errors"] == 0
    assert tuple(res["matrix"]["ops"]) == matrix.OPS


def test_the_cli_flag_carries_a_passing_matrix_result(repo):
    def run(*flags):
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag",
                            "--level", "1", "--device", "0", "--format", "json", *flags], capture_output=True, text=True,
                           timeout=300, cwd=repo)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    tests = run("--matrix")
    assert tests["matrix"]["pass"] and tests["matrix"]["errors"] == 0 and len(tests["matrix"]["ops"]) == 34
    assert "matrix" not in run()
