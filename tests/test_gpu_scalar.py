"""libmi355x_scalar.so on an MI355X: one application of every op held against the host's model result for result and
SCC for SCC, the chains clean at the smallest shapes and at the default grid, the SGPR file and the scalar loads
clean, all four self-check hooks, and the opt-in wiring up to ``mi355x-diag --scalar``.

These tests plant wrong values in data; none provokes a GPU fault.  No rate is asserted: the rates are reported
(profiles/scalar_mi355x.json) and never judged.

The model is csrc/scalar/scalar_ref.h itself, compiled here with the host compiler into a small program that answers
"op a b scc" lines; tests/test_scalar_cpu.py holds that model against an independent implementation."""
import functools
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
# the operand set of tests/test_scalar_cpu.py: the edge values, the shift and field operands, seeded random pairs
EDGES_A = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff, 0x7fffffffffffffff, 0x8000000000000000, M64, 0x100000000,
           0xffffffff00000000)
SHIFTS = (0, 31, 32, 63, 64)
FIELDS = tuple(off | (w << 16) for off in SHIFTS for w in (0, 1, 32, 64))
EDGES_B = EDGES_A + SHIFTS + FIELDS + (0x00050003, 0x0008001c, 0x00100038)
HOOKED = ("s_addc_u32", "s_mul_hi_u32", "s_bfe_i64", "s_cselect_b32", "s_cmp_lt_u32")  # carry, multiplier, shifter,
#                                                                                       an SCC reader, a compare

ANSWER_CPP = r"""
#include <cinttypes>
#include <cstdio>
#include "scalar_ref.h"
int main() {
  int op, scc;
  unsigned long long a, b;
  while (scanf("%d %llx %llx %d", &op, &a, &b, &scc) == 4) {
    const ScalarOut o = scalar_apply(op, a, b, static_cast<uint32_t>(scc));
    printf("%" PRIx64 " %u\n", o.result, o.scc);
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def operands():
    rng = random.Random(0x5CA1A)
    rows = [(a, b, scc) for a in EDGES_A for b in EDGES_B for scc in (0, 1)]
    rows += [(rng.getrandbits(64), rng.getrandbits(64), i & 1) for i in range(64)]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def model_answers():
    """{op name: [(result, scc_out) for every row of operands()]} from scalar_ref.h, computed once."""
    from k8s_gpu_node_checker_amd import build as B
    from k8s_gpu_node_checker_amd.ops import scalar as S
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    stdin = "".join(f"{k} {a:x} {b:x} {scc}\n" for k in range(len(S.OPS)) for a, b, scc in operands())
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "scalar_answer.cpp"), os.path.join(tmp, "scalar_answer")
        with open(src, "w") as f:
            f.write(ANSWER_CPP)
        subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(B.CSRC, "scalar"), src, "-o", exe], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], input=stdin, check=True, capture_output=True, text=True, timeout=60).stdout
    rows = [(int(f[0], 16), int(f[1])) for f in (ln.split() for ln in out.splitlines())]
    n = len(operands())
    assert len(rows) == n * len(S.OPS)
    return {op: rows[k * n:(k + 1) * n] for k, op in enumerate(S.OPS)}


@pytest.fixture(scope="module")
def scalar():
    from k8s_gpu_node_checker_amd.ops import scalar as S
    assert S.device_count() >= 1
    return S


@pytest.fixture(scope="module")
def cus():
    from k8s_gpu_node_checker_amd.ops import diag
    return int(diag.device_info(0)["cus"])


def test_one_application_of_every_op_equals_the_model(scalar):
    """apply() of every op on the whole operand set: the device's result and SCC against the model's.  A disagreement
    is a finding: the ISA's rule decides which side is wrong."""
    wrong = []
    for op in scalar.OPS:
        got = scalar.apply_many(op, operands())
        for row, g, w in zip(operands(), got, model_answers()[op]):
            if g != w:
                wrong.append((op, hex(row[0]), hex(row[1]), row[2], "device", hex(g[0]), g[1], "model", hex(w[0]), w[1]))
    print(f"{len(scalar.OPS)} ops x {len(operands())} operand rows, {len(wrong)} disagreements")
    for w in wrong[:40]:
        print(*w)
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("iters", (1, 65))
def test_the_chains_are_clean_at_the_smallest_shapes(scalar, iters):
    r = scalar.scalar_test(0, parts=("salu",), blocks=8, iters=iters, reps=1)
    bad = {k: v for k, v in r["parts"]["salu"]["ops"].items() if v["errors"]}
    assert r["pass"] and r["errors"] == 0 and not bad, bad
    assert r["blocks"] == {"salu": 8} and tuple(r["parts"]["salu"]["ops"]) == scalar.OPS and r["simds"] >= 4


def test_the_chains_are_clean_at_the_default_grid(scalar, cus):
    r = scalar.scalar_test(0, parts=("salu",), iters=64, reps=1)
    assert r["errors"] == 0 and r["pass"], r["detail"]
    assert r["xcds"] == 8 and r["simds"] == 4 * cus and r["blocks"] == {"salu": 4 * cus}
    assert "bad_simds" not in r


def test_the_sgpr_file_is_clean_and_covers_the_stamped_range(scalar, cus):
    from k8s_gpu_node_checker_amd.ops import diag
    for blocks in (8, None):
        r = scalar.scalar_test(0, parts=("sgpr",), blocks=blocks, reps=1)
        p = r["parts"]["sgpr"]
        print("sgpr", blocks, json.dumps(p))
        assert r["pass"] and p["errors"] == 0 and p["first_bad"] is None, r["detail"]
        assert p["regs_per_wave"] == 75 and p["range"] == "s20-s95 without s32"
    assert "s20-31,s33-95" in diag.KERNEL_REVISION["scalar"]  # 12 + 63 registers: the count above
    assert r["blocks"] == {"sgpr": 7 * cus} and r["simds"] == 4 * cus and r["xcds"] == 8
    assert p["waves_per_simd"]["min"] >= 1 and p["bytes_per_simd"]["max"] == p["waves_per_simd"]["max"] * 75 * 4


@pytest.mark.parametrize("large_bytes", (4096, 64 * 1024))
def test_the_scalar_loads_are_clean(scalar, large_bytes):
    r = scalar.scalar_test(0, parts=("smem",), blocks=64, reps=1, small_bytes=4096, large_bytes=large_bytes, loads=128)
    kinds = r["parts"]["smem"]["kinds"]
    assert tuple(kinds) == scalar.SMEM_KINDS
    assert r["pass"] and all(v["errors"] == 0 and v["first_bad"] is None for v in kinds.values()), r["detail"]
    assert all(v["ms_hit"] > 0 and v["ms_miss"] > 0 for v in kinds.values())


def test_the_flip_hook_gives_one_wrong_word(scalar):
    for op in HOOKED:
        r = scalar.scalar_test(0, parts=("salu",), ops=HOOKED, blocks=8, iters=16, reps=1, inject_op=op, inject_block=5)
        rows = r["parts"]["salu"]["ops"]
        assert not r["pass"] and r["errors"] == 1 and {k: v["errors"] for k, v in rows.items() if v["errors"]} == {op: 1}
        bad = rows[op]["first_bad"]
        assert bad["chain"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10 and bad["where"].startswith("xcd")
        assert len(r["bad_simds"]) == 1 and r["bad_simds"][0] == f"{bad['where']} (1)"
    again = scalar.scalar_test(0, parts=("salu",), ops=HOOKED, blocks=8, iters=16, reps=1)
    assert again["pass"] and again["errors"] == 0  # an un-hooked call in the same process is clean again


def test_the_skip_hook_shows_in_that_op_only(scalar):
    for op in HOOKED:
        for step in (0, 15):
            r = scalar.scalar_test(0, parts=("salu",), ops=HOOKED, blocks=8, iters=16, reps=1, inject_op=op,
                                   inject_block=2, inject_skip_iter=step)
            rows = r["parts"]["salu"]["ops"]
            assert 1 <= rows[op]["errors"] <= scalar.CHAINS and r["errors"] == rows[op]["errors"], (op, step, r["detail"])
            assert rows[op]["first_bad"]["got"] != rows[op]["first_bad"]["want"]
    assert scalar.scalar_test(0, parts=("salu",), ops=HOOKED, blocks=8, iters=16, reps=1)["pass"]


def test_the_register_hook_names_the_register(scalar):
    rng = scalar.sgpr_range()
    for which, reg in (("lo", rng["lo"]), ("hi", rng["hi"])):
        r = scalar.scalar_test(0, parts=("sgpr",), blocks=8, reps=1, inject_reg=which, inject_block=3)
        p = r["parts"]["sgpr"]
        assert not r["pass"] and r["errors"] == p["errors"] == 1, r["detail"]
        bad = p["first_bad"]
        assert bad["reg"] == f"s{reg}" and bad["pattern"] == "hash" and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
        assert r["bad_simds"] == [f"{bad['where']} (1)"]
    assert scalar.scalar_test(0, parts=("sgpr",), blocks=8, reps=1)["pass"]


def test_the_table_hook_is_seen_by_every_kind_that_reads_the_word(scalar):
    r = scalar.scalar_test(0, parts=("smem",), blocks=8, reps=1, large_bytes=4096, loads=16, inject_word=77)
    for kind, row in r["parts"]["smem"]["kinds"].items():
        assert row["errors"] > 0 and row["first_bad"]["word"] == 77, (kind, row)
        assert int(row["first_bad"]["got"], 16) == int(row["first_bad"]["want"], 16) ^ 0x10
    assert not r["pass"]
    assert scalar.scalar_test(0, parts=("smem",), blocks=8, reps=1, large_bytes=4096, loads=16)["pass"]


def test_refusals(scalar):
    for kw in ({"iters": 0}, {"reps": 0}, {"blocks": 8, "inject_op": "s_add_u32", "inject_block": 8},
               {"parts": ("smem",), "small_bytes": 4000}, {"parts": ("smem",), "inject_word": 1024},
               {"parts": ("sgpr",), "hold": -1}):
        with pytest.raises(RuntimeError, match=r"scalar failed \(-2\)"):
            scalar.scalar_test(0, **kw)
    with pytest.raises(RuntimeError, match=r"scalar failed \(-2\)"):
        scalar.scalar_test(scalar.device_count())


def test_diag_run_and_the_cli_carry_the_three_parts(scalar):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(level=1, device=0, extra=("scalar",))
    r = res["scalar"]
    print("scalar via diag.run:", diag._summary("scalar", r), "wall", r["wall_s"])
    assert list(res)[-1] == "scalar" and r["pass"] and r["errors"] == 0, r.get("detail")
    assert tuple(r["parts"]) == scalar.PARTS and r["xcds"] == 8
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                        "--scalar"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    doc = json.loads(p.stdout)
    assert doc["pass"] and doc["devices"]["0"]["tests"]["scalar"]["pass"]
    assert set(doc["devices"]["0"]["tests"]["scalar"]["parts"]) == set(scalar.PARTS)
