"""Level 3 on CPU: the vector-ALU burn-in's host expectation (csrc/diag/valu_ref.h) against exact arithmetic, the
level tables and CLIs, and whole agent cycles at level 3 through the fake C ABI (testing/fake_native.py).  The
kernels themselves run on an MI355X in tests/test_gpu_simd.py."""
import functools
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import pytest

from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeDiagLib, FakeFabricLib
from k8s_gpu_node_checker_amd.testing.mock_apiserver import write_kubeconfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "k8s_gpu_node_checker_amd", "csrc", "diag")

LANES = (0, 1, 31, 63)
ITERS = (1, 16)

# prints, per kind / lane / chain / iters: the operands' bits, the expected bits, and the extremes of every
# intermediate; then the tables valu_tables() hands the kernel, to show they hold the same values
DUMP_CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "valu_ref.h"
static unsigned long long b64(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
static unsigned b32(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
int main() {
  const int lanes[] = {0, 1, 31, 63};
  const int iters[] = {1, 16};
  printf("consts %d %d %d %d\n", VALU_KINDS, VALU_CHAINS, VALU_UNROLL, VALU_LANES);
  for (int it : iters) {
    const long steps = static_cast<long>(it) * VALU_UNROLL;
    std::vector<uint64_t> ops[3], ex[3];
    for (int k = 0; k < 3; ++k) {
      ops[k].resize(3 * VALU_LANES * VALU_CHAINS);
      ex[k].resize(VALU_LANES * VALU_CHAINS);
      valu_tables(k, steps, ops[k].data(), ex[k].data());
    }
    for (int l : lanes)
      for (int c = 0; c < VALU_CHAINS; ++c) {
        const int i = l * VALU_CHAINS + c;
        const ValuFloatOps d = valu_float_ops(l, c, 0);
        double lo = d.x0, hi = d.x0;
        const double r = valu_expect_f64(l, c, steps, &lo, &hi);
        printf("f64 %d %d %d %016llx %016llx %016llx %016llx %016llx %016llx\n", it, l, c, b64(d.x0), b64(d.a), b64(d.b),
               b64(r), b64(lo), b64(hi));
        if (ops[0][3 * i] != b64(d.x0) || ops[0][3 * i + 1] != b64(d.a) || ops[0][3 * i + 2] != b64(d.b) ||
            ex[0][i] != b64(r)) return 3;
        unsigned long long packed[4] = {0, 0, 0, 0};
        for (int h = 0; h < 2; ++h) {
          const ValuFloatOps f = valu_float_ops(l, c, h);
          float flo = static_cast<float>(f.x0), fhi = flo;
          const float fr = valu_expect_f32(l, c, h, steps, &flo, &fhi);
          const float x0 = static_cast<float>(f.x0), a = static_cast<float>(f.a), b = static_cast<float>(f.b);
          if (x0 != f.x0 || a != f.a || b != f.b) return 4;  // every float operand is exact in fp32
          printf("f32 %d %d %d %d %08x %08x %08x %08x %08x %08x\n", it, l, c, h, b32(x0), b32(a), b32(b), b32(fr),
                 b32(flo), b32(fhi));
          packed[0] |= static_cast<unsigned long long>(b32(x0)) << (32 * h);
          packed[1] |= static_cast<unsigned long long>(b32(a)) << (32 * h);
          packed[2] |= static_cast<unsigned long long>(b32(b)) << (32 * h);
          packed[3] |= static_cast<unsigned long long>(b32(fr)) << (32 * h);
        }
        if (ops[1][3 * i] != packed[0] || ops[1][3 * i + 1] != packed[1] || ops[1][3 * i + 2] != packed[2] ||
            ex[1][i] != packed[3]) return 5;
        const ValuIntOps n = valu_int_ops(l, c);
        const uint64_t ir = valu_expect_i32(l, c, steps);
        printf("i32 %d %d %d %016llx %08x %016llx %016llx\n", it, l, c, (unsigned long long)n.x0, n.a,
               (unsigned long long)n.b, (unsigned long long)ir);
        if (ops[2][3 * i] != n.x0 || ops[2][3 * i + 1] != n.a || ops[2][3 * i + 2] != n.b || ex[2][i] != ir) return 6;
      }
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _dump():
    """valu_ref.h compiled with the host compiler into a stand-alone program; its output, parsed."""
    import tempfile
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "valu_dump.cpp"), os.path.join(tmp, "valu_dump")
        with open(src, "w") as f:
            f.write(DUMP_CPP)
        subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], check=True,
                       capture_output=True, text=True)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    assert rows[0] == ["consts", "3", "8", "4", "64"], rows[0]
    return rows[1:]


def _round(x: Fraction, bits: int) -> Fraction:
    """x > 0 rounded once to ``bits`` significant bits, to nearest, ties to even (no overflow or underflow here)."""
    assert x > 0
    e = 0
    while x >= Fraction(2) ** (e + 1):
        e += 1
    while x < Fraction(2) ** e:
        e -= 1
    ulp = Fraction(2) ** (e - bits + 1)
    q, r = divmod(x, ulp)
    if r > ulp / 2 or (r == ulp / 2 and q % 2 == 1):
        q += 1
    return q * ulp


def _f64(bits: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(bits, 16)))[0]


def _f32(bits: str) -> float:
    return struct.unpack("<f", struct.pack("<I", int(bits, 16)))[0]


def _check_float_chain(x0, a, b, want, lo, hi, steps, bits):
    # the stated operand ranges: a just below 1, the fixed point b / (1 - a) and x0 inside [0.75, 2)
    assert 1 - 32 / 1024 <= a < 1 and 1 <= x0 < 2 and 0.75 <= b / (1 - a) < 1.25, (x0, a, b)
    x, fa, fb = Fraction(x0), Fraction(a), Fraction(b)
    seen = [x]
    for _ in range(steps):
        x = _round(x * fa + fb, bits)   # the exact product-sum, rounded once
        seen.append(x)
    assert Fraction(want) == x, (x0, a, b, want, float(x))
    assert Fraction(lo) == min(seen) and Fraction(hi) == max(seen)
    # every intermediate normal and inside the stated range
    assert all(Fraction(1, 2) <= s < 2 for s in seen), (float(min(seen)), float(max(seen)))


def test_valu_ref_f64_matches_a_single_rounding_reference():
    rows = [r for r in _dump() if r[0] == "f64"]
    assert len(rows) == len(ITERS) * len(LANES) * 8
    ops = set()
    for _, it, lane, chain, x0, a, b, want, lo, hi in rows:
        assert int(it) in ITERS and int(lane) in LANES
        _check_float_chain(_f64(x0), _f64(a), _f64(b), _f64(want), _f64(lo), _f64(hi), 4 * int(it), 53)
        ops.add((x0, a, b))
    assert len(ops) == len(LANES) * 8, "operands must differ per lane and chain"


def test_valu_ref_pk_f32_matches_a_single_rounding_reference():
    rows = [r for r in _dump() if r[0] == "f32"]
    assert len(rows) == len(ITERS) * len(LANES) * 8 * 2
    ops = set()
    for _, it, lane, chain, half, x0, a, b, want, lo, hi in rows:
        _check_float_chain(_f32(x0), _f32(a), _f32(b), _f32(want), _f32(lo), _f32(hi), 4 * int(it), 24)
        ops.add((x0, a, b))
    assert len(ops) == len(LANES) * 8 * 2, "operands must differ per lane, chain and half"


def test_valu_ref_i32_matches_python_integers():
    rows = [r for r in _dump() if r[0] == "i32"]
    assert len(rows) == len(ITERS) * len(LANES) * 8
    ops = set()
    for _, it, lane, chain, x0, a, b, want in rows:
        x, ia, ib = int(x0, 16), int(a, 16), int(b, 16)
        assert ia % 2 == 1 and ia < 1 << 32
        for _ in range(4 * int(it)):
            x = ((x & 0xFFFFFFFF) * ia + ib) % (1 << 64)
        assert x == int(want, 16), (lane, chain, it)
        ops.add((x0, a, b))
    assert len(ops) == len(LANES) * 8


# ------------------------------------------------------------------------------------------------------ levels
def test_levels_one_and_two_are_unchanged_and_three_adds_the_simd_tests():
    assert diag.LEVELS[1] == ("gemm_quick", "gemm_fp8_quick", "hbm_quick", "hbm_xcd", "mfma", "lds", "l2")
    assert diag.LEVELS[2] == ("gemm", "gemm_fp8", "hbm", "hbm_xcd", "memtest", "mfma", "lds", "l2", "host_link")
    assert diag.LEVELS[3] == ("gemm", "gemm_fp8", "hbm", "hbm_xcd", "memtest", "mfma", "lds", "l2", "valu", "regfile",
                              "host_link")
    assert sorted(diag.LEVELS) == [0, 1, 2, 3]
    assert diag.uses_dma(3) and diag.uses_dma(2) and not diag.uses_dma(1)
    assert "valu" not in diag.REFERENCE_RATES or set(diag.REFERENCE_RATES["valu"]) <= set(diag.VALU_KINDS)
    assert "regfile" not in diag.REFERENCE_RATES  # no rate verdict
    assert diag.KERNEL_REVISION["valu"] and diag.KERNEL_REVISION["regfile"]
    assert diag.VALU_KINDS == ("f64", "pk_f32", "i32")


@pytest.fixture
def node(monkeypatch):
    """``node(n, **FakeDiagLib kwargs)``: an n x MI355X node on the fake diag / fabric libraries."""
    def install(n=1, **kw):
        lib = FakeDiagLib(n=n, **kw)
        fab = FakeFabricLib()
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(fabric, "_lib", fab)
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return lib
    return install


def test_the_three_clis_accept_level_three_and_refuse_four(node, capsys):
    lib = node(1)
    assert diag.main(["--level", "3", "--format", "text"]) == 0
    text = capsys.readouterr().out
    valu = next(ln for ln in text.splitlines() if ln.split()[:1] == ["valu"])
    regfile = next(ln for ln in text.splitlines() if ln.split()[:1] == ["regfile"])
    assert " pass " in valu and "f64" in valu and "pk_f32" in valu and "i32" in valu and "256 CUs" in valu, valu
    assert " pass " in regfile and "1024 SIMDs x 126 KiB (504 registers), 0 bad words" in regfile, regfile
    assert text.rstrip().endswith("result: PASS")
    assert lib.calls.count("valu") == 3 and lib.calls.count("regfile") == 1
    with pytest.raises(SystemExit):
        diag.main(["--level", "4"])
    assert A.build_parser().parse_args(["--diag-level", "3"]).diag_level == 3
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(["--diag-level", "4"])
    assert node_cycle.main(["--devices", "0", "--level", "3", "--no-fabric"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        node_cycle.main(["--devices", "0", "--level", "4"])
    capsys.readouterr()


def test_levels_one_and_two_do_not_run_the_simd_tests(node):
    lib = node(1)
    for level in (1, 2):
        res = diag.run(level, 0)
        assert "valu" not in res and "regfile" not in res
    assert "valu" not in lib.calls and "regfile" not in lib.calls


# ----------------------------------------------------------------------------------------------- agent cycles
def test_level_three_cycle_publishes_both_tests(node):
    node(2)
    ag = A.Agent("n2", source="fake", diag_level=3, expect_gpus=2, diag_timeout=60)
    rep = ag.probe_once()
    for g in rep["gpus"]:
        assert set(g["diag"]) == set(t for t in diag.LEVELS[3]), g["diag"].keys()
        assert all(r["pass"] and not r.get("degraded") for r in g["diag"].values()), g["diag"]
        v, r = g["diag"]["valu"], g["diag"]["regfile"]
        assert set(v["kinds"]) == set(diag.VALU_KINDS) and v["numerics"] == "" and v["map"]["cus"] == 256
        assert set(v["expect"]) <= set(diag.VALU_KINDS) and set(v["rates"]) == set(diag.VALU_KINDS)
        assert r["errors"] == 0 and r["simds"] == 1024 and r["by_file"] == {"vgpr": 0, "agpr": 0}
        assert r["regs_per_lane"] == 504 and r["bytes_per_simd"] == 504 * 256 and r["scratch_bytes"] == 0
    assert "fabric" in rep  # everything the agent does at level >= 2 holds for 3
    assert rep["state"] == H.HEALTHY and ag.evaluate(rep).state == H.HEALTHY


def test_a_regfile_error_makes_the_node_unhealthy_and_names_the_simd(node, mock_cluster, run_cli, tmp_path):
    # xcd5 / se1 / cu6 / simd2: one VGPR word and two AGPR words wrong on gpu1
    row = (((5 << 7) | (1 << 5) | 6) << 2) | 2
    node(2, regfile_bad={(1, row): (1, 2)})
    ag = A.Agent("n2", source="fake", diag_level=3, expect_gpus=2)
    rep = ag.probe_once()
    r = rep["gpus"][1]["diag"]["regfile"]
    assert not r["pass"] and r["errors"] == 3 and r["by_file"] == {"vgpr": 1, "agpr": 2}
    assert r["bad_simds"] == ["xcd5/se1/cu6/simd2 (vgpr 1, agpr 2)"]
    assert rep["gpus"][0]["diag"]["regfile"]["pass"]
    v = ag.evaluate(rep)
    assert rep["state"] == H.UNHEALTHY and v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (1, 2)
    reason = next(x for x in v.reasons if x.startswith("gpu1: diag regfile failed"))
    assert "xcd5/se1/cu6/simd2 (vgpr 1, agpr 2)" in reason and "3 register words wrong" in reason
    text = diag.render_text({"devices": {1: {"info": {}, "tests": rep["gpus"][1]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["regfile"])
    assert "FAIL" in line and "3 bad words" in line and "xcd5/se1/cu6/simd2" in text
    assert any(ln.split()[:2] == ["valu", "pass"] for ln in text.splitlines())
    # check-gpu-node --explain on the published report: the GPU's row and the reason name the test and the SIMD
    n = fixtures.realistic_node("n2", index=0, annotations=fixtures.health_annotation(rep),
                                extra_conditions=[fixtures.health_condition(rep, 2)])
    kc = write_kubeconfig(str(tmp_path / "kc"), mock_cluster([n]).url)
    p = run_cli(["--kubeconfig", kc, "--explain", "n2"])
    assert p.returncode == 3, p.stdout + p.stderr
    assert "reason: gpu1: diag regfile failed" in p.stdout and "xcd5/se1/cu6/simd2" in p.stdout
    row1 = next(ln for ln in p.stdout.splitlines() if ln.startswith("  1 "))
    assert "fail: regfile" in row1, row1


def test_a_wrong_valu_lane_fails_and_names_the_cu(node):
    slot = (2 << 7) | (3 << 5) | 4
    node(1, valu_errors={(0, 0): 2}, valu_bad_cu={(0, 0): slot})
    ag = A.Agent("n1", source="fake", diag_level=3, expect_gpus=1)
    rep = ag.probe_once()
    r = rep["gpus"][0]["diag"]["valu"]
    assert not r["pass"] and r["kinds"]["f64"]["errors"] == 2 and r["kinds"]["i32"]["errors"] == 0
    assert r["map"]["bad_cus"] == ["xcd2/se3/cu4 (f64 2)"] and "f64: 2 wrong results" in r["numerics"]
    v = ag.evaluate(rep)
    assert v.state == H.UNHEALTHY
    assert any(x.startswith("gpu0: diag valu failed") and "xcd2/se3/cu4" in x for x in v.reasons), v.reasons


def test_a_lagging_xcd_in_valu_is_degraded_not_failed(node, mock_cluster, run_cli, tmp_path):
    node(1, valu_slow_xcd={6: 1.3})
    ag = A.Agent("n1", source="fake", diag_level=3, expect_gpus=1)
    rep = ag.probe_once()
    d = rep["gpus"][0]["diag"]
    r = d["valu"]
    assert r["pass"] and r["degraded"] and r["numerics"] == "", r
    assert r["lag"] == ["xcd6 waves take 1.30x the median XCD's time"] and r["detail"] == r["lag"][0]
    assert d["mfma"]["pass"] and not d["mfma"].get("degraded")  # the matrix-core waves of that XCD keep up
    v = ag.evaluate(rep)
    assert v.state != H.UNHEALTHY and any("diag valu slow" in w and "xcd6" in w for w in v.warnings), (v.state, v.warnings)
    text = diag.render_text({"devices": {0: {"info": {}, "tests": d}}, "pass": True})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["valu"])
    assert "DEGRADED" in line and "xcd6 waves take 1.30x" in text
    assert any(ln.split()[:2] == ["regfile", "pass"] for ln in text.splitlines())
    n = fixtures.realistic_node("n1", index=0, annotations=fixtures.health_annotation(rep),
                                extra_conditions=[fixtures.health_condition(rep, 1)])
    kc = write_kubeconfig(str(tmp_path / "kc"), mock_cluster([n]).url)
    p = run_cli(["--kubeconfig", kc, "--explain", "n1"])
    row0 = next(ln for ln in p.stdout.splitlines() if ln.startswith("  0 "))
    assert "slow: valu" in row0 and "diag valu slow" in p.stdout, p.stdout


def test_self_check_hooks_through_the_fake_abi(node):
    node(1)
    for i, reg in enumerate(diag.REGFILE_REGS):
        r = diag.regfile_test(0, rounds=1, inject_block=5, inject_reg=reg)
        assert r["errors"] == 1 and r["by_file"] == ({"vgpr": 1, "agpr": 0} if i < 2 else {"vgpr": 0, "agpr": 1}), r
        assert not r["pass"] and len(r["bad_simds"]) == 1 and len(r["simd_map"]) == 3 * 4096
    r = diag.valu_burn(0, kinds=("pk_f32",), iters=16, reps=1, inject_block=5)
    assert r["kinds"]["pk_f32"]["errors"] == 1 and not r["pass"] and r["rates"]["pk_f32"] > 0
    assert diag._one("regfile", 0, diag.FULL)["pass"] and diag._one("valu", 0, diag.FULL)["pass"]
    assert diag.simd_name((((7 << 7) | (2 << 5) | (1 << 4) | 9) << 2) | 3) == "xcd7/se2/cu9/sh1/simd3"
