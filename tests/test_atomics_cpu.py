"""The atomics diagnostic on CPU: the C ABI of csrc/atomics/atomics.hip against ops/atomics.py and its fake, the
reference header against the element types' own arithmetic in shuffled orders, the instructions the kernels compile
to, the opt-in wiring (ops/diag.run(extra=...), the CLIs, whole agent cycles in both isolation modes) and the build
target.  The kernels themselves run on an MI355X in tests/test_gpu_atomics.py."""
import ctypes
import functools
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, atomics, diag, fabric
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeAtomicsLib, FakeDiagLib, FakeFabricLib,
                                                          c_exports)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "atomics")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")


# --- 1. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    import inspect
    exports, sig = c_exports("atomics"), atomics._signatures()
    assert set(exports) == set(sig) == {"atomics_last_error", "atomics_device_count", "atomics_test"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeAtomicsLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["atomics_test"]) == 17
    assert len(atomics.KINDS) == FakeAtomicsLib.KINDS == 8 and atomics.MAX_ADDERS == 32


# --- 2. the reference header, alone under the host compiler ----------------------------------------------------

REF_CPP = r"""
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "atomics_ref.h"

static float f32_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static double f64_of(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }
// bf16 as the memory-side adder keeps it: the fp32 sum rounded to nearest-even at 8 significant bits after every add
static uint32_t bf16_add(uint32_t a, uint32_t b) {
  uint32_t u = atomics_f32_bits(f32_of(a << 16) + f32_of(b << 16));
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
// one operand applied to an element, in the element type's own arithmetic
static uint64_t apply(int kind, uint64_t x, uint64_t v) {
  switch (kind) {
    case ATOMICS_ADD_U32: return static_cast<uint32_t>(static_cast<uint32_t>(x) + static_cast<uint32_t>(v));
    case ATOMICS_ADD_U64: return x + v;
    case ATOMICS_ADD_F32: return atomics_f32_bits(f32_of(static_cast<uint32_t>(x)) + f32_of(static_cast<uint32_t>(v)));
    case ATOMICS_ADD_F64: return atomics_f64_bits(f64_of(x) + f64_of(v));
    case ATOMICS_PK_BF16:
      return bf16_add(x & 0xffff, v & 0xffff) | (bf16_add((x >> 16) & 0xffff, (v >> 16) & 0xffff) << 16);
    case ATOMICS_MAX_U32: return std::max(x, v);
    default: return x ^ v;
  }
}

int main() {
  std::mt19937_64 rng(12345);
  long checked = 0;
  const int adders_of[3] = {1, 8, 32};
  for (int kind = 0; kind < ATOMICS_TICKET; ++kind) {
    for (int adders : adders_of) {
      for (uint64_t i = 0; i < 300; ++i) {
        const uint64_t seed = 0xA70C5 + 977 * i, elem = i * 7919 + (i % 3 ? 0 : (1ULL << 31) - 150);
        std::vector<int> order(adders);
        for (int a = 0; a < adders; ++a) order[a] = a;
        const uint64_t want = atomics_expected(kind, elem, adders, seed);
        for (int trial = 0; trial < 8; ++trial) {  // as dealt, reversed, then shuffled
          if (trial == 1) std::reverse(order.begin(), order.end());
          if (trial > 1) std::shuffle(order.begin(), order.end(), rng);
          const int without = trial % 4 == 3 ? order[trial % adders] : -1;  // some orders lose one operand
          uint64_t x = atomics_init(kind, elem, seed);
          for (int a : order) {
            const uint64_t v = atomics_operand(kind, elem, a, seed);
            if (kind != ATOMICS_MAX_U32 && (v & (atomics_elem_bytes(kind) == 8 ? ~0ULL : 0xffffffffULL)) == 0) {
              printf("zero operand kind %d elem %llu adder %d\n", kind, (unsigned long long)elem, a);
              return 1;
            }
            if (a != without) x = apply(kind, x, v);
          }
          const uint64_t w = without < 0 ? want : atomics_expected(kind, elem, adders, seed, without);
          if (x != w) {
            printf("kind %d adders %d elem %llu trial %d without %d: got %llx want %llx\n", kind, adders,
                   (unsigned long long)elem, trial, without, (unsigned long long)x, (unsigned long long)w);
            return 1;
          }
          if (without >= 0 && kind != ATOMICS_MAX_U32 && w == want) {
            printf("kind %d: a lost operand does not show\n", kind);
            return 1;
          }
          ++checked;
        }
      }
    }
  }
  // the stated magnitudes of the float kinds' integers
  for (uint64_t h = 0; h < 200000; ++h) {
    const uint64_t r = atomics_hash(h, 3, h, 1);
    for (int slot = 0; slot < 2; ++slot) {
      const long long f = atomics_int(r, ATOMICS_F32_MAX, slot), d = atomics_int(r, ATOMICS_F64_MAX, slot);
      const int p = atomics_pk_int(r, 0, slot), q = atomics_pk_int(r, 1, slot);
      if (f < -ATOMICS_F32_MAX || f > ATOMICS_F32_MAX || d < -ATOMICS_F64_MAX || d > ATOMICS_F64_MAX || p < -7 || p > 7 ||
          q < -7 || q > 7 || (slot && (!f || !d || !p || !q))) {
        printf("operand out of range\n");
        return 1;
      }
    }
  }
  // the ticket plan: draws in element order fill every counter and mark every hit word once
  const uint64_t shapes[8] = {1, 63, 64, 65, 1000, 4097, 16384 * 3 + 5, (1u << 20) + 77};
  for (uint64_t words : shapes) {
    for (int adders : adders_of) {
      const AtomicsTicketPlan p = atomics_ticket_plan(words, adders);
      if (p.words > words || p.words > ATOMICS_TICKET_MAX_WORDS || (p.counters < 64 && p.counters != p.words)) {
        printf("ticket plan %llu\n", (unsigned long long)words);
        return 1;
      }
      std::vector<uint32_t> mem(p.elements(), 0);
      for (int a = 0; a < adders; ++a)
        for (uint64_t i = 0; i < p.words; ++i) {
          const uint64_t c = i % p.counters, t = mem[p.hits() + c]++;
          if (t >= p.tickets) {
            printf("ticket beyond the row: words %llu adders %d\n", (unsigned long long)words, adders);
            return 1;
          }
          ++mem[c * p.tickets + t];
        }
      for (uint64_t e = 0; e < p.elements(); ++e)
        if (mem[e] != atomics_ticket_expected(p, e, adders)) {
          printf("ticket words %llu adders %d element %llu\n", (unsigned long long)words, adders, (unsigned long long)e);
          return 1;
        }
      ++checked;
    }
  }
  printf("ok %ld\n", checked);
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _ref_program(sanitize):
    """atomics_ref.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "atomics_ref.cpp"), os.path.join(tmp, "atomics_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


def test_every_order_of_arrival_gives_the_expected_value():
    rc, out = _ref_program(False)
    assert rc == 0, out
    # 7 kinds x 3 adder counts x 300 elements x 8 orders, and 8 x 3 ticket plans
    assert out.strip() == f"ok {7 * 3 * 300 * 8 + 8 * 3}", out


def test_the_reference_is_clean_under_the_host_sanitizers():
    rc, out = _ref_program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and out.strip().startswith("ok "), out


# --- 3. instructions -------------------------------------------------------------------------------------------

def test_every_kind_compiles_to_its_native_instruction():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "atomics.s")
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(CSRC, "atomics.hip"), "-o", asm], check=True, capture_output=True, text=True)
        with open(asm) as f:
            text = f.read()
    for pattern in (r"global_atomic_add\s", r"global_atomic_add_x2\s", r"global_atomic_add_f32\s",
                    r"global_atomic_add_f64\s", r"global_atomic_pk_add_bf16\s", r"global_atomic_umax\s",
                    r"global_atomic_xor\s", r"global_atomic_add\s[^\n]*\bsc0\b"):  # the last: the returning form
        assert re.search(r"^\s*" + pattern, text, re.M), pattern
    assert "cmpswap" not in text  # no compare-and-swap loop stands in for an atomic
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # and no kernel spills


# --- 4. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, atomics_kw, **FakeDiagLib kwargs)`` -> (FakeDiagLib, FakeAtomicsLib) for an n x MI355X node."""
    def install(n=1, atomics_kw=None, **kw):
        lib, alib = FakeDiagLib(n=n, **kw), FakeAtomicsLib(n=n, **(atomics_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(atomics, "lib", lambda: alib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return lib, alib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}


def test_off_by_default_and_on_when_asked(node):
    lib, alib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and alib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and alib.calls == []
    res = diag.run(1, 0, extra=("atomics",))
    assert list(res)[-1] == "atomics" and set(res) == LEVEL1 | {"atomics"} and alib.calls == ["atomics0"]
    r = res["atomics"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["words"] == 16 << 20 and r["adders"] == 8
    assert set(r) == {"pass", "errors", "kinds", "words", "adders", "ms", "wall_s", "detail"}
    assert set(r["kinds"]) == set(atomics.KINDS)
    for row in r["kinds"].values():
        assert set(row) >= {"errors", "first_bad", "got", "want", "ops", "xcds", "gbs"}
        assert row["xcds"] == 8 and row["ops"] == (16 << 20) * 8 and row["first_bad"] is None and row["gbs"] > 0
    assert diag.run(0, 0, extra=("atomics",)).keys() == {"atomics"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("atomics" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["atomics"] and "atomics" not in diag.REFERENCE_RATES
    assert "atomics" not in diag.DMA_TESTS | diag.SHARED_TESTS
    line = diag._summary("atomics", r)
    assert "16777216 elements x 8 adders from 8 XCDs, 0 wrong" in line and "pk_bf16" in line


def test_a_wrong_element_fails_the_gpu_and_the_node(node):
    lib, alib = node(4, {"wrong": {(2, atomics.KINDS.index("add_f32")): 3}})
    r = diag.run(1, 2, extra=("atomics",))["atomics"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == "3 elements wrong in add_f32 (first at +0x1a40: got 0x47800000, want 0x47800100)"
    assert r["kinds"]["add_f32"]["first_bad"] == 0x690 and r["kinds"]["add_u32"]["errors"] == 0
    assert diag.run(1, 1, extra=("atomics",))["atomics"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_atomics=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag atomics failed ("))
    assert "3 elements wrong in add_f32" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["atomics"])
    assert "FAIL" in line and "3 wrong" in line and "first at +0x1a40" in text


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    monkeypatch.setitem(diag._TESTS, "atomics", ("atomics_test", {"adders": 33}))
    r = diag.run(1, 0, extra=("atomics",))["atomics"]
    assert r["pass"] is False and "atomics failed (-2)" in r["detail"] and "adders 1..32" in r["detail"]
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(atomics, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("atomics",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, monkeypatch, isolation):
    node(8, {"wrong": {(5, 0): 1}})
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "atomics": {"wrong": {(5, 0): 1}}})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_atomics=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"atomics"}, (d, g["diag"].keys())
        assert g["diag"]["atomics"]["pass"] is (d != 5), (d, g["diag"]["atomics"])
    assert "1 elements wrong in add_u32" in rep["gpus"][5]["diag"]["atomics"]["detail"]  # each child ran its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    lib, alib = node(2)
    assert diag.main(["--level", "1", "--atomics", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["atomics", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(alib.calls) == ["atomics0", "atomics1"]  # one thread per GPU: in either order
    assert diag.main(["--level", "1"]) == 0
    assert "atomics" not in capsys.readouterr().out and len(alib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--atomics", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [("atomics",), None]
    capsys.readouterr()
    monkeypatch.undo()
    lib, alib = node(1)
    b = diag.burn_in(1, [0], 0.0, extra=("atomics",))
    assert b["pass"] and b["rounds"] == 1 and alib.calls == ["atomics0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--atomics"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and alib.calls == ["atomics0", "atomics0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(alib.calls) == 2
    assert A.build_parser().parse_args(["--node", "n", "--diag-atomics"]).diag_atomics is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_atomics is False
    for main, flag in ((diag.main, "--atomics"), (node_cycle.main, "--atomics"), (A.main, "--diag-atomics")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 5. build --------------------------------------------------------------------------------------------------

def test_the_build_has_an_atomics_target(tmp_path, monkeypatch):
    t = B._targets()
    assert "atomics" in t and t["atomics"]["out"].endswith("libmi355x_atomics.so")
    assert t["atomics"]["cmd"] == t["xgmi"]["cmd"] and t["atomics"]["headers"][0].endswith("atomics_ref.h")
    assert "libmi355x_atomics.so" in B.__doc__
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    monkeypatch.setattr(B, "OUT", str(tmp_path))  # a fresh output directory: the tree's own library stays as it is
    msgs = B.build(only=["atomics"])
    assert msgs == [f"atomics: built {os.path.relpath(os.path.join(str(tmp_path), 'libmi355x_atomics.so'), os.path.dirname(B.PKG))}"]
    L = ctypes.CDLL(os.path.join(str(tmp_path), "libmi355x_atomics.so"))
    for name in atomics._signatures():
        getattr(L, name)  # AttributeError: not exported
    assert B.build(only=["atomics"]) == []  # up to date
