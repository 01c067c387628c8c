"""The lanes diagnostic on CPU: the model of csrc/lanes/lanes_ref.h against tables worked by hand from the ISA's
rules, the condition that no op's chain hides a crossing that did not happen, the C ABI of csrc/lanes/lanes.hip
against ops/lanes.py and its fake, the instructions the kernels compile to, the opt-in wiring (ops/diag.run(extra=...),
the CLIs, whole agent cycles) and the build target.  The kernels themselves run on an MI355X in
tests/test_gpu_lanes.py."""
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
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, atomics, diag, fabric, lanes
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeAtomicsLib, FakeDiagLib, FakeFabricLib, FakeLanesLib,
                                                          c_exports)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "lanes")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
M = 0xffffffff


# --- 1. the reference header, alone under the host compiler ----------------------------------------------------

# Prints, for every op: its name, one application at steps 0 and 5 on x[i] = i, y[i] = ~i (both registers), the
# ds_(b)permute lane map, whether a skipped crossing shows (iters 8, skip 0 / 1 / 7), and a checksum of the expected
# words at iters 3.
REF_CPP = r"""
#include <cstdio>
#include "lanes_ref.h"

static void row(const char* tag, int op, int it, const uint32_t* v) {
  printf("%s %d %d", tag, op, it);
  for (int i = 0; i < LANES_WAVE; ++i) printf(" %u", v[i]);
  printf("\n");
}

int main() {
  for (int op = 0; op < LANES_OPS; ++op) {
    printf("op %d %s\n", op, LANES_OP_TABLE[op].name);
    for (int it = 0; it <= 5; it += 5) {
      uint32_t x[LANES_WAVE], y[LANES_WAVE];
      for (int i = 0; i < LANES_WAVE; ++i) x[i] = static_cast<uint32_t>(i), y[i] = ~x[i];
      lanes_apply(op, static_cast<uint32_t>(it), x, y);
      row("x", op, it, x);
      row("y", op, it, y);
    }
    uint32_t idx[LANES_WAVE];
    for (int i = 0; i < LANES_WAVE; ++i) idx[i] = static_cast<uint32_t>(lanes_perm_index(op, i));
    row("index", op, 0, idx);
    const int iters = 8, skips[3] = {0, 1, iters - 1};
    uint32_t want[LANES_WAVE * LANES_CHAINS], got[LANES_WAVE * LANES_CHAINS];
    lanes_expected(op, 0x1A7E5, iters, -1, want);
    for (int s : skips) {
      lanes_expected(op, 0x1A7E5, iters, s, got);
      int differ = 0;
      for (int i = 0; i < LANES_WAVE * LANES_CHAINS; ++i) differ += got[i] != want[i];
      printf("skip %d %d %d\n", op, s, differ);
    }
    lanes_expected(op, 0x1A7E5, 3, -1, want);
    uint32_t sum = 0;
    for (int i = 0; i < LANES_WAVE * LANES_CHAINS; ++i) sum = sum * 31u + want[i];
    printf("sum3 %d %u\n", op, sum);
  }
  printf("ok %d\n", LANES_OPS);
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _ref_program(sanitize):
    """lanes_ref.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lanes_ref.cpp"), os.path.join(tmp, "lanes_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


@functools.lru_cache(maxsize=None)
def _model():
    """The driver's output parsed: names, {(reg, op name, step): 64 words}, {op name: lane map}, {(op name, skip):
    differing words}."""
    rc, out = _ref_program(False)
    assert rc == 0 and out.strip().endswith(f"ok {len(lanes.OPS)}"), out
    names, regs, index, skips = {}, {}, {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "op":
            names[int(f[1])] = f[2]
        elif f[0] in ("x", "y"):
            regs[(f[0], names[int(f[1])], int(f[2]))] = [int(v) for v in f[3:]]
        elif f[0] == "index":
            index[names[int(f[1])]] = [int(v) for v in f[3:]]
        elif f[0] == "skip":
            skips[(names[int(f[1])], int(f[2]))] = int(f[3])
    return names, regs, index, skips


def test_the_op_table_is_the_python_one():
    names = _model()[0]
    assert tuple(names[k] for k in range(len(names))) == lanes.OPS
    assert len(set(lanes.OPS)) == len(lanes.OPS) == FakeLanesLib.OPS <= 64


def old(i):
    return ~i & M


def row16(i):
    return i // 16


# What each op must leave in x for x[i] = i, old = y[i] = ~i, worked by hand from the ISA's rules (not from the
# header): a row is 16 lanes, a bank 4 lanes of a row, out-of-range sources and masked-off lanes keep `old`.
HAND_X = {
    "dpp_quad_perm_1032": [i ^ 1 for i in range(64)],
    "dpp_quad_perm_2301": [i ^ 2 for i in range(64)],
    "dpp_quad_perm_3210": [i ^ 3 for i in range(64)],
    "dpp_quad_perm_0000": [i & ~3 for i in range(64)],
    "dpp_row_shl1": [old(i) if i % 16 == 15 else i + 1 for i in range(64)],
    "dpp_row_shr1": [old(i) if i % 16 == 0 else i - 1 for i in range(64)],  # lanes 0, 16, 32, 48 keep old
    "dpp_row_shr2": [old(i) if i % 16 < 2 else i - 2 for i in range(64)],
    "dpp_row_shr3": [old(i) if i % 16 < 3 else i - 3 for i in range(64)],
    "dpp_row_shr8": [old(i) if i % 16 < 8 else i - 8 for i in range(64)],
    "dpp_row_ror1": [16 * row16(i) + (i - 1) % 16 for i in range(64)],
    "dpp_row_ror4": [16 * row16(i) + (i - 4) % 16 for i in range(64)],
    "dpp_wave_shl1": [old(63) if i == 63 else i + 1 for i in range(64)],
    "dpp_wave_shr1": [old(0) if i == 0 else i - 1 for i in range(64)],      # only lane 0 keeps old
    "dpp_wave_rol1": [(i + 1) % 64 for i in range(64)],
    "dpp_wave_ror1": [(i - 1) % 64 for i in range(64)],                     # lane 0 = 63
    "dpp_row_mirror": [16 * row16(i) + 15 - i % 16 for i in range(64)],
    "dpp_row_half_mirror": [8 * (i // 8) + 7 - i % 8 for i in range(64)],
    # row_mask 0xa: rows 1 and 3 are written, with lane 15 / lane 47; rows 0 and 2 keep old
    "dpp_row_bcast15": [old(i) for i in range(16)] + [15] * 16 + [old(i) for i in range(32, 48)] + [47] * 16,
    # row_mask 0xc: rows 2 and 3 are written with lane 31; rows 0 and 1 keep old
    "dpp_row_bcast31": [old(i) for i in range(32)] + [31] * 32,
    "dpp_row_shr1_bound_ctrl": [0 if i % 16 == 0 else i - 1 for i in range(64)],  # those lanes are 0
    # row_mask 0x5: rows 0 and 2; bank_mask 0xa: banks 1 and 3 (lanes 4-7 and 12-15 of a row)
    "dpp_row_shr1_masked": [i - 1 if row16(i) in (0, 2) and (i % 16) // 4 in (1, 3) else old(i) for i in range(64)],
    "swizzle_xor1": [i ^ 1 for i in range(64)],
    "swizzle_xor2": [i ^ 2 for i in range(64)],
    "swizzle_xor4": [i ^ 4 for i in range(64)],
    "swizzle_xor8": [i ^ 8 for i in range(64)],
    "swizzle_xor16": [i ^ 16 for i in range(64)],
    "swizzle_reverse32": [32 * (i // 32) + 31 - i % 32 for i in range(64)],
    "swizzle_bcast0": [0] * 32 + [32] * 32,
    "swizzle_quad_2031": [4 * (i // 4) + (2, 0, 3, 1)[i % 4] for i in range(64)],
    "bpermute_xor32": [i ^ 32 for i in range(64)],
    "bpermute_rot1": [(i + 1) % 64 for i in range(64)],
    "permute_rot17": [(i - 17) % 64 for i in range(64)],  # lane i writes lane i + 17: lane j holds lane j - 17's
    # vdst[32..63] <-> src[0..31]: the upper half of x now holds y's lower half (~0 .. ~31)
    "permlane32_swap": list(range(32)) + [old(i - 32) for i in range(32, 64)],
    # the odd rows of vdst <-> the even rows of src: x rows 1 and 3 now hold y's rows 0 and 2
    "permlane16_swap": [old(i - 16) if row16(i) % 2 else i for i in range(64)],
    "readlane": [3] * 64,  # step 0: lane (7 * 0 + 3) & 63
    "readfirstlane": [0] * 64,  # step 0: every lane is active, the first is lane 0
}
HAND_Y = {  # the second register, where the op writes it
    "permlane32_swap": [i + 32 for i in range(32)] + [old(i) for i in range(32, 64)],
    "permlane16_swap": [old(i) if row16(i) % 2 else i + 16 for i in range(64)],
}
HAND_X_STEP5 = {
    "readlane": [(7 * 5 + 3) & 63] * 64,
    "readfirstlane": [0, 1, 2, 3, 4] + [5] * 59,  # under `if (lane >= 5)`: lanes 0-4 are inactive and keep theirs
}


@pytest.mark.parametrize("name", sorted(HAND_X))
def test_the_model_gives_the_hand_worked_table(name):
    regs = _model()[1]
    assert regs[("x", name, 0)] == [v & M for v in HAND_X[name]]
    assert regs[("y", name, 0)] == HAND_Y.get(name, [old(i) for i in range(64)])  # untouched unless the op swaps
    if name in HAND_X_STEP5:
        assert regs[("x", name, 5)] == HAND_X_STEP5[name]
    else:
        assert regs[("x", name, 5)] == regs[("x", name, 0)]  # only the lane port depends on the step


def test_every_op_has_a_hand_worked_table_or_a_checked_map():
    index, regs = _model()[2], _model()[1]
    seeded = set(lanes.OPS) - set(HAND_X)
    assert seeded == {"bpermute_seeded", "bpermute_gather", "permute_seeded"}
    # the seeded ds_permute maps are bijections (who wins a collision is never relied on) ...
    for name in ("permute_rot17", "permute_seeded", "bpermute_seeded"):
        assert sorted(index[name]) == list(range(64)), name
    assert index["permute_seeded"] != index["bpermute_seeded"] and index["permute_seeded"] != list(range(64))
    # ... the gather is not injective, and both are applied as their instruction's rule says
    assert len(set(index["bpermute_gather"])) < 64
    for name in ("bpermute_seeded", "bpermute_gather"):
        assert regs[("x", name, 0)] == index[name]  # a gather: lane i reads lane index[i]
    scattered = [None] * 64
    for i, dst in enumerate(index["permute_seeded"]):
        scattered[dst] = i  # a scatter: lane i writes lane index[i]
    assert regs[("x", "permute_seeded", 0)] == scattered


@pytest.mark.parametrize("name", lanes.OPS)
def test_no_op_is_degenerate(name):
    """A chain whose crossing was left out once (at its first, second or last step of 8) must end different from the
    expected words in at least one lane: otherwise the test could not see that crossing fail."""
    skips = _model()[3]
    for s in (0, 1, 7):
        assert skips[(name, s)] > 0, (name, s)


def test_the_reference_is_clean_under_the_host_sanitizers():
    rc, out = _ref_program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and out.strip().endswith(f"ok {len(lanes.OPS)}"), out
    assert len(re.findall(r"^sum3 ", out, re.M)) == len(lanes.OPS)  # every op's model ran at iters 3


# --- 2. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    import inspect
    exports, sig = c_exports("lanes"), lanes._signatures()
    assert set(exports) == set(sig) == {"lanes_last_error", "lanes_device_count", "lanes_slots", "lanes_test",
                                        "lanes_apply"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeLanesLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["lanes_test"]) == 16 and len(exports["lanes_apply"]) == 7
    with open(os.path.join(CSRC, "lanes_ref.h")) as f:
        ref = f.read()
    assert re.findall(r'^    \{"(\w+)", "', ref, re.M) == list(lanes.OPS)  # the C op table, in the enum's order


# --- 3. instructions -------------------------------------------------------------------------------------------

def test_every_op_compiles_to_its_native_instruction_without_scratch_or_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "lanes.s")
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(CSRC, "lanes.hip"), "-o", asm], check=True, capture_output=True, text=True)
        with open(asm) as f:
            text = f.read()
    bodies = {int(k): body for k, body in re.findall(r"^_ZN\w*12lanes_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                     re.M | re.S)}
    assert sorted(bodies) == list(range(len(lanes.OPS)))
    dpp = {"quad_perm_1032": r"quad_perm:\[1,0,3,2\]", "quad_perm_2301": r"quad_perm:\[2,3,0,1\]",
           "quad_perm_3210": r"quad_perm:\[3,2,1,0\]", "quad_perm_0000": r"quad_perm:\[0,0,0,0\]",
           "row_shr1_bound_ctrl": r"row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1",
           "row_shr1_masked": r"row_shr:1 row_mask:0x5 bank_mask:0xa", "row_bcast15": r"row_bcast:15 row_mask:0xa",
           "row_bcast31": r"row_bcast:31 row_mask:0xc", "row_mirror": r"row_mirror ", "row_half_mirror": "row_half_mirror "}
    for k, name in enumerate(lanes.OPS):
        if name.startswith("dpp_"):
            ctrl = dpp.get(name[4:]) or re.sub(r"(\d+)$", r":\1 row_mask:0xf bank_mask:0xf\\s", name[4:])
            pattern = r"v_mov_b32_dpp [^\n]*" + ctrl
        elif name.startswith("swizzle_"):
            pattern = r"ds_swizzle_b32 "
        elif name.startswith("bpermute_"):
            pattern = r"ds_bpermute_b32 "
        elif name.startswith("permute_"):
            pattern = r"ds_permute_b32 "
        else:
            pattern = rf"v_{name}_b32"
        found = re.findall(r"^\s*" + pattern, bodies[k], re.M)
        # one per chain, in the one loop (every kernel also reads its wave's index once with v_readfirstlane)
        assert len(found) == lanes.CHAINS + (name == "readfirstlane"), (name, pattern, len(found))
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {"0"}    # nor an LDS allocation
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}


# --- 4. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, lanes_kw, **FakeDiagLib kwargs)`` -> (FakeLanesLib, FakeAtomicsLib) for an n x MI355X node."""
    def install(n=1, lanes_kw=None, **kw):
        lib, llib, alib = FakeDiagLib(n=n, **kw), FakeLanesLib(n=n, **(lanes_kw or {})), FakeAtomicsLib(n=n)
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(lanes, "lib", lambda: llib)
        monkeypatch.setattr(atomics, "lib", lambda: alib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return llib, alib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}


def test_off_by_default_and_on_when_asked(node):
    llib, alib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and llib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and llib.calls == []
    res = diag.run(1, 0, extra=("lanes",))
    assert list(res)[-1] == "lanes" and set(res) == LEVEL1 | {"lanes"} and llib.calls == ["lanes0"]
    r = res["lanes"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["iters"] == 2000 and r["blocks"] == 1024
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "iters", "ops", "ms", "wall_s", "detail"}
    assert r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["ops"]) == lanes.OPS
    for row in r["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "gops"}
        assert row["errors"] == 0 and row["first_bad"] is None and row["gops"] > 0
    json.dumps(r)
    assert alib.calls == []
    both = diag.run(1, 0, extra=("atomics", "lanes"))  # the two opt-in tests combine
    assert list(both)[-2:] == ["atomics", "lanes"] and alib.calls == ["atomics0"] and llib.calls == ["lanes0"] * 2
    assert diag.run(0, 0, extra=("lanes",)).keys() == {"lanes"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("lanes" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["lanes"] and "lanes" not in diag.REFERENCE_RATES
    assert "lanes" not in diag.DMA_TESTS | diag.SHARED_TESTS
    line = diag._summary("lanes", r)
    assert "39 ops x 2000 steps on 1024 SIMDs of 8 XCDs, 0 wrong lanes" in line


def test_a_wrong_lane_fails_the_gpu_and_names_the_simd(node):
    llib, _ = node(4, {"bad": {(2, lanes.OPS.index("dpp_row_shr1")): 3}})
    r = diag.run(1, 2, extra=("lanes",))["lanes"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == "3 wrong lanes in dpp_row_shr1 on xcd5/se1/cu7/simd2"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    bad = r["ops"]["dpp_row_shr1"]["first_bad"]
    assert bad == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "chain": 1, "got": "0x5eed1b9e", "want": "0x5eed1a9e"}
    assert r["ops"]["dpp_row_shr2"]["errors"] == 0 and r["ops"]["dpp_row_shr2"]["first_bad"] is None
    assert diag.run(1, 1, extra=("lanes",))["lanes"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_lanes=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag lanes failed ("))
    assert "3 wrong lanes in dpp_row_shr1 on xcd5/se1/cu7/simd2" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["lanes"])
    assert "FAIL" in line and "3 wrong lanes" in line and "xcd5/se1/cu7/simd2" in text


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    monkeypatch.setitem(diag._TESTS, "lanes", ("lanes_test", {"iters": 0}))
    r = diag.run(1, 0, extra=("lanes",))["lanes"]
    assert r["pass"] is False and "lanes failed (-2)" in r["detail"] and "iters 1..2^20" in r["detail"]
    with pytest.raises(ValueError):
        lanes.lanes_test(0, ops=("dpp_row_shr1",), inject_op="readlane")
    with pytest.raises(ValueError):
        lanes.lanes_test(0, ops=("no_such_op",))
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(lanes, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("lanes",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, isolation):
    bad = {"bad": {(5, 0): 1}}
    node(8, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "lanes": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_lanes=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"lanes"}, (d, g["diag"].keys())
        assert g["diag"]["lanes"]["pass"] is (d != 5), (d, g["diag"]["lanes"])
    assert "1 wrong lanes in dpp_quad_perm_1032" in rep["gpus"][5]["diag"]["lanes"]["detail"]  # each child its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", diag_lanes=True, diag_atomics=True, **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 | {"atomics", "lanes"} for g in rep["gpus"])
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    llib, alib = node(2)
    assert diag.main(["--level", "1", "--lanes", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["lanes", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(llib.calls) == ["lanes0", "lanes1"] and alib.calls == []  # one thread per GPU: in either order
    assert diag.main(["--level", "1"]) == 0
    assert "lanes" not in capsys.readouterr().out and len(llib.calls) == 2
    assert diag.main(["--level", "1", "--atomics"]) == 0
    assert "lanes" not in capsys.readouterr().out and len(llib.calls) == 2 and len(alib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--lanes", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--atomics", "--lanes", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--atomics", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [("lanes",), ("atomics", "lanes"), ("atomics",), None]
    capsys.readouterr()
    monkeypatch.undo()
    llib, alib = node(1)
    b = diag.burn_in(1, [0], 0.0, extra=("lanes",))
    assert b["pass"] and b["rounds"] == 1 and llib.calls == ["lanes0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--lanes"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and llib.calls == ["lanes0", "lanes0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(llib.calls) == 2 and alib.calls == []
    assert A.build_parser().parse_args(["--node", "n", "--diag-lanes"]).diag_lanes is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_lanes is False
    for main, flag in ((diag.main, "--lanes"), (node_cycle.main, "--lanes"), (A.main, "--diag-lanes")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 5. build --------------------------------------------------------------------------------------------------

def test_the_build_has_a_lanes_target(tmp_path, monkeypatch):
    t = B._targets()
    assert "lanes" in t and t["lanes"]["out"].endswith("libmi355x_lanes.so")
    assert t["lanes"]["cmd"] == t["xgmi"]["cmd"] and t["lanes"]["headers"][0].endswith("lanes_ref.h")
    assert "libmi355x_lanes.so" in B.__doc__
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    monkeypatch.setattr(B, "OUT", str(tmp_path))  # a fresh output directory: the tree's own library stays as it is
    msgs = B.build(only=["lanes"])
    assert msgs == [f"lanes: built {os.path.relpath(os.path.join(str(tmp_path), 'libmi355x_lanes.so'), os.path.dirname(B.PKG))}"]
    L = ctypes.CDLL(os.path.join(str(tmp_path), "libmi355x_lanes.so"))
    for name in lanes._signatures():
        getattr(L, name)  # AttributeError: not exported
    assert B.build(only=["lanes"]) == []  # up to date
