"""libmi355x_lanes.so on an MI355X: one application of every op held against the host's model word for word (and
every full-mask DPP op against the device's own ds_bpermute), the chains clean at the smallest shapes and at the
default grid, both self-check hooks, and the opt-in wiring up to ``mi355x-diag --lanes``.

These tests plant wrong values in data; none provokes a GPU fault.  No rate is asserted: the rates are reported
(profiles/lanes_mi355x.json) and never judged.

The model is csrc/lanes/lanes_ref.h itself, compiled here with the host compiler into a small program.  A crossing
only moves words, so the program applies each op to tagged inputs (x[i] = 1 + i, y[i] = 65 + i; 0 is the constant of
bound_ctrl) and prints where every output word comes from; the tests then move hashed words the same way."""
import functools
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu

STEPS = (0, 1, 63, 64)  # the lane port's index and floor wrap at 64
HOOKED = ("dpp_row_shr1", "bpermute_seeded", "permlane32_swap")  # one DPP, one ds_, one permlane swap
M = 0xffffffff

TAG_CPP = r"""
#include <cstdio>
#include "lanes_ref.h"
int main() {
  const int steps[4] = {0, 1, 63, 64};
  for (int op = 0; op < LANES_OPS; ++op)
    for (int it : steps) {
      uint32_t x[LANES_WAVE], y[LANES_WAVE];
      for (int i = 0; i < LANES_WAVE; ++i) x[i] = 1u + i, y[i] = 65u + i;
      lanes_apply(op, static_cast<uint32_t>(it), x, y);
      printf("%s %d", LANES_OP_TABLE[op].name, it);
      for (int i = 0; i < LANES_WAVE; ++i) printf(" %u", x[i]);
      for (int i = 0; i < LANES_WAVE; ++i) printf(" %u", y[i]);
      printf("\n");
    }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def model_tags():
    """{(op name, step): (64 tags of x, 64 tags of y)} from lanes_ref.h: tag 0 the constant 0, 1 + i lane i of the
    input x, 65 + i lane i of the input y."""
    from k8s_gpu_node_checker_amd import build as B
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lanes_tags.cpp"), os.path.join(tmp, "lanes_tags")
        with open(src, "w") as f:
            f.write(TAG_CPP)
        subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(B.CSRC, "lanes"), src, "-o", exe], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    tags = {}
    for line in out.splitlines():
        f = line.split()
        words = [int(v) for v in f[2:]]
        tags[(f[0], int(f[1]))] = (words[:64], words[64:])
    return tags


def moved(tags, x, y):
    return [0 if t == 0 else (x[t - 1] if t <= 64 else y[t - 65]) for t in tags]


def hashed(salt):
    """64 distinct, full-width words"""
    return [((i + 1) * 0x9E3779B1 + salt * 0x85EBCA6B) & M ^ ((i * 0xC2B2AE35 + salt) >> 7 & M) for i in range(64)]


@pytest.fixture(scope="module")
def lanes():
    from k8s_gpu_node_checker_amd.ops import lanes as la
    assert la.device_count() >= 1
    return la


def test_one_application_of_every_op_matches_the_model_word_for_word(lanes):
    tags = model_tags()
    assert len(tags) == len(lanes.OPS) * len(STEPS)
    wrong = []
    for k, op in enumerate(lanes.OPS):
        for it in STEPS:
            x, y = hashed(3 * k + 1), hashed(3 * k + 2)  # y independent of x: `old` and the swaps' second register
            gx, gy = lanes.apply(op, x, y, iter=it)
            tx, ty = tags[(op, it)]
            if gx != moved(tx, x, y) or gy != moved(ty, x, y):
                lanes_off = [i for i in range(64) if gx[i] != moved(tx, x, y)[i] or gy[i] != moved(ty, x, y)[i]]
                wrong.append((op, it, lanes_off))
    print("ops x steps checked:", len(tags), "disagreeing:", wrong)
    assert not wrong, wrong


def test_every_full_mask_dpp_op_is_the_devices_own_bpermute(lanes):
    """The DPP network and the LDS crossbar are two pieces of hardware: with the model's lane map as ds_bpermute's
    address, both must move the same words wherever the DPP source is in range."""
    tags = model_tags()
    full = [op for op in lanes.OPS if op.startswith("dpp_")
            and op not in ("dpp_row_bcast15", "dpp_row_bcast31", "dpp_row_shr1_masked")]
    assert len(full) == 18
    for op in full:
        x = hashed(100 + lanes.OPS.index(op))
        tx, _ = tags[(op, 0)]
        src = [t - 1 if 1 <= t <= 64 else None for t in tx]  # None: out of range (old, or 0 under bound_ctrl)
        assert sum(s is not None for s in src) >= 32, op  # the fewest: row_shr:8, the upper half of every row
        via_dpp, _ = lanes.apply(op, x)
        via_lds, _ = lanes.apply(lanes.BPERMUTE_Y, x, [4 * (i if s is None else s) for i, s in enumerate(src)])
        off = [i for i, s in enumerate(src) if s is not None and via_dpp[i] != via_lds[i]]
        assert not off, (op, off)
        assert [via_lds[i] for i in range(64)] == [x[i if s is None else s] for i, s in enumerate(src)], op


def _clean(lanes, r):
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and "bad_simds" not in r, r
    assert tuple(r["ops"]) == lanes.OPS
    for op, row in r["ops"].items():
        assert row["errors"] == 0 and row["first_bad"] is None and row["ms"] > 0 and row["gops"] > 0, (op, row)
    for slot in r["slots"]:
        name = lanes.simd_name(slot)
        m = re.fullmatch(r"xcd(\d+)/se(\d)/cu(\d+)(/sh1)?/simd(\d)", name)
        assert m and int(m.group(1)) < 8 and int(m.group(5)) < 4, (slot, name)
    assert r["simds"] == len(r["slots"]) >= 1


@pytest.mark.parametrize("iters", (1, 2, 65))
def test_one_workgroup_is_clean_at_the_smallest_shapes(lanes, iters):
    r = lanes.lanes_test(0, blocks=1, iters=iters, reps=1, slots=True)
    print(iters, {k: v for k, v in r.items() if k != "ops"})
    _clean(lanes, r)
    # the map adds up over a warm-up and a timed launch of every op, each launch's four waves placed anew
    assert r["blocks"] == 1 and r["iters"] == iters and 1 <= r["simds"] <= 4 * 2 * len(lanes.OPS) and r["xcds"] >= 1


def test_the_default_grid_is_clean_on_every_xcd(lanes):
    from k8s_gpu_node_checker_amd.ops import diag
    r = lanes.lanes_test(0, iters=50, reps=2, slots=True)
    print(json.dumps({k: v for k, v in r.items() if k not in ("ops", "slots")}))
    _clean(lanes, r)
    cus = diag.device_info(0)["cus"]
    assert r["blocks"] == 4 * cus and r["simds"] <= 4 * cus
    if cus == 256:
        assert r["xcds"] == 8


@pytest.mark.parametrize("op", HOOKED)
def test_an_injected_flip_is_one_wrong_lane_in_that_op_only(lanes, op):
    r = lanes.lanes_test(0, blocks=8, iters=4, reps=1, inject_op=op, inject_block=5)
    print(op, r["detail"], r["ops"][op])
    assert r["pass"] is False and r["errors"] == 1
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    bad = r["ops"][op]["first_bad"]
    assert bad["lane"] == 0 and bad["chain"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert re.fullmatch(r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]", bad["where"]), bad
    assert r["detail"] == f"1 wrong lanes in {op} on {bad['where']}" and r["bad_simds"] == [f"{bad['where']} (1)"]


@pytest.mark.parametrize("op", HOOKED)
def test_a_crossing_that_did_not_happen_shows_in_that_op_only(lanes, op):
    r = lanes.lanes_test(0, blocks=8, iters=4, reps=1, inject_op=op, inject_block=5, inject_skip_iter=0)
    print(op, r["detail"], r["ops"][op])
    assert r["pass"] is False and 0 < r["errors"] <= 64  # one wave's lanes at the most
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    assert r["ops"][op]["first_bad"]["got"] != r["ops"][op]["first_bad"]["want"]


def test_refused_calls(lanes):
    for kw in (dict(iters=0), dict(reps=0), dict(blocks=4, inject_op="readlane", inject_block=4),
               dict(iters=4, inject_op="readlane", inject_block=0, inject_skip_iter=4)):
        with pytest.raises(RuntimeError, match=r"lanes failed \(-2\)"):
            lanes.lanes_test(0, **kw)


def test_a_call_on_another_device_leaves_the_threads_device_as_it_was(lanes):
    """Refused after the library has made the other device current, and passing: either way the calling thread's HIP
    device is the one it had.  The refused call launches nothing."""
    import ctypes
    if lanes.device_count() < 2:
        pytest.skip("needs two devices")
    hip = ctypes.CDLL("libamdhip64.so")  # the runtime the library has loaded

    def current():
        dev = ctypes.c_int(-1)
        assert hip.hipGetDevice(ctypes.byref(dev)) == 0
        return dev.value

    before = current()
    other = 0 if before == 1 else 1
    with pytest.raises(RuntimeError, match=r"lanes failed \(-2\)"):
        lanes.lanes_test(other, blocks=4, iters=1, reps=1, inject_op="readlane", inject_block=4)
    assert current() == before
    r = lanes.lanes_test(other, blocks=1, iters=1, reps=1)
    assert r["pass"] and r["errors"] == 0, r
    assert current() == before


def test_the_cli_flag_carries_a_passing_lanes_result(repo):
    def run(*flags):
        p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                            "--format", "json", *flags], capture_output=True, text=True, timeout=300, cwd=repo)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    tests = run("--lanes")
    assert tests["lanes"]["pass"] and tests["lanes"]["errors"] == 0 and len(tests["lanes"]["ops"]) == 39
    assert "lanes" not in run()
