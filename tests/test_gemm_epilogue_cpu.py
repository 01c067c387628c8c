"""The walk that empties a wave's LDS patch (``csrc/diag/gemm_epilogue.h``), on the host compiler.

GEMM v3, v4 and v4's tail send C through a patch of 16 rows x ``NB * 16`` fp32 columns and are compared bit for bit,
so all of them must empty it by the same rule.  For ``NB`` in {4, 8} and both output types the 64 lanes over all steps
read every element exactly once, every lane's piece is 16-byte aligned in the output row, and the map equals the
shifts and masks the kernels carried before they shared it (restated below, not imported; v4 still carries them).
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "k8s_gpu_node_checker_amd", "csrc", "diag", "gemm_epilogue.h")

# (NB, fp32 elements per lane and step, bytes per output element): bf16 leaves 8 at a time, fp32 4
WALKS = [(4, 8, 2), (4, 4, 4), (8, 8, 2), (8, 4, 4)]
# (NB, ELEMS) -> (lane shift, lane mask, steps, rows per step) as the kernels spelled them out
PARENT = {(4, 8): (3, 7, 2, 8), (4, 4): (4, 15, 4, 4), (8, 8): (4, 15, 4, 4), (8, 4): (5, 31, 8, 2)}

DRIVER = r"""
#include <cstdio>
#include "gemm_epilogue.h"

static_assert(PatchWalk<4, 8>::row(63, 1) == 15 && PatchWalk<8, 4>::col(33) == 4, "usable in constant expressions");

template <int NB, int ELEMS>
void dump(bool first) {
  using W = PatchWalk<NB, ELEMS>;
  std::printf("%s{\"nb\": %d, \"elems\": %d, \"ld\": %d, \"steps\": %d, \"map\": [", first ? "" : ",", NB, ELEMS, W::LD,
              W::STEPS);
  for (int q = 0; q < W::STEPS; ++q)
    for (int lane = 0; lane < 64; ++lane)
      std::printf("%s[%d,%d]", q || lane ? "," : "", W::row(lane, q), W::col(lane));
  std::printf("]}");
}

int main() {
  std::printf("[");
  dump<4, 8>(true);
  dump<4, 4>(false);
  dump<8, 8>(false);
  dump<8, 4>(false);
  std::printf("]\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gemm_epilogue")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout)
    return {(w["nb"], w["elems"]): w for w in got}


@pytest.mark.parametrize("nb,elems,out_bytes", WALKS, ids=["nb%d_%s" % (w[0], "bf16" if w[2] == 2 else "f32")
                                                            for w in WALKS])
def test_patch_walk(walks, nb, elems, out_bytes):
    w = walks[(nb, elems)]
    shift, mask, steps, rows_per_step = PARENT[(nb, elems)]
    assert w["ld"] == nb * 16 + 4 and w["steps"] == steps and len(w["map"]) == steps * 64
    # (a) every element of the 16 x NB*16 patch is read exactly once
    seen = sorted((r, c + e) for r, c in w["map"] for e in range(elems))
    assert seen == [(r, c) for r in range(16) for c in range(nb * 16)]
    # (b) a lane's piece is 16 bytes, 16-byte aligned in the output row and in the patch row (LD * 4 is too)
    assert elems * out_bytes == 16
    assert all(c * out_bytes % 16 == 0 and c * 4 % 16 == 0 for _, c in w["map"]) and w["ld"] * 4 % 16 == 0
    # (c) the constants the kernels carried
    assert w["map"] == [[q * rows_per_step + (lane >> shift), (lane & mask) * elems]
                        for q in range(steps) for lane in range(64)]
