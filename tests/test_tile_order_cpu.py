"""The GEMM kernels' tile order (``csrc/diag/tile_order.h``), on the host compiler.

Every GEMM kernel finds its output tile through this header, and ``gemm_checksum`` names the XCD of a bad tile through
its ``tile_xcds``: here the order is a bijection, equals the formula the kernels carried before they shared it
(restated below, not imported), and agrees with the XCD map.  v4's shortened launch plus its tail's index walk must
reach every tile exactly once.
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "k8s_gpu_node_checker_amd", "csrc", "diag", "tile_order.h")

GRIDS = [(1, 1, 8), (3, 5, 8), (5, 3, 4), (9, 7, 4), (16, 16, 4), (17, 16, 4), (24, 24, 4), (32, 32, 8)]
TAIL_NWG = [257, 272, 288, 320, 576, 832]

DRIVER = r"""
#include <cstdio>
#include "tile_order.h"

static_assert(xcd_remap(9, 17) == 4 && tile_of(5, 3, 5, 8).tm == 2, "usable in constant expressions");

int main() {
  const int grids[][3] = {%(grids)s};
  const int tails[] = {%(tails)s};
  std::printf("{\"grids\": [");
  for (unsigned g = 0; g < sizeof(grids) / sizeof(grids[0]); ++g) {
    const int tm_ = grids[g][0], tn_ = grids[g][1], gm = grids[g][2], nwg = tm_ * tn_;
    std::printf("%%s{\"tiles\": [", g ? "," : "");
    for (int b = 0; b < nwg; ++b) {
      const TileMN t = tile_of(xcd_remap(b, nwg), tm_, tn_, gm);
      std::printf("%%s[%%d,%%d]", b ? "," : "", t.tm, t.tn);
    }
    std::printf("], \"xcds\": [");
    const std::vector<int> x = tile_xcds(tm_, tn_, gm);
    for (int i = 0; i < nwg; ++i) std::printf("%%s%%d", i ? "," : "", x[i]);
    std::printf("]}");
  }
  std::printf("], \"tails\": [");
  for (unsigned i = 0; i < sizeof(tails) / sizeof(tails[0]); ++i) {
    const int nwg = tails[i], main_wg = v4_tail_main(nwg);
    std::printf("%%s{\"applies\": %%d, \"main\": %%d, \"remap\": [", i ? "," : "", v4_tail_applies(nwg), main_wg);
    for (int b = 0; b < main_wg; ++b) std::printf("%%s%%d", b ? "," : "", xcd_remap(b, nwg));
    std::printf("], \"walk\": [");
    for (int t = 0; t <= nwg - main_wg; ++t) std::printf("%%s%%d", t ? "," : "", v4_tail_idx(t, nwg));
    std::printf("]}");
  }
  std::printf("]}\n");
  return 0;
}
"""


def parent_tile(b, tiles_m, tiles_n, group_m):
    """The tile of dispatch index b as every kernel spelled it out before tile_order.h."""
    nwg = tiles_m * tiles_n
    q, r, xcd = nwg // 8, nwg % 8, b % 8
    bid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + b // 8
    first_m = bid // (group_m * tiles_n) * group_m
    gsize = min(tiles_m - first_m, group_m)
    return [first_m + (bid % (group_m * tiles_n)) % gsize, (bid % (group_m * tiles_n)) // gsize]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("tile_order")
    src, exe = d / "order.cpp", d / "order"
    src.write_text(DRIVER % {"grids": ", ".join("{%d, %d, %d}" % g for g in GRIDS),
                             "tails": ", ".join(map(str, TAIL_NWG))})
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout)


@pytest.mark.parametrize("i", range(len(GRIDS)), ids=["%dx%d_g%d" % g for g in GRIDS])
def test_tile_order_of_a_grid(tables, i):
    tiles_m, tiles_n, group_m = GRIDS[i]
    nwg = tiles_m * tiles_n
    got = tables["grids"][i]
    # (a) a bijection onto the grid
    assert sorted(map(tuple, got["tiles"])) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)]
    # (b) the formula the kernels carried
    assert got["tiles"] == [parent_tile(b, tiles_m, tiles_n, group_m) for b in range(nwg)]
    # (c) the host's map names the XCD the workgroup ran on
    assert len(got["xcds"]) == nwg
    for b, (tm, tn) in enumerate(got["tiles"]):
        assert got["xcds"][tm * tiles_n + tn] == b % 8, (b, tm, tn)


@pytest.mark.parametrize("i", range(len(TAIL_NWG)), ids=[str(n) for n in TAIL_NWG])
def test_v4_main_launch_and_tail_cover_every_tile_once(tables, i):
    nwg = TAIL_NWG[i]
    got = tables["tails"][i]
    assert bool(got["applies"]) == (nwg % 256 <= 64)
    assert got["main"] == nwg // 256 * 256
    walk = got["walk"]
    assert len(walk) == nwg - got["main"] + 1
    assert sorted(got["remap"] + walk[:-1]) == list(range(nwg))
    assert walk[-1] == -1  # the first t past the tail
