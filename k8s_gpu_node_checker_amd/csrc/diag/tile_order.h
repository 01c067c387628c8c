// Where a GEMM workgroup's output tile is: the one statement of the tile order, for the kernels (gemm_v1.h to
// gemm_v4.h) and for the host's map from a bad tile back to the XCD that computed it (gemm_checksum).  Plain
// constexpr C++, no HIP: tests/test_tile_order_cpu.py compiles it with the host compiler.
#ifndef K8S_GPU_NODE_CHECKER_AMD_TILE_ORDER_H_
#define K8S_GPU_NODE_CHECKER_AMD_TILE_ORDER_H_

#include <cstddef>
#include <vector>

// Workgroup b is dispatched to XCD b % 8 (round robin).  Of a grid of nwg = 8 * q + r tiles XCD x owns the
// contiguous tile indices [xcd_base, xcd_base + xcd_cnt), so it walks a compact 2D patch of the output.
constexpr int xcd_base(int x, int r, int q) { return x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q; }
constexpr int xcd_cnt(int x, int r, int q) { return q + (x < r ? 1 : 0); }
// dispatch index b of a grid of nwg workgroups -> tile index
constexpr int xcd_remap(int b, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  return xcd_base(b % 8, r, q) + b / 8;
}

// tile index -> (tm, tn): groups of group_m tile rows, walked column by column, down each column first
struct TileMN {
  int tm, tn;
};
constexpr int tile_min(int a, int b) { return a < b ? a : b; }
constexpr TileMN tile_of(int idx, int tiles_m, int tiles_n, int group_m) {
  const int first_m = idx / (group_m * tiles_n) * group_m;
  const int gsize = tile_min(tiles_m - first_m, group_m);
  return {first_m + (idx % (group_m * tiles_n)) % gsize, (idx % (group_m * tiles_n)) / gsize};
}

// v4's tail: with a short last wave the v4 launch covers only the whole 256-CU waves, v4_tail_main(nwg)
// workgroups, which leaves each XCD's chunk computed up to its first v4_tail_main(nwg) / 8 indices.
constexpr int v4_tail_main(int nwg) { return nwg / 256 * 256; }
// only a short tail is worth it: a quarter wave of 256^2 tiles is one 2-per-CU wave of 128^2 quadrants
constexpr bool v4_tail_applies(int nwg) { return nwg > 256 && nwg % 256 != 0 && nwg % 256 <= 64; }
// the tile index tail tile t computes (the rest of XCD 0's chunk, then XCD 1's, ...), or -1 past the tail;
// gemm_v4_tail_kernel keeps this loop's text inline (a call changed its code) on the same xcd_cnt / xcd_base
constexpr int v4_tail_idx(int t, int nwg) {
  const int q = nwg / 8, r = nwg % 8, qmain = v4_tail_main(nwg) / 8;
  for (int x = 0; x < 8; ++x) {  // v4 computed the first qmain tiles of XCD x's chunk
    const int cnt = xcd_cnt(x, r, q), base = xcd_base(x, r, q);
    if (t < cnt - qmain) return base + qmain + t;
    t -= cnt - qmain;
  }
  return -1;
}

// The XCD that computed each tile, indexed tm * tiles_n + tn.
__attribute__((always_inline)) inline std::vector<int> tile_xcds(int tiles_m, int tiles_n, int group_m) {
  const int nwg = tiles_m * tiles_n;
  std::vector<int> out(static_cast<size_t>(nwg), -1);
  for (int b = 0; b < nwg; ++b) {
    const TileMN t = tile_of(xcd_remap(b, nwg), tiles_m, tiles_n, group_m);
    out[static_cast<size_t>(t.tm) * tiles_n + t.tn] = b % 8;
  }
  return out;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_TILE_ORDER_H_
