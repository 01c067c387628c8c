"""The host half of the GEMM diagnostics' verdict (``csrc/diag/gemm_verdict.h``), on the host compiler.

The ``gemm`` / ``gemm_fp8`` diagnostics decide whether a GPU computes correctly; this header holds every part of that
decision that needs no GPU: the E4M3 decode, the sample positions, what a bf16 output's rounding forgives, the
checksum verdict with its tile and XCD bookkeeping, and the sampled-error reduction.  A g++ driver with its own
``main`` reads commands and prints JSON (doubles as C hex floats, so nothing is rounded on the way); the expected
values are worked out here, from the formats and from hand-made arrays.
"""
import json
import math
import os
import shutil
import subprocess

import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(HERE, "..", "k8s_gpu_node_checker_amd", "csrc", "diag")

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "gemm_verdict.h"

static double next_double() {
  char tok[64];
  if (std::scanf("%63s", tok) != 1) std::exit(3);
  return std::strtod(tok, nullptr);
}
static long long next_int() {
  long long v;
  if (std::scanf("%lld", &v) != 1) std::exit(3);
  return v;
}
static void put(double v, bool first) { std::printf("%s\"%a\"", first ? "" : ",", v); }

int main() {
  char cmd[32];
  bool first_cmd = true;
  std::printf("[");
  while (std::scanf("%31s", cmd) == 1) {
    std::printf("%s", first_cmd ? "" : ",\n");
    first_cmd = false;
    if (!std::strcmp(cmd, "e4m3")) {
      std::printf("[");
      for (int b = 0; b < 256; ++b) put(e4m3_value(static_cast<uint8_t>(b)), b == 0);
      std::printf("]");
    } else if (!std::strcmp(cmd, "samples")) {
      unsigned long long seed;
      if (std::scanf("%llu", &seed) != 1) return 3;
      const int nsamp = static_cast<int>(next_int()), M = static_cast<int>(next_int()), N = static_cast<int>(next_int());
      std::vector<int> rows, cols;
      sample_indices(seed, nsamp, M, N, rows, cols);
      std::printf("{\"rows\": [");
      for (int i = 0; i < nsamp; ++i) std::printf("%s%d", i ? "," : "", rows[i]);
      std::printf("], \"cols\": [");
      for (int i = 0; i < nsamp; ++i) std::printf("%s%d", i ? "," : "", cols[i]);
      std::printf("]}");
    } else if (!std::strcmp(cmd, "bf16")) {
      const long long n = next_int();
      std::printf("[");
      for (long long i = 0; i < n; ++i) {
        const double got = next_double(), ref = next_double();
        put(beyond_bf16_rounding(got, ref), i == 0);
      }
      std::printf("]");
    } else if (!std::strcmp(cmd, "verdict")) {
      // halves nblk N rows cols group_m tol, three fill values (ref mag csum), then k overrides (array index value)
      const int halves = static_cast<int>(next_int()), nblk = static_cast<int>(next_int());
      const int N = static_cast<int>(next_int());
      TileGeom g;
      g.rows = static_cast<int>(next_int()), g.cols = static_cast<int>(next_int());
      g.group_m = static_cast<int>(next_int());
      const double tol = next_double();
      const size_t cnt = static_cast<size_t>(nblk) * N;
      const double fr = next_double(), fm = next_double(), fc = next_double();
      std::vector<double> arr[3] = {std::vector<double>(cnt, fr), std::vector<double>(cnt, fm),
                                    std::vector<double>(cnt * halves, fc)};
      const long long k = next_int();
      for (long long i = 0; i < k; ++i) {
        const long long a = next_int(), idx = next_int();
        arr[a].at(static_cast<size_t>(idx)) = next_double();
      }
      double max_err = -1.0, floor = -1.0;
      long long out[kCkOut];
      std::vector<double> judged(cnt, -1.0);
      checksum_verdict(arr[0].data(), arr[1].data(), arr[2].data(), halves, nblk, N, g, tol, &max_err, out, &floor,
                       judged.data());
      std::printf("{\"max_err\": \"%a\", \"floor\": \"%a\", \"out\": [", max_err, floor);
      for (int i = 0; i < kCkOut; ++i) std::printf("%s%lld", i ? "," : "", out[i]);
      std::printf("], \"xcds\": [");
      const std::vector<int> x = tile_xcds(nblk, N / g.cols, g.group_m);
      for (size_t i = 0; i < x.size(); ++i) std::printf("%s%d", i ? "," : "", x[i]);
      std::printf("], \"judged\": [");
      for (size_t i = 0; i < cnt; ++i) put(judged[i], i == 0);
      std::printf("]}");
    } else if (!std::strcmp(cmd, "sampled")) {
      const int n = static_cast<int>(next_int()), fused = static_cast<int>(next_int());
      const int by_mag = static_cast<int>(next_int());
      std::vector<float> got(n);
      std::vector<double> ref(n), mag(n);
      for (int i = 0; i < n; ++i) got[i] = static_cast<float>(next_double());
      for (int i = 0; i < n; ++i) ref[i] = next_double();
      for (int i = 0; i < n; ++i) mag[i] = next_double();
      std::printf("\"%a\"", sampled_worst(got.data(), ref.data(), mag.data(), n, fused != 0, by_mag != 0));
    } else {
      return 4;
    }
  }
  std::printf("]\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gemm_verdict")
    src, exe = d / "verdict.cpp", d / "verdict"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=120)

    def run(*commands):
        """Each command is a list of tokens (floats are sent as hex); returns one parsed result per command."""
        text = "\n".join(" ".join(x.hex() if isinstance(x, float) else str(x) for x in c) for c in commands)
        out = subprocess.run([str(exe)], input=text + "\n", check=True, capture_output=True, text=True, timeout=60)
        return json.loads(out.stdout)
    return run


def fx(s):
    return float.fromhex(s)


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1, a) == math.copysign(1, b))


# ------------------------------------------------------------------------------------------------- e4m3_value
def test_e4m3_value_is_float8_e4m3fn_on_all_256_codes(driver):
    """torch.uint8 -> float8_e4m3fn -> float64 is the format; 0x7F / 0xFF are its NaN (not +-480)."""
    got = [fx(s) for s in driver(["e4m3"])[0]]
    want = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).tolist()
    assert len(got) == 256 and sum(math.isnan(w) for w in want) == 2
    for code, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (hex(code), g, w)


# ------------------------------------------------------------------------------------------------- sample_indices
SAMPLE_SHAPES = [(256, 256), (256, 1280), (2304, 128)]
SAMPLE_SEEDS = [0x243F6A8885A308D3, 0x13198A2E03707344]  # the bf16 and the fp8 diagnostic's


def lcg_samples(seed, nsamp, m, n):
    """Knuth's MMIX 64-bit LCG; a row from the top 31 bits of one step, its column from those of the next."""
    x, rows, cols = seed, [], []
    for _ in range(nsamp):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        rows.append((x >> 33) % m)
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        cols.append((x >> 33) % n)
    return rows, cols


@pytest.mark.parametrize("m,n", SAMPLE_SHAPES)
def test_sample_indices_stay_inside_the_output_and_never_move(driver, m, n):
    """Results are compared across releases through the baseline, so the sample set is pinned to the LCG restated
    above; rows index M and columns N also where M != N."""
    for seed in SAMPLE_SEEDS:
        a, b = driver(["samples", seed, 4096, m, n], ["samples", seed, 4096, m, n])
        assert a == b
        assert len(a["rows"]) == len(a["cols"]) == 4096
        assert all(0 <= r < m for r in a["rows"]) and all(0 <= c < n for c in a["cols"])
        rows, cols = lcg_samples(seed, 4096, m, n)
        assert a["rows"] == rows and a["cols"] == cols
        if m > n:  # the rows really range over M (a row taken modulo N would stay below N)
            assert max(a["rows"]) >= n
        if n > m:
            assert max(a["cols"]) >= m


# ------------------------------------------------------------------------------------------- beyond_bf16_rounding
def bf16_positive_normals():
    """All 254 x 128 positive normal bf16 values, as float64 (exact)."""
    bits = torch.arange(0x0080, 0x7F80, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).to(torch.float64)


def bf16_round(x64):
    """float64 -> bf16 (round to nearest even) -> float64; the inputs here are exact in fp32."""
    assert bool((x64.to(torch.float32).to(torch.float64) == x64).all())
    return x64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def test_beyond_bf16_rounding_forgives_exactly_the_outputs_own_rounding(driver):
    """got = bf16_round(ref) must cost nothing: ref at every positive normal bf16 value, half an ulp above it (a tie)
    and half an ulp below it.  (The one ref that rounds to infinity, half an ulp above the largest value, is left
    out: an infinite output is an error.)"""
    v = bf16_positive_normals()
    assert v.numel() == 254 * 128
    ulp = torch.ldexp(torch.ones_like(v), torch.floor(torch.log2(v)).to(torch.int64) - 7)
    assert bool((bf16_round((v + ulp)[:-1]) == v[1:]).all())  # ulp is the spacing above each value
    refs = torch.cat([v, (v + ulp / 2)[:-1], v - ulp / 2])
    gots = bf16_round(refs)
    assert bool(torch.isfinite(gots).all()) and bool((gots != refs).any())
    pairs = [x for g, r in zip(gots.tolist(), refs.tolist()) for x in (g, r)]
    out = [fx(s) for s in driver(["bf16", len(refs)] + pairs)[0]]
    bad = [(g, r, o) for g, r, o in zip(gots.tolist(), refs.tolist(), out) if not same(o, 0.0)]
    assert not bad, bad[:5]
    # the same with both signs flipped
    out = [fx(s) for s in driver(["bf16", len(refs)] + [-x for x in pairs])[0]]
    assert all(same(o, 0.0) for o in out)


def test_beyond_bf16_rounding_reports_a_four_ulp_error_exactly_and_keeps_nan(driver):
    """An error of 4 ulps costs |got - ref| - 1.01 * 2^-8 * max(|got|, |ref|), to the bit; NaN in gives NaN out; the
    result is never negative."""
    v = bf16_positive_normals()[::97][:-1]
    ulp = torch.ldexp(torch.ones_like(v), torch.floor(torch.log2(v)).to(torch.int64) - 7)
    cases = []
    for val, u in zip(v.tolist(), ulp.tolist()):
        cases += [(val + 4 * u, val), (val, val + 4 * u), (-(val + 4 * u), -val), (val - 4 * u, val)]
    out = [fx(s) for s in driver(["bf16", len(cases)] + [x for c in cases for x in c])[0]]
    for (got, ref), o in zip(cases, out):
        want = abs(got - ref) - math.ldexp(max(abs(got), abs(ref)), -8) * 1.01
        assert want > 0 and same(o, want), (got, ref, o, want)
        # 4 ulps are 2^-5 .. 2^-6 of the value: nearly all of the error is reported
        assert o > 0.7 * abs(got - ref)
    nan, inf = float("nan"), float("inf")
    specials = [(nan, 1.0), (1.0, nan), (nan, nan), (inf, 1.0), (1.0, 1.0), (0.0, 0.0), (1.0, 1.0 + 2.0 ** -9),
                (1.0, -1.0), (0.0, 2.0 ** -130), (3.0, 3.0 * (1 + 2.0 ** -8))]
    out = [fx(s) for s in driver(["bf16", len(specials)] + [x for c in specials for x in c])[0]]
    assert all(math.isnan(o) for o in out[:4])  # (inf - inf is NaN too: an infinite output is never forgiven)
    assert out[4] == 0.0 and out[5] == 0.0 and out[6] == 0.0
    assert out[7] == 2.0 - math.ldexp(1.0, -8) * 1.01
    assert all(o >= 0.0 for o in out[4:])


# ------------------------------------------------------------------------------------------- the checksum verdict
# the two geometries of the diagnostics (rows, columns, group_m) and a hand-made one whose tiles are not square, so
# that a tile column taken from the tile height shows
GEOMS = {"128": (128, 128, 8), "256": (256, 256, 4), "256x128": (256, 128, 4)}
GRIDS = [(1, 1), (9, 3), (3, 5)]
TOL = 1e-7
REF0, MAG0 = 1000.0, 1.0e6


class Case:
    """Hand-made checksum arrays: every column's sum equals its reference REF0 and has magnitude MAG0 until changed.
    With two halves the sum is split unevenly (400 + 600) over the 128-row halves."""

    def __init__(self, nblk, tiles_n, geom, halves=1, tol=TOL):
        self.nblk, self.tiles_n, self.geom, self.halves, self.tol = nblk, tiles_n, geom, halves, tol
        self.n = tiles_n * geom[1]
        self.over = []
        if halves == 2:
            for tb in range(nblk):
                for j in range(self.n):
                    self.over.append((2, (2 * tb) * self.n + j, 400.0))
                    self.over.append((2, (2 * tb + 1) * self.n + j, 600.0))

    def mag(self, tb, j, value):
        self.over.append((1, tb * self.n + j, float(value)))
        return self

    def csum(self, tb, j, value, half=0):
        self.over.append((2, (tb * self.halves + half) * self.n + j, float(value)))
        return self

    def command(self):
        rows, cols, group_m = self.geom
        return (["verdict", self.halves, self.nblk, self.n, rows, cols, group_m, self.tol, REF0, MAG0, REF0,
                 len(self.over)] + [x for o in self.over for x in o])


def verdict(driver, case):
    r = driver(case.command())[0]
    r["max_err"], r["floor"] = fx(r["max_err"]), fx(r["floor"])
    return r


def xcd_counts(r, tiles, tiles_n):
    counts = [0] * 8
    for tm, tn in tiles:
        counts[r["xcds"][tm * tiles_n + tn]] += 1
    return counts


def expect_tiles(r, tiles, columns, tiles_n):
    tiles = sorted(set(tiles))
    assert r["out"][0] == len(tiles) and r["out"][1] == columns, r["out"]
    assert r["out"][2:10] == xcd_counts(r, tiles, tiles_n), (r["out"], tiles)
    assert r["out"][10:12] == (list(tiles[0]) if tiles else [-1, -1]), (r["out"], tiles)


ALL = [(g, nblk, tn) for g in GEOMS for nblk, tn in GRIDS]
ALL_IDS = ["g%s_%dx%d" % c for c in ALL]


@pytest.mark.parametrize("g,nblk,tiles_n", ALL, ids=ALL_IDS)
def test_clean_checksums_give_zeros_and_the_floor_is_tol_times_the_largest_magnitude(driver, g, nblk, tiles_n):
    geom = GEOMS[g]
    n = tiles_n * geom[1]
    r = verdict(driver, Case(nblk, tiles_n, geom).mag(nblk - 1, n - 1, 3.0 * MAG0).mag(0, 0, 0.5 * MAG0))
    assert r["out"] == [0] * 10 + [-1, -1] and r["max_err"] == 0.0
    assert r["floor"] == TOL * (3.0 * MAG0)
    assert len(r["xcds"]) == nblk * tiles_n and set(r["xcds"]) <= set(range(8))


@pytest.mark.parametrize("g,nblk,tiles_n", ALL, ids=ALL_IDS)
def test_the_threshold_is_tol_times_the_columns_own_magnitude(driver, g, nblk, tiles_n):
    """One column off by 1.01 x tol x mag is flagged, by 0.99 x it is not -- against that column's magnitude, which
    here differs from every other column's (the floor, from the largest, is 4x higher)."""
    geom = GEOMS[g]
    n = tiles_n * geom[1]
    tb, j = nblk - 1, n - 1
    own = 0.25 * MAG0
    for sign in (1.0, -1.0):
        hit = verdict(driver, Case(nblk, tiles_n, geom).mag(tb, j, own).csum(tb, j, REF0 + sign * 1.01 * TOL * own))
        expect_tiles(hit, [(tb, tiles_n - 1)], 1, tiles_n)
        assert 1.005 * TOL < hit["max_err"] < 1.015 * TOL and hit["floor"] == TOL * MAG0
        miss = verdict(driver, Case(nblk, tiles_n, geom).mag(tb, j, own).csum(tb, j, REF0 + sign * 0.99 * TOL * own))
        expect_tiles(miss, [], 0, tiles_n)
        assert 0.985 * TOL < miss["max_err"] < 0.995 * TOL


@pytest.mark.parametrize("g,nblk,tiles_n", ALL, ids=ALL_IDS)
def test_columns_and_tiles_are_counted_apart_and_tile_boundaries_hold(driver, g, nblk, tiles_n):
    """A flagged column at a tile's last column and one at the next tile's first column are two tiles; three more
    columns inside the first add columns, not tiles.  In a one-tile grid the same columns are one tile."""
    geom = GEOMS[g]
    cols = geom[1]
    tb = nblk // 2
    off = REF0 + 2.0 * TOL * MAG0
    c = Case(nblk, tiles_n, geom)
    if tiles_n > 1:
        last_tile = tiles_n - 1  # the boundary between the last two tile columns
        edge = last_tile * cols
        for j in (edge - 1, edge, edge - 2, edge - cols, edge - 7):
            c.csum(tb, j, off)
        expect_tiles(verdict(driver, c), [(tb, last_tile - 1), (tb, last_tile)], 5, tiles_n)
        two = Case(nblk, tiles_n, geom).csum(tb, last_tile * cols - 1, off).csum(tb, last_tile * cols, off)
        expect_tiles(verdict(driver, two), [(tb, last_tile - 1), (tb, last_tile)], 2, tiles_n)
    else:
        for j in (0, cols - 1, 5):
            c.csum(tb, j, off)
        expect_tiles(verdict(driver, c), [(0, 0)], 3, tiles_n)
    if nblk > 1:  # the same column in two neighbouring row blocks: two tiles, one above the other
        c = Case(nblk, tiles_n, geom).csum(tb - 1, 3, off).csum(tb, 3, off)
        expect_tiles(verdict(driver, c), [(tb - 1, 0), (tb, 0)], 2, tiles_n)


@pytest.mark.parametrize("g,nblk,tiles_n", [c for c in ALL if c[1] > 1],
                         ids=[i for c, i in zip(ALL, ALL_IDS) if c[1] > 1])
def test_the_first_bad_tile_is_the_lowest_in_row_major_order_and_every_tile_maps_to_its_xcd(driver, g, nblk, tiles_n):
    geom = GEOMS[g]
    cols = geom[1]
    off = REF0 - 3.0 * TOL * MAG0
    # (2, 0) comes after (1, tiles_n - 1) in row-major order although its column is lower
    c = Case(nblk, tiles_n, geom).csum(2, 0, off).csum(1, (tiles_n - 1) * cols + 1, off)
    expect_tiles(verdict(driver, c), [(1, tiles_n - 1), (2, 0)], 2, tiles_n)
    # every tile flagged once: the per-XCD counts are the XCD map's own histogram
    c = Case(nblk, tiles_n, geom)
    for tb in range(nblk):
        for tn in range(tiles_n):
            c.csum(tb, tn * cols + (tb + tn) % cols, off)
    r = verdict(driver, c)
    expect_tiles(r, [(tb, tn) for tb in range(nblk) for tn in range(tiles_n)], nblk * tiles_n, tiles_n)
    assert sum(r["out"][2:10]) == nblk * tiles_n
    assert max(r["out"][2:10]) - min(r["out"][2:10]) <= 1  # dealt round robin


@pytest.mark.parametrize("g,nblk,tiles_n", ALL, ids=ALL_IDS)
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_a_nan_or_infinite_sum_is_bad_and_makes_the_error_infinite(driver, g, nblk, tiles_n, poison):
    geom = GEOMS[g]
    j = geom[1] * tiles_n - 1
    r = verdict(driver, Case(nblk, tiles_n, geom).csum(0, j, poison))
    expect_tiles(r, [(0, tiles_n - 1)], 1, tiles_n)
    assert r["max_err"] == float("inf")
    # ... and stays infinite when a finite error follows it
    r = verdict(driver, Case(nblk, tiles_n, geom).csum(0, 0, poison).csum(nblk - 1, j, REF0 + 5.0 * TOL * MAG0))
    assert r["max_err"] == float("inf") and r["out"][1] == 2


@pytest.mark.parametrize("nblk,tiles_n", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_the_two_128_row_halves_are_added_before_they_are_judged(driver, nblk, tiles_n):
    """The fused kernels give one column sum per 128 rows, two per 256-row tile, in consecutive rows of csum:
    half 0 + half 1 is judged.  A delta in half 1 alone is seen; opposite deltas in the two halves cancel; the sums
    the verdict judged are the two halves' sum for every row block."""
    geom = GEOMS["256"]
    n = tiles_n * 256
    tb, j = nblk - 1, n - 256  # the last row block: its halves are csum rows 2 * nblk - 2 and 2 * nblk - 1
    delta = 1.01 * TOL * MAG0
    clean = verdict(driver, Case(nblk, tiles_n, geom, halves=2))
    expect_tiles(clean, [], 0, tiles_n)
    assert clean["max_err"] == 0.0 and all(fx(s) == REF0 for s in clean["judged"])
    r = verdict(driver, Case(nblk, tiles_n, geom, halves=2).csum(tb, j, 600.0 + delta, half=1))
    expect_tiles(r, [(tb, tiles_n - 1)], 1, tiles_n)
    judged = [fx(s) for s in r["judged"]]
    assert judged[tb * n + j] == 400.0 + (600.0 + delta) and sum(x != REF0 for x in judged) == 1
    r = verdict(driver, Case(nblk, tiles_n, geom, halves=2).csum(tb, j, 400.0 + delta, half=0))
    expect_tiles(r, [(tb, tiles_n - 1)], 1, tiles_n)
    r = verdict(driver, Case(nblk, tiles_n, geom, halves=2).csum(tb, j, 400.0 + 64.0, half=0)
                .csum(tb, j, 600.0 - 64.0, half=1))
    expect_tiles(r, [], 0, tiles_n)
    assert r["max_err"] == 0.0


def test_a_zero_tolerance_flags_any_difference_and_only_that(driver):
    geom = GEOMS["256"]
    r = verdict(driver, Case(3, 5, geom, tol=0.0))
    expect_tiles(r, [], 0, 5)
    assert r["floor"] == 0.0
    r = verdict(driver, Case(3, 5, geom, tol=0.0).csum(1, 700, math.nextafter(REF0, 2 * REF0)))
    expect_tiles(r, [(1, 2)], 1, 5)


# ------------------------------------------------------------------------------------------- the sampled reduction
def sampled(driver, got, ref, mag, fused, by_mag):
    n = len(got)
    return fx(driver(["sampled", n, int(fused), int(by_mag)] + [float(x) for x in got] + [float(x) for x in ref]
                     + [float(x) for x in mag])[0])


def test_the_sampled_reduction_divides_by_the_documented_denominators(driver):
    """bf16: |got - ref| / max(1, |ref|); fp8: |got - ref| / mag; the worst of the samples is returned."""
    got, ref, mag = [10.5, 0.75, -40.0, 2.0], [10.0, 0.25, -44.0, 2.0], [4.0, 16.0, 8.0, 1.0]
    assert sampled(driver, got, ref, mag, False, False) == max(0.5 / 10.0, 0.5 / 1.0, 4.0 / 44.0, 0.0)
    assert sampled(driver, got[:1], ref[:1], mag[:1], False, False) == 0.5 / 10.0
    assert sampled(driver, got[2:3], ref[2:3], mag[2:3], False, False) == 4.0 / 44.0
    assert sampled(driver, got, ref, mag, False, True) == max(0.5 / 4.0, 0.5 / 16.0, 4.0 / 8.0, 0.0)
    assert sampled(driver, got[:2], ref[:2], mag[:2], False, True) == 0.5 / 4.0
    assert sampled(driver, [2.0, 3.0], [2.0, 3.0], [1.0, 0.0], False, True) == 0.0
    assert sampled(driver, [0.5], [0.0], [0.0], False, True) == 0.5 / 1e-30  # an empty magnitude cannot hide an error


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("by_mag", [False, True])
def test_a_nan_output_makes_the_sampled_error_infinite(driver, fused, by_mag):
    nan = float("nan")
    assert sampled(driver, [1.0, nan, 2.0], [1.0, 5.0, 2.0], [1.0, 1.0, 1.0], fused, by_mag) == float("inf")
    assert sampled(driver, [1.0, 5.0, 2.0], [1.0, nan, 2.0], [1.0, 1.0, 1.0], fused, by_mag) == float("inf")


def test_the_fused_flag_routes_the_sampled_error_through_the_bf16_forgiveness(driver):
    ref = 100.0 + 2.0 ** -4  # not a bf16 value: bf16 spacing at 100 is 0.5
    got1, got4 = 100.0, 102.0  # the rounded output, and one four ulps higher
    assert sampled(driver, [got1], [ref], [50.0], True, False) == 0.0
    assert sampled(driver, [got1], [ref], [50.0], False, False) == (ref - got1) / ref
    beyond = abs(got4 - ref) - math.ldexp(max(got4, ref), -8) * 1.01
    assert sampled(driver, [got4], [ref], [50.0], True, False) == beyond / ref
    assert sampled(driver, [got4], [ref], [50.0], True, True) == beyond / 50.0
    assert sampled(driver, [got1, got4], [ref, ref], [50.0, 50.0], True, True) == beyond / 50.0
