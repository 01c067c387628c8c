"""MI355X-only: the referee of the ``gemm`` / ``gemm_fp8`` diagnostics against an fp64 model, at its edge shapes.

The diagnostics decide whether a GPU computes correctly; the code that makes the call -- the sampled reference
kernels, the checksum kernels, the fills, and the host verdict behind them -- is run here through
``diag.gemm_verify`` on buffers this file owns.  Operands and C are built on the CPU and copied over; C is the model's
product, never a kernel's, and no GEMM kernel is launched.  The model (``gemm_cases.referee_model``) runs in float64
torch on the CPU.  A referee that is too lenient looks exactly like a healthy GPU, so every number it produces is
held to the model: bit for bit where the operands make fp64 exact, else to bounds derived from the arithmetic.

Shapes are the smallest that reach each guard: N = 384 and N = 1280 put half of a 256-column block of
``ck_ref_kernel`` past N, 1152 = 9 x 128 and 2304 = 9 x 256 rows reach the second CK_TB group of row blocks and its
``tb0 + t < nblk`` guard, K = 64 / 128 sit behind ``ck_asum_kernel``'s ``k >= K`` guard, M != N everywhere but the
one-tile shapes.  The host half of the verdict has its own CPU tests (test_gemm_verdict_cpu.py).
"""
import math
import zlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gemm_cases as G  # noqa: E402
from test_gpu import _tile_xcd  # noqa: E402

NSAMP = 4096
# (dtype, geom, M, N, the two K of the shape): every shape with its smallest K and one other
SHAPES = [("bf16", 0, 128, 128, (64, 1024)), ("bf16", 0, 1152, 384, (64, 192)), ("bf16", 0, 384, 1152, (64, 1024)),
          ("bf16", 1, 256, 256, (64, 192)), ("bf16", 1, 2304, 256, (64, 1024)), ("bf16", 1, 512, 1280, (64, 192)),
          ("fp8", 1, 256, 256, (128, 384)), ("fp8", 1, 2304, 256, (128, 1024)), ("fp8", 1, 512, 1280, (128, 384))]
CASES = [(dt, g, m, n, k) for dt, g, m, n, ks in SHAPES for k in ks]
# fp32 C everywhere; bf16 C with fused column sums where the diagnostics have it (256^2 tiles)
MODES = [c + (fused,) for c in CASES for fused in ((False, True) if c[1] == 1 else (False,))]
GEOM = {0: (128, 128, 8), 1: (256, 256, 4)}  # tile rows, tile columns, group_m
SMALLEST_K = {"bf16": 64, "fp8": 128}


def _id(c):
    return "%s-g%d-%dx%dx%d" % c[:5] + ("" if len(c) < 6 else "-bf16C" if c[5] else "-fp32C")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _tol(dtype):
    from k8s_gpu_node_checker_amd.ops import diag
    return diag.GEMM_CK_TOL if dtype == "bf16" else diag.GEMM_FP8_CK_TOL


def _device_copy(t, fill, dev):
    """``t`` (2-D) on the device between guard bands: NaN round operands and C, so a read outside shows."""
    b = G.banded(t.shape[0], t.shape[1] * t.element_size(), fill, dev)
    b.put(t.to(dev))
    return b


class Problem:
    """One (operands, model, outputs) set: everything the tests of a shape share, computed once and left unchanged
    (a test that edits an output on the device puts the old value back)."""

    def __init__(self, dtype, geom, m, n, k, family, dev):
        self.dtype, self.geom, self.m, self.n, self.k = dtype, geom, m, n, k
        self.rb, self.cols, self.group_m = GEOM[geom]
        gen = torch.Generator().manual_seed(zlib.crc32(repr((dtype, geom, m, n, k, family)).encode()))
        if family == "int":
            (a, a64), (bt, bt64) = G.integer_operand(dtype, m, k, gen), G.integer_operand(dtype, n, k, gen)
        elif dtype == "fp8":
            (a, a64), (bt, bt64) = G.wide_fp8_operand(m, k, gen), G.wide_fp8_operand(n, k, gen)
        else:
            (a, a64), (bt, bt64) = G.wide_bf16_operand(m, k, gen), G.wide_bf16_operand(n, k, gen)
        self.a64, self.bt64 = a64, bt64
        self.model = G.referee_model(a64, bt64, self.rb)
        self.c32 = self.model["c"].to(torch.float32)
        raw = (lambda t: t.view(torch.uint8)) if dtype == "fp8" else (lambda t: t)
        self.A, self.Bt = _device_copy(raw(a), dtype, dev), _device_copy(raw(bt), dtype, dev)
        self.C32 = _device_copy(self.c32, "bf16", dev)
        self.c32_dev = self.C32.view(torch.float32)
        if geom == 1:
            self.c16 = self.model["c"].to(torch.float32).to(torch.bfloat16)
            self.cs = G.block_sums(self.model["c"], 128)  # the fused sums come from the accumulators, not from bf16 C
            self.C16, self.CS = _device_copy(self.c16, "bf16", dev), _device_copy(self.cs, "bf16", dev)
            self.c16_dev, self.cs_dev = self.C16.view(torch.bfloat16), self.CS.view(torch.float64)

    def verify(self, fused, tol, nsamp=NSAMP):
        from k8s_gpu_node_checker_amd.ops import diag
        r = diag.gemm_verify(self.dtype, self.A.data_ptr(), self.Bt.data_ptr(),
                             self.C16.data_ptr() if fused else self.C32.data_ptr(),
                             self.CS.data_ptr() if fused else None, self.m, self.n, self.k, self.geom, nsamp, tol)
        for b in (self.A, self.Bt, self.C32):
            assert b.intact()
        return r

    def tile_of(self, row, col):
        return row // self.rb, col // self.cols

    def xcd_of(self, tile):
        return _tile_xcd(tile[0], tile[1], self.m // self.rb, self.n // self.cols, self.group_m)


_problems = {}


def problem(dev, dtype, geom, m, n, k, family="int"):
    key = (dtype, geom, m, n, k, family)
    if key not in _problems:
        _problems[key] = Problem(*key, dev)
    return _problems[key]


def _t(values, shape=None):
    t = torch.tensor(values, dtype=torch.float64)
    return t if shape is None else t.view(shape)


def _clean_out(r):
    return r["ck_out"] == [0] * 10 + [-1, -1]


def _one_tile(p, r, tile, columns=1):
    want = [1, columns] + [1 if x == p.xcd_of(tile) else 0 for x in range(8)] + list(tile)
    assert r["ck_out"] == want, (r["ck_out"], want)


# ---------------------------------------------------------------------------------------------- integer operands
@pytest.mark.parametrize("case", MODES, ids=_id)
def test_integer_operands_every_referee_number_equals_the_model_bit_for_bit(dev, case):
    """Independent integers in -8..8 on both sides: |C| <= 64 K < 2^24 is exact in fp32, and every reference,
    magnitude and column sum is an integer below 2^53, exact in fp64 in any order.  So the sampled ref and mag, the
    per-column ref, mag and csum and the floor must equal the model exactly, and the clean C has error exactly 0.
    With bf16 C (the model rounded) the fused sums are ``block_sums(model, 128)``: the two 128-row halves must be
    added, and ``gather_kernel<__bf16>``'s outputs forgiven their rounding."""
    dtype, geom, m, n, k, fused = case
    p = problem(dev, dtype, geom, m, n, k)
    tol = _tol(dtype)
    r = p.verify(fused, tol)
    rows, cols = torch.tensor(r["rows"]), torch.tensor(r["cols"])
    assert len(rows) == NSAMP and bool(((rows >= 0) & (rows < m) & (cols >= 0) & (cols < n)).all())
    if m > n:
        assert int(rows.max()) >= n  # rows range over M
    if n > m:
        assert int(cols.max()) >= m
    assert torch.equal(_t(r["ref"]), p.model["c"][rows, cols])
    want_mag = p.model["mag"][rows, cols] if dtype == "fp8" else torch.zeros(NSAMP, dtype=torch.float64)
    assert torch.equal(_t(r["mag"]), want_mag)
    shape = (m // p.rb, n)
    assert torch.equal(_t(r["ck_ref"], shape), p.model["ck_ref"])
    assert torch.equal(_t(r["ck_mag"], shape), p.model["ck_mag"])
    assert torch.equal(_t(r["ck_csum"], shape), G.block_sums(p.model["c"], p.rb))
    assert torch.equal(p.model["ck_ref"], G.block_sums(p.model["c"], p.rb))  # (the identity the checksums rest on)
    assert r["ck_floor"] == tol * float(p.model["ck_mag"].max())
    assert r["ck_err"] == 0.0 and r["max_err"] == 0.0 and _clean_out(r), r["ck_out"]


# ------------------------------------------------------------------------------------------------- wide operands
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "fp8"], ids=_id)
def test_wide_fp8_operands_stay_bit_for_bit(dev, case):
    """Every one of the 254 finite E4M3 codes, cycled in a random order per row.  Products carry 8 significant bits
    between 2^-18 and 2^18 and K <= 1024, so every sum the fp8 referee forms in fp64 is exact
    (test_gemm_exact_inputs_cpu.py has the count) and equals the model whatever the order: the sampled ref and mag
    and the per-column ref and mag.  C is the model rounded to fp32: each output is within 2^-24 of itself, hence
    of its sum |a b|, so the sampled error is at most 2^-24 and a column's residual at most 2^-24 mag plus the
    gamma_256(2^-53) of ``ck_csum_kernel``'s fp64 sum of 256 fp32 values."""
    dtype, geom, m, n, k = case
    p = problem(dev, dtype, geom, m, n, k, "wide")
    r = p.verify(False, _tol(dtype))
    rows, cols = torch.tensor(r["rows"]), torch.tensor(r["cols"])
    assert torch.equal(_t(r["ref"]), p.model["c"][rows, cols])
    assert torch.equal(_t(r["mag"]), p.model["mag"][rows, cols])
    shape = (m // p.rb, n)
    assert torch.equal(_t(r["ck_ref"], shape), p.model["ck_ref"])
    assert torch.equal(_t(r["ck_mag"], shape), p.model["ck_mag"])
    want = (p.c32.to(torch.float64)[rows, cols] - p.model["c"][rows, cols]).abs() / p.model["mag"][rows, cols]
    assert r["max_err"] == float(want.max()) and r["max_err"] <= 2.0 ** -24
    csum, sums = _t(r["ck_csum"], shape), G.block_sums(p.c32, p.rb)
    assert bool(((csum - sums).abs() <= G.gamma(p.rb, 2.0 ** -53) * G.block_sums(p.c32.abs(), p.rb)).all())
    assert r["ck_err"] <= 2.0 ** -24 + 2 * G.gamma(p.rb, 2.0 ** -53) and _clean_out(r)
    assert r["ck_floor"] == _tol(dtype) * float(p.model["ck_mag"].max())


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "bf16"], ids=_id)
def test_wide_bf16_operands_stay_inside_bounds_that_depend_on_no_measurement(dev, case):
    """``randn`` scaled over about 40 binades per row, so sums cancel and fp64 is no longer exact.  With
    gamma_n(u) = n u / (1 - n u):

    * the sampled reference is a serial fp32 sum of K products that are exact in fp32 (8 x 8 significant bits):
      |ref - model| <= gamma_K(2^-24) sum |a b|;
    * a column reference is an fp64 sum over the rb rows of a block, then an fp64 dot product over K:
      |ck_ref - model| <= gamma_{K + rb}(2^-53) ck_mag, and ck_mag itself, a sum of non-negative terms formed the
      same way, is within gamma_{K + rb}(2^-53) of the model's;
    * ``ck_csum_kernel`` adds rb fp32 values in fp64: |csum - sum| <= gamma_rb(2^-53) sum |C|;
    * C is the model rounded to fp32, each output within 2^-24 |c| <= 2^-24 sum |a b| of the model, so a column's
      residual is at most (2^-24 + 3 gamma_{K + rb}(2^-53)) ck_mag: below GEMM_CK_TOL, nothing is flagged.

    (The model's own float64 sums obey the same gamma; the referee is held to one gamma of the model all the same,
    which is the stricter reading.)"""
    dtype, geom, m, n, k = case
    p = problem(dev, dtype, geom, m, n, k, "wide")
    tol = _tol(dtype)
    r = p.verify(False, tol)
    rows, cols = torch.tensor(r["rows"]), torch.tensor(r["cols"])
    g32, g64 = G.gamma(k, 2.0 ** -24), G.gamma(k + p.rb, 2.0 ** -53)
    assert bool(((_t(r["ref"]) - p.model["c"][rows, cols]).abs() <= g32 * p.model["mag"][rows, cols]).all())
    shape = (m // p.rb, n)
    ck_ref, ck_mag, csum = _t(r["ck_ref"], shape), _t(r["ck_mag"], shape), _t(r["ck_csum"], shape)
    assert bool(((ck_ref - p.model["ck_ref"]).abs() <= g64 * p.model["ck_mag"]).all())
    assert bool(((ck_mag - p.model["ck_mag"]).abs() <= g64 * p.model["ck_mag"]).all())
    sums, sums_abs = G.block_sums(p.c32, p.rb), G.block_sums(p.c32.abs(), p.rb)
    assert bool(((csum - sums).abs() <= G.gamma(p.rb, 2.0 ** -53) * sums_abs).all())
    assert r["ck_err"] <= 2.0 ** -24 + 3 * g64 and r["ck_err"] < tol and _clean_out(r)
    assert abs(r["ck_floor"] - tol * float(p.model["ck_mag"].max())) <= 2 * g64 * r["ck_floor"]
    # the sampled error of the rounded model against the fp32 reference, as the library divides it
    ref = _t(r["ref"])
    got = p.c32.to(torch.float64)[rows, cols]
    assert r["max_err"] == float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
    bound = (2.0 ** -24 * p.model["c"][rows, cols].abs() + g32 * p.model["mag"][rows, cols]) / ref.abs().clamp_min(1.0)
    assert r["max_err"] <= float(bound.max()) * (1 + 2.0 ** -20)


# ----------------------------------------------------------------------------------------------- sharp threshold
def _positions(p, fused):
    """(row, column, why) of the outputs raised by delta."""
    m, n, rb, cols = p.m, p.n, p.rb, p.cols
    out = [(0, 0, "first"), (m - 1, n - 1, "last")]
    if m > rb:
        out += [(rb - 1, 5, "last row of a tile"), (rb, 5, "first row of the next")]
    if n > cols:
        out += [(7, cols - 1, "last column of a tile"), (7, cols, "first column of the next")]
    if fused:
        out += [(128 + 3, 9, "second 128-row half of a tile"), (m - 1 - 2, n - cols, "second half of the last tile row")]
    if m // rb == 9:
        out += [(8 * rb + 1, n - 3, "row block 8")]
    return out


def _raise_output(p, fused, row, col, delta):
    """Raise one output by delta on the device: in fp32 C, or in the fused sum of the output's 128-row half (the
    checksums of the bf16-output kernels never read C).  Returns (the change of the column's sum as the referee
    will see it, undo): fp32 C holds the nearest fp32 value, and the two halves are added in fp64."""
    if fused:
        half = row // 128
        cell = p.cs_dev[half]
        old = float(p.cs[half, col])
        new = old + delta
        pair = [float(p.cs[half - half % 2, col]), float(p.cs[half - half % 2 + 1, col])]
        before = pair[0] + pair[1]
        pair[half % 2] = new
        took = (pair[0] + pair[1]) - before
    else:
        cell = p.c32_dev[row]
        old = float(p.c32[row, col])
        new = float(torch.tensor(old + delta, dtype=torch.float64).to(torch.float32))
        took = new - old  # the other outputs of the column are integers: the fp64 sum moves by exactly this
    cell[col] = new
    torch.cuda.synchronize()

    def undo():
        cell[col] = old
        torch.cuda.synchronize()
    return took, undo


@pytest.mark.parametrize("case", [c for c in MODES if c[4] == SMALLEST_K[c[0]]], ids=_id)
def test_one_output_raised_by_delta_is_flagged_exactly_above_tol_times_its_columns_magnitude(dev, case):
    """On integer operands the clean residual is exactly 0, so the threshold of column j of row block tb is exactly
    tol x mag[tb][j], taken from the model.  One output raised by 0.99 x that: nothing flagged; by 1.01 x that, or by
    2 x floor: exactly its tile, one column, first bad tile and XCD right (the XCD map restated in test_gpu.py, also at
    M != N).  fp32 C cannot hold every delta, nor can the fp64 sum of two halves: the delta that took effect is worked
    out, must lie within half a percent of the factor asked for, and gives the expected error to the bit."""
    dtype, geom, m, n, k, fused = case
    p = problem(dev, dtype, geom, m, n, k)
    tol = _tol(dtype)
    floor = tol * float(p.model["ck_mag"].max())
    for row, col, why in _positions(p, fused):
        tile = p.tile_of(row, col)
        mag = float(p.model["ck_mag"][tile[0], col])
        for factor, delta in ((0.99, 0.99 * tol * mag), (1.01, 1.01 * tol * mag), (None, 2 * floor)):
            took, undo = _raise_output(p, fused, row, col, delta)
            try:
                r = p.verify(fused, tol, nsamp=16)
            finally:
                undo()
            if factor is not None:
                assert abs(took / (tol * mag) - factor) < 0.005, (why, took, delta)
            assert r["ck_err"] == abs(took) / mag, (why, factor, r["ck_err"], took / mag)
            if factor == 0.99:
                assert _clean_out(r), (why, r["ck_out"])
            else:
                _one_tile(p, r, tile)
            assert r["ck_floor"] == floor
    assert p.verify(fused, tol, nsamp=16)["ck_err"] == 0.0  # everything was put back


def test_a_zero_tolerance_flags_any_difference_and_a_negative_one_checks_nothing(dev):
    p = problem(dev, "bf16", 1, 512, 1280, 64)
    r = p.verify(False, 0.0)
    assert r["ck_err"] == 0.0 and r["ck_floor"] == 0.0 and _clean_out(r)
    row, col = 300, 1279
    took, undo = _raise_output(p, False, row, col, 2.0 ** -8)  # |C| <= 4096: above its fp32 ulp
    try:
        assert took != 0.0
        r0, rneg = p.verify(False, 0.0), p.verify(False, -1.0)
    finally:
        undo()
    _one_tile(p, r0, (1, 4))
    assert r0["ck_err"] == abs(took) / float(p.model["ck_mag"][1, col]) and r0["ck_floor"] == 0.0
    # no checksums: their outputs stay as the caller set them (the binding: zeros) and nothing is gathered
    assert rneg["ck_err"] == 0.0 and rneg["ck_out"] == [0] * 12 and rneg["ck_floor"] == 0.0
    assert rneg["ck_ref"] == [] and len(rneg["ref"]) == NSAMP


# ------------------------------------------------------------------------------------------------- sampled check
@pytest.mark.parametrize("case", [("bf16", 0, 384, 1152, 64), ("bf16", 1, 512, 1280, 192), ("fp8", 1, 512, 1280, 128),
                                  ("fp8", 1, 2304, 256, 1024)], ids=_id)
def test_the_sampled_error_of_fp32_c_is_delta_over_the_documented_denominator(dev, case):
    """A sampled output raised by delta: max_err = delta / max(1, |ref|) (bf16) or delta / mag (fp8), evaluated as
    the library does; exactly 0 without it.  A NaN at an output no sample reads leaves max_err 0, flags its tile
    and makes the checksum error infinite."""
    dtype, geom, m, n, k = case
    p = problem(dev, dtype, geom, m, n, k)
    tol = _tol(dtype)
    clean = p.verify(False, tol)
    assert clean["max_err"] == 0.0
    sampled = set(zip(clean["rows"], clean["cols"]))
    for i in (0, NSAMP - 1):
        row, col = clean["rows"][i], clean["cols"][i]
        took, undo = _raise_output(p, False, row, col, 0.5)
        try:
            r = p.verify(False, tol)
        finally:
            undo()
        assert took == 0.5  # |C| < 2^22: exact in fp32
        ref = float(p.model["c"][row, col])
        denom = float(p.model["mag"][row, col]) if dtype == "fp8" else max(1.0, abs(ref))
        assert r["max_err"] == 0.5 / denom, (r["max_err"], 0.5 / denom)
    row, col = next((r_, c_) for r_ in range(m - 1, -1, -1) for c_ in range(n - 1, -1, -1)
                    if (r_, c_) not in sampled)
    _, undo = _raise_output(p, False, row, col, float("nan"))
    try:
        r = p.verify(False, tol)
    finally:
        undo()
    assert r["max_err"] == 0.0 and r["ck_err"] == float("inf")
    _one_tile(p, r, p.tile_of(row, col))


def _beyond(got, ref):
    """gemm_verdict.h's beyond_bf16_rounding, restated (test_gemm_verdict_cpu.py holds the original to it)."""
    e = abs(got - ref) - math.ldexp(max(abs(got), abs(ref)), -8) * 1.01
    return e if e > 0.0 else 0.0


@pytest.mark.parametrize("case", [("bf16", 1, 512, 1280, 192), ("fp8", 1, 2304, 256, 1024)], ids=_id)
def test_the_sampled_error_of_bf16_c_lies_beyond_the_outputs_own_rounding(dev, case):
    """bf16 C = the model rounded: error 0.  One ulp more is forgiven where the forgiveness 1.01 x 2^-8 x |value|
    (between half an ulp and one ulp) covers it -- a value in the top of its binade -- and is reported as what lies
    beyond it where it does not; four ulps (towards zero) are reported as ``beyond_bf16_rounding`` over the type's denominator; NaN
    at a sampled output gives infinity."""
    dtype, geom, m, n, k = case
    p = problem(dev, dtype, geom, m, n, k)
    clean = p.verify(True, -1.0)
    assert clean["max_err"] == 0.0
    c16 = p.c16.to(torch.float64)

    def ulp(v):
        return math.ldexp(1.0, math.frexp(abs(v))[1] - 8)

    def run(row, col, value):
        old = p.c16[row, col].clone()
        p.c16_dev[row, col] = value
        torch.cuda.synchronize()
        try:
            return p.verify(True, -1.0)["max_err"]
        finally:
            p.c16_dev[row, col] = old
            torch.cuda.synchronize()

    def denom(row, col):
        ref = float(p.model["c"][row, col])
        return float(p.model["mag"][row, col]) if dtype == "fp8" else max(1.0, abs(ref))

    samples = list(dict.fromkeys(zip(clean["rows"], clean["cols"])))
    big = [(r_, c_) for r_, c_ in samples if abs(float(c16[r_, c_])) >= 2.0]
    one_more = {rc: float(c16[rc]) + math.copysign(ulp(float(c16[rc])), float(c16[rc])) for rc in big}
    forgiven = next(rc for rc in big if _beyond(one_more[rc], float(p.model["c"][rc])) == 0.0)
    reported = next(rc for rc in big if _beyond(one_more[rc], float(p.model["c"][rc])) > 0.0)
    assert run(*forgiven, one_more[forgiven]) == 0.0
    want = _beyond(one_more[reported], float(p.model["c"][reported])) / denom(*reported)
    assert run(*reported, one_more[reported]) == want and want > 0.0
    for rc in (forgiven, reported):
        v = float(c16[rc])
        got = v - math.copysign(4 * ulp(v), v)  # towards zero: the spacing only gets finer, so still a bf16 value
        assert float(torch.tensor(got).to(torch.bfloat16)) == got
        want = _beyond(got, float(p.model["c"][rc])) / denom(*rc)
        assert run(*rc, got) == want and want > 0.0
    assert run(*forgiven, float("nan")) == float("inf")


# ----------------------------------------------------------------------------------------------------- the fills
FILL_N = 2048 * 256 * 2 + 5  # more than two grid-stride passes of the fills' 2048 x 256 threads, and a ragged end


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_the_fills_stay_in_their_documented_value_sets_and_inside_their_buffer(dev, dtype):
    from k8s_gpu_node_checker_amd.ops import diag
    size = 2 if dtype == "bf16" else 1
    bufs = [G.banded(FILL_N, size, dtype, dev) for _ in range(3)]
    for b, seed in zip(bufs, (0x1234, 0x1234, 0xBEEF)):
        diag.gemm_fill(dtype, b.data_ptr(), FILL_N, seed)
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    a, again, other = (b.payload.cpu() for b in bufs)
    assert torch.equal(a, again) and not torch.equal(a, other)
    if dtype == "bf16":
        v = a.view(torch.bfloat16).to(torch.float64).flatten()
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 1.0
        assert float(v.min()) < -0.99 and float(v.max()) > 0.99 and abs(float(v.mean())) < 0.01
    else:
        want = sorted(s << 7 | e << 3 | f for s in (0, 1) for e in range(9) for f in range(8))
        assert len(want) == 144 and sorted(a.flatten().unique().tolist()) == want


def test_e4m3_decodes_on_the_device_as_on_the_host(dev):
    """K = 128 holds half of the 254 finite codes: even rows of A carry the first 127 and a zero, odd rows the
    rest, against columns of ones.  The fp8 sampled ref is then the sum of the row's decoded codes and mag the sum
    of their magnitudes, both exact -- every finite code's device decode, against the format."""
    from k8s_gpu_node_checker_amd.ops import diag
    m = n = 256
    halves = [G.FP8_FINITE[:127] + [0], G.FP8_FINITE[127:] + [0]]
    a = torch.tensor([halves[r % 2] for r in range(m)], dtype=torch.uint8)
    perm = torch.stack([torch.randperm(128, generator=torch.Generator().manual_seed(r)) for r in range(m)])
    a = torch.gather(a, 1, perm)
    bt = torch.full((n, 128), 0x38, dtype=torch.uint8)
    a64 = G.decode_e4m3(a)
    c = a64.sum(dim=1, keepdim=True).expand(m, n).contiguous()
    A, Bt, C = _device_copy(a, "fp8", dev), _device_copy(bt, "fp8", dev), _device_copy(c.to(torch.float32), "bf16", dev)
    r = diag.gemm_verify("fp8", A.data_ptr(), Bt.data_ptr(), C.data_ptr(), None, m, n, 128, 1, NSAMP, -1.0)
    rows = torch.tensor(r["rows"])
    assert set((rows % 2).tolist()) == {0, 1}
    assert torch.equal(_t(r["ref"]), a64.sum(dim=1)[rows])
    assert torch.equal(_t(r["mag"]), a64.abs().sum(dim=1)[rows])


# ------------------------------------------------------------------------------------------------ argument checks
def test_refused_arguments_raise_before_anything_is_launched(dev):
    from k8s_gpu_node_checker_amd.ops import diag
    p = problem(dev, "bf16", 1, 256, 256, 64)
    a, bt, c32, c16, cs = (b.data_ptr() for b in (p.A, p.Bt, p.C32, p.C16, p.CS))

    def refused(match, dtype="bf16", a=a, bt=bt, c=c32, csum=None, m=256, n=256, k=64, geom=1, samples=16):
        with pytest.raises(RuntimeError, match=match):
            diag.gemm_verify(dtype, a, bt, c, csum, m, n, k, geom, samples, 1e-7)

    refused("multiples of the tile", m=200)
    refused("multiples of the tile", n=64, geom=0)
    refused("multiples of the tile", k=96)
    refused("multiples of the tile", dtype="fp8", k=64)
    refused("multiples of the tile", m=384)          # geom 1 with M off 256
    refused("multiples of the tile", n=128)          # geom 1 with N off 256
    refused("multiples of the tile", m=0)
    refused("nsamp must be at least 1", samples=0)
    refused("null operand", a=None)
    refused("null operand", bt=None)
    refused("null operand", c=None)
    refused("geom 1.*only", c=c16, csum=cs, geom=0)
    refused("geom 0 .*bf16 only", dtype="fp8", k=128, geom=0)
    refused("geom 0 .*or 1", geom=2)
    with pytest.raises(RuntimeError, match="gemm_fill"):
        diag.gemm_fill("bf16", None, 16, 1)
    with pytest.raises(RuntimeError, match="gemm_fill"):
        diag.gemm_fill("fp8", a, 0, 1)
    assert p.verify(False, 1e-7, nsamp=1)["max_err"] == 0.0  # one sample is enough
