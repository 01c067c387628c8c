"""Helpers for the GEMM kernel tests (no tests here): guard-banded buffers, the product of the public GEMM knobs,
and operands whose product is exact in fp32 whatever the accumulation order.

Used by test_gemm_exact_inputs_cpu.py (which proves the helpers on the CPU), test_gpu_gemm_matrix.py and
test_gpu_gemm_referee.py (the operands and the fp64 model of the diagnostics' referee, at the end of the file).
"""
import itertools
import math

import torch

BAND_ROWS = 256  # one 256-row panel before and one after the payload

# Band contents, by what the buffer holds.  Inputs: NaN where the format has one, so a *used* read outside the
# matrix poisons C; fp4 has no NaN, there 0x77 = (+6, +6), the largest magnitude, and the fp64 comparison sees it.
# Outputs: a fixed bit pattern, compared bit for bit after a launch.
BAND_BYTES = {
    "bf16": (0xC0, 0x7F),   # 0x7FC0 little-endian: the bf16 quiet NaN
    "fp8": (0x7F,),         # E4M3 (float8_e4m3fn) NaN
    "fp4": (0x77,),
    "out": (0xA5, 0x5A, 0xC3, 0x3C),  # no float format reads this as NaN, and no kernel writes it
}

K_TILE = {"bf16": 64, "fp8": 128, "fp4": 256}   # columns of one K-tile
ELEM_BYTES = {"bf16": 2.0, "fp8": 1.0, "fp4": 0.5}  # operand bytes per K column


class Banded:
    """``rows x row_bytes`` payload bytes between two bands of ``BAND_ROWS * row_bytes`` bytes, one allocation."""

    def __init__(self, rows, row_bytes, fill, device="cpu"):
        self.rows, self.row_bytes, self.fill = rows, row_bytes, fill
        self.band_bytes = BAND_ROWS * row_bytes  # a multiple of 256 B: the payload keeps the allocation's alignment
        pat = BAND_BYTES[fill]
        assert row_bytes % len(pat) == 0 and row_bytes > 0 and rows > 0
        self.raw = torch.empty(2 * self.band_bytes + rows * row_bytes, dtype=torch.uint8, device=device)
        self._pattern = torch.tensor(pat, dtype=torch.uint8, device=device).repeat(self.band_bytes // len(pat))
        self.before = self.raw[:self.band_bytes]
        self.after = self.raw[self.band_bytes + rows * row_bytes:]
        self.payload = self.raw[self.band_bytes:self.band_bytes + rows * row_bytes].view(rows, row_bytes)
        self.before.copy_(self._pattern)
        self.after.copy_(self._pattern)
        self.payload.zero_()

    def view(self, dtype):
        """The payload as ``rows x (row_bytes / itemsize)`` of ``dtype`` (a view: writes go to the buffer)."""
        return self.payload.view(dtype)

    def put(self, t):
        """Copy ``t`` (``rows`` rows, ``row_bytes`` bytes each) into the payload; returns the payload view."""
        v = self.view(t.dtype)
        assert v.shape == t.shape, (v.shape, t.shape)
        v.copy_(t)
        return v

    def data_ptr(self):
        return self.payload.data_ptr()

    def intact(self):
        """Both bands still hold their pattern, bit for bit (compared as integers: NaN never equals NaN)."""
        return bool(torch.equal(self.before, self._pattern)) and bool(torch.equal(self.after, self._pattern))


def banded(nbytes_rows, row_bytes, fill, device="cpu"):
    """A buffer of ``nbytes_rows`` rows of ``row_bytes`` bytes between two guard bands of one 256-row panel each.
    ``fill`` names the band contents: ``bf16`` / ``fp8`` / ``fp4`` for an operand, ``out`` for an output."""
    return Banded(nbytes_rows, row_bytes, fill, device)


def knob_matrix(dtype):
    """Every combination of the public v3 knobs as ``diag.gemm_config`` kwargs (all knobs spelled out, so a case
    inherits nothing), plus the other kernels of the dtype.  Where a knob is ignored two entries launch the same
    kernel; that is harmless, and which instantiation a combination reaches is not the test's business."""
    forms = (True, False) if dtype == "fp8" else (True,)
    out = [dict(variant="v3", epilogue=e, buffer_loads=b, schedule=s, fp8_unscaled=u, tail=True)
           for e, b, s, u in itertools.product((True, False), (False, True), (1, 0), forms)]
    others = {"bf16": ("v1", "v2", "v4", "v4t"), "fp8": ("v4", "v4t"), "fp4": ()}[dtype]
    out += [dict(variant=v, epilogue=True, buffer_loads=False, schedule=1, fp8_unscaled=True, tail=True)
            for v in others]
    return out


def ck_matrix(dtype):
    """The configurations of the bf16-output kernel with fused column sums (``gemm_launch_ck``): v3 under both
    restaging orders and, for fp8, both MFMA forms; v4; v4t."""
    forms = (True, False) if dtype == "fp8" else (True,)
    out = [dict(variant="v3", epilogue=True, buffer_loads=False, schedule=s, fp8_unscaled=u, tail=True)
           for s, u in itertools.product((1, 0), forms)]
    out += [dict(variant=v, epilogue=True, buffer_loads=False, schedule=1, fp8_unscaled=True, tail=True)
            for v in ("v4", "v4t")]
    return out


def label(cfg):
    return " ".join(f"{k}={v}" for k, v in cfg.items())


# --- exact operands -------------------------------------------------------------------------------------------------

def decode_e4m3(codes):
    """OCP E4M3 (float8_e4m3fn) codes -> float64, written out from the format: 4 exponent bits (bias 7), 3 mantissa
    bits, subnormals at exponent field 0, 0x7F / 0xFF NaN, no infinities."""
    c = codes.to(torch.int64)
    sign = torch.where((c & 0x80) != 0, -1.0, 1.0).to(torch.float64)
    e, f = (c >> 3) & 0xF, (c & 7).to(torch.float64)
    normal = torch.ldexp(1.0 + f / 8.0, e - 7)
    sub = torch.ldexp(f / 8.0, torch.full_like(e, -6))
    v = sign * torch.where(e == 0, sub, normal)
    return torch.where((c & 0x7F) == 0x7F, torch.full_like(v, float("nan")), v)


# fp8: the 127 finite non-negative E4M3 codes, 0x00 (zero) and the 126 positive ones from the subnormal 2^-9
# (0x01) to 448 (0x7E).  (E4M3 has 126 positive finite codes; the zero row makes up the 127 and must come out 0.)
FP8_CODES = list(range(0x00, 0x7F))

# bf16: all 128 significands, each at two exponents; the exponent steps evenly over the list from 2^-120 to 2^117,
# so 256 rows carry every significand twice and about every exponent in between once.  The bottom keeps inputs and
# every non-zero output (at least v * 1) normal in bf16 / fp32, so the matrix core's denormal policy is not under
# test.  The top is 2^117, not 2^120: |C| can reach v * K, and (2 - 2^-7) * 2^117 * 640 < 2^128 keeps the largest
# K used (640) from overflowing fp32 in any partial sum.
BF16_EXP_LO, BF16_EXP_HI, BF16_EXP_STEPS = -120, 117, 2


def bf16_values():
    """[(significand index 0..127, exponent)] of the bf16 value list, in list order."""
    n = 128 * BF16_EXP_STEPS
    return [(i % 128, BF16_EXP_LO + (i * (BF16_EXP_HI - BF16_EXP_LO)) // (n - 1)) for i in range(n)]


def exact_operands(dtype, m, n, k, side, gen):
    """Operands (on the CPU, from the CPU generator ``gen``) whose GEMM ``A @ Bt.T`` is exact in fp32 in any
    accumulation order: the ``side`` operand (``"A"`` or ``"B"``) has one magnitude per row, ``+-v_r`` with random
    signs, ``v_r`` cycling through the dtype's value list; the other is drawn from {-1, 0, +1}.  Every product is
    ``+-v`` or 0 and every partial sum ``v x integer`` with |integer| <= k: 8 + 10 significant bits at most.

    Returns ``(a, bt, a64, bt64)``: the operands in ``dtype`` and their values in float64, decoded here from the
    bit patterns and not by a cast.  Each output row (side A) or column (side B) is a multiple of its own value, so
    a permuted or transposed write is off by a whole value."""
    assert side in ("A", "B") and dtype in ("bf16", "fp8")
    assert k <= 640, "the bf16 value list stays below fp32 overflow for K <= 640"
    rows_mag, rows_tern = (m, n) if side == "A" else (n, m)
    neg = torch.randint(0, 2, (rows_mag, k), generator=gen, dtype=torch.int64)
    tern = torch.randint(-1, 2, (rows_tern, k), generator=gen, dtype=torch.int64)
    r = torch.arange(rows_mag)
    if dtype == "fp8":
        codes = torch.tensor(FP8_CODES, dtype=torch.int64)[r % len(FP8_CODES)]
        mag_bits = (codes[:, None] | (neg << 7)).to(torch.uint8)
        tern_bits = torch.where(tern == 0, 0x00, torch.where(tern > 0, 0x38, 0xB8)).to(torch.uint8)  # 0x38 = 1.0
        mag, ter = mag_bits.view(torch.float8_e4m3fn), tern_bits.view(torch.float8_e4m3fn)
        mag64 = decode_e4m3(mag_bits)
    else:
        vals = bf16_values()
        sig = torch.tensor([s for s, _ in vals], dtype=torch.int64)[r % len(vals)]
        exp = torch.tensor([e for _, e in vals], dtype=torch.int64)[r % len(vals)]
        bits = (neg << 15) | ((exp[:, None] + 127) << 7) | sig[:, None]
        mag_bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
        tern_bits = torch.where(tern == 0, 0x0000, torch.where(tern > 0, 0x3F80, 0xBF80 - 0x10000)).to(torch.int16)
        mag, ter = mag_bits.view(torch.bfloat16), tern_bits.view(torch.bfloat16)
        mag64 = torch.ldexp(1.0 + sig.to(torch.float64) / 128.0, exp)[:, None] * (1 - 2 * neg).to(torch.float64)
    ter64 = tern.to(torch.float64)
    return (mag, ter, mag64, ter64) if side == "A" else (ter, mag, ter64, mag64)


def magnitude_bits(dtype, t):
    """The set of magnitude bit patterns (sign cleared) in operand ``t``."""
    if dtype == "fp8":
        return set((t.view(torch.uint8).to(torch.int64) & 0x7F).unique().tolist())
    return set((t.view(torch.int16).to(torch.int64) & 0x7FFF).unique().tolist())


def expected_magnitude_bits(dtype):
    if dtype == "fp8":
        return set(FP8_CODES)
    return {((e + 127) << 7) | s for s, e in bf16_values()}


def block_sums(c, rows=128):
    """fp64 column sums of ``c`` over every ``rows``-row block: what the fused column sums must equal."""
    m, n = c.shape
    return c.double().view(m // rows, rows, n).sum(dim=1)


def bf16_line(k):
    """The project's bf16 pass line: |c - ref| / max(1, |ref|) below this."""
    return 1e-4 * max(1.0, k / 512)


def shape_k(dtype, ktiles):
    return ktiles * K_TILE[dtype]


def row_bytes(dtype, k):
    b = k * ELEM_BYTES[dtype]
    assert b == math.floor(b)
    return int(b)


# --- the referee's operands and its fp64 model ----------------------------------------------------------------------

# E4M3 codes of the integers 0..8 (1.0 = 0x38: exponent field 7; 3 = 1.5 * 2, 5 = 1.25 * 4, 7 = 1.75 * 4)
FP8_INT_CODES = (0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50)
# the 254 finite E4M3 codes: every byte but the two NaNs
FP8_FINITE = [c for c in range(256) if c & 0x7F != 0x7F]


def integer_operand(dtype, rows, k, gen):
    """``rows x k`` independent integers in -8..8, exact in bf16 and in E4M3: ``(operand in dtype, values as
    float64)``.  The fp8 bytes come from the code table above, not from a cast."""
    v = torch.randint(-8, 9, (rows, k), generator=gen, dtype=torch.int64)
    if dtype == "fp8":
        bits = torch.tensor(FP8_INT_CODES, dtype=torch.int64)[v.abs()] | ((v < 0).to(torch.int64) << 7)
        return bits.to(torch.uint8).view(torch.float8_e4m3fn), v.to(torch.float64)
    return v.to(torch.bfloat16), v.to(torch.float64)


def wide_bf16_operand(rows, k, gen):
    """Normal deviates scaled by 2^-20 .. 2^20 element by element, so a row spans about 40 binades: ``(bf16,
    its values as float64)``."""
    x = torch.randn(rows, k, generator=gen, dtype=torch.float64)
    e = torch.randint(-20, 21, (rows, k), generator=gen, dtype=torch.int64)
    t = torch.ldexp(x, e).to(torch.float32).to(torch.bfloat16)
    return t, t.to(torch.float64)


def wide_fp8_operand(rows, k, gen):
    """Every finite E4M3 code, cycled along each row in a random order of the row's own: ``(float8_e4m3fn, values as
    float64 decoded from the bits)``."""
    order = torch.rand(rows, len(FP8_FINITE), generator=gen).argsort(dim=1)
    codes = torch.tensor(FP8_FINITE, dtype=torch.int64)[order][:, torch.arange(k) % len(FP8_FINITE)]
    bits = codes.to(torch.uint8)
    return bits.view(torch.float8_e4m3fn), decode_e4m3(bits)


def referee_model(a64, bt64, tile_rows):
    """What the diagnostics' referee must compute for ``C = a64 @ bt64.T``, in float64: the product ``c``, each
    output's ``mag`` = sum |a b|, and for every ``tile_rows``-high block of rows tb and column j the checksum
    reference ``ck_ref`` = sum_k (sum_i a[i][k]) bt[j][k] and its magnitude ``ck_mag`` with absolute values."""
    return {"c": a64 @ bt64.T, "mag": a64.abs() @ bt64.abs().T,
            "ck_ref": block_sums(a64, tile_rows) @ bt64.T,
            "ck_mag": block_sums(a64.abs(), tile_rows) @ bt64.abs().T}


def gamma(n, u):
    """Higham's gamma_n(u) = n u / (1 - n u): the relative error bound of n roundings of unit roundoff u."""
    assert n * u < 1
    return n * u / (1 - n * u)
