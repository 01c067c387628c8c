"""The helpers of the GEMM kernel tests (gemm_cases.py), proven on the CPU: the operands that the GPU tests call
exact are exact for the reference alone -- fp32 sums in several orders equal the fp64 product bit for bit -- they
carry every value of their lists, and the guard-banded buffers have the layout the GPU tests rely on."""
import pytest

torch = pytest.importorskip("torch")

import gemm_cases as G  # noqa: E402

M, N, K = 256, 256, 640


def _sum_fp32(a32, b32, order):
    acc = torch.zeros(a32.shape[0], b32.shape[0], dtype=torch.float32)
    for kk in order:
        acc += a32[:, kk, None] * b32[None, :, kk]
    return acc


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_exact_operands_are_exact_in_fp32_in_any_order(dtype, side):
    gen = torch.Generator().manual_seed(1234 + (side == "B"))
    a, bt, a64, bt64 = G.exact_operands(dtype, M, N, K, side, gen)
    assert a.shape == (M, K) and bt.shape == (N, K)
    assert a.dtype == bt.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float8_e4m3fn)
    # the float64 values decoded from the bit patterns are what a cast of the operands gives
    a32, b32 = a.float(), bt.float()
    assert torch.equal(a32.double(), a64) and torch.equal(b32.double(), bt64)
    ref64 = a64 @ bt64.t()
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64)  # the fp64 product fits fp32: nothing is rounded away
    assert torch.isfinite(ref32).all()
    nz = ref32[ref32 != 0].abs()
    assert nz.numel() > M * N // 2 and nz.min().item() >= 2.0 ** -126  # no fp32 subnormal output
    kt = G.K_TILE[dtype]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(99)).tolist()
    sums = {"forward": _sum_fp32(a32, b32, range(K)),
            "reversed": _sum_fp32(a32, b32, range(K - 1, -1, -1)),
            "permuted": _sum_fp32(a32, b32, perm),
            "matmul": a32 @ b32.t()}
    chunked = torch.zeros(M, N, dtype=torch.float32)
    for k0 in range(0, K, kt):  # each K-tile summed from zero, then added
        chunked += _sum_fp32(a32, b32, range(k0, k0 + kt))
    sums["per K-tile"] = chunked
    for name, s in sums.items():
        assert torch.equal(s, ref32), name
    # bf16 C is the rounded fp32 C; the rows (side A) / columns (side B) identify themselves: a row of C divided
    # by its value is an integer matrix with |entry| <= K
    mag64 = (a64 if side == "A" else bt64).abs()[:, 0]
    ints = (ref64 / mag64.clamp_min(1e-300)[:, None]) if side == "A" else (ref64 / mag64.clamp_min(1e-300)[None, :])
    assert torch.equal(ints, ints.round()) and ints.abs().max().item() <= K


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_every_listed_value_is_on_the_magnitude_side(dtype, side):
    gen = torch.Generator().manual_seed(7)
    a, bt, a64, bt64 = G.exact_operands(dtype, M, N, K, side, gen)
    mag, other = (a, bt) if side == "A" else (bt, a)
    want = G.expected_magnitude_bits(dtype)
    assert len(want) == (127 if dtype == "fp8" else 128 * G.BF16_EXP_STEPS)
    assert G.magnitude_bits(dtype, mag) == want
    # one magnitude per row, both signs in every row
    bits = mag.view(torch.uint8 if dtype == "fp8" else torch.int16).to(torch.int64)
    mask, sign = (0x7F, 0x80) if dtype == "fp8" else (0x7FFF, 0x8000)
    assert ((bits & mask) == (bits & mask)[:, :1]).all()
    assert ((bits & sign) != 0).any(dim=1).all() and ((bits & sign) == 0).any(dim=1).all()
    assert set(other.float().unique().tolist()) == {-1.0, 0.0, 1.0}
    if dtype == "fp8":
        v = G.decode_e4m3(torch.tensor(G.FP8_CODES))
        assert v[0].item() == 0.0 and v[1].item() == 2.0 ** -9 and v[7].item() == 7 * 2.0 ** -9
        assert v[8].item() == 2.0 ** -6 and v[-1].item() == 448.0 and (v[1:] > v[:-1]).all()
        assert torch.isnan(G.decode_e4m3(torch.tensor([0x7F, 0xFF]))).all()
    else:
        vals = G.bf16_values()
        assert {s for s, _ in vals} == set(range(128))
        assert min(e for _, e in vals) == -120 and max(e for _, e in vals) == 117
        assert len({e for _, e in vals}) >= 200  # the exponents step over the whole range, not two values
        assert (2 - 2.0 ** -7) * 2.0 ** 117 * 640 < 2.0 ** 128  # v * K stays finite in fp32


@pytest.mark.parametrize("fill,dtype,rows,cols", [("bf16", torch.bfloat16, 256, 64), ("fp8", torch.float8_e4m3fn, 512, 384),
                                                  ("fp4", torch.uint8, 256, 128), ("out", torch.float32, 384, 256),
                                                  ("out", torch.bfloat16, 256, 512), ("out", torch.float64, 2, 256)])
def test_banded_layout(fill, dtype, rows, cols):
    item = torch.empty(0, dtype=dtype).element_size()
    b = G.banded(rows, cols * item, fill)
    v = b.view(dtype)
    assert v.shape == (rows, cols) and v.is_contiguous()
    band = 256 * cols * item
    assert b.before.numel() == b.after.numel() == band and band % 256 == 0
    assert b.raw.numel() == 2 * band + rows * cols * item
    assert v.data_ptr() == b.data_ptr() == b.raw.data_ptr() + band
    assert b.after.data_ptr() == b.raw.data_ptr() + band + rows * cols * item
    assert b.intact()
    # input bands read as NaN where the format has one; output bands are finite in every output format
    if fill == "bf16":
        assert torch.isnan(b.before.view(torch.bfloat16)).all() and torch.isnan(b.after.view(torch.bfloat16)).all()
        assert (b.before.view(torch.int16) == 0x7FC0).all()
    elif fill == "fp8":
        assert torch.isnan(b.before.view(torch.float8_e4m3fn).float()).all() and (b.after == 0x7F).all()
    elif fill == "fp4":
        assert (b.before == 0x77).all() and (b.after == 0x77).all()
    else:
        assert torch.isfinite(b.before.view(dtype).double()).all()
    # a write into the payload leaves the bands alone; one byte before or after it breaks them
    v.view(torch.uint8).fill_(0xFF)
    assert b.intact()
    b.raw[band - 1] ^= 1
    assert not b.intact()
    b.raw[band - 1] ^= 1
    assert b.intact()
    b.raw[band + rows * cols * item] ^= 0x80
    assert not b.intact()


def test_knob_matrix_is_the_full_product():
    for dtype, others in (("bf16", {"v1", "v2", "v4", "v4t"}), ("fp8", {"v4", "v4t"}), ("fp4", set())):
        cfgs = G.knob_matrix(dtype)
        v3 = [c for c in cfgs if c["variant"] == "v3"]
        forms = 2 if dtype == "fp8" else 1
        assert len(v3) == 8 * forms
        assert len({(c["epilogue"], c["buffer_loads"], c["schedule"], c["fp8_unscaled"]) for c in v3}) == 8 * forms
        assert {c["variant"] for c in cfgs} - {"v3"} == others
        assert all(set(c) == {"variant", "epilogue", "buffer_loads", "schedule", "fp8_unscaled", "tail"} for c in cfgs)


# --- the referee's operands and model (test_gpu_gemm_referee.py) ----------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_integer_operands_are_the_integers_they_claim(dtype):
    gen = torch.Generator().manual_seed(5)
    t, v = G.integer_operand(dtype, 64, 192, gen)
    assert set(v.unique().tolist()) == {float(i) for i in range(-8, 9)}
    if dtype == "fp8":
        assert torch.equal(G.decode_e4m3(t.view(torch.uint8)), v)  # the code table, by the format
    assert torch.equal(t.to(torch.float64), v)  # ... and by the cast
    # a product of K = 1024 such operands is exact in fp32 and its checksums in fp64
    assert 64 * 1024 < 2 ** 24 and 256 * 8 * 8 * 1024 < 2 ** 53


def test_wide_fp8_rows_hold_every_finite_code_and_their_products_stay_exact_in_fp64():
    gen = torch.Generator().manual_seed(6)
    t, v = G.wide_fp8_operand(16, 384, gen)
    bits = t.view(torch.uint8).to(torch.int64)
    assert len(G.FP8_FINITE) == 254 and bool(torch.isfinite(v).all())
    assert torch.equal(t.to(torch.float64), v)
    for r in range(16):
        assert sorted(bits[r, :254].tolist()) == G.FP8_FINITE and torch.equal(bits[r, 254:], bits[r, :130])
    assert not torch.equal(bits[0], bits[1])
    t128, _ = G.wide_fp8_operand(4, 128, gen)
    assert all(len(set(t128.view(torch.uint8)[r].tolist())) == 128 for r in range(4))
    # values are multiples of 2^-9 up to 448, so every product and partial sum is a multiple of 2^-18.  A row holds
    # each code at most ceil(K / 254) times, so by the rearrangement inequality sum_k |a_k b_k| of two such rows is
    # at most ceil(K / 254) * sum_c v_c^2; over 256 rows and K = 1024 that stays below 2^53 units of 2^-18: exact.
    nz = v[v != 0].abs()
    assert float(nz.min()) == 2.0 ** -9 and float(nz.max()) == 448.0
    squares = float((G.decode_e4m3(torch.tensor(G.FP8_FINITE)) ** 2).sum())
    assert 256 * -(-1024 // 254) * squares / 2.0 ** -18 < 2.0 ** 53


def test_wide_bf16_rows_span_about_forty_binades():
    gen = torch.Generator().manual_seed(7)
    t, v = G.wide_bf16_operand(8, 1024, gen)
    assert t.dtype == torch.bfloat16 and torch.equal(t.to(torch.float64), v) and bool(torch.isfinite(v).all())
    span = torch.log2(v.abs().clamp_min(1e-300))
    for r in range(8):
        assert 36 <= float(span[r].max() - span[r][v[r] != 0].min()) <= 60


def test_referee_model_on_a_problem_small_enough_to_write_out():
    a = torch.tensor([[1.0, -2.0], [3.0, 4.0], [-5.0, 6.0], [7.0, 8.0]], dtype=torch.float64)
    bt = torch.tensor([[1.0, 1.0], [2.0, -1.0], [0.0, -3.0]], dtype=torch.float64)
    m = G.referee_model(a, bt, 2)
    assert m["c"].tolist() == [[-1.0, 4.0, 6.0], [7.0, 2.0, -12.0], [1.0, -16.0, -18.0], [15.0, 6.0, -24.0]]
    assert m["mag"].tolist() == [[3.0, 4.0, 6.0], [7.0, 10.0, 12.0], [11.0, 16.0, 18.0], [15.0, 22.0, 24.0]]
    assert m["ck_ref"].tolist() == [[6.0, 6.0, -6.0], [16.0, -10.0, -42.0]]  # the column sums of c per 2-row block
    assert m["ck_mag"].tolist() == [[10.0, 14.0, 18.0], [26.0, 38.0, 42.0]]
    assert torch.equal(m["ck_ref"], G.block_sums(m["c"], 2))
    assert G.gamma(1024, 2.0 ** -24) == 1024 * 2.0 ** -24 / (1 - 1024 * 2.0 ** -24)
