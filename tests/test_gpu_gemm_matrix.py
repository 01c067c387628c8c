"""MI355X-only: every GEMM kernel the public knobs reach, at the tile counts and K-tile counts where the kernels
take different paths, with guard bands round every operand and output and with operands whose product is exact.

Each launch is checked four ways: no output left unwritten (C is pre-filled with NaN), nothing written outside the
output (the bands on both sides of C, bf16 C and the column sums keep their bit pattern), nothing *used* that was read
outside an operand (the operands' bands are NaN, so C would be NaN), and the values themselves: within the
project's error line of an fp64 reference and bit-identical across the knobs, or exactly equal to it where the
operands make the product exact (gemm_cases.exact_operands, proven on the CPU by test_gemm_exact_inputs_cpu.py).

Shapes are M x N x K-tiles; one K-tile is 64 bf16, 128 fp8 or 256 fp4 columns.  1-5 K-tiles are the prologue and
tail paths of the two-stage, four-phase pipeline; 5 x 3 tiles is one full group_m = 4 group of tile rows plus a
partial one with nwg % 8 == 7, 3 x 5 fewer tile rows than a group.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gemm_cases as G  # noqa: E402
from test_gpu import _fp4_operand  # noqa: E402

SHAPES = [(256, 256, 1), (256, 512, 2), (512, 256, 3), (768, 1280, 4), (1280, 768, 5)]
# v1 is the only kernel that takes 128-multiples
V1_SHAPES = [(128, 384, 1), (128, 384, 3)]
PRODUCTION = {"variant": "auto", "epilogue": True, "buffer_loads": False, "schedule": 1, "fp8_unscaled": True,
              "tail": True}
V3_DEFAULT = dict(PRODUCTION, variant="v3")
FP4_MAX_ERR = 4e-5  # the fp4 line of test_gpu.test_mxfp4_gemm_matches_fp64_reference

_worst = {}  # dtype -> worst error seen so far, as a fraction of the dtype's pass line


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Case:
    """Operands in guard-banded buffers, and guard-banded outputs that are reset to NaN before each launch."""

    def __init__(self, dtype, a, bt, m, n, k, dev, ck=False):
        from k8s_gpu_node_checker_amd.ops import diag
        self.diag, self.dtype, self.m, self.n, self.k = diag, dtype, m, n, k
        rb = G.row_bytes(dtype, k)
        self.A, self.Bt = G.banded(m, rb, dtype, dev), G.banded(n, rb, dtype, dev)
        self.A.put(a.to(dev))
        self.Bt.put(bt.to(dev))
        self.C32 = G.banded(m, 4 * n, "out", dev)
        self.buffers = {"A": self.A, "Bt": self.Bt, "C fp32": self.C32}
        if ck:
            self.C16 = G.banded(m, 2 * n, "out", dev)
            self.CS = G.banded(m // 128, 8 * n, "out", dev)
            self.buffers.update({"C bf16": self.C16, "column sums": self.CS})

    def _bands(self, what):
        for name, b in self.buffers.items():
            assert b.intact(), f"{what}: the guard bands of {name} changed"

    def f32(self, cfg):
        """One fp32-output launch under ``cfg``: C (a copy), bands checked, no NaN."""
        launch = {"bf16": self.diag.gemm_launch, "fp8": self.diag.gemm_fp8_launch,
                  "fp4": self.diag.gemm_fp4_launch}[self.dtype]
        c = self.C32.view(torch.float32)
        c.fill_(float("nan"))
        with self.diag.gemm_config(**cfg):
            launch(self.A.data_ptr(), self.Bt.data_ptr(), c.data_ptr(), self.m, self.n, self.k, _stream())
            torch.cuda.synchronize()
        self._bands(G.label(cfg))
        assert not torch.isnan(c).any(), G.label(cfg)
        return c.clone()

    def ck(self, cfg):
        """One bf16-output launch with fused column sums under ``cfg``: (bf16 C, sums), bands checked, no NaN."""
        c16, cs = self.C16.view(torch.bfloat16), self.CS.view(torch.float64)
        c16.fill_(float("nan"))
        cs.fill_(float("nan"))
        with self.diag.gemm_config(**cfg):
            self.diag.gemm_launch_ck(self.dtype, self.A.data_ptr(), self.Bt.data_ptr(), c16.data_ptr(), cs.data_ptr(),
                                     self.m, self.n, self.k, _stream())
            torch.cuda.synchronize()
        self._bands("ck " + G.label(cfg))
        assert not torch.isnan(c16).any() and not torch.isnan(cs).any(), G.label(cfg)
        return c16.clone(), cs.clone()


def _random_operands(dtype, m, n, k, dev, seed):
    """(a, bt, a64, bt64): randn operands (fp4: random codes) and their values in fp64."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if dtype == "fp4":
        a, av = _fp4_operand(m, k, g, dev)
        bt, bv = _fp4_operand(n, k, g, dev)
        return a, bt, av.double(), bv.double()
    t = torch.bfloat16 if dtype == "bf16" else torch.float8_e4m3fn
    a = torch.randn(m, k, device=dev, generator=g).to(t)
    bt = torch.randn(n, k, device=dev, generator=g).to(t)
    return a, bt, a.double(), bt.double()


def _error_ratio(dtype, c, ref, mag, k):
    """The worst error of ``c`` as a fraction of the dtype's pass line (< 1 passes), and the error itself."""
    from k8s_gpu_node_checker_amd.ops import diag
    if dtype == "bf16":
        err = ((c.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
        return err / G.bf16_line(k), err
    err = ((c.double() - ref).abs() / mag.clamp_min(1e-30)).max().item()
    return err / (diag.GEMM_FP8_MAX_ERR if dtype == "fp8" else FP4_MAX_ERR), err


@pytest.mark.parametrize("dtype,m,n,ktiles", [(d, *s) for d in ("bf16", "fp8", "fp4") for s in SHAPES] +
                         [("bf16", *s) for s in V1_SHAPES])
def test_every_v3_knob_combination(dev, dtype, m, n, ktiles):
    """Every combination of epilogue x buffer_loads x schedule (x the fp8 MFMA form) of the v3 kernels, and v1, v2, v4
    and v4t where the dtype has them, on one set of randn operands (fp4: random codes): no NaN, bands intact, within
    the dtype's line of an fp64 reference, and C bit-identical to the default configuration's (bf16: v3 with the
    default knobs, since ``auto`` below 256 tiles is v1; v1 and v2 accumulate in another order and take the fp64 line
    alone).  128 x 384 is v1's own shape: no other kernel takes 128-multiples."""
    from k8s_gpu_node_checker_amd.ops import diag
    assert diag.get_gemm_config() == PRODUCTION
    k = G.shape_k(dtype, ktiles)
    a, bt, a64, bt64 = _random_operands(dtype, m, n, k, dev, m + 3 * n + 7 * k)
    case = _Case(dtype, a, bt, m, n, k, dev)
    ref, mag = a64 @ bt64.t(), a64.abs() @ bt64.abs().t()
    if m % 256:
        configs, base = [c for c in G.knob_matrix("bf16") if c["variant"] == "v1"] + [dict(PRODUCTION)], None
    else:
        configs = G.knob_matrix(dtype)
        base = case.f32(V3_DEFAULT if dtype == "bf16" else PRODUCTION)
    worst = 0.0
    for cfg in configs:
        c = case.f32(cfg)
        ratio, err = _error_ratio(dtype, c, ref, mag, k)
        worst = max(worst, ratio)
        assert ratio < 1.0, (G.label(cfg), err)
        if base is not None and cfg["variant"] not in ("v1", "v2"):
            assert torch.equal(c, base), G.label(cfg)
    assert diag.get_gemm_config() == PRODUCTION
    _worst[dtype] = max(_worst.get(dtype, 0.0), worst)
    print(f"gemm matrix {dtype} {m}x{n}x{k}: {len(configs)} configs, worst error {worst:.4f} of the line; "
          f"worst so far for {dtype}: {_worst[dtype]:.4f}")


@pytest.mark.parametrize("m,n,ktiles", SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_ck_outputs_under_every_knob(dev, dtype, m, n, ktiles):
    """The bf16-output kernel with fused column sums under v3 (both restaging orders; fp8: both MFMA forms), v4 and
    v4t: bf16 C is the same configuration's fp32 C rounded, bit for bit, and the sums are the fp64 sums of that fp32
    C over every 128-row block; the bands round bf16 C and the sums stay intact."""
    k = G.shape_k(dtype, ktiles)
    a, bt, _, _ = _random_operands(dtype, m, n, k, dev, m + 7 * n + 13 * k)
    case = _Case(dtype, a, bt, m, n, k, dev, ck=True)
    for cfg in G.ck_matrix(dtype):
        c32 = case.f32(cfg)
        c16, cs = case.ck(cfg)
        assert torch.equal(c16, c32.to(torch.bfloat16)), G.label(cfg)
        want, mag = G.block_sums(c32), G.block_sums(c32.abs())
        assert ((cs - want).abs() / mag.clamp_min(1e-300)).max().item() < 1e-12, G.label(cfg)


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_exact_operands_every_kernel(dev, dtype, side):
    """Operands whose product is exact in fp32 in any order -- one side +-v per row, v running over every E4M3 code
    from the subnormals to 448 (bf16: every significand, 2^-120 to 2^117), the other side from {-1, 0, +1} -- through
    every kernel of the dtype: fp32 C equals the fp64 product, bf16 C its rounding, and the fp8 column sums the fp64
    block sums, exactly (bf16 sums: to 1e-12 of sum|c|, the magnitudes span more than fp64 holds).  A flushed
    subnormal, a dropped low bit or a row written in another row's place is off by at least one unit of the row's
    value."""
    for m, n, ktiles in ((256, 512, 2), (1280, 768, 5)):
        k = G.shape_k(dtype, ktiles)
        gen = torch.Generator().manual_seed(1000 * ktiles + (side == "B"))
        a, bt, a64, bt64 = G.exact_operands(dtype, m, n, k, side, gen)
        ref64 = (a64 @ bt64.t()).to(dev)
        ref32 = ref64.float()
        assert torch.equal(ref32.double(), ref64)
        ref16 = ref32.to(torch.bfloat16)
        want, mag = G.block_sums(ref64), G.block_sums(ref64.abs())
        case = _Case(dtype, a, bt, m, n, k, dev, ck=True)
        for cfg in G.knob_matrix(dtype):
            c = case.f32(cfg)
            assert torch.equal(c, ref32), (m, n, k, G.label(cfg), _first_diff(c, ref32))
        for cfg in G.ck_matrix(dtype):
            c16, cs = case.ck(cfg)
            assert torch.equal(c16, ref16), (m, n, k, G.label(cfg), _first_diff(c16.float(), ref16.float()))
            if dtype == "fp8":
                assert torch.equal(cs, want), (m, n, k, G.label(cfg), _first_diff(cs, want))
            else:
                assert ((cs - want).abs() / mag.clamp_min(1e-300)).max().item() < 1e-12, (m, n, k, G.label(cfg))


def _first_diff(got, want):
    """Where two outputs first differ, for the failure message: (count, row, column, got, wanted)."""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return None
    i, j = bad[0].tolist()
    return int(bad.shape[0]), i, j, got[i, j].item(), want[i, j].item()


@pytest.mark.parametrize("m,n", [(256, 65792), (3328, 5120)])
@pytest.mark.parametrize("ktiles", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tail_smallest_cases(dev, dtype, ktiles, m, n):
    """The smallest tails of v4's short last wave: 257 tiles (one tail tile: only XCD 0 has one) and 13 x 20 = 260
    (four), with 1, 2, 3 and 5 K-tiles, bf16 and fp8, under v4 and v4t.  fp32 C, bf16 C and the column sums sit between
    guard bands -- the tail kernel finds its tile with a loop of its own, and a store one tile off would land outside
    C.  As test_v4_tail_wave_is_bit_identical: C and bf16 C equal v3's bit for bit; the sums bit for bit for v4 and to
    1e-14 of sum|c| for v4t, which adds in another order.  That the tail kernel ran at all is not asserted from
    inside: with and without ``tail`` the outputs agree bitwise."""
    k = G.shape_k(dtype, ktiles)
    a, bt, _, _ = _random_operands(dtype, m, n, k, dev, m + 5 * n + 11 * k)
    case = _Case(dtype, a, bt, m, n, k, dev, ck=True)
    outs = {}
    for name, variant, tail in (("v3", "v3", True), ("v4", "v4", True), ("v4-notail", "v4", False),
                                ("v4t", "v4t", True)):
        cfg = dict(PRODUCTION, variant=variant, tail=tail)
        outs[name] = (case.f32(cfg),) + case.ck(cfg)  # (no NaN in C, bf16 C or the sums; bands intact)
    for name in ("v4", "v4-notail", "v4t"):
        assert torch.equal(outs["v3"][0], outs[name][0]), name
        assert torch.equal(outs["v3"][1], outs[name][1]), name
    assert torch.equal(outs["v3"][2], outs["v4"][2]) and torch.equal(outs["v3"][2], outs["v4-notail"][2])
    for i in range(3):
        assert torch.equal(outs["v4"][i], outs["v4-notail"][i]), i
    mag = G.block_sums(outs["v3"][0].abs())
    assert ((outs["v3"][2] - outs["v4t"][2]).abs() / mag.clamp_min(1e-300)).max().item() < 1e-14
