"""Fault injection into every active diagnostic's verifier (MI355X only, ``pytest -m gpu``).

A verifier that never fires looks the same as a healthy GPU, so each one is shown a known fault -- one lane, one
word, one element, one output -- and must report its exact count and place; the same call without the fault must
be clean.  Sizes are the smallest that still reach every path (tails, partial blocks, the second pass); no test
depends on a rate.
"""
import functools
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MIB = 1 << 20


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _xcd_slots(x):
    """The CU slots of XCD ``x`` (``wave_slot()``: xcd << 7 | se << 5 | sh << 4 | cu)."""
    return range(128 * x, 128 * (x + 1))


def _present_xcds(cu_map):
    return [x for x in range(8) if any(cu_map[3 * s] for s in _xcd_slots(x))]


# ------------------------------------------------------------------------------------------------ mfma_burn
@pytest.mark.parametrize("kind", ["bf16", "fp8", "mxfp8", "mxfp4"])
def test_mfma_burn_counts_and_locates_one_wrong_lane(dev, kind):
    """One lane of one wave made wrong by 1.0 in the warm-up launch: the comparison, the ballot count and the
    per-CU map row each see exactly that lane, and the rate is still reported."""
    from k8s_gpu_node_checker_amd.ops import diag
    ok = diag.mfma_burn(0, kinds=(kind,), iters=64, reps=1)
    assert ok["kinds"][kind]["errors"] == 0 and ok["numerics"] == "" and "bad_cus" not in ok["map"], ok
    r = diag.mfma_burn(0, kinds=(kind,), iters=64, reps=1, inject_block=5)
    assert r["kinds"][kind]["errors"] == 1 and not r["pass"] and "1 wrong results" in r["numerics"], r
    flat = r["cu_maps"][kind]
    wrong = {s: flat[3 * s + 1] for s in range(len(flat) // 3) if flat[3 * s + 1]}
    assert len(wrong) == 1 and list(wrong.values()) == [1], wrong
    slot = next(iter(wrong))
    assert flat[3 * slot] > 0, "the wrong lane is on a slot that ran no wave"
    assert r["map"]["bad_cus"] == [f"{diag.slot_name(slot)} ({kind} 1)"], r["map"]
    # every wave of both launches (2 workgroups of 4 waves per CU each) is in the map, injected or not
    assert sum(flat[0::3]) == 2 * 2 * 4 * diag.device_info(0)["cus"], sum(flat[0::3])
    assert r["kinds"][kind]["tflops"] > 0 and r["rates"][kind] > 0, r
    with pytest.raises(RuntimeError, match="outside the grid"):
        diag.mfma_burn(0, kinds=(kind,), iters=64, reps=1, inject_block=1 << 20)


# ------------------------------------------------------------------------------------ l2_bandwidth / hbm_xcd
@functools.lru_cache(maxsize=None)
def _l2_clean(slice_kib):
    from k8s_gpu_node_checker_amd.ops import diag
    return diag.l2_bandwidth(0, slice_kib=slice_kib, passes=2, blocks_per_cu=1)


# 64 KiB = 4096 16-byte vectors = 2 x (8 x 256): only the 8-deep unrolled loop runs; 65 KiB = 4160 vectors leaves a
# tail of 64 for the plain loop, and the slice's last word lies in it
@pytest.mark.parametrize("slice_kib,word", [(64, 0), (64, 64 * 256 - 1), (65, 65 * 256 - 1)])
def test_l2_bandwidth_counts_a_flipped_word_on_its_xcd(dev, slice_kib, word):
    """One bit of one word of one XCD's slice flipped before the first read.  Every workgroup of that XCD reads
    the whole slice ``passes`` times, so the wrong words are passes x its workgroups, all on CUs of that XCD --
    which also shows that a workgroup reads the slice of the XCC_ID it reports."""
    from k8s_gpu_node_checker_amd.ops import diag
    passes = 2
    assert (slice_kib * 64) % (8 * 256) == (0 if slice_kib == 64 else 64)
    ok = _l2_clean(slice_kib)
    assert ok["errors"] == 0 and ok["numerics"] == "" and "bad_cus" not in ok["map"], ok
    xcds = sorted(int(x) for x in ok["map"]["xcds"])
    x = xcds[len(xcds) // 2]
    r = diag.l2_bandwidth(0, slice_kib=slice_kib, passes=passes, blocks_per_cu=1, inject_xcd=x, inject_word=word)
    cu = r["cu_map"]
    waves = sum(cu[3 * s] for s in _xcd_slots(x))
    assert waves > 0 and waves % 4 == 0, waves
    assert r["errors"] == passes * (waves // 4), (r["errors"], waves)
    assert not r["pass"] and f"{r['errors']} wrong words" in r["numerics"], r
    # per slot: the wave that reads the word is one of its workgroup's four, on the same CU
    for s in range(len(cu) // 3):
        want = passes * (cu[3 * s] // 4) if s in _xcd_slots(x) else 0
        assert cu[3 * s + 1] == want, (s, cu[3 * s], cu[3 * s + 1])
    assert r["map"]["bad_cus"] and all(b.startswith(f"xcd{x}/") for b in r["map"]["bad_cus"]), r["map"]
    with pytest.raises(RuntimeError, match="inside the slice"):
        diag.l2_bandwidth(0, slice_kib=slice_kib, passes=1, blocks_per_cu=1, inject_xcd=x,
                          inject_word=slice_kib * 256)


@functools.lru_cache(maxsize=None)
def _hbm_xcd_clean():
    from k8s_gpu_node_checker_amd.ops import diag
    return diag.hbm_xcd(0, slice_mib=1, passes=1)


@pytest.mark.parametrize("word", [0, MIB // 4 - 1])
def test_hbm_xcd_counts_a_flipped_word_on_its_xcd(dev, word):
    """One bit of one word of one XCD's slice flipped.  The XCD's workgroups share the slice chunk by chunk, so
    every run that streams it reads the word ``passes`` times.  diag_hbm_xcd's launches: a warm-up of all XCDs
    (errors and map zeroed after it), the timed run of all XCDs (the map is copied here: ``passes`` wrong
    words), one untimed lone run of the first present XCD, then a lone run of every present XCD; the error
    count is read after those.  For an XCD that is not the first present one that is passes x (1 + 1)."""
    from k8s_gpu_node_checker_amd.ops import diag
    passes = 1
    ok = _hbm_xcd_clean()
    assert ok["errors"] == 0 and ok["numerics"] == "" and "bad_cus" not in ok["map"], ok
    xcds = sorted(int(x) for x in ok["map"]["xcds"])
    x = xcds[-1]
    runs = 2 + (1 if x == xcds[0] else 0)  # (a device of a single XCD: the untimed lone run is its own as well)
    r = diag.hbm_xcd(0, slice_mib=1, passes=passes, inject_xcd=x, inject_word=word)
    cu = r["cu_map"]
    assert _present_xcds(cu) == xcds
    assert sum(cu[3 * s + 1] for s in _xcd_slots(x)) == passes, [cu[3 * s + 1] for s in _xcd_slots(x)]
    assert sum(cu[1::3]) == passes, "wrong words attributed outside the injected XCD"
    assert r["errors"] == passes * runs, r
    assert not r["pass"] and "wrong words" in r["numerics"], r
    assert len(r["map"]["bad_cus"]) == 1 and r["map"]["bad_cus"][0].startswith(f"xcd{x}/"), r["map"]
    assert sorted(int(k) for k in r["alone_tbs"]) == xcds, r


# ---------------------------------------------------------------------------------------------- hbm streams
# 32 MiB + 77 elements: the last workgroup of every stream kernel is partial; + 5 bytes: not a whole element
HBM_BYTES = 32 * MIB + 16 * 77


@pytest.mark.parametrize("extra", [0, 5])
def test_hbm_streams_move_every_byte(dev, extra):
    """The copy leaves the source's fill in every element of the destination and the write its value, up to the
    last element of a buffer that is no multiple of the 256-element workgroup (or of 16 bytes)."""
    from k8s_gpu_node_checker_amd.ops import diag
    nbytes = HBM_BYTES + extra
    assert (nbytes // 16) % 256 == 77 and nbytes % 16 == extra
    r = diag.hbm(0, gib=nbytes / (1 << 30), iters=1)
    assert int(r["gib"] * (1 << 30)) == nbytes
    assert r["errors"] == 0 and r["numerics"] == "", r
    assert r["copy_tbs"] > 0 and r["read_tbs"] > 0 and r["write_tbs"] > 0, r


@pytest.mark.parametrize("phase", ["copy", "write"])
@pytest.mark.parametrize("last", [False, True])
def test_hbm_streams_count_one_wrong_element(dev, phase, last):
    from k8s_gpu_node_checker_amd.ops import diag
    n = HBM_BYTES // 16
    r = diag.hbm(0, gib=HBM_BYTES / (1 << 30), iters=1, inject_word=n - 1 if last else 0, inject_phase=phase)
    assert r["errors"] == 1 and not r["pass"] and "1 wrong 16-byte elements" in r["numerics"], r
    with pytest.raises(RuntimeError, match="outside the buffer"):
        diag.hbm(0, gib=HBM_BYTES / (1 << 30), iters=1, inject_word=n, inject_phase=phase)


# -------------------------------------------------------------------------------------------------- memtest
MT_WORDS = 16 * MIB // 16          # a whole number of 256-word workgroups
MT_ODD_WORDS = MT_WORDS + 100      # the last workgroup checks 100 words


@functools.lru_cache(maxsize=None)
def _memtest_clean(words, passes):
    from k8s_gpu_node_checker_amd.ops import diag
    return diag.memtest(0, gib=words * 16 / (1 << 30), passes=passes)


@pytest.mark.parametrize("words,passes,word,inject_pass,invert", [
    (MT_WORDS, 1, 0, 0, False),
    (MT_WORDS, 1, MT_WORDS - 1, 0, False),
    (MT_ODD_WORDS, 1, MT_ODD_WORDS - 40, 0, False),   # in the final, partial workgroup
    (MT_ODD_WORDS, 1, MT_ODD_WORDS - 1, 0, True),
    (MT_WORDS, 1, 123457, 0, True),                   # the inverted half of pass 0
    (MT_WORDS, 2, 54321, 1, False),                   # the plain half of pass 1
    (MT_WORDS, 2, 777, 1, True)])
def test_memtest_counts_and_locates_every_write(dev, words, passes, word, inject_pass, invert):
    from k8s_gpu_node_checker_amd.ops import diag
    ok = _memtest_clean(words, passes)
    assert ok["errors"] == 0 and ok["pass"], ok
    r = diag.memtest(0, gib=words * 16 / (1 << 30), passes=passes, inject_word=word, inject_pass=inject_pass,
                     inject_invert=invert)
    assert not r["pass"] and r["errors"] == 1 and r["first_bad_byte"] == word * 16, r


def test_memtest_two_words_counts_both_and_keeps_the_lower(dev):
    from k8s_gpu_node_checker_amd.ops import diag
    r = diag.memtest(0, gib=MT_ODD_WORDS * 16 / (1 << 30), inject_word=900001, inject_word2=4242)
    assert not r["pass"] and r["errors"] == 2 and r["first_bad_byte"] == 4242 * 16, r
    with pytest.raises(RuntimeError, match="outside the passes"):
        diag.memtest(0, gib=MT_WORDS * 16 / (1 << 30), passes=1, inject_word=1, inject_pass=1)
    with pytest.raises(RuntimeError, match="outside the buffer"):
        diag.memtest(0, gib=MT_WORDS * 16 / (1 << 30), inject_word=1, inject_word2=MT_WORDS)


# ------------------------------------------------------------------------------------------- GEMM checksums
def _operand_mean_square(kind):
    """E[x^2] of the diagnostics' operand fills: bf16 uniform in [-1, 1); fp8 an E4M3 byte with its exponent field
    uniform in 0..8 and its mantissa in 0..7 (fill_bf16_kernel / fill_fp8_kernel in csrc/diag/diag.hip)."""
    if kind == "gemm":
        return 1.0 / 3.0
    vals = [m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7) for e in range(9) for m in range(8)]
    return sum(v * v for v in vals) / len(vals)


@pytest.mark.parametrize("kind,n,tile,group_m", [("gemm", 4096, 256, 4), ("gemm", 2048, 128, 8),
                                                  ("gemm_fp8", 4096, 256, 4), ("gemm_fp8", 2048, 256, 4)])
def test_gemm_checksums_catch_an_error_of_twice_their_floor(dev, kind, n, tile, group_m):
    """The smallest wrong output the checksums are sure to catch.  A column is flagged when its sum is off by
    more than tol x mag_col; ``checksum_floor`` = tol x max mag >= that threshold in every column, and the healthy
    residual is below tol / 10 x mag_col (asserted).  So one output off by 2 x floor moves its column's sum by at
    least 2 x floor - tol / 10 x mag_col > tol x mag_col: its tile, and only its tile, must fail."""
    from k8s_gpu_node_checker_amd.ops import diag
    from test_gpu import _tile_xcd
    fn = getattr(diag, kind)
    tol = diag.GEMM_CK_TOL if kind == "gemm" else diag.GEMM_FP8_CK_TOL
    ok = fn(0, size=n, warmup=1, iters=2)
    assert ok["checksum_bad_tiles"] == 0 and ok["checksum_err"] < tol / 10 and ok["numerics"] == "", ok
    floor = ok["checksum_floor"]
    assert floor > 0 and math.isfinite(floor), ok
    # the outputs are sums of n products of independent zero-mean operands: RMS = sqrt(n) x E[x^2]
    rms = math.sqrt(n) * _operand_mean_square(kind)
    print(f"{kind} {n}^3 ({ok['output']}): checksum_floor {floor:.4g} = {floor / rms:.3g} of the output RMS {rms:.4g}")
    row, col = n // 2 + 297, n // 3 + 501
    r = fn(0, size=n, warmup=1, iters=2, inject_elem=row * n + col, inject_delta=2 * floor)
    assert r["checksum_floor"] == floor, (r["checksum_floor"], floor)
    assert not r["pass"] and r["checksum_bad_tiles"] == 1, r
    assert r["checksum_first_bad_tile"] == [row // tile, col // tile], r
    xcd = _tile_xcd(row // tile, col // tile, n // tile, n // tile, group_m)
    assert r["checksum_bad_xcds"] == {str(xcd): 1}, r
    assert "fail their checksums" in r["detail"], r


@pytest.mark.parametrize("kind,limit_key,limit", [("gemm", "max_rel_err", "GEMM_MAX_REL_ERR"),
                                                  ("gemm_fp8", "max_err_over_mag", "GEMM_FP8_MAX_ERR")])
def test_gemm_fp32_output_path_checks_and_locates_an_overwritten_output(dev, kind, limit_key, limit):
    """The v3 kernel with direct stores writes fp32 C and no column sums of its own: the runner then checks the
    sampled outputs as they are and forms the tile checksums from C (256^2 tiles, groups of 4).  Clean, nothing
    is flagged; one output overwritten away from the origin fails exactly its tile, charged to the XCD that
    computed it.  The thread's knobs are back afterwards."""
    from k8s_gpu_node_checker_amd.ops import diag
    from test_gpu import _tile_xcd
    fn, n, tile = getattr(diag, kind), 2048, 256
    before = diag.get_gemm_config()
    with diag.gemm_config(variant="v3", epilogue=False):
        ok = fn(0, size=n, warmup=1, iters=2, samples=512)
        row, col = n // 2 + 297, n // 3 + 501
        r = fn(0, size=n, warmup=1, iters=2, samples=512, inject_elem=row * n + col)
    assert diag.get_gemm_config() == before, (diag.get_gemm_config(), before)
    print(f"{kind} {n}^3 v3 direct stores: {ok}")
    assert ok["output"] == "fp32" and r["output"] == "fp32", (ok, r)
    assert ok[limit_key] <= getattr(diag, limit) and ok["numerics"] == "", ok
    assert ok["checksum_bad_tiles"] == 0, ok
    assert r["checksum_bad_tiles"] == 1 and not r["pass"], r
    assert r["checksum_first_bad_tile"] == [row // tile, col // tile], r
    xcd = _tile_xcd(row // tile, col // tile, n // tile, n // tile, 4)
    assert r["checksum_bad_xcds"] == {str(xcd): 1}, r
