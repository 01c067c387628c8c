"""The cvt diagnostic on an MI355X: one application of every op held against the host's model word for word (shaped
rows, every code of the narrow sources), clean runs on one workgroup, on nine and on the default grid, the float
mode, the self-check hooks, refused calls and the opt-in wiring.  tests/test_cvt_cpu.py holds the model itself
against an exact referee: the expected words here come from the library's own host model (cvt.model, the
cvt_convert() of csrc/cvt/cvt_ref.h), and they are worth what that CPU file shows -- the same header, compiled alone,
equal to a Fraction referee over the shaped domain and over every code of the narrow sources."""
import json
import re
import subprocess
import sys

import pytest

from k8s_gpu_node_checker_amd.ops.cvt import OPS as _OPS

pytestmark = pytest.mark.gpu

ONE = 0x3f800000
SCALES = (ONE, 0x3b800000, 0x43800000)  # 1, 2^-8, 2^8
# one op of each group: classic, bf16, fp8, scalef32
HOOKED = ("f16_f32", "pk_bf16_f32", "pk_fp8_f32_hi", "scalef32_pk_fp4_f32_b2")
SIMD = r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]"
NARROW_SOURCE = re.compile(r"(scalef32_)?(pk_)?(f32|f16|bf16)_(fp8|bf8|fp4)_")
FINITE_PARTNER = 0x38  # 1.0 in E4M3, 0.5 in E5M2: beside it every code is compared, whatever the code is


def _special(op, code):
    """'nan' / 'inf' / None for a source code of op's 8-bit format (fp4 has neither)."""
    if "fp8" in op:
        return "nan" if code & 0x7f == 0x7f else None
    if "bf8" in op:
        return None if code & 0x7c != 0x7c else "inf" if code & 3 == 0 else "nan"
    return None


def _results(op, got, c):
    """The result values (as (bits, width)) that stem from the code under test, given the row's result registers:
    for a packed op each register or half holds one value."""
    sixteen = re.match(r"scalef32_(pk_)?(f16|bf16)_", op)
    if not sixteen:
        return [(got[0], 32), (got[1], 32)] if "pk_" in op else [(got[0], 32)]
    if sixteen[1]:
        return [(got[0] & 0xffff, 16), (got[0] >> 16, 16)]
    return [((got[0] >> 16 if op.endswith("_hi") else got[0]) & 0xffff, 16)]


def _is_special(op, bits, width, what):
    if width == 32:
        e, m = bits >> 23 & 0xff, bits & 0x7fffff
        return e == 0xff and (m != 0) == (what == "nan")
    e, m = (bits >> 7 & 0xff, bits & 0x7f) if "bf16" in op else (bits >> 10 & 0x1f, bits & 0x3ff)
    return e == (0xff if "bf16" in op else 0x1f) and (m != 0) == (what == "nan")


@pytest.fixture(scope="module")
def cvt():
    from k8s_gpu_node_checker_amd.ops import cvt as cv
    assert cv.device_count() >= 1
    return cv


def _clean(r):
    assert r["pass"] is True and r["errors"] == 0 and r["detail"] == "", r["detail"]
    assert "bad_simds" not in r
    assert all(row["errors"] == 0 and row["first_bad"] is None for row in r["ops"].values())
    assert r["mode"] == {"round": 0, "denorm": 15, "nearest_even": True, "denormals_kept": True}


def _is_nan(op, word):
    return (word & 0x7f800000) == 0x7f800000 and (word & 0x7fffff) != 0


@pytest.mark.parametrize("op", _OPS)
def test_one_application_matches_the_model_word_for_word(cvt, op):
    rows = cvt.shaped_rows(op, 256, seed=0xA11CE)
    if NARROW_SOURCE.match(op):
        _every_code(cvt, op)
    elif re.match(r"scalef32_pk32_(f32|f16|bf16)_(fp6|bf6)", op):  # every six-bit code in every one of the 32 positions
        for s in SCALES:
            for r in range(64):
                bits = sum(((j + r) % 64) << 6 * j for j in range(32))
                rows.append((*[bits >> 32 * i & 0xffffffff for i in range(6)], *[0] * 26, s))
    elif op in ("f32_f16", "f32_bf16"):  # all 65,536 codes: 1,024 wave-rows in one call
        rows = [(c, 0, 0, ONE) for c in range(1 << 16)]
    want, got = cvt.model(op, rows), cvt.apply_many(op, rows)
    assert len(want) == len(got) == len(rows)
    refused = 0
    for row, w, g in zip(rows, want, got):
        if w is None:  # an Inf or NaN code: outside the model; a NaN source must at least give a NaN
            refused += 1
            src = row[0] & 0xffff if op in ("f32_f16", "f32_bf16") else None
            nan16 = src is not None and (src & (0x7c00 if op == "f32_f16" else 0x7f80)) == (0x7c00 if op == "f32_f16" else 0x7f80) \
                and src & (0x3ff if op == "f32_f16" else 0x7f)
            if nan16:
                assert _is_nan(op, g[0]), (op, hex(src), hex(g[0]))
            continue
        assert g == w, (op, [hex(v) for v in row], [hex(v) for v in g], [hex(v) for v in w])
    assert refused < len(rows) // 8
    if not NARROW_SOURCE.match(op) and op not in ("f32_f16", "f32_bf16"):
        assert refused == 0  # the shapes stay inside the domain


def _every_code(cvt, op):
    """All 256 source codes (fp4: all 256 bytes) in each position of the selected byte or word, the other position a
    finite partner, under three scales: a finite code against the model word for word, a NaN code as `is a NaN`, an
    Inf code (bf8) as an Inf.  A packed op's every result is looked at."""
    scales = SCALES if op.startswith("scalef32") else (ONE,)
    if re.search(r"_(f16)_(fp8)", op):
        scales = (ONE, 0x3b800000, 0x43000000)  # 2^7 at most: 448 * 2^8 is no f16
    if re.search(r"_(f16)_(bf8)", op):
        scales = (ONE, 0x3b800000, 0x3f000000)  # 1 at most: 57344 * 2 is no f16
    packed8 = "pk_" in op and "fp4" not in op
    rows, meta = [], []
    for s in scales:
        for pos in ((0, 1) if packed8 else (0,)):
            for code in range(256):
                word = (code | FINITE_PARTNER << 8) if pos == 0 else (FINITE_PARTNER | code << 8)
                word = word * 0x00010001 if packed8 else code * 0x01010101
                rows.append((word, 0, 0xa5a5a5a5, s))
                meta.append((code, pos))
    want, got = cvt.model(op, rows), cvt.apply_many(op, rows)
    compared = 0
    for (code, pos), row, w, g in zip(meta, rows, want, got):
        what = _special(op, code)
        if what is None:
            assert w is not None and g == w, (op, hex(code), pos, [hex(v) for v in row], [hex(v) for v in g], w)
            compared += 1
            continue
        assert w is None, (op, hex(code))  # the model refuses it
        res = _results(op, g, row[2])
        bits, width = res[pos] if len(res) > 1 else res[0]
        assert _is_special(op, bits, width, what), (op, hex(code), pos, what, hex(bits))
        if op.startswith("scalef32_f16_"):  # the other half of the destination is kept here too
            kept = g[0] & 0xffff if op.endswith("_hi") else g[0] >> 16
            assert kept == row[2] & 0xffff and g[1] == 0, (op, hex(code), hex(g[0]))
        if len(res) > 1:  # the finite partner beside it is converted as if alone
            alone = cvt.model(op, [((FINITE_PARTNER | FINITE_PARTNER << 8) * 0x00010001, 0, row[2], row[3])])[0]
            other = _results(op, alone, row[2])[1 - pos]
            assert res[1 - pos] == other, (op, hex(code), pos, hex(res[1 - pos][0]), hex(other[0]))
    assert compared == len(rows) - len(scales) * (2 if packed8 else 1) * {"fp8": 2, "bf8": 8}.get(
        "fp8" if "fp8" in op else "bf8" if "bf8" in op else "", 0)


def test_one_workgroup_two_steps_is_clean(cvt):
    r = cvt.cvt_test(0, blocks=1, iters=2, reps=1)
    _clean(r)
    assert r["blocks"] == 1 and tuple(r["ops"]) == cvt.OPS


def test_nine_workgroups_share_an_xcd_and_are_clean(cvt):
    r = cvt.cvt_test(0, blocks=9, iters=3, reps=1)  # workgroups 0 and 8 run on the same XCD
    _clean(r)
    assert r["blocks"] == 9 and r["xcds"] == 8


def test_the_default_grid_is_clean_on_every_xcd_in_the_models_float_mode(cvt):
    r = cvt.cvt_test(0, iters=2, reps=1, slots=True)
    _clean(r)
    assert r["xcds"] == 8 and r["simds"] == 1024 and r["blocks"] == 1024
    assert all(re.fullmatch(SIMD, cvt.simd_name(s)) for s in r["slots"])
    assert r["mode"]["nearest_even"] and r["mode"]["denormals_kept"]


@pytest.mark.parametrize("op", HOOKED)
def test_an_injected_flip_is_one_wrong_word_in_that_op_only(cvt, op):
    r = cvt.cvt_test(0, blocks=8, iters=3, reps=1, inject_op=op, inject_block=5)
    assert r["pass"] is False and r["errors"] == 1 and len(r["bad_simds"]) == 1
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    bad = r["ops"][op]["first_bad"]
    assert bad["lane"] == 0 and bad["chain"] == 0 and re.fullmatch(SIMD, bad["where"])
    assert int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert r["detail"] == f"1 wrong words in {op} on {bad['where']}"


@pytest.mark.parametrize("op", HOOKED)
def test_a_skipped_conversion_shows_in_that_op_only(cvt, op):
    r = cvt.cvt_test(0, blocks=8, iters=3, reps=1, inject_op=op, inject_block=5, inject_skip_iter=1)
    assert r["pass"] is False and 0 < r["errors"] <= 64 * cvt.CHAINS
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    assert re.fullmatch(SIMD, r["ops"][op]["first_bad"]["where"])


def test_refused_calls(cvt):
    for kw in (dict(iters=0), dict(iters=(1 << 16) + 1), dict(reps=0), dict(blocks=-1),
               dict(blocks=4, inject_op=cvt.OPS[0], inject_block=4),
               dict(iters=4, inject_op=cvt.OPS[0], inject_block=0, inject_skip_iter=4)):
        with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
            cvt.cvt_test(0, ops=cvt.OPS[:1], **{"blocks": 2, "iters": 2, "reps": 1, **kw})
    with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
        cvt.cvt_test(99, ops=cvt.OPS[:1], blocks=1, iters=1, reps=1)
    with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
        cvt.apply_many(cvt.OPS[0], [(0, 0, 0, ONE)] * (64 * 4097))
    with pytest.raises(RuntimeError, match=r"cvt failed \(-2\)"):
        cvt.apply_many(cvt.OPS[0], [(0, 0, 0, ONE)], device=99)


def test_diag_run_carries_a_passing_cvt_result(cvt):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(0, 0, extra=("cvt",))
    assert list(res) == ["cvt"] and res["cvt"]["pass"] and res["cvt"]["errors"] == 0
    assert tuple(res["cvt"]["ops"]) == cvt.OPS and res["cvt"]["iters"] == cvt.DEFAULT_ITERS


def test_the_cli_flag_carries_a_passing_cvt_result(repo):
    def run(*flags):
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag",
                            "--level", "1", "--device", "0", "--format", "json", *flags], capture_output=True, text=True,
                           timeout=300, cwd=repo)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    tests = run("--cvt")
    assert tests["cvt"]["pass"] and tests["cvt"]["errors"] == 0 and tuple(tests["cvt"]["ops"]) == _OPS
    assert "cvt" not in run()
