"""ops.fastpath.loads (native JSON parser of the health annotation) == json.loads, value for value and
type for type; every document it cannot prove identical goes to json.loads (same result / exception)."""
import json
import math

import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from k8s_gpu_node_checker_amd.ops import fastpath
from k8s_gpu_node_checker_amd.testing import fixtures

pytestmark = pytest.mark.skipif(fastpath.ext() is None, reason="native extension not built")


def same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return a == b and math.copysign(1, a) == math.copysign(1, b)
    return a == b


def check(doc):
    try:
        ref = json.loads(doc)
    except Exception as e:
        with pytest.raises(type(e)):
            fastpath.loads(doc)
        return
    got = fastpath.loads(doc)
    assert same(got, ref), (doc, got, ref)


json_values = st.recursive(
    st.none() | st.booleans() | st.integers(min_value=-10**30, max_value=10**30) |
    st.floats(allow_nan=True, allow_infinity=True) | st.text(),
    lambda kids: st.lists(kids, max_size=4) | st.dictionaries(st.text(max_size=5), kids, max_size=4), max_leaves=20)


@settings(max_examples=600, deadline=None)
@given(json_values, st.booleans(), st.booleans())
def test_roundtrip_of_generated_documents(v, ascii_, as_bytes):
    doc = json.dumps(v, ensure_ascii=ascii_, indent=None if ascii_ else 1)
    check(doc.encode("utf-8", "surrogatepass") if as_bytes else doc)
    # the native parser really handled the representable ones (no silent fallback)
    if not as_bytes and not any(0xD800 <= ord(c) <= 0xDFFF for c in doc):
        assert same(fastpath.ext().loads(doc), json.loads(doc))


@settings(max_examples=800, deadline=None)
@given(st.text(alphabet='{}[]",:0123456789.eE+-tfnulrsaINy \t\n\\/u\x01é', max_size=24))
def test_arbitrary_text(doc):
    check(doc)


CASES = ['{"a": 1, "a": 2, "b": 3}', '[1, -0, -0.0, 1e400, -1e400, 1E-400, 0.5e+3]', "NaN", "-Infinity",
         "[Infinity, NaN]", "-NaN", '"\\ud83d\\ude00"', '"\\ud83d"', '"\\ude00x"', '"a\\u0000b"', '"tab\there"',
         '"\\x"', "01", "1.", ".5", "1e", "-", "[1,]", '{"a":1,}', "[] x", "﻿{}", "", "  ", "1" * 5000,
         '{"k": ' * 300 + "1" + "}" * 300, "[" * 100 + "]" * 100, '" "', "true", "nul", "[1 2]",
         '{"a" 1}', '{1: 2}', '"unterminated', "12345678901234567890123", "-12345678901234567890123.5"]


@pytest.mark.parametrize("doc", CASES)
def test_edge_cases(doc):
    check(doc)
    check(doc.encode("utf-8", "surrogatepass"))


@pytest.mark.parametrize("raw", [b"\xef\xbb\xbf{}", b'"\xff"', b'"\xed\xa0\x80"', b"{\x00}", bytearray(b"[1]"),
                                 memoryview(b'{"x": [true]}')])
def test_bytes_inputs(raw):
    check(raw)


def test_real_annotation_is_parsed_natively():
    rep = fixtures.mi355x_probe_report("n", gpus=8)
    raw = fixtures.health_annotation(rep)["amd.com/mi355x-health"]
    assert fastpath.ext().loads(raw) == json.loads(raw) == rep


# The C ABI of the active diagnostics (csrc/diag/diag.hip): one export per diagnostic, each declared to ctypes by
# ops/diag.py with the C signature's arity.  The list is explicit so that a second generation of an entry point
# (a suffixed sibling that forwards to, or is forwarded to by, the first) fails here.
DIAG_EXPORTS = frozenset((
    "diag_last_error", "diag_device_count", "diag_device_arch",
    "diag_set_gemm_variant", "diag_set_gemm_epilogue", "diag_set_gemm_tail", "diag_set_gemm_buffer_loads",
    "diag_set_gemm_schedule", "diag_set_gemm_fp8_unscaled",
    "diag_get_gemm_variant", "diag_get_gemm_epilogue", "diag_get_gemm_tail", "diag_get_gemm_buffer_loads",
    "diag_get_gemm_schedule", "diag_get_gemm_fp8_unscaled",
    "diag_gemm_bf16_launch", "diag_gemm_fp8_launch", "diag_gemm_fp4_launch", "diag_gemm_launch_ck", "diag_gemm_ck_path",
    "diag_gemm_verify", "diag_gemm_fill", "diag_gemm_bf16", "diag_gemm_fp8", "diag_hbm_bandwidth", "diag_memtest",
    "diag_mfma_burn_slots", "diag_mfma_burn",
    "diag_lds_test", "diag_regfile_slots", "diag_regfile_test", "diag_valu_burn", "diag_l2_bandwidth", "diag_hbm_xcd",
    "diag_host_link", "diag_poll_selftest", "diag_p2p_copy", "diag_p2p_fan"))


def test_diag_exports_match_their_ctypes_signatures(monkeypatch):
    import ctypes
    import os

    from k8s_gpu_node_checker_amd.ops import diag, native
    from k8s_gpu_node_checker_amd.testing.fake_native import c_exports
    if not os.path.exists(os.path.join(native.NATIVE_DIR, "libmi355x_diag.so")):
        pytest.skip("libmi355x_diag.so not built (no hipcc)")
    monkeypatch.setattr(diag, "_lib", None)  # the real library, whatever another test installed
    L = diag.lib()
    assert isinstance(L, ctypes.CDLL)
    exports = c_exports("diag")
    assert len(DIAG_EXPORTS) == 38 and set(exports) == DIAG_EXPORTS, sorted(set(exports) ^ DIAG_EXPORTS)
    for name, params in exports.items():
        fn = getattr(L, name)  # AttributeError: not exported
        if not params:
            continue
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, params, fn.argtypes)
        pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)  # (c_char_p: diag_device_arch's buffer)
        for p, t in zip(params, fn.argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)


def quoted_includes(path, seen=None):
    """Every file reachable from `path` through ``#include "..."``, each resolved relative to the file that names it."""
    import os
    import re
    seen = set() if seen is None else seen
    with open(path) as f:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            if target not in seen:
                seen.add(target)
                quoted_includes(target, seen)
    return seen


def test_every_build_target_lists_the_headers_its_sources_reach():
    """build._stale() rebuilds a library when a file of ``sources`` + ``headers`` is newer than it: a header missing
    from the list would leave a stale .so after an edit, so every reachable one must be listed (and exist)."""
    import os

    from k8s_gpu_node_checker_amd import build
    targets = build._targets()
    assert {"diag", "xgmi", "atomics", "fabric"} <= set(targets)
    for name, spec in targets.items():
        listed = {os.path.normpath(p) for p in list(spec["sources"]) + list(spec.get("headers", []))}
        assert all(os.path.exists(p) for p in listed), (name, sorted(p for p in listed if not os.path.exists(p)))
        reached = set()
        for src in spec["sources"]:
            quoted_includes(os.path.normpath(src), reached)
        assert reached <= listed, (name, sorted(reached - listed))
    # the HIP libraries share their host helpers and one build line
    hip = [targets[n] for n in ("diag", "xgmi", "atomics", "fabric")]
    assert all(any(h.endswith(os.path.join("common", "hip_host.h")) for h in t["headers"]) for t in hip)
    assert all(t["cmd"] == hip[0]["cmd"] and "-I" not in t["cmd"] for t in hip)
