"""The scratch diagnostic on CPU: csrc/scratch/scratch_ref.h (the mix, the classifier, the co-residency sweep, the
frames routines) compiled with the host compiler alone and held against an independent Python implementation; the C
ABI of csrc/scratch/scratch.hip against ops/scratch.py and its fake; the opt-in wiring (ops/diag.run(extra=...), the
CLIs, the agent's flag); what the kernels compile to (no spills, a private segment in every kernel, the compiler's
own scratch accesses, four real calls) and the build target.  The kernels themselves run on an MI355X in
tests/test_gpu_scratch.py."""
import ctypes
import functools
import inspect
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, lanes, scratch
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeDiagLib, FakeFabricLib, FakeLanesLib, FakeScratchLib,
                                                          c_exports)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "scratch")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
M = 0xffffffff
SEED = scratch.DEFAULT_SEED


# --- 1. an independent model -----------------------------------------------------------------------------------

def mix(x):
    x &= M
    x ^= x >> 16
    x = x * 0x85ebca6b & M
    x ^= x >> 13
    x = x * 0xc2b2ae35 & M
    x ^= x >> 16
    return x


def preset(seed, wave, lane, walk, word):
    return mix(mix(seed ^ (wave * 64 + lane)) + walk * 0x9e3779b9 + word * 0x85ebca77 + 1)


def start(seed, wave, lane, walk):
    return mix(preset(seed, wave, lane, walk, 0xffff) ^ 0x5c4a7c15)


def unmix(x):
    x ^= x >> 16
    x = x * pow(0xc2b2ae35, -1, 1 << 32) & M
    x ^= (x >> 13) ^ (x >> 26)
    x = x * pow(0x85ebca6b, -1, 1 << 32) & M
    x ^= x >> 16
    return x


def pack(rnd, wave, lane, word):
    return (rnd << 28) | (wave << 14) | (lane << 8) | word


def iso_word(seed, rnd, wave, lane, word):
    return mix(pack(rnd, wave, lane, word)) ^ seed


def frames_index(seed, wave, lane, steps):
    a = [0] * 64
    x = start(seed, wave, lane, 0x1dec5)
    for i in range(64):
        a[(i * 29 + lane) & 63] = mix(x + i)
    for t in range(steps):
        j = x & 63
        x = (mix(x ^ a[j]) + t) & M
        k = (x >> 6) & 63
        a[k] = (a[k] + (x | 1)) & M
        if x & 0x1000:
            a[j] = a[k] ^ (x >> 3)
    return [a[k] ^ a[k + 16] ^ a[k + 32] ^ a[k + 48] for k in range(16)] + [x]


def chain(depth, up, x):
    buf = [mix(x + k * 0x9e3779b9 + depth) ^ up[(k * 7 + depth) & 15] for k in range(16)]
    for k in range(16):
        j = (x >> k) & 15
        buf[j] ^= (up[(j * 5 + k) & 15] + x) & M
        x = mix(x + buf[(x >> 4) & 15])
        up[x & 15] = (up[x & 15] + (buf[k] | 1)) & M
    if depth + 1 < 4:
        x = chain(depth + 1, buf, x)
    for k in range(16):
        up[k] ^= buf[(k + x) & 15]
    return mix(x ^ up[x & 15])


def frames_calls(seed, wave, lane, steps):
    x = start(seed, wave, lane, 0xca11)
    top = [mix(x ^ k) for k in range(16)]
    for t in range(0, steps, 32):
        x = chain(0, top, (x + t) & M)
    return top + [x]


# --- 2. the reference header, alone under the host compiler ----------------------------------------------------

REF_CPP = r"""
#include <cstdio>
#include <initializer_list>
#include "scratch_ref.h"

int main() {
  const uint32_t seed = %du;
  for (uint32_t x : {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x0fffffffu, 0x10000000u, 0x3fffu, 0x4000u, 0xffu, 0x100u})
    printf("mix %%u %%u %%u\n", x, scratch_mix(x), scratch_unmix(scratch_mix(x)));
  for (uint32_t i = 0; i < 4096; ++i) {
    const uint32_t x = i * 0x9e3779b9u + 12345u;
    if (scratch_unmix(scratch_mix(x)) != x || scratch_mix(scratch_unmix(x)) != x) printf("mix broken %%u\n", x);
  }
  printf("word %%u %%u\n", scratch_pack(15, 16383, 63, 255), scratch_iso_word(seed, 1, 5, 0, 77));
  // hand-made wrong words at the cell (round 1, wave 5, lane 0, word 77) of a launch of 256 waves and 2 rounds
  const uint32_t cell = scratch_pack(1, 5, 0, 77), want = scratch_iso_word(seed, 1, 5, 0, 77);
  const struct { const char* what; uint32_t got; } made[] = {
      {"alias_wave", scratch_iso_word(seed, 1, 6, 0, 77)},   {"alias_lane", scratch_iso_word(seed, 1, 5, 9, 77)},
      {"alias_word", scratch_iso_word(seed, 1, 5, 0, 78)},   {"alias_behind", scratch_iso_word(seed, 0, 200, 3, 77)},
      {"stale", scratch_iso_word(seed, 0, 5, 0, 77)},        {"flip", want ^ 0x10u},
      {"outside_waves", scratch_iso_word(seed, 1, 256, 0, 77)}, {"outside_rounds", scratch_iso_word(seed, 2, 5, 0, 77)},
      {"zero", 0u}};
  for (const auto& m : made) {
    const ScratchVerdict v = scratch_classify(seed, cell, m.got, 256, 2);
    printf("class %%s %%d %%d %%u %%u %%u %%u\n", m.what, v.cls, v.age, v.round, v.wave, v.lane, v.word);
  }
  {
    const ScratchVerdict v = scratch_classify(seed, scratch_pack(3, 5, 0, 77), scratch_iso_word(seed, 0, 5, 0, 77), 256, 4);
    printf("class stale3 %%d %%d %%u %%u %%u %%u\n", v.cls, v.age, v.round, v.wave, v.lane, v.word);
  }
  for (uint32_t stride : {37u}) {
    bool seen[256] = {};
    for (uint32_t i = 0; i < 256; ++i) seen[scratch_iso_index(i, 11, stride)] = true;
    int n = 0;
    for (bool b : seen) n += b;
    printf("perm %%u %%d\n", stride, n);
  }
  const unsigned long long t[] = {10, 20, 15, 30, 20, 25, 40, 50, 12, 13};
  unsigned long long pad[20];
  printf("live %%u %%u\n", scratch_co_resident(t, 5, pad), scratch_co_resident(t + 6, 1, pad));
  for (uint32_t wave : {0u, 7u})
    for (uint32_t lane : {0u, 1u, 63u}) {
      uint32_t o[SCRATCH_FRAMES_OUT];
      scratch_frames_index(seed, wave, lane, SCRATCH_FRAMES_STEPS, o);
      printf("index %%u %%u", wave, lane);
      for (uint32_t v : o) printf(" %%x", v);
      scratch_frames_calls(seed, wave, lane, SCRATCH_FRAMES_STEPS, o);
      printf("\ncalls %%u %%u", wave, lane);
      for (uint32_t v : o) printf(" %%x", v);
      printf("\n");
    }
  printf("ok %%d %%d %%d %%d\n", SCRATCH_ROWS, SCRATCH_ISO_WORDS, SCRATCH_FRAMES_OUT, SCRATCH_FRAMES_STEPS);
  return 0;
}
""" % SEED


@functools.lru_cache(maxsize=None)
def _model():
    """scratch_ref.h compiled with the host compiler alone into a stand-alone program; its output by first field."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "scratch_ref.cpp"), os.path.join(tmp, "scratch_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    assert out.strip().endswith(f"ok {len(scratch.ROWS)} {scratch.ISO_WORDS} {scratch.FRAMES_OUT} 96"), out[-300:]
    rows = {}
    for line in out.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(f[1:])
    return rows


def test_the_header_compiles_alone_and_has_no_hip_include():
    _model()
    with open(os.path.join(CSRC, "scratch_ref.h")) as f:
        assert re.findall(r"#include\s+[<\"]([^>\"]+)", f.read()) == ["cstddef", "cstdint"]


def test_the_mix_is_a_bijection():
    assert "broken" not in [f[0] for f in _model()["mix"]]
    for x, mixed, back in _model()["mix"]:
        assert int(mixed) == mix(int(x)) and int(back) == int(x) and unmix(int(mixed)) == int(x)
    assert len({f[1] for f in _model()["mix"]}) == len(_model()["mix"])
    assert _model()["word"] == [[str(M), str(iso_word(SEED, 1, 5, 0, 77))]]  # the four fields fill the word
    assert _model()["perm"] == [["37", "256"]]


def test_the_classifier_on_hand_made_words():
    ALIAS, STALE, CORRUPT = (scratch.CLASSES.index(c) for c in ("alias", "stale", "corrupt"))
    got = {f[0]: tuple(int(v) for v in f[1:]) for f in _model()["class"]}
    assert got["alias_wave"] == (ALIAS, 0, 1, 6, 0, 77) and got["alias_lane"] == (ALIAS, 0, 1, 5, 9, 77)
    assert got["alias_word"] == (ALIAS, 0, 1, 5, 0, 78) and got["alias_behind"] == (ALIAS, 1, 0, 200, 3, 77)
    assert got["stale"] == (STALE, 1, 0, 5, 0, 77) and got["stale3"] == (STALE, 3, 0, 5, 0, 77)
    assert got["flip"][0] == CORRUPT and got["flip"][1] == 0
    assert got["outside_waves"][:2] == (CORRUPT, 0) and got["outside_rounds"][:2] == (CORRUPT, 0)
    assert got["zero"][0] == CORRUPT
    t = unmix((iso_word(SEED, 1, 5, 0, 77) ^ 0x10) ^ SEED)  # the flipped word decodes outside this launch
    assert (t >> 14) & 16383 >= 256 or t >> 28 >= 2
    assert _model()["live"] == [["3", "1"]]


def test_the_frames_routines_are_the_independent_ones():
    for part, fn in (("index", frames_index), ("calls", frames_calls)):
        rows = _model()[part]
        assert len(rows) == 6
        for f in rows:
            assert [int(v, 16) for v in f[2:]] == fn(SEED, int(f[0]), int(f[1]), 96), (part, f[:2])
        assert len({tuple(f[2:]) for f in rows}) == 6


# --- 3. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("scratch"), scratch._signatures()
    assert set(exports) == set(sig) == {"scratch_last_error", "scratch_device_count", "scratch_slots", "scratch_rows",
                                        "scratch_test"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeScratchLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["scratch_test"]) == 20
    assert scratch.ROWS == ("isolate/1k", "frames/index", "frames/calls")
    with open(os.path.join(CSRC, "scratch_ref.h")) as f:
        ref = f.read()
    for name, value in (("SCRATCH_THREADS", scratch.THREADS), ("SCRATCH_ISO_WORDS", scratch.ISO_WORDS),
                        ("SCRATCH_ISO_MAX_WAVES", scratch.ISO_MAX_WAVES), ("SCRATCH_ISO_MAX_ROUNDS", scratch.ISO_MAX_ROUNDS),
                        ("SCRATCH_ISO_DEFAULT_ROUNDS", scratch.DEFAULT_ROUNDS), ("SCRATCH_FRAMES_OUT", scratch.FRAMES_OUT)):
        assert re.search(rf"constexpr \w+ {name} = {value};", ref), name
    assert scratch.CLASSES == (None, "alias", "stale", "corrupt")
    assert re.search(r"enum ScratchClass \{ SCRATCH_CLASS_NONE = 0, SCRATCH_CLASS_ALIAS, SCRATCH_CLASS_STALE, "
                     r"SCRATCH_CLASS_CORRUPT \}", ref)


# --- 4. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, scratch_kw, **FakeDiagLib kwargs)`` -> (FakeScratchLib, FakeLanesLib) for an n x MI355X node."""
    def install(n=1, scratch_kw=None, **kw):
        lib, slib, llib = FakeDiagLib(n=n, **kw), FakeScratchLib(n=n, **(scratch_kw or {})), FakeLanesLib(n=n)
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(scratch, "lib", lambda: slib)
        monkeypatch.setattr(lanes, "lib", lambda: llib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return slib, llib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}
ROW_KEYS = {"errors", "words_checked", "launches", "ms", "frame_bytes", "first_bad"}
ISO = scratch.ROWS.index("isolate/1k")


def test_off_by_default_and_on_when_asked(node):
    slib, llib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and slib.calls == []
    res = diag.run(1, 0, extra=("scratch",))
    assert list(res)[-1] == "scratch" and set(res) == LEVEL1 | {"scratch"} and slib.calls == ["scratch0"]
    r = res["scratch"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and "bad_simds" not in r
    assert {"pass", "errors", "rows", "simds", "xcds", "frame_bytes", "co_resident_waves", "detail"} <= set(r)
    assert r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["rows"]) == scratch.ROWS
    assert r["isolate_waves"] == 16384 and r["isolate_blocks"] == 4096 and r["blocks"] == 256
    assert r["frame_bytes"] == {"isolate": 1040, "frames": 400} and r["co_resident_waves"] > 1
    for name, row in r["rows"].items():
        assert set(row) == ROW_KEYS and row["errors"] == 0 and row["first_bad"] is None and row["launches"] == 2
        blocks = 4096 if name == "isolate/1k" else 256
        assert row["words_checked"] == 2 * scratch.words_per_launch(name, blocks), name
        assert 0 < row["frame_bytes"] <= 1088
    json.dumps(r)
    assert "slots" in scratch.scratch_test(0, slots=True)
    both = diag.run(1, 0, extra=("lanes", "scratch"))  # the opt-in tests combine
    assert list(both)[-2:] == ["lanes", "scratch"] and llib.calls == ["lanes0"]
    assert diag.run(0, 0, extra=("scratch",)).keys() == {"scratch"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("scratch" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["scratch"] and "scratch" not in diag.REFERENCE_RATES
    assert "scratch" not in diag.DMA_TESTS | diag.SHARED_TESTS and "scratch_test" in diag._UNSCALED
    line = diag._summary("scratch", r)
    assert "3 rows (isolate/1k, frames/index, frames/calls) on 1024 SIMDs of 8 XCDs" in line and "0 wrong words;" in line


def test_a_wrong_word_fails_the_gpu_and_is_classified(node):
    dword = scratch.ROWS.index("frames/index")
    node(4, {"bad": {(2, ISO): 3, (3, dword): 1}, "classes": {ISO: "alias"}})
    r = diag.run(1, 2, extra=("scratch",))["scratch"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == ("3 wrong words in isolate/1k on xcd5/se1/cu7/simd2 (alias, written by wave 4 on "
                           "xcd1/se0/cu0/simd0)")
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    bad = r["rows"]["isolate/1k"]["first_bad"]
    assert bad == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "wave": 3, "word": 37, "round": 1, "got": "0x5c7a7d11",
                   "want": "0x5c7a7c11", "class": "alias", "age": 0,
                   "writer": {"wave": 4, "where": "xcd1/se0/cu0/simd0"}, "launch": 1}
    r = diag.run(1, 3, extra=("scratch",))["scratch"]
    assert r["pass"] is False and r["detail"] == "1 wrong words in frames/index on xcd5/se1/cu7/simd2 (corrupt)"
    assert diag.run(1, 1, extra=("scratch",))["scratch"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_scratch=True)
    rep = ag.probe_once()
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["scratch"])
    assert "FAIL" in line and "3 wrong words" in line
    assert rep["gpus"][1]["diag"]["scratch"]["pass"] and not rep["gpus"][3]["diag"]["scratch"]["pass"]


def test_every_hook_on_the_fake(node):
    node(1)
    kw = dict(rows=("isolate/1k", "frames/index", "frames/calls"), blocks=8, isolate_blocks=64, rounds=2)
    r = scratch.scratch_test(0, inject_row="isolate/1k", inject_wave=5, **kw)
    bad = r["rows"]["isolate/1k"]["first_bad"]
    assert r["errors"] == 1 and r["pass"] is False and [k for k, v in r["rows"].items() if v["errors"]] == ["isolate/1k"]
    assert bad["class"] == "corrupt" and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10 and bad["launch"] == 0
    assert (bad["wave"], bad["lane"], bad["word"], bad["round"], bad["writer"]) == (5, 0, 0, 0, None)
    r = scratch.scratch_test(0, inject_row="isolate/1k", inject_wave=5, inject_alias=True, **kw)
    bad = r["rows"]["isolate/1k"]["first_bad"]
    assert r["errors"] == 1 and bad["class"] == "alias" and bad["writer"]["wave"] == 6 and bad["age"] == 0
    assert "alias, written by wave 6 on " + bad["writer"]["where"] in r["detail"]
    r = scratch.scratch_test(0, inject_row="isolate/1k", inject_wave=5, inject_stale_word=77, **kw)
    bad = r["rows"]["isolate/1k"]["first_bad"]
    assert r["errors"] == 1 and bad["class"] == "stale" and bad["age"] == 1 and (bad["word"], bad["round"]) == (77, 1)
    assert "stale, 1 rounds old" in r["detail"]
    for row in ("frames/index", "frames/calls"):
        r = scratch.scratch_test(0, inject_row=row, inject_wave=3, **kw)
        bad = r["rows"][row]["first_bad"]
        assert r["errors"] == 1 and bad["class"] == "corrupt" and (bad["wave"], bad["lane"], bad["word"]) == (3, 0, 0)
        assert int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    iso = dict(rows=("isolate/1k",), inject_row="isolate/1k")
    for kw, said in ((dict(isolate_blocks=4097), "at most 16384 waves"), (dict(rounds=0), "rounds 1..16"),
                     (dict(rounds=17), "rounds 1..16"),
                     (dict(reps=0), "reps >= 1"),
                     (dict(isolate_blocks=64, inject_wave=255, inject_alias=True, **iso), "an alias needs wave + 1"),
                     (dict(inject_stale_word=3, inject_round=0, **iso), "round 0 has no round before"),
                     (dict(inject_stale_word=256, **iso), "inside the frame"),
                     (dict(inject_stale_word=3, inject_alias=True, **iso), "one hook at a time"),
                     (dict(rows=("frames/index",), inject_row="frames/index", inject_alias=True), "only the isolate row"),
                     (dict(rows=("frames/index",), blocks=8, inject_row="frames/index", inject_wave=32), "inside the row's grid")):
        with pytest.raises(RuntimeError, match=r"scratch failed \(-2\)") as e:
            scratch.scratch_test(0, **kw)
        assert said in str(e.value), (kw, str(e.value))
    for kw in (dict(rows=("forms/load_dword",)), dict(rows=()), dict(rows=("frames/index", "frames/index")),
               dict(rows=("frames/index",), inject_row="frames/calls"), dict(inject_row="no/row")):
        with pytest.raises(ValueError):
            scratch.scratch_test(0, **kw)
    monkeypatch.setitem(diag._TESTS, "scratch", ("scratch_test", {"rounds": 0}))
    r = diag.run(1, 0, extra=("scratch",))["scratch"]
    assert r["pass"] is False and "scratch failed (-2)" in r["detail"]
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(scratch, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("scratch",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


def test_the_flags(node, capsys, monkeypatch):
    slib, llib = node(2)
    assert diag.main(["--level", "1", "--scratch", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["scratch", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(slib.calls) == ["scratch0", "scratch1"] and llib.calls == []
    assert diag.main(["--level", "1"]) == 0
    assert "scratch" not in capsys.readouterr().out and len(slib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--scratch", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--lanes", "--scratch", "--duration", "0.001"]) == 0
    assert seen == [("scratch",), ("lanes", "scratch")]
    capsys.readouterr()
    monkeypatch.undo()
    slib, llib = node(1)
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--scratch"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and slib.calls == ["scratch0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(slib.calls) == 1
    assert A.build_parser().parse_args(["--node", "n", "--diag-scratch"]).diag_scratch is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_scratch is False
    for main, flag in ((diag.main, "--scratch"), (node_cycle.main, "--scratch"), (A.main, "--diag-scratch")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 5. the compiled kernels and the build ---------------------------------------------------------------------

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def _kernels():
    """``hipcc --save-temps`` of scratch.hip: the device assembly, and per kernel symbol its metadata."""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--save-temps", "-c", "--cuda-device-only",
                        os.path.join(CSRC, "scratch.hip"), "-o", os.path.join(tmp, "scratch.o")], check=True,
                       capture_output=True, text=True, cwd=tmp)
        (name,) = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f]
        with open(os.path.join(tmp, name)) as f:
            text = f.read()
    meta = {}
    for block in re.findall(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.M | re.S):
        sym = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[sym] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s+(\d+)", block)}
    return text, meta


@needs_hipcc
def test_no_kernel_spills_and_every_kernel_has_a_private_segment():
    text, meta = _kernels()
    assert len(meta) == 3
    for sym, m in meta.items():
        assert 0 < m["private_segment_fixed_size"] <= 1088, sym
        assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, sym
    (iso,) = [m for s, m in meta.items() if "isolate_kernel" in s]
    assert iso["private_segment_fixed_size"] >= 1024 and iso["vgpr_spill_count"] == 0 and iso["sgpr_spill_count"] == 0
    # the isolate frame is written and read by the compiler's own runtime-indexed scratch accesses, and only sleeps between
    body = re.search(r"^_ZN\w*14isolate_kernel\w*:(.*?)^\.Lfunc_end", text, re.M | re.S).group(1)
    assert re.search(r"^\s+scratch_store_dword v\d+, v\d+, ", body, re.M) and re.search(r"^\s+scratch_load_dword v\d+, v\d+, ", body, re.M)
    assert "s_sleep 16" in body and "s_barrier" not in body and "global_load" not in body
    # the chain is four real calls
    assert len(set(re.findall(r"^(_Z13scratch_chainILi\dEEjPjj):", text, re.M))) == 4 and "s_swappc_b64" in text


def test_the_build_has_a_scratch_target():
    t = B._targets()
    assert "scratch" in t and t["scratch"]["out"].endswith("libmi355x_scratch.so")
    assert t["scratch"]["cmd"] == t["xgmi"]["cmd"] and t["scratch"]["headers"][0].endswith("scratch_ref.h")
    assert [os.path.basename(h) for h in t["scratch"]["headers"][1:]] == ["hip_host.h", "simd_report.h"]
    assert "libmi355x_scratch.so" in B.__doc__
    with open(os.path.join(CSRC, "scratch.hip")) as f:
        src = f.read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../common/hip_host.h", "../common/simd_report.h", "scratch_ref.h"]
    out = t["scratch"]["out"]
    if not os.path.exists(out):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(out)
    for name in scratch._signatures():
        getattr(L, name)  # AttributeError: not exported
    assert L.scratch_rows() == len(scratch.ROWS)
