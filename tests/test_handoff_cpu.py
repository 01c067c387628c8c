"""The handoff diagnostic on CPU: csrc/handoff/handoff_ref.h (the expected word, the partner maps, the classifier)
against an independent Python implementation and hand-made rows; the C ABI of csrc/handoff/handoff.hip against
ops/handoff.py and its fake; what the four kernels compile to (the write-back and the invalidate with their waits,
``sc1`` on every store and load of a write-through slab, the atomic add, the 8-byte granule accesses, no scratch, the
LDS size the library allows); the opt-in wiring (ops/diag.run(extra=...), the CLIs, whole agent cycles) and the build
target.  The kernels themselves run on an MI355X in tests/test_gpu_handoff.py."""
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
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, handoff, lanes
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeDiagLib, FakeFabricLib, FakeHandoffLib, FakeLanesLib,
                                                          c_exports)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "handoff")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
M = 0xffffffff
M64 = (1 << 64) - 1
SEED = handoff.DEFAULT_SEED
GRIDS = (16, 24, 256)


# --- 1. an independent model -----------------------------------------------------------------------------------

def mix32(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x & M


def word(seed, w, r, i):
    return mix32(((seed + 0x9E3779B97F4A7C15 * (r + 1)) & M64) ^ ((w << 32) | i))


def jitter(seed, w, r):
    return mix32((seed ^ 0x6A09E667F3BCC908) + ((r << 32) | w))


# --- 2. the reference header, alone under the host compiler ----------------------------------------------------

REF_CPP = r"""
#include <cstdio>
#include <initializer_list>
#include "handoff_ref.h"

int main() {
  const uint64_t seed = %dULL;
  for (uint32_t w : {0u, 1u, 15u, 255u})
    for (uint32_t r : {0u, 1u, 63u, 32767u})
      for (uint32_t i : {0u, 1u, 511u, 1023u})
        printf("word %%u %%u %%u %%u\n", w, r, i, handoff_word(seed, w, r, i));
  for (int G : {16, 24, 256})
    for (int placement = 0; placement < HANDOFF_PLACEMENTS; ++placement) {
      printf("map %%d %%d", G, placement);
      for (int w = 0; w < G; ++w) printf(" %%d:%%d", handoff_producer(placement, w, G), handoff_consumer(placement, w, G));
      printf("\n");
    }
  for (uint32_t w = 0; w < 16; ++w)
    for (uint32_t r = 0; r < 8; ++r) {
      const uint32_t j = handoff_jitter(seed, w, r);
      printf("jitter %%u %%u %%u %%u %%u\n", w, r, j, handoff_sleeps(j), handoff_passes(j));
    }
  // hand-made rows: producer 5, word 77, read in `round`; got = the word of `round - back`, or a flipped bit
  for (uint32_t round : {0u, 1u, 8u, 9u, 40u})
    for (uint32_t back = 0; back <= 10; ++back) {
      if (back > round) continue;
      int age = -1;
      const int cls = handoff_classify(seed, 5, round, 77, handoff_word(seed, 5, round - back, 77), &age);
      printf("class %%u %%u %%d %%d\n", round, back, cls, age);
    }
  for (uint32_t round : {0u, 3u}) {
    int age = -1;
    const int cls = handoff_classify(seed, 5, round, 77, handoff_word(seed, 5, round, 77) ^ 0x10u, &age);
    printf("flip %%u %%d %%d\n", round, cls, age);
    const int other = handoff_classify(seed, 5, round, 77, handoff_word(seed, 6, round ? round - 1 : 0, 77), &age);
    printf("other %%u %%d %%d\n", round, other, age);
  }
  printf("index %%llu\n", (unsigned long long)handoff_index(255, 32767, 1023));
  for (int f = 0; f < HANDOFF_FORMS; ++f) printf("form %%d %%s\n", f, HANDOFF_FORM_TABLE[f].name);
  for (int p = 0; p < HANDOFF_PLACEMENTS; ++p) printf("placement %%d %%s\n", p, HANDOFF_PLACEMENT_TABLE[p]);
  printf("ok %%d %%d %%d %%d\n", HANDOFF_ROWS, HANDOFF_SLAB_WORDS, HANDOFF_GRANULES, HANDOFF_LDS_BYTES);
  return 0;
}
""" % SEED


@functools.lru_cache(maxsize=None)
def _model():
    """handoff_ref.h compiled with the host compiler alone into a stand-alone program; its output by first field."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "handoff_ref.cpp"), os.path.join(tmp, "handoff_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], check=True,
                       capture_output=True, text=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    assert out.strip().endswith(f"ok {len(handoff.ROWS)} {handoff.SLAB_WORDS} {handoff.GRANULES} {handoff.LDS_BYTES}"), out[-500:]
    rows = {}
    for line in out.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(f[1:])
    return rows


def test_the_header_compiles_alone_and_has_no_hip_include():
    _model()
    with open(os.path.join(CSRC, "handoff_ref.h")) as f:
        assert re.findall(r"#include\s+[<\"]([^>\"]+)", f.read()) == ["cstdint"]


def test_the_word_is_the_independent_one():
    rows = _model()["word"]
    assert len(rows) == 64
    for w, r, i, v in rows:
        assert int(v) == word(SEED, int(w), int(r), int(i)), (w, r, i)
    assert len({int(f[3]) for f in rows}) == 64  # the block, the round and the index all reach the word
    for w, r, j, sleeps, passes in _model()["jitter"]:
        assert int(j) == jitter(SEED, int(w), int(r)) and int(sleeps) == int(j) % 32 < 32
        assert int(passes) == (((int(j) >> 8) % 5) if (int(j) >> 5) & 1 else 0) <= 4
    assert len({f[3] for f in _model()["jitter"]}) > 8 and len({f[4] for f in _model()["jitter"]}) > 2  # uneven


def test_both_partner_maps_are_permutations_without_fixed_points():
    maps = {(int(f[0]), int(f[1])): [tuple(int(x) for x in pair.split(":")) for pair in f[2:]] for f in _model()["map"]}
    assert sorted(maps) == [(G, p) for G in GRIDS for p in (0, 1)]
    for (G, placement), pairs in maps.items():
        producers, consumers = [p for p, _ in pairs], [c for _, c in pairs]
        assert sorted(producers) == sorted(consumers) == list(range(G))  # permutations
        assert all(p != w for w, p in enumerate(producers))               # nobody hands to itself
        stride = 8 if handoff.PLACEMENTS[placement] == "same" else 1
        assert producers == [(w + stride) % G for w in range(G)]          # same: w + 8, cross: w + 1
        assert all(consumers[producers[w]] == w for w in range(G))        # the consumer map is the inverse
    assert handoff.MIN_BLOCKS == 16 and (0 + 8) % 8 == 0  # at G = 8 the `same` map would pair a workgroup with itself


def test_the_classifier_on_hand_made_rows():
    got = {(int(r), int(b)): (int(c), int(a)) for r, b, c, a in _model()["class"]}
    STALE, CORRUPT = handoff.CLASSES.index("stale"), handoff.CLASSES.index("corrupt")
    assert got[(1, 1)] == (STALE, 1) and got[(9, 1)] == (STALE, 1) and got[(40, 1)] == (STALE, 1)  # the round before
    assert got[(8, 8)] == (STALE, 8) and got[(9, 8)] == (STALE, 8) and got[(40, 8)] == (STALE, 8)  # eight back
    assert got[(9, 9)] == (CORRUPT, 0) and got[(40, 9)] == (CORRUPT, 0) and got[(40, 10)] == (CORRUPT, 0)  # nine back
    for age in range(1, handoff.STALE_ROUNDS + 1):
        assert got[(40, age)] == (STALE, age)
    assert [k for k in got if k[0] == 0] == [(0, 0)]  # round 0 has no round before ...
    assert all(c == CORRUPT and a == 0 for (r, b), (c, a) in got.items() if b == 0)  # ... and the right word is not stale
    assert sorted(_model()["flip"]) == [["0", str(CORRUPT), "0"], ["3", str(CORRUPT), "0"]]   # a flipped bit
    assert sorted(_model()["other"]) == [["0", str(CORRUPT), "0"], ["3", str(CORRUPT), "0"]]  # another producer's word
    assert _model()["index"] == [[str((255 << 32) | (32767 << 16) | 1023)]]


# --- 3. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("handoff"), handoff._signatures()
    assert set(exports) == set(sig) == {"handoff_last_error", "handoff_device_count", "handoff_slots", "handoff_lds_bytes",
                                        "handoff_test"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeHandoffLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["handoff_test"]) == 23
    assert [f[1] for f in _model()["form"]] == list(handoff.FORMS)
    assert [f[1] for f in _model()["placement"]] == list(handoff.PLACEMENTS)
    assert handoff.ROWS == tuple(f"{f}/{p}" for f in handoff.FORMS for p in handoff.PLACEMENTS) and len(handoff.ROWS) == 8
    with open(os.path.join(CSRC, "handoff_ref.h")) as f:
        ref = f.read()
    for name, value in (("HANDOFF_THREADS", handoff.THREADS), ("HANDOFF_SLAB_WORDS", handoff.SLAB_WORDS),
                        ("HANDOFF_GRANULES", handoff.GRANULES), ("HANDOFF_MIN_BLOCKS", handoff.MIN_BLOCKS),
                        ("HANDOFF_STALE_ROUNDS", handoff.STALE_ROUNDS), ("HANDOFF_DEFAULT_ROUNDS", handoff.DEFAULT_ROUNDS),
                        ("HANDOFF_DEFAULT_SPIN_MS", handoff.DEFAULT_SPIN_MS)):
        assert re.search(rf"constexpr \w+ {name} = {value};", ref), name
    assert handoff.LDS_BYTES == 82944 > 80 * 1024 and "HANDOFF_LDS_BYTES = 81 * 1024" in ref
    assert FakeHandoffLib.LDS == handoff.LDS_BYTES
    assert handoff.WAITS == (None, "flag", "ack", "granule") and handoff.CLASSES == (None, "stale", "corrupt")
    assert re.search(r"enum HandoffWait \{ HANDOFF_WAIT_NONE = 0, HANDOFF_WAIT_FLAG, HANDOFF_WAIT_ACK, HANDOFF_WAIT_GRANULE \}", ref)
    assert re.search(r"enum HandoffClass \{ HANDOFF_CLASS_NONE = 0, HANDOFF_CLASS_STALE, HANDOFF_CLASS_CORRUPT \}", ref)


# --- 4. instructions -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _kernels():
    """``hipcc --save-temps`` of handoff.hip: (the device assembly, the body of every instantiation by form)."""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--save-temps", "-c", "--cuda-device-only",
                        os.path.join(CSRC, "handoff.hip"), "-o", os.path.join(tmp, "handoff.o")], check=True,
                       capture_output=True, text=True, cwd=tmp)
        (name,) = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f]
        with open(os.path.join(tmp, name)) as f:
            text = f.read()
    bodies = {int(k): body for k, body in re.findall(r"^_ZN\w*14handoff_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text, re.M | re.S)}
    return text, {handoff.FORMS[k]: body for k, body in bodies.items()}


def _instructions(body):
    """the instructions of a kernel in file order, comments, labels and directives dropped"""
    out = []
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if line and not line.endswith(":") and not line.startswith("."):
            out.append(line)
    return out


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@needs_hipcc
def test_no_kernel_has_scratch_and_every_kernel_declares_the_lds_the_library_allows():
    text, bodies = _kernels()
    assert sorted(bodies) == sorted(handoff.FORMS)  # one instantiation per form
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {str(handoff.LDS_BYTES)}
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}
    assert set(re.findall(r"\.sgpr_spill_count: (\d+)", text)) == {"0"}
    assert 2 * handoff.LDS_BYTES > 160 * 1024  # two workgroups do not fit one CU's LDS
    for body in bodies.values():
        ins = _instructions(body)
        assert not [i for i in ins if i.startswith(("flat_", "scratch_"))]  # every shared word: a global access
        assert [i for i in ins if i.startswith("s_sleep")]                  # the polls sleep


@needs_hipcc
def test_the_fence_form_writes_back_and_invalidates_each_behind_its_wait():
    ins = _instructions(_kernels()[1]["fence"])
    (wb,) = [n for n, i in enumerate(ins) if i.startswith("buffer_wbl2")]
    (inv,) = [n for n, i in enumerate(ins) if i.startswith("buffer_inv")]
    assert ins[wb] == "buffer_wbl2 sc1" and ins[inv] == "buffer_inv sc1"
    # the write-back: waited for (the fence's own wait and the asm statement's) before the flag store
    flag = next(n for n in range(wb + 1, len(ins)) if ins[n].startswith(("global_store", "global_atomic")))
    assert re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\] sc1$", ins[flag]), ins[flag]
    between = ins[wb + 1:flag]
    assert between.count("s_waitcnt vmcnt(0)") >= 1 and "s_barrier" not in between
    # ... and it follows the stores of the slab: plain dwordx4, every wave's wait, the barrier
    slab = max(n for n in range(wb) if ins[n].startswith("global_store_dwordx4"))
    assert re.match(r"global_store_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off$", ins[slab]), ins[slab]
    assert "s_waitcnt vmcnt(0)" in ins[slab + 1:wb] and "s_barrier" in ins[slab + 1:wb]
    assert ins[slab + 1:wb].index("s_waitcnt vmcnt(0)") < ins[slab + 1:wb].index("s_barrier")
    # the invalidate: waited for before the barrier, and the loads of the slab come behind that barrier, plain
    barrier = next(n for n in range(inv + 1, len(ins)) if ins[n] == "s_barrier")
    assert "s_waitcnt vmcnt(0)" in ins[inv + 1:barrier]
    load = next(n for n in range(barrier + 1, len(ins)) if ins[n].startswith("global_load_dwordx4"))
    assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off$", ins[load]), ins[load]
    assert not [i for i in ins[inv + 1:barrier] if i.startswith("global_load_dwordx4")]


@needs_hipcc
@pytest.mark.parametrize("form", ("wt", "wt_add"))
def test_the_write_through_forms_have_no_fence_and_sc1_on_every_access_of_the_slab(form):
    ins = _instructions(_kernels()[1][form])
    assert not [i for i in ins if i.startswith(("buffer_wbl2", "buffer_inv"))]
    x4_stores = [i for i in ins if i.startswith("global_store_dwordx4") and ", off" in i]  # the asm statements
    x4_loads = [i for i in ins if i.startswith("global_load_dwordx4")]
    # stores: the slab with sc1, and the private region's plain one; loads: the pre-read (plain, thrown away), the slab's sc1
    assert sorted(i.endswith(" sc1") for i in x4_stores) == [False, True], x4_stores
    assert sorted(i.endswith(" sc1") for i in x4_loads) == [False, True], x4_loads
    slab = next(n for n, i in enumerate(ins) if i.startswith("global_store_dwordx4") and i.endswith("off sc1"))
    pre = next(n for n, i in enumerate(ins) if i.startswith("global_load_dwordx4") and i.endswith(", off"))
    load = next(n for n, i in enumerate(ins) if i.startswith("global_load_dwordx4") and i.endswith("off sc1"))
    assert pre < slab < load  # the plain pre-read lies before the produce, far from the consume
    # every storing wave waits, then the barrier, then the signal
    after = ins[slab + 1:load]
    assert after[0] == "s_waitcnt vmcnt(0)" and "s_barrier" in after
    adds = [i for i in after if re.match(r"global_atomic_add v\d+, v\d+, s\[\d+:\d+\]$", i)]  # to the counter's own line
    flags = [i for i in after[after.index("s_barrier"):] if re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\] sc1$", i)]
    if form == "wt_add":
        assert len(adds) == 1 and after.index(adds[0]) > after.index("s_barrier")
    else:
        assert not adds and flags
    # the poll is an sc1 load of one dword, and a barrier lies between it and the loads of the slab
    polls = [n for n in range(slab, load) if re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\] sc1$", ins[n])]
    assert polls and "s_barrier" in ins[polls[-1]:load]


@needs_hipcc
def test_the_granule_form_stores_and_loads_eight_bytes_with_sc1_and_has_no_flag():
    ins = _instructions(_kernels()[1]["granule"])
    assert not [i for i in ins if i.startswith(("buffer_wbl2", "buffer_inv"))]
    stores = [i for i in ins if i.startswith("global_store_dwordx2")]
    loads = [i for i in ins if i.startswith("global_load_dwordx2")]
    assert len(stores) == 2 and len(loads) == 2  # two granules per lane, ONE store each
    assert all(re.match(r"global_store_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:\d+)? sc1$", i) for i in stores), stores
    assert all(re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:\d+)? sc1$", i) for i in loads), loads
    first, last = ins.index(stores[0]), ins.index(loads[-1])
    assert not [i for i in ins[first:last] if i.startswith("global_atomic_add")]  # no counter between produce and consume


# --- 5. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, handoff_kw, **FakeDiagLib kwargs)`` -> (FakeHandoffLib, FakeLanesLib) for an n x MI355X node."""
    def install(n=1, handoff_kw=None, **kw):
        lib, hlib, llib = FakeDiagLib(n=n, **kw), FakeHandoffLib(n=n, **(handoff_kw or {})), FakeLanesLib(n=n)
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(handoff, "lib", lambda: hlib)
        monkeypatch.setattr(lanes, "lib", lambda: llib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return hlib, llib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}
ROW_KEYS = {"errors", "words_checked", "launches", "timeouts", "complete", "first_timeout", "pairs_cross_xcd",
            "pairs_same_xcd", "pairs_same_cu", "ms", "us_per_round", "first_bad"}


def test_off_by_default_and_on_when_asked(node):
    hlib, llib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and hlib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and hlib.calls == []
    res = diag.run(1, 0, extra=("handoff",))
    assert list(res)[-1] == "handoff" and set(res) == LEVEL1 | {"handoff"} and hlib.calls == ["handoff0"]
    r = res["handoff"]
    assert r["pass"] and r["errors"] == 0 and r["complete"] and r["detail"] == "" and r["blocks"] == 256
    assert set(r) == {"pass", "errors", "complete", "simds", "xcds", "blocks", "rounds", "rows", "ms", "wall_s", "detail"}
    assert r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["rows"]) == handoff.ROWS and r["rounds"] == 64
    for name, row in r["rows"].items():
        assert set(row) == ROW_KEYS and row["errors"] == 0 and row["timeouts"] == 0 and row["complete"]
        assert row["first_bad"] is None and row["first_timeout"] is None and row["launches"] == 3
        assert row["words_checked"] == 256 * 64 * handoff.words_per_round(name) * 3 and row["us_per_round"] > 0
        assert row["pairs_same_cu"] == 0 and row["pairs_cross_xcd"] + row["pairs_same_xcd"] == 256
        assert (row["pairs_cross_xcd"] if name.endswith("/cross") else row["pairs_same_xcd"]) == 256
    json.dumps(r)
    assert "slots" in handoff.handoff_test(0, slots=True)
    both = diag.run(1, 0, extra=("lanes", "handoff"))  # the opt-in tests combine
    assert list(both)[-2:] == ["lanes", "handoff"] and llib.calls == ["lanes0"] and hlib.calls == ["handoff0"] * 3
    assert diag.run(0, 0, extra=("handoff",)).keys() == {"handoff"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("handoff" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["handoff"] and "handoff" not in diag.REFERENCE_RATES
    assert "handoff" not in diag.DMA_TESTS | diag.SHARED_TESTS and "handoff_test" in diag._UNSCALED
    line = diag._summary("handoff", r)
    assert "8 rows x 64 rounds on 256 workgroups, 1024 SIMDs of 8 XCDs" in line and "0 wrong words;" in line
    assert "incomplete" not in line


def test_a_wrong_word_fails_the_gpu_names_both_cus_and_is_classified(node):
    fence_same, granule_cross = handoff.ROWS.index("fence/same"), handoff.ROWS.index("granule/cross")
    node(4, {"bad": {(2, fence_same): 3, (3, granule_cross): 1}, "corrupt": (granule_cross,)})
    r = diag.run(1, 2, extra=("handoff",))["handoff"]
    assert r["pass"] is False and r["errors"] == 3 and r["complete"]
    assert r["detail"] == "3 wrong words in fence/same on xcd5/se1/cu7/simd2 (stale, 1 rounds old, from xcd3/se0/cu0)"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    assert r["rows"]["fence/same"]["first_bad"] == {
        "where": "xcd5/se1/cu7/simd2", "lane": 9, "producer": "xcd3/se0/cu0", "producer_block": 3, "round": 5, "word": 37,
        "got": "0x0dd0ff1c", "want": "0x4a2d0ff1", "class": "stale", "age": 1, "launch": 1}
    assert [k for k, v in r["rows"].items() if v["errors"]] == ["fence/same"]
    r = diag.run(1, 3, extra=("handoff",))["handoff"]
    bad = r["rows"]["granule/cross"]["first_bad"]
    assert r["pass"] is False and bad["class"] == "corrupt" and bad["age"] == 0 and bad["got"] == "0x4a2d0ef1"
    assert r["detail"] == "1 wrong words in granule/cross on xcd5/se1/cu7/simd2 (corrupt, from xcd3/se0/cu0)"
    assert diag.run(1, 1, extra=("handoff",))["handoff"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_handoff=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (2, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag handoff failed ("))
    assert "3 wrong words in fence/same on xcd5/se1/cu7/simd2 (stale" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["handoff"])
    assert "FAIL" in line and "3 wrong words" in line and "xcd5/se1/cu7/simd2" in text


def test_every_hook_on_the_fake(node):
    node(1)
    r = handoff.handoff_test(0, blocks=16, rounds=8, reps=1, inject_row="wt/same", inject_block=5, inject_round=3)
    bad = r["rows"]["wt/same"]["first_bad"]
    assert r["errors"] == 1 and [k for k, v in r["rows"].items() if v["errors"]] == ["wt/same"] and r["pass"] is False
    assert bad["class"] == "corrupt" and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10 and bad["launch"] == 0
    assert bad["producer_block"] == 13 and bad["round"] == 3 and bad["word"] == 0 and bad["where"] in r["detail"]
    r = handoff.handoff_test(0, blocks=16, rounds=8, reps=1, inject_row="granule/same", inject_block=6, inject_round=7,
                             inject_stale_word=300)
    bad = r["rows"]["granule/same"]["first_bad"]
    assert r["errors"] == 1 and bad["class"] == "stale" and bad["age"] == 1
    assert (bad["producer_block"], bad["round"], bad["word"]) == (6, 7, 300)
    assert "stale, 1 rounds old" in r["detail"]
    r = handoff.handoff_test(0, rows=("fence/cross", "wt/cross"), blocks=16, rounds=8, reps=1, spin_ms=2,
                             inject_row="wt/cross", inject_block=6, inject_round=7, inject_mute=True)
    assert tuple(r["rows"]) == ("fence/cross", "wt/cross")
    row = r["rows"]["wt/cross"]
    assert r["pass"] is True and r["errors"] == 0 and r["complete"] is False
    assert row["timeouts"] == 1 and row["complete"] is False and r["rows"]["fence/cross"]["complete"]
    assert row["first_timeout"] == {"who": 5, "for": "flag", "producer": 6, "round": 7}
    assert row["words_checked"] < 16 * 8 * 1024 * 2
    assert r["detail"].startswith("incomplete, not failed (wt/cross: 1 waits ran out, first workgroup 5 for the flag of 6 "
                                  "in round 7)") and "re-run on an idle device" in r["detail"]
    assert "incomplete (1 waits ran out" in diag._summary("handoff", r)


def test_a_timeout_is_reported_and_does_not_fail_the_gpu(node):
    k = handoff.ROWS.index("wt_add/cross")
    node(2, {"timeout": {(1, k): 4}})
    res = diag.run(1, 1, extra=("handoff",))
    r = res["handoff"]
    assert r["pass"] is True and r["complete"] is False and r["errors"] == 0
    assert r["rows"]["wt_add/cross"]["first_timeout"] == {"who": 2, "for": "flag", "producer": 3, "round": 5}
    assert "4 waits ran out" in r["detail"] and "re-run on an idle device" in r["detail"]
    ag = A.Agent("n2", source="fake", diag_level=1, expect_gpus=2, diag_timeout=60, diag_handoff=True)
    v = H.evaluate_report(ag.probe_once(), 2)
    assert v.state == H.HEALTHY and (v.gpus_ok, v.gpus_seen) == (2, 2)


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    for kw, said in ((dict(blocks=8), "multiple of 8 from 16"), (dict(blocks=20), "multiple of 8 from 16"),
                     (dict(blocks=264), "to the CU count 256, not 264"), (dict(rounds=0), "rounds 1..2^15"),
                     (dict(spin_ms=0), "spin_ms 1..1000"), (dict(reps=0), "reps >= 1"),
                     (dict(inject_row="fence/cross", inject_block=1, inject_round=0, inject_stale_word=3), "round 0 has no round before"),
                     (dict(inject_row="granule/cross", inject_round=1, inject_stale_word=512), "inside the slab"),
                     (dict(inject_row="fence/cross", inject_round=1, inject_stale_word=3, inject_mute=True), "one hook at a time"),
                     (dict(blocks=16, inject_row="fence/cross", inject_block=16), "inside the grid")):
        with pytest.raises(RuntimeError, match=r"handoff failed \(-2\)") as e:
            handoff.handoff_test(0, **kw)
        assert said in str(e.value), (kw, str(e.value))
    for kw in (dict(rows=("fence/diagonal",)), dict(rows=()), dict(rows=("wt/same", "wt/same")),
               dict(rows=("wt/same",), inject_row="wt/cross"), dict(inject_row="no/row")):
        with pytest.raises(ValueError):
            handoff.handoff_test(0, **kw)
    monkeypatch.setitem(diag._TESTS, "handoff", ("handoff_test", {"rounds": 0}))
    r = diag.run(1, 0, extra=("handoff",))["handoff"]
    assert r["pass"] is False and "handoff failed (-2)" in r["detail"] and "rounds 1..2^15" in r["detail"]
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(handoff, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("handoff",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, isolation):
    bad = {"bad": {(5, 0): 1}}
    node(8, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "handoff": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_handoff=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"handoff"}, (d, g["diag"].keys())
        assert g["diag"]["handoff"]["pass"] is (d != 5), (d, g["diag"]["handoff"])
    assert "1 wrong words in fence/cross" in rep["gpus"][5]["diag"]["handoff"]["detail"]  # each child its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", diag_handoff=True, diag_lanes=True, **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 | {"lanes", "handoff"} for g in rep["gpus"])
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    hlib, llib = node(2)
    assert diag.main(["--level", "1", "--handoff", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["handoff", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(hlib.calls) == ["handoff0", "handoff1"] and llib.calls == []
    assert diag.main(["--level", "1"]) == 0
    assert "handoff" not in capsys.readouterr().out and len(hlib.calls) == 2
    assert diag.main(["--level", "1", "--lanes"]) == 0
    assert "handoff" not in capsys.readouterr().out and len(hlib.calls) == 2 and len(llib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--handoff", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--lanes", "--handoff", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [("handoff",), ("lanes", "handoff"), None]
    capsys.readouterr()
    monkeypatch.undo()
    hlib, llib = node(1)
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--handoff"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and hlib.calls == ["handoff0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(hlib.calls) == 1 and llib.calls == []
    assert A.build_parser().parse_args(["--node", "n", "--diag-handoff"]).diag_handoff is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_handoff is False
    for main, flag in ((diag.main, "--handoff"), (node_cycle.main, "--handoff"), (A.main, "--diag-handoff")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 6. build --------------------------------------------------------------------------------------------------

def test_the_build_has_a_handoff_target():
    t = B._targets()
    assert "handoff" in t and t["handoff"]["out"].endswith("libmi355x_handoff.so")
    assert t["handoff"]["cmd"] == t["xgmi"]["cmd"] and t["handoff"]["headers"][0].endswith("handoff_ref.h")
    assert [os.path.basename(h) for h in t["handoff"]["headers"][1:]] == ["hip_host.h", "simd_report.h"]
    assert "libmi355x_handoff.so" in B.__doc__
    with open(os.path.join(CSRC, "handoff.hip")) as f:
        src = f.read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../common/hip_host.h", "../common/simd_report.h", "handoff_ref.h"]
    out = t["handoff"]["out"]
    if not os.path.exists(out):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(out)
    for name in handoff._signatures():
        getattr(L, name)  # AttributeError: not exported
    L.handoff_lds_bytes.restype = ctypes.c_int
    assert L.handoff_lds_bytes() == handoff.LDS_BYTES
