"""The hbmscan diagnostic on CPU: csrc/hbmscan/hbmscan_ref.h -- the expected word, the plan, the classifier -- compiled
alone by g++ into a stand-alone program (once more under the address and undefined-behaviour sanitizers) and held
against the independent Python model below; the C ABI of csrc/hbmscan/hbmscan.hip against ops/hbmscan.py and its fake;
the opt-in wiring (ops/diag.run(extra=...), the CLIs, agent cycles) and the build target.  The kernels themselves run on
an MI355X in tests/test_gpu_hbmscan.py, which imports the model from here."""
import ctypes
import functools
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
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, hbmscan
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeDiagLib, FakeFabricLib, FakeHbmscanLib, c_exports

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "hbmscan")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
EXPORTS = {"hbmscan_last_error", "hbmscan_device_count", "hbmscan_plan", "hbmscan_want", "hbmscan_classify",
           "hbmscan_test"}
GIB, MIB = 1 << 30, 1 << 20
# hipMemGetInfo on an otherwise unused MI355X (profiles/hbmscan_mi355x.json "whole_device")
MI355X_TOTAL, MI355X_FREE = 309220868096, 308394590208


# --- 1. the model: written from the issue's table, not from the header -----------------------------------------

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
FIXED = (0x00000000, 0x55555555, 0x33333333, 0x0F0F0F0F)


def mix32(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x & M32


def model_steps(phase, random_passes=1):
    return {"addr": 3, "invert": 16, "random": 4 * random_passes, "fade": 3}[phase]


def model_kind(phase, step):
    """What a step does: a moving inversion is write, verify+write, verify+write, verify; addr and fade are write,
    verify+write, verify."""
    if phase in ("addr", "fade"):
        return ("write", "verify_write", "verify")[step]
    return ("write", "verify_write", "verify_write", "verify")[step % 4]


def model_want(phase, step, g, seed):
    """The four lanes of global word ``g`` after ``step`` of ``phase``."""
    if phase == "addr":
        lanes, inv = [g & M32, g >> 32, ~g & M32, ~(g >> 32) & M32], step >= 1
    elif phase == "fade":
        lanes, inv = [mix32(4 * g + lane + (seed ^ 0xFADEFADEFADEFADE)) for lane in range(4)], step >= 1
    elif phase == "invert":
        lanes, inv = [FIXED[step // 4]] * 4, step % 4 == 1
    else:
        s = seed + 0x9E3779B97F4A7C15 * (step // 4)
        lanes, inv = [mix32(4 * g + lane + s) for lane in range(4)], step % 4 == 1
    return tuple(x ^ M32 if inv else x for x in lanes)


def model_bit(phase, step, g, seed, bit):
    return (model_want(phase, step, g, seed)[bit // 32] >> (bit % 32)) & 1


# --- 2. the header, alone under the host compiler ---------------------------------------------------------------

REF_CPP = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hbmscan_ref.h"

// Commands on stdin, one per line; one line of output each.
int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "want")) {
      int phase, step;
      uint64_t g, seed;
      if (scanf("%d %d %" SCNu64 " %" SCNu64, &phase, &step, &g, &seed) != 4) return 2;
      const HbmscanWord w = hbmscan_ref_want(phase, step, g, seed);
      printf("%08x %08x %08x %08x %d\n", w.w[0], w.w[1], w.w[2], w.w[3], hbmscan_step_kind(phase, step));
    } else if (!strcmp(cmd, "steps")) {
      int passes;
      if (scanf("%d", &passes) != 1) return 2;
      printf("%d %d %d %d\n", hbmscan_steps(0, passes), hbmscan_steps(1, passes), hbmscan_steps(2, passes),
             hbmscan_steps(3, passes));
    } else if (!strcmp(cmd, "plan")) {
      uint64_t a[5];
      for (uint64_t& x : a)
        if (scanf("%" SCNu64, &x) != 1) return 2;
      std::vector<uint64_t> out(HBMSCAN_MAX_CHUNKS, 0);
      const int n = hbmscan_ref_plan(a[0], a[1], a[2], a[3], a[4], out.data());
      uint64_t sum = 0;
      bool body = true;
      for (int i = 0; i < n; ++i) {
        sum += out[i];
        body = body && (i + 1 == n || out[i] == a[4]);
      }
      printf("%d %" PRIu64 " %" PRIu64 " %d\n", n, sum, n > 0 ? out[n - 1] : 0, body ? 1 : 0);
    } else if (!strcmp(cmd, "classify")) {
      uint64_t base, tested;
      int n, nh;
      if (scanf("%" SCNu64 " %" SCNu64 " %d %d", &base, &tested, &n, &nh) != 4) return 2;
      std::vector<HbmscanRecord> recs(n > 0 ? n : 1);
      for (int i = 0; i < n; ++i) {
        HbmscanRecord& r = recs[i];
        r.pad = 0;
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64, &r.phase, &r.step, &r.chunk, &r.word,
                  &r.global) != 5) return 2;
        for (int l = 0; l < 4; ++l)
          if (scanf("%" SCNx32, &r.got[l]) != 1) return 2;
        for (int l = 0; l < 4; ++l)
          if (scanf("%" SCNx32, &r.want[l]) != 1) return 2;
      }
      std::vector<uint64_t> hist(HBMSCAN_HIST, 0);
      for (int i = 0; i < nh; ++i) {
        int at;
        uint64_t count;
        if (scanf("%d %" SCNu64, &at, &count) != 2 || at < 0 || at >= HBMSCAN_HIST) return 2;
        hist[at] = count;
      }
      HbmscanFinding f;
      hbmscan_ref_classify(recs.data(), n, hist.data(), base, tested, &f);
      printf("%d %d %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", f.kind, f.bit, f.direction, f.chunk, f.victim, f.source,
             f.span);
    } else {
      return 2;
    }
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _program(sanitize):
    """The harness built once per flavour; (path, temporary directory kept alive) or (None, the compiler's words)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    tmp = tempfile.TemporaryDirectory()
    src, exe = os.path.join(tmp.name, "hbmscan_ref.cpp"), os.path.join(tmp.name, "hbmscan_ref")
    with open(src, "w") as f:
        f.write(REF_CPP)
    c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    return (exe, tmp) if c.returncode == 0 else (None, c.stderr)


def ask(lines, sanitize=False):
    """One run of the stand-alone program over ``lines`` of commands -> its output lines, split."""
    exe, why = _program(sanitize)
    if exe is None and sanitize and re.search(r"cannot find|asan|ubsan|unrecognized", why):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert exe is not None, why
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    return [ln.split() for ln in p.stdout.splitlines()]


INDICES = (0, (1 << 32) - 1, 1 << 32, 1 << 36)
SEEDS = (0x5CA9, 0xFFFFFFFFFFFFFFFF)
PASSES = 2


def _all_steps():
    return [(ph, st) for ph in hbmscan.PHASES for st in range(model_steps(ph, PASSES))]


def _want_lines():
    return [f"want {hbmscan.PHASES.index(ph)} {st} {g} {seed}" for ph, st in _all_steps() for g in INDICES for seed in SEEDS]


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "asan+ubsan"))
def test_want_equals_the_model_in_every_phase_and_step(sanitize):
    out = ask([f"steps {PASSES}"] + _want_lines(), sanitize)
    assert [int(x) for x in out[0]] == [model_steps(ph, PASSES) for ph in hbmscan.PHASES] == [3, 16, 8, 3]
    cases = [(ph, st, g, seed) for ph, st in _all_steps() for g in INDICES for seed in SEEDS]
    assert len(out) - 1 == len(cases) == 30 * 4 * 2
    kinds = ("write", "verify_write", "verify")
    for (ph, st, g, seed), row in zip(cases, out[1:]):
        assert tuple(int(x, 16) for x in row[:4]) == model_want(ph, st, g, seed), (ph, st, g, seed, row)
        assert kinds[int(row[4])] == model_kind(ph, st) == hbmscan.step_kind(ph, st), (ph, st)
    assert [hbmscan.steps(ph, PASSES) for ph in hbmscan.PHASES] == [3, 16, 8, 3]


def test_the_steps_chain_and_cover_every_bit():
    seed, g = 0x5CA9, (1 << 32) + 12345
    rows = {(ph, st): tuple(int(x, 16) for x in row[:4])
            for (ph, st), row in zip(_all_steps(), ask([f"want {hbmscan.PHASES.index(ph)} {st} {g} {seed}"
                                                        for ph, st in _all_steps()]))}
    inv = lambda w: tuple(x ^ M32 for x in w)  # noqa: E731
    for (ph, st), w in rows.items():
        kind = model_kind(ph, st)
        if kind == "verify_write":  # writes the inverse of what it verified
            assert w == inv(rows[ph, st - 1]), (ph, st)
        if kind == "verify":  # writes nothing
            assert w == rows[ph, st - 1], (ph, st)
        assert (kind == "write") == (st == 0 or model_kind(ph, st - 1) == "verify"), (ph, st)
    # the two addr passes are inverses of each other, and the first is the raw index
    assert rows["addr", 0] == (g & M32, g >> 32, ~g & M32, ~(g >> 32) & M32) and rows["addr", 1] == inv(rows["addr", 0])
    # within invert every bit of the 128-bit word is written as 0 and as 1, in every pattern
    for p in range(4):
        held = [sum(x << (32 * i) for i, x in enumerate(rows["invert", 4 * p + sub])) for sub in range(3)]
        assert held[0] | held[1] == (1 << 128) - 1 and held[0] & held[1] == 0 and held[2] == held[0]
        assert rows["invert", 4 * p][0] == FIXED[p]
    # the hashed phases differ from word to word and from pass to pass
    assert rows["random", 0] != rows["random", 4] != rows["fade", 0]


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "asan+ubsan"))
def test_plan(sanitize):
    chunk, reserve = 4 * GIB, 2 * GIB
    cases = {
        "free below the reserve": (GIB, MI355X_TOTAL, reserve, 0, chunk),
        "free equal to the reserve": (reserve, MI355X_TOTAL, reserve, 0, chunk),
        "fifteen bytes": (reserve + 15, MI355X_TOTAL, reserve, 0, chunk),
        "limit under one chunk": (MI355X_FREE, MI355X_TOTAL, reserve, 5 * MIB + 48 + 7, chunk),
        "exact multiple": (reserve + 3 * chunk, MI355X_TOTAL, reserve, 0, chunk),
        "ragged tail": (reserve + 3 * chunk + 4096 + 5, MI355X_TOTAL, reserve, 0, chunk),
        "limit above what is free": (reserve + 2 * chunk, MI355X_TOTAL, reserve, 100 * chunk, chunk),
        "gib=None on an MI355X": (MI355X_FREE, MI355X_TOTAL, reserve, 0, chunk),
        "small chunks": (MI355X_FREE, MI355X_TOTAL, reserve, 5 * MIB + 48, MIB),
        "free above total": (MI355X_TOTAL + 1, MI355X_TOTAL, reserve, 0, chunk),
        "chunk not a multiple of 16": (MI355X_FREE, MI355X_TOTAL, reserve, 0, chunk + 8),
        "chunk above 16 GiB": (MI355X_FREE, MI355X_TOTAL, reserve, 0, 16 * GIB + 16),
        "more than 4096 chunks": (MI355X_FREE, MI355X_TOTAL, reserve, 0, MIB),
    }
    out = {name: [int(x) for x in row] for name, row in
           zip(cases, ask(["plan " + " ".join(map(str, c)) for c in cases.values()], sanitize))}
    for name in ("free below the reserve", "free equal to the reserve", "fifteen bytes", "free above total",
                 "chunk not a multiple of 16", "chunk above 16 GiB", "more than 4096 chunks"):
        assert out[name][0] == -2, (name, out[name])
    # (chunks, bytes in all, the last chunk, every other chunk is `chunk`)
    assert out["limit under one chunk"] == [1, 5 * MIB + 48, 5 * MIB + 48, 1]
    assert out["exact multiple"] == [3, 3 * chunk, chunk, 1]
    assert out["ragged tail"] == [4, 3 * chunk + 4096, 4096, 1]
    assert out["limit above what is free"] == [2, 2 * chunk, chunk, 1]
    assert out["small chunks"] == [6, 5 * MIB + 48, 48, 1]
    target = (MI355X_FREE - reserve) // 16 * 16
    assert out["gib=None on an MI355X"] == [-(-target // chunk), target, target % chunk or chunk, 1]
    assert out["gib=None on an MI355X"][0] == 72 and target / MI355X_TOTAL > 0.99


def _rec(phase, step, chunk, word, g, got, want):
    return (f"{hbmscan.PHASES.index(phase)} {step} {chunk} {word} {g} " + " ".join(f"{x:x}" for x in got) + " "
            + " ".join(f"{x:x}" for x in want))


def _classify(records, hist, base=0, tested=1 << 30, sanitize=False):
    lines = [f"classify {base} {tested} {len(records)} {len(hist)}"] + records + [f"{i} {c}" for i, c in hist.items()]
    kind, bit, direction, chunk, victim, source, span = (int(x) for x in ask(lines, sanitize)[0])
    return hbmscan.FINDINGS[kind], bit, direction, chunk, victim, source, span


def _flip(phase, step, chunk, word, g, bit, seed=0x5CA9):
    """The record of one flipped bit and its histogram entry."""
    want = model_want(phase, step - 1, g, seed)
    got = list(want)
    got[bit // 32] ^= 1 << (bit % 32)
    return _rec(phase, step, chunk, word, g, got, want), 2 * bit + ((got[bit // 32] >> (bit % 32)) & 1)


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "asan+ubsan"))
def test_classify_names_each_of_the_five_findings(sanitize):
    words = 1 << 18  # per chunk, in these synthetic records: 4 MiB chunks
    assert _classify([], {}, sanitize=sanitize) == ("none", -1, -1, -1, 0, 0, 0)
    # stuck_bit: ten wrong words in ten chunks, bit 37 reading 1 where 0 was written, one other bit among them (10/11)
    recs = [_flip("invert", 1, c, 77 + c, c * words + 77 + c, 37)[0] for c in range(10)]
    assert _classify(recs, {2 * 37 + 1: 10, 2 * 5 + 0: 1}, sanitize=sanitize)[:3] == ("stuck_bit", 37, 1)
    assert _classify(recs, {2 * 100 + 0: 9, 2 * 5 + 1: 1}, sanitize=sanitize)[:3] == ("stuck_bit", 100, 0)  # exactly 90 %
    # 89 % on one bit, records in several chunks: scattered
    assert _classify(recs, {2 * 37 + 1: 89, 2 * 5 + 0: 11}, sanitize=sanitize)[0] == "scattered"
    # alias: in addr step 1 word b reads as word a's own-address content; one index bit apart names the bit
    base = (1 << 32) - 100
    for a, b, bit in ((200, 200 + (1 << 7), 7), (5, 5 + (1 << 33), 33), (300, 300 + 3, -1), (1 << 20, 1, -1)):
        ga, gb = base + a, base + b
        for step, polarity in ((1, 0), (2, 1)):  # verifying the first pass, and the inverted one
            got, want = model_want("addr", polarity, ga, 0), model_want("addr", polarity, gb, 0)
            rec = _rec("addr", step, 0, b, gb, got, want)
            hist = {}
            for i in range(128):
                if ((got[i // 32] ^ want[i // 32]) >> (i % 32)) & 1:
                    hist[2 * i + ((got[i // 32] >> (i % 32)) & 1)] = 1
            assert _classify([rec], hist, base, 1 << 36, sanitize) == ("alias", bit if (ga ^ gb) & ((ga ^ gb) - 1) == 0 else -1,
                                                                        -1, -1, gb, ga, 0), (a, b, step)
    # ... the near misses: two differing index bits name no bit (above); content of a word outside the tested set,
    # the wrong polarity for the step, or a phase other than addr is no alias
    got, want = model_want("addr", 0, base + 200, 0), model_want("addr", 0, base + 328, 0)
    hist = {2 * 7 + 0: 1, 2 * 71 + 1: 1}
    assert _classify([_rec("addr", 1, 0, 328, base + 328, got, want)], hist, base, 150, sanitize)[0] == "region"
    assert _classify([_rec("invert", 1, 0, 328, base + 328, got, want)], hist, base, 1 << 36, sanitize)[0] == "region"
    inv = tuple(x ^ M32 for x in got)
    assert _classify([_rec("addr", 1, 0, 328, base + 328, inv, want)], {2 * 7 + 1: 64, 2 * 9: 64}, base, 1 << 36,
                     sanitize)[0] == "region"
    # region: every record in one aligned 2 MiB span of one chunk (different bits, both directions)
    span = (2 * MIB) // 16
    r1, h1 = _flip("random", 1, 3, 2 * span + 1, 3 * words + 2 * span + 1, 3)
    r2, h2 = _flip("random", 2, 3, 3 * span - 1, 3 * words + 3 * span - 1, 90)
    assert h1 != h2
    assert _classify([r1, r2], {h1: 1, h2: 1}, sanitize=sanitize) == ("region", -1, -1, 3, 0, 0, 2 * 2 * MIB)
    # scattered: the next span, or the same span of another chunk
    r3, h3 = _flip("random", 2, 3, 3 * span, 3 * words + 3 * span, 90)
    assert _classify([r1, r3], {h1: 1, h3: 1}, sanitize=sanitize)[0] == "scattered"
    r4, h4 = _flip("random", 2, 4, 2 * span + 1, 4 * words + 2 * span + 1, 90)
    assert _classify([r1, r4], {h1: 1, h4: 1}, sanitize=sanitize) == ("scattered", -1, -1, -1, 0, 0, 0)


# --- 3. ABI -----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    import inspect
    exports, sig = c_exports("hbmscan"), hbmscan._signatures()
    assert set(exports) == set(sig) == EXPORTS
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeHbmscanLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["hbmscan_test"]) == 26 and len(exports["hbmscan_plan"]) == 6
    # the structures ctypes passes are the header's, field for field
    with open(os.path.join(CSRC, "hbmscan_ref.h")) as f:
        header = f.read()
    assert ctypes.sizeof(hbmscan.Record) == 64 and ctypes.sizeof(hbmscan.Finding) == 40
    for struct, cls in (("HbmscanRecord", hbmscan.Record), ("HbmscanFinding", hbmscan.Finding)):
        body = re.search(r"struct %s \{(.*?)\};" % struct, header, re.S).group(1)
        names = [n.split("[")[0] for decl in re.findall(r"^\s*u?int\d+_t ([^;]+);", body, re.M) for n in decl.split(", ")]
        assert [n.replace("global", "global_word") for n in names] == [f[0] for f in cls._fields_], struct
    for const, value in (("HBMSCAN_MAX_RECORDS = 64", hbmscan.MAX_RECORDS), ("HBMSCAN_HIST = 256", hbmscan.HIST),
                         ("HBMSCAN_MAX_CHUNKS = 4096", hbmscan.MAX_CHUNKS)):
        assert const in header and int(const.split()[-1]) == value
    assert "#include <hip" not in header  # plain C++: the host compiler takes it alone


# --- 4. wiring on the fakes -------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, hbmscan_kw, **FakeDiagLib kwargs)`` -> (FakeDiagLib, FakeHbmscanLib) for an n x MI355X node."""
    def install(n=1, hbmscan_kw=None, **kw):
        lib, hlib = FakeDiagLib(n=n, **kw), FakeHbmscanLib(n=n, **(hbmscan_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(hbmscan, "lib", lambda: hlib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return lib, hlib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}
KEYS = {"pass", "errors", "total_gib", "free_gib", "tested_gib", "coverage", "chunks", "cached", "complete", "phases",
        "records", "finding", "wall_s", "detail"}


def test_off_by_default_and_on_when_asked(node):
    lib, hlib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and hlib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and hlib.calls == []
    res = diag.run(1, 0, extra=("hbmscan",))
    assert list(res)[-1] == "hbmscan" and set(res) == LEVEL1 | {"hbmscan"} and hlib.calls == ["hbmscan0"]
    r = res["hbmscan"]
    assert set(r) >= KEYS and r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["records"] == []
    assert r["complete"] and not r["cached"] and r["finding"] == {"kind": "none"}
    assert (r["total_gib"], r["free_gib"], r["tested_gib"], r["chunks"]) == (287.984, 287.0, 285.0, 72)
    assert r["coverage"] == round(285 * GIB / FakeHbmscanLib.TOTAL, 4) and set(r["phases"]) == set(hbmscan.PHASES)
    assert all(p["errors"] == 0 and p["gbs"] == 5000.0 for p in r["phases"].values())
    assert hlib.deadlines == [0.0]  # no deadline given: none passed
    assert diag.run(0, 0, extra=("hbmscan",)).keys() == {"hbmscan"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("hbmscan" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["hbmscan"] and "hbmscan" not in diag.REFERENCE_RATES
    assert "hbmscan" not in diag.DMA_TESTS | diag.SHARED_TESTS and "hbmscan_test" in diag._UNSCALED
    line = diag._summary("hbmscan", r)
    assert "285 of 288 GiB (99.0%) in 72 chunks, 0 wrong words, finding none" in line, line
    # a limit and a deadline reach the library: a share of what is left of run()'s deadline
    import time
    r = diag.run(0, 0, extra=("hbmscan",), options={"hbmscan": {"gib": 1}}, deadline=time.monotonic() + 100)["hbmscan"]
    assert r["tested_gib"] == 1.0 and r["cached"] and r["pass"] and "cells are not proven" in r["detail"]
    assert 40 < hlib.deadlines[-1] <= 100 * diag.HBMSCAN_SHARE
    assert "cached: cells not proven" in diag._summary("hbmscan", r)


def test_a_wrong_word_fails_the_gpu_and_the_node(node):
    lib, hlib = node(4, {"bad": {2: 3}})
    r = diag.run(1, 2, extra=("hbmscan",))["hbmscan"]
    assert r["pass"] is False and r["errors"] == 3 and r["phases"]["invert"]["errors"] == 3
    assert r["detail"] == "3 wrong 16-byte words; stuck bit 37 (0->1); first at +0x1a2b3c40 of chunk 5 (invert step 1)"
    assert r["finding"] == {"kind": "stuck_bit", "bit": 37, "direction": "0->1"} and len(r["records"]) == 3
    first = r["records"][0]
    assert first["chunk"] == 5 and first["chunk_offset"] == 0x1a2b3c40 and first["offset"] == 5 * 4 * GIB + 0x1a2b3c40
    assert first["flipped"] == [[37, "0->1"]] and int(first["got"], 16) == int(first["want"], 16) ^ (1 << 37)
    assert diag.run(1, 1, extra=("hbmscan",))["hbmscan"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_hbmscan=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)  # by the path a failed memtest takes: the GPU's diag results
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag hbmscan failed ("))
    assert "3 wrong 16-byte words; stuck bit 37 (0->1)" in reason
    assert 0 < hlib.deadlines[-1] <= 0.9 * 60 * diag.HBMSCAN_SHARE  # the agent passes a share of --diag-timeout
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["hbmscan"])
    assert "FAIL" in line and "3 wrong words, finding stuck bit 37 (0->1)" in line and "first at +0x1a2b3c40" in text


def test_incomplete_is_reported_and_not_failed(node):
    lib, hlib = node(2, {"incomplete": (1,)})
    r = diag.run(1, 1, extra=("hbmscan",))["hbmscan"]
    assert r["pass"] and r["complete"] is False and r["reached"] == {"phase": "random", "step": 1}
    assert r["detail"] == "stopped by its deadline after random step 1: incomplete, not failed"
    assert ", incomplete," in diag._summary("hbmscan", r)
    ag = A.Agent("n2", source="fake", diag_level=1, expect_gpus=2, diag_timeout=60, diag_hbmscan=True)
    rep = ag.probe_once()
    assert H.evaluate_report(rep, 2).state == H.HEALTHY
    assert rep["gpus"][1]["diag"]["hbmscan"]["complete"] is False and rep["gpus"][0]["diag"]["hbmscan"]["complete"]


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    monkeypatch.setitem(diag._TESTS, "hbmscan", ("hbmscan_test", {"random_passes": 65}))
    r = diag.run(1, 0, extra=("hbmscan",))["hbmscan"]
    assert r["pass"] is False and "hbmscan failed (-2)" in r["detail"] and "random_passes 1..64" in r["detail"]
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(hbmscan, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("hbmscan",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, isolation):
    node(8, {"bad": {5: 1}})
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "hbmscan": {"bad": {5: 1}}})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_hbmscan=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"hbmscan"}, (d, g["diag"].keys())
        assert g["diag"]["hbmscan"]["pass"] is (d != 5), (d, g["diag"]["hbmscan"])
    assert "1 wrong 16-byte words" in rep["gpus"][5]["diag"]["hbmscan"]["detail"]  # each child ran its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    lib, hlib = node(2)
    assert diag.main(["--level", "1", "--hbmscan", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["hbmscan", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(hlib.calls) == ["hbmscan0", "hbmscan1"]  # one thread per GPU: in either order
    assert diag.main(["--level", "1"]) == 0
    assert "hbmscan" not in capsys.readouterr().out and len(hlib.calls) == 2
    assert diag.main(["--level", "1", "--device", "0", "--hbmscan", "--hbmscan-gib", "0.0625"]) == 0
    r = json.loads(capsys.readouterr().out)["devices"]["0"]["tests"]["hbmscan"]
    assert r["tested_gib"] == 0.0625 and r["cached"] and r["chunks"] == 1
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append((k.get("extra"), k.get("options")))
                        or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--hbmscan", "--hbmscan-gib", "2", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--hbmscan", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [(("hbmscan",), {"hbmscan": {"gib": 2.0}}), (("hbmscan",), None), (None, None)]
    capsys.readouterr()
    monkeypatch.undo()
    lib, hlib = node(1)
    b = diag.burn_in(1, [0], 0.0, extra=("hbmscan",), options={"hbmscan": {"gib": 4}})
    assert b["pass"] and b["rounds"] == 1 and hlib.calls == ["hbmscan0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--hbmscan"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and hlib.calls == ["hbmscan0", "hbmscan0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(hlib.calls) == 2
    assert A.build_parser().parse_args(["--node", "n", "--diag-hbmscan"]).diag_hbmscan is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_hbmscan is False
    for main, flag in ((diag.main, "--hbmscan-gib"), (node_cycle.main, "--hbmscan"), (A.main, "--diag-hbmscan")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 5. build ---------------------------------------------------------------------------------------------------

def test_the_build_has_an_hbmscan_target(tmp_path, monkeypatch):
    t = B._targets()
    assert "hbmscan" in t and t["hbmscan"]["out"].endswith("libmi355x_hbmscan.so")
    assert t["hbmscan"]["cmd"] == t["xgmi"]["cmd"] == t["atomics"]["cmd"]
    assert [os.path.relpath(h, os.path.dirname(CSRC)) for h in t["hbmscan"]["headers"]] == [
        os.path.join("hbmscan", "hbmscan_ref.h"), os.path.join("common", "hip_host.h")]
    assert "libmi355x_hbmscan.so" in B.__doc__
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    monkeypatch.setattr(B, "OUT", str(tmp_path))  # a fresh output directory: the tree's own library stays as it is
    msgs = B.build(only=["hbmscan"])
    assert msgs == [f"hbmscan: built {os.path.relpath(os.path.join(str(tmp_path), 'libmi355x_hbmscan.so'), os.path.dirname(B.PKG))}"]
    L = ctypes.CDLL(os.path.join(str(tmp_path), "libmi355x_hbmscan.so"))
    for name in hbmscan._signatures():
        getattr(L, name)  # AttributeError: not exported
    assert B.build(only=["hbmscan"]) == []  # up to date
    # the pure exports answer without a GPU, as the stand-alone program does
    monkeypatch.setattr(hbmscan, "_lib", None)
    assert hbmscan.plan(MI355X_FREE, MI355X_TOTAL)[:2] == [4 * GIB, 4 * GIB] and len(hbmscan.plan(MI355X_FREE, MI355X_TOTAL)) == 72
    with pytest.raises(RuntimeError, match=r"hbmscan failed \(-2\)"):
        hbmscan.plan(GIB, MI355X_TOTAL)
    assert hbmscan.want("addr", 1, (1 << 32) + 5) == model_want("addr", 1, (1 << 32) + 5, hbmscan.DEFAULT_SEED)
    assert hbmscan.want("random", 5, 1 << 36, 77) == model_want("random", 5, 1 << 36, 77)
    with pytest.raises(RuntimeError, match=r"hbmscan failed \(-2\)"):
        hbmscan.want("addr", 3, 0)
    g, want = 1000, model_want("invert", 4, 1000, 0)
    rec = {"phase": "invert", "step": 5, "chunk": 0, "word": g, "global_word": g, "got": (want[0] ^ 2,) + want[1:], "want": want}
    assert hbmscan.classify([rec], [1 if i == 2 * 1 + 1 else 0 for i in range(256)], 0, 1 << 20) == {
        "kind": "stuck_bit", "bit": 1, "direction": "0->1"}
