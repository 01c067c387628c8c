"""The ifetch diagnostic on CPU: the model of csrc/ifetch/ifetch_ref.h against an independent Python implementation
of the constant hash, a block, a path and every branch op; the coverage condition (the default and the test shapes
visit every block, the shape that does not is refused); the C ABI of csrc/ifetch/ifetch.hip against ops/ifetch.py and
its fake; what the kernels compile to; the opt-in wiring (ops/diag.run(extra=...), the CLIs, whole agent cycles) and
the build target.  The kernels themselves run on an MI355X in tests/test_gpu_ifetch.py."""
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
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, ifetch, lanes
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import (FakeDiagLib, FakeFabricLib, FakeIfetchLib, FakeLanesLib,
                                                          c_exports)

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "ifetch")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
M = 0xffffffff
M64 = (1 << 64) - 1
SEED = ifetch.DEFAULT_SEED


# --- 1. an independent model -----------------------------------------------------------------------------------

def mix32(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x & M


def K(block, j):
    return mix32(((block + 1) << 32) | (j + 1))


def lit(block, j):
    return (K(block, j) & 0x7fffffff) | 0x00800001


def rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def row_of(block):
    """the constants of a block, in the order its instructions use them: (rot, xor, add) x ST, then the walker's"""
    return [(1 + K(block, 3 * s) % 31, lit(block, 3 * s + 1), lit(block, 3 * s + 2)) for s in range(ifetch.ST)] + \
           [lit(block, 3 * ifetch.ST)]


def block_x(block, x):
    for r, kx, ka in row_of(block)[:-1]:
        x = ((rotl(x, r) ^ kx) + ka) & M
    return x


def pmix(v):
    v = v * 0x9E3779B1 & M
    v ^= v >> 15
    v = v * 0x85EBCA6B & M
    v ^= v >> 13
    return v


def block_p(block, p):
    return pmix(p ^ row_of(block)[-1])


def path(seed, q, steps, nb, skip=-1):
    """(final x of 64 lanes, final p, blocks run) of path q"""
    p = mix32(seed * 0x9E3779B97F4A7C15 + 0x1F37 + q)
    x = [mix32((seed ^ 0x5851F42D4C957F2D) * 0xD6E8FEB86659FD93 + (q << 8) + lane) for lane in range(64)]
    ran = []
    for s in range(steps):
        if s == skip:
            continue
        b = p % nb
        ran.append(b)
        x = [block_x(b, v) for v in x]
        p = block_p(b, p)
    return x, p, ran


ON_ZERO = ("s_cbranch_scc0", "s_cbranch_vccz", "s_cbranch_execz")


def branch(op, w, cond):
    k = ifetch.NB + ifetch.OPS.index(op)
    taken = (cond == 0) if op in ON_ZERO else (cond != 0)
    return (w + lit(k, 0)) & M if taken else w ^ lit(k, 1)


def chains(op, seed, iters, skip=-1):
    seed = (seed + 0x9E3779B97F4A7C15 * (ifetch.OPS.index(op) + 1)) & M64
    out = []
    for ch in range(ifetch.CHAINS):
        x, c = mix32(seed * 4 + ch), mix32((seed ^ 0xC0DEC0DE) * 4 + ch) | 1
        for it in range(iters):
            r = x if it == skip else branch(op, x, (x >> 13) & 1)
            x = mix32(((x << 32) | r) + c)
        out.append(x)
    return out


# --- 2. the reference header, alone under the host compiler ----------------------------------------------------

REF_CPP = r"""
#include <cstdio>
#include <vector>
#include "ifetch_ref.h"

int main() {
  const uint64_t seed = %dULL;
  for (uint32_t b : {0u, 1u, 511u, 1023u, 1024u, 1033u}) {
    printf("k %%u", b);
    for (uint32_t j = 0; j <= 3 * IFETCH_ST; ++j) printf(" %%u", ifetch_k(b, j));
    printf("\n");
  }
  for (uint32_t b = 0; b < IFETCH_NB; ++b) {
    printf("row %%u", b);
    for (uint32_t s = 0; s < IFETCH_ST; ++s) printf(" %%u %%u %%u", ifetch_rot(b, s), ifetch_xor(b, s), ifetch_add(b, s));
    printf(" %%u\n", ifetch_pk(b));
    printf("block %%u %%u %%u %%u\n", b, ifetch_block_x(b, 0x12345678u + b), ifetch_block_x(b, 0u), ifetch_block_p(b, 0xDEADBEEFu ^ b));
  }
  std::vector<uint32_t> x(IFETCH_WAVE);
  uint32_t p;
  for (int skip : {-1, 0, 5}) {
    ifetch_walk(seed, 3, 24, 16, skip, x.data(), &p, nullptr);
    printf("walk %%d %%u", skip, p);
    for (uint32_t v : x) printf(" %%u", v);
    printf("\n");
  }
  std::vector<uint32_t> table(IFETCH_TABLE_WORDS);
  for (int steps : {IFETCH_DEFAULT_STEPS, 64})
    for (uint32_t nb : {8u, 64u, 256u, IFETCH_NB})
      printf("visited %%d %%u %%d\n", steps, nb, ifetch_expected(seed, steps, nb, table.data()));
  ifetch_expected(seed, 24, 16, table.data());
  uint32_t sum = 0;
  for (uint32_t v : table) sum = sum * 31u + v;
  printf("table %%u %%u %%u\n", sum, table[3 * IFETCH_WAVE + 5], table[IFETCH_PATHS * IFETCH_WAVE + 3]);
  for (int op = 0; op < IFETCH_BRANCH_OPS; ++op) {
    printf("op %%d %%s %%u %%u", op, IFETCH_BRANCH_TABLE[op].name, ifetch_branch_lit_t(op), ifetch_branch_lit_n(op));
    for (uint32_t w : {0u, 1u, 0x80000000u, 0xffffffffu, 0x2000u})
      printf(" %%u %%u", ifetch_branch_apply(op, w, 0), ifetch_branch_apply(op, w, 1));
    printf("\n");
    uint32_t out[IFETCH_CHAINS];
    for (int skip : {-1, 0, 63}) {
      ifetch_branch_expected(op, ifetch_op_seed(seed, op), 64, skip, out);
      printf("chains %%d %%d %%u %%u %%u %%u\n", op, skip, out[0], out[1], out[2], out[3]);
    }
  }
  printf("mask %%llu %%llu %%llu\n", (unsigned long long)ifetch_branch_mask(0xfcu, 1), (unsigned long long)ifetch_branch_mask(0u, 1),
         (unsigned long long)ifetch_branch_mask(0xfcu, 0));
  printf("ok %%u %%u %%d\n", IFETCH_NB, IFETCH_ST, IFETCH_BRANCH_OPS);
  return 0;
}
""" % SEED


@functools.lru_cache(maxsize=None)
def _ref_program(sanitize):
    """ifetch_ref.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ifetch_ref.cpp"), os.path.join(tmp, "ifetch_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


@functools.lru_cache(maxsize=None)
def _model():
    rc, out = _ref_program(False)
    assert rc == 0 and out.strip().endswith(f"ok {ifetch.NB} {ifetch.ST} {len(ifetch.OPS)}"), out[-2000:]
    rows = {}
    for line in out.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(f[1:])
    return rows


def test_the_header_compiles_alone_and_has_no_hip_include():
    _model()
    with open(os.path.join(CSRC, "ifetch_ref.h")) as f:
        assert re.findall(r"#include\s+[<\"]([^>\"]+)", f.read()) == ["cstdint"]


def test_the_reference_is_clean_under_the_host_sanitizers():
    rc, out = _ref_program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and out.strip().endswith(f"ok {ifetch.NB} {ifetch.ST} {len(ifetch.OPS)}"), out[-2000:]
    assert out == _ref_program(False)[1]  # and computes the same under them


def test_the_constant_hash_is_the_independent_one():
    for f in _model()["k"]:
        b = int(f[0])
        assert [int(v) for v in f[1:]] == [K(b, j) for j in range(3 * ifetch.ST + 1)], b


def test_every_block_is_the_independent_one():
    rows, blocks = _model()["row"], _model()["block"]
    assert [int(f[0]) for f in rows] == list(range(ifetch.NB)) == [int(f[0]) for f in blocks]
    for f in rows:
        b, v = int(f[0]), [int(w) for w in f[1:]]
        want = row_of(b)
        assert v == [w for step in want[:-1] for w in step] + [want[-1]], b
    for f in blocks:
        b = int(f[0])
        assert [int(w) for w in f[1:]] == [block_x(b, (0x12345678 + b) & M), block_x(b, 0), block_p(b, 0xDEADBEEF ^ b)], b


def test_no_two_blocks_share_a_constant_row_and_every_literal_takes_its_own_dword():
    rows = [tuple(int(w) for w in f[1:]) for f in _model()["row"]]
    assert len(set(rows)) == ifetch.NB
    literals = [w for r in rows for i, w in enumerate(r) if i % 3 or i == 3 * ifetch.ST]
    assert len(literals) == ifetch.NB * (2 * ifetch.ST + 1)
    assert len(set(literals)) == len(literals)  # not one literal twice in the whole kernel
    inline = {0x3f000000, 0x3f800000, 0x40000000, 0x40800000, 0x3e22f983}  # 0.5, 1, 2, 4, 1 / 2 pi
    assert all(64 < w < 1 << 31 and w not in inline for w in literals)  # none fits an inline constant
    assert all(1 <= r[3 * s] <= 31 for r in rows for s in range(ifetch.ST))


def test_a_path_is_the_independent_one_and_a_skipped_block_shows():
    walks = {int(f[0]): ([int(v) for v in f[2:]], int(f[1])) for f in _model()["walk"]}
    for skip in (-1, 0, 5):
        x, p, ran = path(SEED, 3, 24, 16, skip)
        assert walks[skip] == (x, p) and len(ran) == 24 - (skip >= 0)
    assert walks[0][0] != walks[-1][0] and walks[5][0] != walks[-1][0]
    # the table: path q's words at 64 q, its walker behind the 64 x 64 words
    (_, at, walker), = _model()["table"]
    x, p, _ = path(SEED, 3, 24, 16)
    assert int(at) == x[5] and int(walker) == p


def test_the_default_and_the_test_shapes_visit_every_block_and_the_one_that_does_not_is_refused():
    visited = {(int(s), int(nb)): int(v) for s, nb, v in _model()["visited"]}
    for nb in ifetch.DEFAULT_NBS:
        assert visited[(ifetch.DEFAULT_STEPS, nb)] == nb, nb
    assert ifetch.DEFAULT_STEPS == 512 and ifetch.DEFAULT_NBS[-1] == ifetch.NB == 1024
    assert visited[(64, 8)] == 8 and visited[(64, ifetch.NB)] < ifetch.NB  # 4,096 draws leave ~18 of 1,024 out
    # the independent count of one case
    ran = set()
    for q in range(ifetch.PATHS):
        ran |= set(path(SEED, q, 64, ifetch.NB)[2])
    assert len(ran) == visited[(64, ifetch.NB)]
    # the library refuses such a walk before it launches anything (ifetch_walk_test of ifetch.hip)
    with open(os.path.join(CSRC, "ifetch.hip")) as f:
        src = f.read()
    body = src[src.index("int ifetch_walk_test("):src.index("int ifetch_branch_test(")]
    refusal = body.index("if (visited[k] != nbs[k])")
    assert refusal < body.index("walk_attributes(") < body.index("read_block_map(") < body.index("hipLaunchKernelGGL(")
    assert "return -2;" in body[refusal:refusal + 400]


def test_every_branch_op_is_the_independent_select():
    ops = _model()["op"]
    assert tuple(f[1] for f in ops) == ifetch.OPS and len(set(ifetch.OPS)) == len(ifetch.OPS) == FakeIfetchLib.OPS
    for f in ops:
        op, k = f[1], ifetch.NB + int(f[0])
        assert (int(f[2]), int(f[3])) == (lit(k, 0), lit(k, 1)) and int(f[2]) != int(f[3])
        got = [int(v) for v in f[4:]]
        want = [branch(op, w, c) for w in (0, 1, 0x80000000, M, 0x2000) for c in (0, 1)]
        assert got == want, op
        assert got[0] != got[1]  # taken and not taken differ
    for f in _model()["chains"]:
        op = ifetch.OPS[int(f[0])]
        assert [int(v) for v in f[2:]] == chains(op, SEED, 64, int(f[1])), (op, f[1])
    clean = {int(f[0]): f[2:] for f in _model()["chains"] if f[1] == "-1"}
    for f in _model()["chains"]:
        if f[1] != "-1":  # a branch that did not happen shows in every chain
            assert all(a != b for a, b in zip(f[2:], clean[int(f[0])])), f
    assert _model()["mask"] == [[str(1 << 63), "1", "0"]]


# --- 3. ABI ----------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    import inspect
    exports, sig = c_exports("ifetch"), ifetch._signatures()
    assert set(exports) == set(sig) == {"ifetch_last_error", "ifetch_device_count", "ifetch_slots", "ifetch_blocks",
                                        "ifetch_block_map", "ifetch_walk_test", "ifetch_branch_test",
                                        "ifetch_apply_blocks", "ifetch_apply"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeIfetchLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["ifetch_walk_test"]) == 17 and len(exports["ifetch_branch_test"]) == 15
    with open(os.path.join(CSRC, "ifetch_ref.h")) as f:
        ref = f.read()
    assert re.findall(r'^    \{"(\w+)", "', ref, re.M) == list(ifetch.OPS)  # the C op table, in the enum's order
    for name, value in (("IFETCH_NB", ifetch.NB), ("IFETCH_ST", ifetch.ST), ("IFETCH_PATHS", ifetch.PATHS),
                        ("IFETCH_CHAINS", ifetch.CHAINS), ("IFETCH_DEFAULT_STEPS", ifetch.DEFAULT_STEPS)):
        assert re.search(rf"constexpr \w+ {name} = {value};", ref), name
    assert ifetch.BLOCK_MIN_BYTES == 128 and "IFETCH_BLOCK_MIN_BYTES = IFETCH_ST * 8" in ref
    assert ifetch.FLOOR_BYTES == 262144 and "IFETCH_FLOOR_BYTES = 256 * 1024" in ref


# --- 4. instructions -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _device_asm():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "ifetch.s")
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(CSRC, "ifetch.hip"), "-o", asm], check=True, capture_output=True, text=True)
        with open(asm) as f:
            return f.read()


def test_the_kernels_have_no_scratch_and_no_lds_and_the_walk_is_one_large_kernel():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    text = _device_asm()
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    assert set(re.findall(r"\.group_segment_fixed_size: (\d+)", text)) == {"0"}    # nor an LDS allocation
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}
    assert set(re.findall(r"\.sgpr_spill_count: (\d+)", text)) == {"0"}
    walks = re.findall(r"^(_ZN\w*11walk_kernel\w*):(.*?)^\.Lfunc_end", text, re.M | re.S)
    assert len(walks) == 1  # one instantiation of the big kernel
    body = walks[0][1]
    # every block is there with its own literals: NB x ST rotates, and the constants of a few rows as they stand
    assert len(re.findall(r"^\s*v_alignbit_b32 ", body, re.M)) == ifetch.NB * ifetch.ST
    assert len(re.findall(r"^\s*s_getpc_b64 ", body, re.M)) >= ifetch.NB  # each records its own address (+ long branches)
    for b in (0, 1, 511, 1023):
        for _, kx, ka in row_of(b)[:-1]:
            assert f"v_xor_b32_e32 v0, 0x{kx:x}, v0" in body or re.search(rf"v_xor_b32_e32 v\d+, 0x{kx:x}, v\d+", body), (b, kx)
            assert re.search(rf"v_add_u32_e32 v\d+, 0x{ka:x}, v\d+", body), (b, ka)
        assert re.search(rf"0x{row_of(b)[-1]:x}\b", body), b
    # 2 literal instructions of 8 bytes per step alone are 256 KiB
    assert ifetch.NB * ifetch.ST * 2 * 8 >= ifetch.FLOOR_BYTES


def test_every_branch_op_compiles_to_its_native_instruction():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    text = _device_asm()
    bodies = {int(k): body for k, body in re.findall(r"^_ZN\w*13branch_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text,
                                                     re.M | re.S)}
    assert sorted(bodies) == list(range(len(ifetch.OPS)))
    for k, name in enumerate(ifetch.OPS):
        inside = re.findall(r";;#ASMSTART(.*?);;#ASMEND", bodies[k], re.S)
        assert len(inside) == ifetch.CHAINS, (name, len(inside))  # one statement per chain, in the one loop
        for stmt in inside:
            assert len(re.findall(rf"^\s*{name} ", stmt, re.M)) >= 1, (name, stmt)
            t, n = lit(ifetch.NB + k, 0), lit(ifetch.NB + k, 1)
            assert re.search(rf"s_add_u32 s\d+, s\d+, 0x{t:x}\b", stmt) and re.search(rf"s_xor_b32 s\d+, s\d+, 0x{n:x}\b", stmt), name
    # the computed targets are assembler-local labels relative to what s_getpc_b64 returns, nothing else
    for k in (ifetch.OPS.index("s_setpc_b64"), ifetch.OPS.index("s_swappc_b64")):
        for stmt in re.findall(r";;#ASMSTART(.*?);;#ASMEND", bodies[k], re.S):
            assert re.search(r"s_getpc_b64 s\[40:41\]\n0:\n\s*s_mov_b32 s\d+, 2f-0b\n\s*s_cmp_lg_u32 s\d+, 0\n\s*s_cmov_b32 s\d+, 1f-0b\n"
                             r"\s*s_add_u32 s40, s40, s\d+\n\s*s_addc_u32 s41, s41, 0\n", stmt), stmt
    # the exec forms save exec, narrow it and restore it inside the same statement
    for k in (ifetch.OPS.index("s_cbranch_execz"), ifetch.OPS.index("s_cbranch_execnz")):
        for stmt in re.findall(r";;#ASMSTART(.*?);;#ASMEND", bodies[k], re.S):
            m = re.search(r"s_mov_b64 (s\[\d+:\d+\]), exec\n\s*s_and_b64 exec, (s\[\d+:\d+\]), s\[\d+:\d+\]\n", stmt)
            assert m and m.group(1) == m.group(2) and stmt.rstrip().endswith(f"s_mov_b64 exec, {m.group(1)}"), stmt


# --- 5. wiring on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, ifetch_kw, **FakeDiagLib kwargs)`` -> (FakeIfetchLib, FakeLanesLib) for an n x MI355X node."""
    def install(n=1, ifetch_kw=None, **kw):
        lib, ilib, llib = FakeDiagLib(n=n, **kw), FakeIfetchLib(n=n, **(ifetch_kw or {})), FakeLanesLib(n=n)
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(ifetch, "lib", lambda: ilib)
        monkeypatch.setattr(lanes, "lib", lambda: llib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return ilib, llib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}
BOTH = ["ifetch_walk0", "ifetch_branch0"]


def test_off_by_default_and_on_when_asked(node):
    ilib, llib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and ilib.calls == []
    assert diag.run_devices(1, [0]).keys() == {0} and ilib.calls == []
    res = diag.run(1, 0, extra=("ifetch",))
    assert list(res)[-1] == "ifetch" and set(res) == LEVEL1 | {"ifetch"} and ilib.calls == BOTH
    r = res["ifetch"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["blocks"] == {"walk": 1024, "branch": 1024}
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "parts", "ms", "wall_s", "detail"}
    assert r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["parts"]) == ifetch.PARTS
    walk, br = r["parts"]["walk"], r["parts"]["branch"]
    assert walk["steps"] == 512 and list(walk["rows"]) == ["nb8", "nb64", "nb256", "nb1024"]
    for name, row in walk["rows"].items():
        assert set(row) == {"nb", "footprint_bytes", "blocks_visited", "errors", "first_bad", "ms", "ns_per_block"}
        assert ifetch.row_name(row["nb"]) == name and row["blocks_visited"] == row["nb"] and row["errors"] == 0
        assert row["first_bad"] is None and row["ns_per_block"] > 0
        assert row["footprint_bytes"] == FakeIfetchLib.BLOCK_BYTES * row["nb"]
    assert walk["rows"]["nb1024"]["footprint_bytes"] >= ifetch.FLOOR_BYTES
    assert br["iters"] == 1024 and tuple(br["ops"]) == ifetch.OPS
    for row in br["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "gops"} and row["errors"] == 0 and row["gops"] > 0
    json.dumps(r)
    assert llib.calls == []
    both = diag.run(1, 0, extra=("lanes", "ifetch"))  # the opt-in tests combine
    assert list(both)[-2:] == ["lanes", "ifetch"] and llib.calls == ["lanes0"] and ilib.calls == BOTH * 2
    assert diag.run(0, 0, extra=("ifetch",)).keys() == {"ifetch"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("ifetch" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["ifetch"] and "ifetch" not in diag.REFERENCE_RATES
    assert "ifetch" not in diag.DMA_TESTS | diag.SHARED_TESTS and "ifetch_test" in diag._UNSCALED
    line = diag._summary("ifetch", r)
    assert "walk 4 footprints (4-456 KiB of code) x 512 blocks per wave" in line
    assert "10 branch ops x 1024 steps on 1024 SIMDs of 8 XCDs, 0 wrong words" in line


def test_a_wrong_word_fails_the_gpu_and_names_the_simd(node):
    node(4, {"bad": {(2, "walk", 256): 3}})
    r = diag.run(1, 2, extra=("ifetch",))["ifetch"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == "3 wrong words in the walk over 256 blocks on xcd5/se1/cu7/simd2"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"]
    bad = r["parts"]["walk"]["rows"]["nb256"]["first_bad"]
    assert bad == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "word": "x", "path": 0, "got": "0x1fe7c5ed",
                   "want": "0x1fe7c4ed"}
    assert r["parts"]["walk"]["rows"]["nb64"]["errors"] == 0 and r["parts"]["branch"]["errors"] == 0
    assert diag.run(1, 1, extra=("ifetch",))["ifetch"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_ifetch=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag ifetch failed ("))
    assert "3 wrong words in the walk over 256 blocks on xcd5/se1/cu7/simd2" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["ifetch"])
    assert "FAIL" in line and "3 wrong words" in line and "xcd5/se1/cu7/simd2" in text


def test_a_wrong_branch_word_and_the_hooks_on_the_fake(node):
    k = ifetch.OPS.index("s_swappc_b64")
    node(2, {"bad": {(1, "branch", k): 2}})
    r = ifetch.ifetch_test(1)
    assert r["pass"] is False and r["detail"] == "2 wrong words in s_swappc_b64 on xcd5/se1/cu7/simd2"
    assert r["parts"]["branch"]["ops"]["s_swappc_b64"]["first_bad"] == {
        "where": "xcd5/se1/cu7/simd2", "chain": 1, "got": "0x1fe7c5ed", "want": "0x1fe7c4ed"}
    assert r["parts"]["walk"]["errors"] == 0
    r = ifetch.ifetch_test(0, inject_part="walk", inject_row=64, inject_block=3)
    assert r["errors"] == 1 and [k for k, v in r["parts"]["walk"]["rows"].items() if v["errors"]] == ["nb64"]
    r = ifetch.ifetch_test(0, inject_part="branch", inject_block=3)  # the part's first row by default
    assert r["errors"] == 1 and [k for k, v in r["parts"]["branch"]["ops"].items() if v["errors"]] == ["s_branch"]
    r = ifetch.ifetch_test(0, parts=("branch",), ops=("s_call_b64",))
    assert tuple(r["parts"]) == ("branch",) and tuple(r["parts"]["branch"]["ops"]) == ("s_call_b64",)


def test_a_refused_call_is_a_failed_result_and_a_missing_library_is_raised(node, monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native
    node(1)
    monkeypatch.setitem(diag._TESTS, "ifetch", ("ifetch_test", {"steps": 0}))
    r = diag.run(1, 0, extra=("ifetch",))["ifetch"]
    assert r["pass"] is False and "ifetch failed (-2)" in r["detail"] and "steps 1..2^16" in r["detail"]
    monkeypatch.setitem(diag._TESTS, "ifetch", ("ifetch_test", {"steps": 8}))  # a walk that cannot cover its blocks
    r = diag.run(1, 0, extra=("ifetch",))["ifetch"]
    assert r["pass"] is False and "ifetch failed (-2)" in r["detail"] and "visit fewer than 256 blocks" in r["detail"]
    for kw in (dict(parts=("walk",), inject_part="branch"), dict(nbs=(8, 8)), dict(nbs=(0,)), dict(nbs=(1025,)),
               dict(ops=("no_such_op",)), dict(inject_part="walk", inject_row=9), dict(parts=("fetch",)),
               dict(inject_part="branch", inject_row="s_nop")):
        with pytest.raises(ValueError):
            ifetch.ifetch_test(0, **kw)
    monkeypatch.undo()
    lib = FakeDiagLib(n=1)
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(ifetch, "_lib", None)
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    with pytest.raises(native.NativeUnavailable):
        diag.run(1, 0, extra=("ifetch",))
    assert set(diag.run(1, 0)) == LEVEL1  # who does not ask needs no library


@pytest.mark.parametrize("isolation", ("thread", "process"))
def test_an_agent_cycle_publishes_it_for_every_gpu_only_when_asked(node, isolation):
    bad = {"bad": {(5, "walk", 8): 1}}
    node(8, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 8, "ifetch": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=8, diag_timeout=60, diag_when="always", isolation=isolation,
              diag_setup=setup)
    rep = A.Agent("n8", diag_ifetch=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"ifetch"}, (d, g["diag"].keys())
        assert g["diag"]["ifetch"]["pass"] is (d != 5), (d, g["diag"]["ifetch"])
    assert "1 wrong words in the walk over 8 blocks" in rep["gpus"][5]["diag"]["ifetch"]["detail"]  # each child its own GPU
    json.dumps(rep)
    rep = A.Agent("n8", diag_ifetch=True, diag_lanes=True, **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 | {"lanes", "ifetch"} for g in rep["gpus"])
    rep = A.Agent("n8", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"])
    assert rep["state"] == H.HEALTHY


def test_the_flags(node, capsys, monkeypatch):
    ilib, llib = node(2)
    assert diag.main(["--level", "1", "--ifetch", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["ifetch", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(ilib.calls) == ["ifetch_branch0", "ifetch_branch1", "ifetch_walk0", "ifetch_walk1"] and llib.calls == []
    assert diag.main(["--level", "1"]) == 0
    assert "ifetch" not in capsys.readouterr().out and len(ilib.calls) == 4
    assert diag.main(["--level", "1", "--lanes"]) == 0
    assert "ifetch" not in capsys.readouterr().out and len(ilib.calls) == 4 and len(llib.calls) == 2
    seen = []
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--level", "1", "--ifetch", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--lanes", "--ifetch", "--duration", "0.001"]) == 0
    assert diag.main(["--level", "1", "--duration", "0.001"]) == 0
    assert seen == [("ifetch",), ("lanes", "ifetch"), None]
    capsys.readouterr()
    monkeypatch.undo()
    ilib, llib = node(1)
    b = diag.burn_in(1, [0], 0.0, extra=("ifetch",))
    assert b["pass"] and b["rounds"] == 1 and ilib.calls == BOTH
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--ifetch"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and ilib.calls == BOTH * 2
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(ilib.calls) == 4 and llib.calls == []
    assert A.build_parser().parse_args(["--node", "n", "--diag-ifetch"]).diag_ifetch is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_ifetch is False
    for main, flag in ((diag.main, "--ifetch"), (node_cycle.main, "--ifetch"), (A.main, "--diag-ifetch")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- 6. build --------------------------------------------------------------------------------------------------

def test_the_build_has_an_ifetch_target():
    t = B._targets()
    assert "ifetch" in t and t["ifetch"]["out"].endswith("libmi355x_ifetch.so")
    assert t["ifetch"]["cmd"] == t["xgmi"]["cmd"] and t["ifetch"]["headers"][0].endswith("ifetch_ref.h")
    assert [os.path.basename(h) for h in t["ifetch"]["headers"][1:]] == ["hip_host.h", "simd_report.h", "op_list.h"]
    assert "libmi355x_ifetch.so" in B.__doc__
    with open(os.path.join(CSRC, "ifetch.hip")) as f:
        src = f.read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../common/hip_host.h", "../common/op_list.h", "../common/simd_report.h",
                                                       "ifetch_ref.h"]
    out = t["ifetch"]["out"]
    if not os.path.exists(out):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(out)  # the tree's own build: the one large kernel is compiled once, by build()
    for name in ifetch._signatures():
        getattr(L, name)  # AttributeError: not exported
