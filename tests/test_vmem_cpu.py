"""The vmem diagnostic on CPU: the model of csrc/vmem/vmem_ref.h (every load and store op, the walks' offsets, the
walks themselves, the bounds rows) against an independent implementation (tests/vmem_model.py) and hand-worked rows,
the C ABI of csrc/vmem/vmem.hip against ops/vmem.py and its fake, the instructions the kernels compile to, the opt-in
wiring on the fakes and the build target.  The kernels themselves run on an MI355X in tests/test_gpu_vmem.py."""
import ctypes
import functools
import inspect
import json
import os
import random
import re
import shutil
import subprocess
import tempfile

import pytest

import vmem_model as M
from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.models import health as H
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric, vmem
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeDiagLib, FakeFabricLib, FakeVmemLib, c_exports

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "vmem")
HIPCC = os.path.join(B.ROCM, "bin", "hipcc")
MEM_BYTES = 16384
PRESETS = (0, 0xffffffff, 0xa5a55a5a)

# Reads cases from stdin ("L op off p0" / "S op off d0 d1 d2 d3" over a memory given as the first line in hex) and
# prints what vmem_load() / vmem_store() make of them; then the op table, offsets of the walks for a few chain words,
# the walks' final words with and without a skipped step, and the slots of the bounds rows.
REF_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "vmem_ref.h"
int main() {
  static char line[1 << 16];
  std::vector<uint8_t> mem;
  if (!fgets(line, sizeof line, stdin)) return 2;
  for (const char* p = line; p[0] > ' ' && p[1] > ' '; p += 2) {
    const char b[3] = {p[0], p[1], 0};
    mem.push_back(static_cast<uint8_t>(strtoul(b, nullptr, 16)));
  }
  while (fgets(line, sizeof line, stdin)) {
    char kind;
    int op;
    unsigned off, d[4] = {0, 0, 0, 0};
    if (sscanf(line, "%c %d %u %x %x %x %x", &kind, &op, &off, &d[0], &d[1], &d[2], &d[3]) < 4) return 3;
    const int width = VMEM_OP_TABLE[op].width;
    if (kind == 'L') {
      uint32_t pre[4] = {d[0], d[1], d[2], d[3]}, out[4] = {0, 0, 0, 0};
      vmem_load(width, mem.data(), off, pre, out);
      printf("L %x %x %x %x\n", out[0], out[1], out[2], out[3]);
    } else {
      std::vector<uint8_t> copy(mem.begin(), mem.begin() + 256);
      const uint32_t data[4] = {d[0], d[1], d[2], d[3]};
      vmem_store(width, copy.data(), off, data);
      printf("S ");
      for (uint8_t b : copy) printf("%02x", b);
      printf("\n");
    }
  }
  std::vector<uint8_t> table(VMEM_TABLE_BYTES), image(VMEM_REGION), image2(VMEM_REGION), touched(VMEM_TABLE_BYTES);
  for (uint32_t i = 0; i < VMEM_TABLE_BYTES / 4; ++i) {
    const uint32_t w = vmem_word(i, 7);
    for (int k = 0; k < 4; ++k) table[4 * i + k] = static_cast<uint8_t>(w >> (8 * k));
  }
  for (int op = 0; op < VMEM_OPS; ++op) {
    const VmemOpInfo& t = VMEM_OP_TABLE[op];
    printf("op %d %s %d %d %d %s%s %d %d %d\n", op, t.name, t.width, t.form, t.imm, t.insn, t.mods, vmem_bytes(t.width),
           vmem_regs(t.width), vmem_is_store(op));
    printf("off %d", op);
    for (uint32_t x = 0; x < 4000; ++x)
      printf(" %u", vmem_off(op, vmem_mix32(x), vmem_is_store(op) ? VMEM_CELL : VMEM_TABLE_BYTES));
    printf("\n");
    uint32_t a[VMEM_WAVE * VMEM_CHAINS], b[VMEM_WAVE * VMEM_CHAINS], c[VMEM_WAVE * VMEM_CHAINS];
    std::fill(touched.begin(), touched.end(), 0);
    vmem_expected(op, vmem_op_seed(5, op), 3, -1, table.data(), a, image.data(), touched.data());
    vmem_expected(op, vmem_op_seed(5, op), 3, -1, table.data(), b, image2.data(), nullptr);
    vmem_expected(op, vmem_op_seed(5, op), 3, 1, table.data(), c, image2.data(), nullptr);
    int same = 0, differ = 0, guards = 0, changed = 0, read = 0;
    for (int i = 0; i < VMEM_WAVE * VMEM_CHAINS; ++i) same += a[i] == b[i], differ += a[i] != c[i];
    if (vmem_is_store(op))
      for (uint32_t i = 0; i < VMEM_REGION; ++i) {
        const bool guard = i < VMEM_CELL || i >= VMEM_REGION - VMEM_CELL;
        guards += guard && image[i] == vmem_background(vmem_op_seed(5, op), i);
        changed += !guard && image[i] != vmem_background(vmem_op_seed(5, op), i);
      }
    for (uint8_t t8 : touched) read += t8;
    printf("walk %d %d %d %d %d %d\n", op, same, differ, guards, changed, read);
  }
  printf("soff");
  for (uint32_t x = 0; x < 600; ++x) printf(" %u", vmem_soff(vmem_mix32(x)));
  printf("\nbounds %u", vmem_bounds_rounds(4096));
  for (uint32_t k = 0; k < vmem_bounds_rounds(4096); ++k)
    for (int lane = 0; lane < VMEM_WAVE; ++lane) printf(" %u", vmem_bounds_slot(4096, lane, k));
  printf("\nnonzero %d\n", vmem_bounds_word(1, 2) != 0 && vmem_bounds_data(1, 2, 3, 0) != 0);
  for (int lane = 0; lane < VMEM_WAVE; ++lane)
    if (vmem_dma_partner(lane) == lane || vmem_dma_slot(9, lane, 3) >= VMEM_TABLE_BYTES / 16) return 4;
  printf("ok %d\n", VMEM_OPS);
  return 0;
}
"""


def _memory():
    """16 KiB: random bytes with every fourth run of bytes drawn from the sign and carry edges."""
    rng = random.Random(20260)
    return bytes(rng.choice((0x00, 0x7f, 0x80, 0xff)) if (i // 3) % 4 == 0 else rng.getrandbits(8) for i in range(MEM_BYTES))


@functools.lru_cache(maxsize=None)
def _cases():
    """[(kind, op name, offset, registers)]: per op the edge offsets x the presets, then seeded random rows."""
    rng = random.Random(7)
    cases = []
    for op in vmem.OPS:
        size, al = M.size(op), M.align(op)
        if op in vmem.LOADS:
            last = (MEM_BYTES - size) // al * al
            edges = [0, last] + [b + d for b in (64, 4096) for d in (-al, 0, al)]
            rows = [(off, [p, p ^ 0x1111, 0, 0]) for off in edges for p in PRESETS]
            rows += [(rng.randrange(0, last + 1, al), [rng.getrandbits(32) for _ in range(4)]) for _ in range(40)]
            cases += [("L", op, off, regs) for off, regs in rows]
        else:
            last = (256 - size) // al * al
            edges = [0, last] + [64 + d for d in (-al, 0, al)]
            rows = [(off, [p, ~p & 0xffffffff, 0x01020304, 0xf1f2f3f4]) for off in edges for p in PRESETS + (0x807f00ff,)]
            rows += [(rng.randrange(0, last + 1, al), [rng.getrandbits(32) for _ in range(4)]) for _ in range(40)]
            cases += [("S", op, off, regs) for off, regs in rows]
    return cases


def _ref_program(sanitize):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    text = _memory().hex() + "\n" + "".join(
        f"{k} {vmem.OPS.index(op)} {off} {regs[0]:x} {regs[1]:x} {regs[2]:x} {regs[3]:x}\n" for k, op, off, regs in _cases())
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "vmem_ref.cpp"), os.path.join(tmp, "vmem_ref")
        with open(src, "w") as f:
            f.write(REF_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


@functools.lru_cache(maxsize=None)
def _model():
    rc, out = _ref_program(False)
    assert rc == 0 and out.strip().endswith(f"ok {len(vmem.OPS)}"), out[-2000:]
    m = {"results": [], "ops": {}, "off": {}, "walk": {}}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "L":
            m["results"].append([int(x, 16) for x in f[1:]])
        elif f[0] == "S":
            m["results"].append(bytes.fromhex(f[1]))
        elif f[0] == "op":
            m["ops"][int(f[1])] = dict(name=f[2], width=int(f[3]), form=int(f[4]), imm=int(f[5]), insn=" ".join(f[6:-3]),
                                       bytes=int(f[-3]), regs=int(f[-2]), store=int(f[-1]))
        elif f[0] in ("off", "walk"):
            m[f[0]][int(f[1])] = [int(x) for x in f[2:]]
        elif f[0] in ("soff", "bounds"):
            m[f[0]] = [int(x) for x in f[1:]]
        elif f[0] == "nonzero":
            m["nonzero"] = int(f[1])
    return m


# --- the model ---------------------------------------------------------------------------------------------------

def test_every_op_matches_the_independent_model_over_edges_and_random_rows():
    mem, cases, results = _memory(), _cases(), _model()["results"]
    assert len(results) == len(cases) and {c[1] for c in cases} == set(vmem.OPS)
    for (kind, op, off, regs), got in zip(cases, results):
        if kind == "L":
            assert got == M.load(op, mem, off, regs), (op, off, [hex(r) for r in regs], [hex(g) for g in got])
        else:
            want = bytearray(mem[:256])
            M.store(op, want, off, regs)
            assert got == bytes(want), (op, off, [hex(r) for r in regs])
            assert sum(a != b for a, b in zip(got, mem[:256])) <= M.size(op)  # no byte beyond the op's own changes


def test_hand_worked_rows():
    """Worked on paper from the ISA's definitions, through the independent model and through vmem_ref.h."""
    # an sbyte of 0x80 is sign-extended to 32 bits whatever the register held; a ubyte is zero-extended.  (The D16
    # loads the issue names here were removed from the library: the device did not keep the other half.)
    assert M.load("global_load_sbyte", b"\x80", 0, [0x12345678]) == [0xffffff80, 0, 0, 0]
    assert M.load("buffer_load_ubyte", b"\x80", 0, [0x12345678]) == [0x00000080, 0, 0, 0]
    assert M.load("global_load_sshort", b"\x00\x80", 0, [0]) == [0xffff8000, 0, 0, 0]
    # a store_byte_d16_hi writes bits 23:16 of the data register, one byte, and leaves its neighbours
    mem = bytearray(b"\x11\x22\x33\x44")
    M.store("global_store_byte_d16_hi", mem, 2, [0xAABBCCDD])
    assert mem == b"\x11\x22\xbb\x44"
    mem = bytearray(b"\x11\x22\x33\x44")
    M.store("buffer_store_short_d16_hi", mem, 2, [0xAABBCCDD])
    assert mem == b"\x11\x22\xbb\xaa"
    # the same rows through vmem_ref.h: the first memory byte that is 0x80, with the case list's presets
    raw, cases, results = _memory(), _cases(), _model()["results"]
    hit = [(c, r) for c, r in zip(cases, results) if c[1] == "global_load_sbyte" and raw[c[2]] == 0x80]
    assert hit
    for (_, _, off, regs), got in hit:
        assert got == [0xffffff80, 0, 0, 0], (off, regs)
    # a structured index at num_records: with 4 KiB covered, element 256 is the first one out of range, and round 0's
    # lane 1 is exactly there while lane 0 starts the first half
    b = _model()["bounds"]
    rounds, slots = b[0], b[1:]
    assert rounds == 8 and slots[0] == 0 and slots[1] == 4096 // 16


def test_the_walks_offsets_are_aligned_inside_their_span_and_spread():
    m = _model()
    for k, t in m["ops"].items():
        name, offs = t["name"], m["off"][k]
        size, al = M.size(name), M.align(name)
        assert t["bytes"] == size and t["store"] == (name in vmem.STORES)
        span = 64 if t["store"] else vmem.TABLE_BYTES
        assert all(o % al == 0 and 0 <= o <= span - size for o in offs), name
        if not t["store"]:
            # the address parts the instruction adds up stay inside the table too
            if t["imm"] > 0:
                assert min(offs) >= 4096, name
            if t["imm"] < 0:
                assert max(offs) + size + 4096 <= span, name
            if name.endswith("offen_soffset_p4095"):
                assert min(offs) - 4095 - max(m["soff"]) >= 0 and all(s % 4 == 1 for s in m["soff"])
        assert len(set(offs)) >= min(200, (span - size) // al // 2), name  # the offsets spread over the span


def test_the_walks_are_deterministic_notice_a_skipped_step_and_keep_the_guard_cells():
    m = _model()
    for k, t in m["ops"].items():
        same, differ, guards, changed, read = m["walk"][k]
        assert same == 256 and differ >= 1, t["name"]  # a skipped access changes what the wave ends with
        if t["store"]:
            assert guards == 128 and changed > 0 and read == 0, t["name"]
        else:
            assert read >= t["bytes"], t["name"]
    assert m["nonzero"] == 1


def test_the_bounds_rows_cover_every_slot_of_both_halves_once():
    b = _model()["bounds"]
    rounds, slots = b[0], b[1:]
    assert len(slots) == rounds * 64 and sorted(slots) == list(range(2 * 4096 // 16))
    for k in range(rounds):
        row = slots[64 * k:64 * k + 64]
        assert all((s >= 256) == bool(lane & 1) for lane, s in enumerate(row))  # both kinds in one wave-instruction
    assert 255 in slots and 256 in slots  # the last element in range and the first out of range


def test_the_reference_is_clean_under_the_host_sanitizers():
    rc, out = _ref_program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0 and out.strip().endswith(f"ok {len(vmem.OPS)}"), out[-3000:]
    assert len(re.findall(r"^walk ", out, re.M)) == len(vmem.OPS)


# --- ABI -------------------------------------------------------------------------------------------------------

def test_exports_match_the_signature_table_and_the_fake():
    exports, sig = c_exports("vmem"), vmem._signatures()
    assert set(exports) == set(sig) == {"vmem_last_error", "vmem_device_count", "vmem_slots", "vmem_ops", "vmem_loads",
                                        "vmem_walk_reads", "vmem_walks", "vmem_bounds", "vmem_l1", "vmem_ldsdma_forms",
                                        "vmem_ldsdma_name", "vmem_ldsdma", "vmem_apply"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        fake = list(inspect.signature(getattr(FakeVmemLib, name)).parameters)[1:]
        assert len(fake) == len(params), (name, fake, params)
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
        assert [p.split()[-1].lstrip("*") for p in params] == fake, name  # the fake names its arguments as the C does
    assert len(exports["vmem_walks"]) == 16 and len(exports["vmem_apply"]) == 10
    with open(os.path.join(CSRC, "vmem_ref.h")) as f:
        ref = f.read()
    assert re.findall(r"^  X\((\w+), VW_", ref, re.M) == list(vmem.OPS)  # the C op lists, in order
    assert [t["name"] for _, t in sorted(_model()["ops"].items())] == list(vmem.OPS)
    assert FakeVmemLib.OPS == len(vmem.OPS) and FakeVmemLib.LOADS == len(vmem.LOADS)
    assert tuple(f.decode() for f in FakeVmemLib.FORMS) == vmem.LDSDMA_FORMS
    assert all(f'"{f}"' in open(os.path.join(CSRC, "vmem.hip")).read() for f in vmem.LDSDMA_FORMS)


# --- instructions ----------------------------------------------------------------------------------------------

def test_every_op_compiles_to_its_native_instruction_without_scratch_or_stray_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-save-temps",
                        os.path.join(CSRC, "vmem.hip"), "-o", os.path.join(tmp, "vmem.o")], check=True,
                       capture_output=True, text=True, cwd=tmp)
        asm = [f for f in os.listdir(tmp) if f.endswith(".s")]
        assert len(asm) == 1, os.listdir(tmp)
        with open(os.path.join(tmp, asm[0])) as f:
            text = f.read()
    walked = {int(k): body for k, body in re.findall(r"^_ZN\w*11walk_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text, re.M | re.S)}
    applied = {int(k): body for k, body in re.findall(r"^_ZN\w*12apply_kernelILi(\d+)E\w*:(.*?)^\.Lfunc_end", text, re.M | re.S)}
    assert sorted(walked) == sorted(applied) == list(range(len(vmem.OPS)))
    ops = _model()["ops"]
    for k, name in enumerate(vmem.OPS):
        insn = ops[k]["insn"].split()  # the mnemonic, then its cache policy
        for body, times in ((walked[k], 4), (applied[k], 1)):
            # the statements written in asm are the lines without the compiler's leading tab
            own = [ln for ln in re.findall(r"^((?:global|flat|buffer)_\w+ .*)$", body, re.M)
                   if not (name in vmem.STORES and ln.startswith("global_load_dwordx4") and ln.endswith("sc1"))]
            assert len(own) == times and all(ln.split()[0] == insn[0] for ln in own), (name, own)
            for ln in own:
                assert ln.split()[-len(insn[1:]):] == insn[1:] if insn[1:] else not re.search(r" (sc0|sc1|nt)$", ln), (name, ln)
                if ops[k]["imm"]:
                    assert f"offset:{ops[k]['imm']}" in ln, (name, ln)
                form = ops[k]["form"]  # VmemForm: 3 offen, 4 idxen, 5 idxen offen, 6 off + soffset, 7 offen + soffset
                assert ("offen" in ln.split()) == (form in (3, 5, 7)) and ("idxen" in ln.split()) == (form in (4, 5)), (name, ln)
        # a descriptor that is not wave-uniform would make the compiler loop over its values: there is no such loop
        assert "s_cbranch_execnz" not in walked[k] and "s_cbranch_execnz" not in applied[k], name
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}  # no kernel has scratch
    lds = re.findall(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)", text)
    assert lds and all((size == "4096") == ("ldsdma_kernel" in kernel) and size in ("0", "4096") for size, kernel in lds), lds
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}
    for form in ("global_load_lds_dword ", "global_load_lds_dwordx4 ", "offen lds"):
        assert form in text, form


# --- wiring on the fakes ---------------------------------------------------------------------------------------

@pytest.fixture
def node(monkeypatch):
    """``node(n, vmem_kw, **FakeDiagLib kwargs)`` -> FakeVmemLib for an n x MI355X node."""
    def install(n=1, vmem_kw=None, **kw):
        lib, vlib = FakeDiagLib(n=n, **kw), FakeVmemLib(n=n, **(vmem_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(vmem, "lib", lambda: vlib)
        monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
        monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=n))
        return vlib
    return install


LEVEL1 = {"gemm", "gemm_fp8", "hbm", "hbm_xcd", "mfma", "lds", "l2"}


def test_off_by_default_and_on_when_asked(node):
    vlib = node(1)
    assert set(diag.run(1, 0)) == LEVEL1 and vlib.calls == []
    res = diag.run(1, 0, extra=("vmem",))
    assert list(res)[-1] == "vmem" and set(res) == LEVEL1 | {"vmem"} and vlib.calls == ["vmem0"]
    r = res["vmem"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and r["iters"] == vmem.DEFAULT_ITERS
    assert set(r) == {"pass", "errors", "simds", "xcds", "blocks", "iters", "ops", "bounds", "l1", "ldsdma", "ms", "wall_s",
                      "detail"}
    assert r["blocks"] == 512 and r["simds"] == 1024 and r["xcds"] == 8 and tuple(r["ops"]) == vmem.OPS
    for row in r["ops"].values():
        assert set(row) == {"errors", "first_bad", "ms", "gops"}
        assert row["errors"] == 0 and row["first_bad"] is None and row["gops"] > 0
    assert tuple(r["bounds"]["rows"]) == vmem.BOUNDS_ROWS and tuple(r["ldsdma"]["forms"]) == vmem.LDSDMA_FORMS
    assert r["l1"]["slice_bytes"] == 8192 and r["l1"]["l1_gain"] == 2.0
    json.dumps(r)
    assert diag.run(0, 0, extra=("vmem",)).keys() == {"vmem"}
    # nothing about the levels moved, and the test has a revision stamp but no reference rate
    assert sorted(diag.LEVELS) == [0, 1, 2, 3] and not any("vmem" in t for t in diag.LEVELS.values())
    assert diag.KERNEL_REVISION["vmem"] and "vmem" not in diag.REFERENCE_RATES
    assert f"59 ops x {vmem.DEFAULT_ITERS} steps on 1024 SIMDs of 8 XCDs, 8 bounds rows, L1 8192 B x " in diag._summary("vmem", r)
    assert "4 LDS-DMA forms, 0 wrong words" in diag._summary("vmem", r)


def test_a_wrong_word_fails_the_gpu_and_names_the_simd(node):
    op = "buffer_load_sbyte"
    node(4, {"bad": {(2, vmem.OPS.index(op)): 3}})
    r = diag.run(1, 2, extra=("vmem",))["vmem"]
    assert r["pass"] is False and r["errors"] == 3
    assert r["detail"] == f"3 wrong words in {op} on xcd5/se1/cu7/simd2"
    assert r["bad_simds"] == ["xcd5/se1/cu7/simd2 (3)"] and r["bad_cus"] == ["xcd5/se1/cu7"]
    assert r["ops"][op]["first_bad"] == {"where": "xcd5/se1/cu7/simd2", "lane": 9, "chain": 1, "got": "0x4a82c74e",
                                         "want": "0x4a82c64e"}
    assert r["ops"]["global_load_dword"]["errors"] == 0 and r["ops"]["global_load_dword"]["first_bad"] is None
    assert diag.run(1, 1, extra=("vmem",))["vmem"]["pass"]
    ag = A.Agent("n4", source="fake", diag_level=1, expect_gpus=4, diag_timeout=60, diag_vmem=True)
    rep = ag.probe_once()
    v = H.evaluate_report(rep, 4)
    assert v.state == H.UNHEALTHY and (v.gpus_ok, v.gpus_seen) == (3, 4)
    reason = next(x for x in v.reasons if x.startswith("gpu2: diag vmem failed ("))
    assert f"3 wrong words in {op} on xcd5/se1/cu7/simd2" in reason
    text = diag.render_text({"devices": {2: {"info": {}, "tests": rep["gpus"][2]["diag"]}}, "pass": False})
    line = next(ln for ln in text.splitlines() if ln.split()[:1] == ["vmem"])
    assert "FAIL" in line and "3 wrong words" in line


def test_a_wrong_l1_read_names_the_cu(node):
    node(2, {"bad_l1": {1: 5}})
    r = diag.run(0, 1, extra=("vmem",))["vmem"]
    assert r["pass"] is False and r["errors"] == 5 and r["l1"]["errors"] == 5
    assert r["l1"]["first_bad"] == {"where": "xcd5/se1/cu7", "slice": 3, "word": 33, "got": "0x4a82c65e", "want": "0x4a82c64e"}
    assert r["detail"] == "5 wrong reads of the L1 slices, first word 33 of slice 3 on xcd5/se1/cu7"
    assert r["bad_cus"] == ["xcd5/se1/cu7"]


def test_refused_calls_and_the_injection_knobs_of_the_fake(node):
    node(1)
    with pytest.raises(ValueError):
        vmem.vmem_test(0, ops=("global_load_dword",), inject_op="flat_load_dword")
    with pytest.raises(ValueError):
        vmem.vmem_test(0, ops=("no_such_op",))
    with pytest.raises(ValueError):
        vmem.vmem_test(0, ops=("global_load_dword", "global_load_dword"))
    for kw in (dict(iters=0), dict(slice_bytes=3000), dict(bounds_bytes=100), dict(passes=0), dict(blocks=8193)):
        with pytest.raises(RuntimeError, match=r"vmem failed \(-2\)"):
            vmem.vmem_test(0, **kw)
    with pytest.raises(ValueError):
        vmem.apply("no_such_op", [0] * 64, [0] * 64)
    with pytest.raises(ValueError):
        vmem.apply("global_load_dword", [0] * 64, [0] * 63)
    r = vmem.vmem_test(0, ops=("global_load_dword", "flat_store_dword"), inject_op="flat_store_dword", inject_block=0)
    assert r["errors"] == 1 and list(r["ops"]) == ["global_load_dword", "flat_store_dword"]
    r = vmem.vmem_test(0, blocks=2, passes=3, inject_l1_block=1, inject_l1_word=7, inject_bounds_leak=True)
    assert r["l1"]["errors"] == 12 and all(row["errors"] > 0 for row in r["bounds"]["rows"].values())


def test_an_agent_cycle_publishes_it_only_when_asked(node):
    bad = {"bad": {(1, 0): 1}}
    node(2, bad)
    setup = ("k8s_gpu_node_checker_amd.testing.fake_native", "install", {"n": 2, "vmem": bad})
    kw = dict(source="fake", diag_level=1, expect_gpus=2, diag_timeout=60, diag_when="always", isolation="process",
              diag_setup=setup)
    rep = A.Agent("n2", diag_vmem=True, **kw).probe_once()
    for d, g in enumerate(rep["gpus"]):
        assert set(g["diag"]) == LEVEL1 | {"vmem"} and g["diag"]["vmem"]["pass"] is (d != 1), (d, g["diag"].keys())
    rep = A.Agent("n2", **kw).probe_once()
    assert all(set(g["diag"]) == LEVEL1 for g in rep["gpus"]) and rep["state"] == H.HEALTHY


def test_a_failing_device_among_run_devices(node):
    node(3, {"bad": {(1, 5): 2}})
    out = diag.run_devices(0, [0, 1, 2], extra=("vmem",))
    assert {d: tests["vmem"]["pass"] for d, tests in out.items()} == {0: True, 1: False, 2: True}
    assert out[1]["vmem"]["errors"] == 2 and "global_load_dwordx2" in out[1]["vmem"]["detail"]


def test_the_flags(node, capsys):
    vlib = node(2)
    assert diag.main(["--level", "1", "--vmem", "--format", "text"]) == 0
    text = capsys.readouterr().out
    assert sum(ln.split()[:2] == ["vmem", "pass"] for ln in text.splitlines()) == 2, text
    assert sorted(vlib.calls) == ["vmem0", "vmem1"]
    assert diag.main(["--level", "1"]) == 0
    assert "vmem" not in capsys.readouterr().out and len(vlib.calls) == 2
    vlib = node(1)
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric", "--vmem"]) == 0
    assert '"verdict":"healthy"' in capsys.readouterr().out and vlib.calls == ["vmem0"]
    assert node_cycle.main(["--devices", "0", "--level", "1", "--no-fabric"]) == 0
    capsys.readouterr()
    assert len(vlib.calls) == 1
    assert A.build_parser().parse_args(["--node", "n", "--diag-vmem"]).diag_vmem is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_vmem is False
    for main, flag in ((diag.main, "--vmem"), (node_cycle.main, "--vmem"), (A.main, "--diag-vmem")):
        with pytest.raises(SystemExit):
            main(["--help"])
        assert flag in capsys.readouterr().out, (main, flag)


# --- build -----------------------------------------------------------------------------------------------------

def test_the_build_has_a_vmem_target():
    t = B._targets()
    assert "vmem" in t and t["vmem"]["out"].endswith("libmi355x_vmem.so")
    assert t["vmem"]["cmd"] == t["xgmi"]["cmd"] and t["vmem"]["headers"][0].endswith("vmem_ref.h")
    assert "libmi355x_vmem.so" in B.__doc__
