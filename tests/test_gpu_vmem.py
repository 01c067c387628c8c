"""libmi355x_vmem.so on an MI355X: one application of every op held against an independent model word for word, the
four parts clean at the smallest shapes that can still go wrong and at the default grid, every self-check hook with
its exact count, and the opt-in wiring up to ``mi355x-diag --vmem``.

These tests plant wrong values in data; none provokes a GPU fault: every address any lane forms, the ones the range
check must reject included, lies inside a buffer the library allocated.  No rate and no ``l1_gain`` is asserted: they
are reported (profiles/vmem_mi355x.json) and never judged.

The model is tests/vmem_model.py, written from the instructions' definitions; tests/test_vmem_cpu.py holds
csrc/vmem/vmem_ref.h, which the library's own walks use, against the same model."""
import json
import random
import re
import subprocess
import sys

import pytest

import vmem_model as M

pytestmark = pytest.mark.gpu

MEM_WORDS = 4096  # 16 KiB: past a 4 KiB boundary, room for the immediates
ROWS = 4          # x 64 lanes = 256 offsets per op
# two sub-dword loads, an saddr form with an immediate, a buffer form with an index, and two stores
HOOKED = ("global_load_sbyte", "buffer_load_sshort", "global_load_dwordx4_saddr_m4096", "buffer_load_dword_idxen",
          "global_store_byte_d16_hi", "buffer_store_dwordx3")
SIMD = r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]"


@pytest.fixture(scope="module")
def vmem():
    from k8s_gpu_node_checker_amd.ops import vmem as vm
    assert vm.device_count() >= 1
    return vm


def _clean(r):
    assert r["pass"] is True and r["errors"] == 0 and r["detail"] == "", r["detail"]
    assert "bad_simds" not in r and "bad_cus" not in r
    for part in (r["ops"], r["bounds"]["rows"], r["ldsdma"]["forms"]):
        assert all(row["errors"] == 0 and row["first_bad"] is None for row in part.values())
    assert r["l1"]["errors"] == 0 and r["l1"]["first_bad"] is None


def _load_offsets(op, rng, nbytes):
    """ROWS x 64 offsets: the edges (the lowest, the last element, around a 64-byte and a 4 KiB boundary), then seeded
    random ones; the soffset form takes one address per row."""
    size, al = M.size(op), M.align(op)
    lo, hi = -(-M.low(op) // al) * al, (nbytes - size - M.room_above(op)) // al * al
    edges = [lo, hi] + [b + d for b in (64, 4096, 8192) for d in (-al, 0, al) if lo <= b + d <= hi]
    offs = [edges[i] if i < len(edges) else rng.randrange(lo, hi + 1, al) for i in range(64 * ROWS)]
    if op.endswith("_soffset"):
        offs = [offs[64 * (i // 64)] for i in range(len(offs))]
    return offs


@pytest.mark.parametrize("op", __import__("k8s_gpu_node_checker_amd.ops.vmem", fromlist=["OPS"]).LOADS)
def test_one_application_of_every_load_matches_the_model_word_for_word(vmem, op):
    rng = random.Random(op)
    words = [rng.choice((0x00, 0x7f, 0x80, 0xff)) | rng.getrandbits(24) << 8 if i % 3 else rng.getrandbits(32)
             for i in range(MEM_WORDS)]
    mem = b"".join(w.to_bytes(4, "little") for w in words)
    offs = _load_offsets(op, rng, len(mem))
    preset = [rng.choice((0, 0xffffffff, 0xa5a55a5a, rng.getrandbits(32))) for _ in range(4 * len(offs))]
    got = vmem.apply(op, words, offs, preset)
    want = [w for i, off in enumerate(offs) for w in M.load(op, mem, off, preset[4 * i:4 * i + 4])]
    wrong = [(i // 4, offs[i // 4], hex(got[i]), hex(want[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (op, len(wrong), wrong[:4])


@pytest.mark.parametrize("op", __import__("k8s_gpu_node_checker_amd.ops.vmem", fromlist=["OPS"]).STORES)
def test_one_application_of_every_store_leaves_the_models_bytes(vmem, op):
    """Lane l stores inside its own 64 bytes (cell l + 1: cell 0 and the last are guard cells), ROWS times."""
    rng = random.Random(op)
    words = [rng.getrandbits(32) for _ in range(16 * 66)]
    mem = bytearray(b"".join(w.to_bytes(4, "little") for w in words))
    size, al = M.size(op), M.align(op)
    offs = [64 * (i % 64 + 1) + rng.choice((0, (64 - size) // al * al, rng.randrange(0, 64 - size + 1, al)))
            for i in range(64 * ROWS)]
    data = [rng.choice((0, 0xffffffff, 0x807f00ff, rng.getrandbits(32))) for _ in range(4 * len(offs))]
    got = vmem.apply(op, words, offs, data)
    for i, off in enumerate(offs):
        M.store(op, mem, off, data[4 * i:4 * i + 4])
    want = [int.from_bytes(mem[4 * i:4 * i + 4], "little") for i in range(len(words))]
    wrong = [(4 * i, hex(got[i]), hex(want[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (op, len(wrong), wrong[:4])


def test_a_lane_at_num_records_reads_zero_and_its_store_is_dropped(vmem):
    """The range check one instruction at a time: a raw descriptor of 512 bytes and a structured one of 32 elements over
    1 KiB; lanes 0..31 in range (the last dword and the last element included), lanes 32..63 at num_records (lane 32
    exactly) and past it."""
    words = [0x01010101 * (i % 251 + 1) for i in range(256)]
    raw = [16 * l for l in range(64)]
    for op, offs in (("buffer_load_dword", [o + 12 if o < 512 else o for o in raw]), ("buffer_load_dwordx4", raw),
                     ("buffer_load_dword_idxen", raw)):
        got = vmem.apply(op, words, offs, None, num_records=32 if "idxen" in op else 512)
        n = 4 if "x4" in op else 1
        for l in range(64):
            want = words[offs[l] // 4:offs[l] // 4 + n] if l < 32 else [0] * n
            assert got[4 * l:4 * l + n] == want, (op, l, got[4 * l:4 * l + 4])
    for op in ("buffer_store_dword", "buffer_store_dwordx4", "buffer_store_dword_idxen"):
        data = [0xD0000000 | (l << 8) | j for l in range(64) for j in range(4)]
        got = vmem.apply(op, words, raw, data, num_records=32 if "idxen" in op else 512)
        want = list(words)
        for l in range(32):
            for j in range(4 if "x4" in op else 1):
                want[raw[l] // 4 + j] = data[4 * l + j]
        assert got == want, (op, [(i, hex(got[i]), hex(want[i])) for i in range(256) if got[i] != want[i]][:4])


def test_one_workgroup_two_steps_is_clean(vmem):
    r = vmem.vmem_test(0, blocks=1, iters=2, reps=1)
    print(json.dumps({k: v for k, v in r.items() if k not in ("ops", "bounds", "ldsdma")}))
    _clean(r)
    assert r["blocks"] == 1 and r["simds"] >= 4 and r["xcds"] >= 1 and tuple(r["ops"]) == vmem.OPS  # a launch: one CU


def test_nine_workgroups_share_an_xcd_and_small_slices_are_clean(vmem):
    r = vmem.vmem_test(0, blocks=9, iters=3, reps=1, slice_bytes=1024, passes=2)
    _clean(r)
    assert r["blocks"] == 9 and r["xcds"] <= 8 and r["l1"]["slice_bytes"] == 1024 and r["l1"]["passes"] == 2
    assert r["bounds"]["num_records_bytes"] == 4096 and tuple(r["bounds"]["rows"]) == vmem.BOUNDS_ROWS


def test_the_default_grid_is_clean_on_every_xcd(vmem):
    from k8s_gpu_node_checker_amd.ops import diag
    r = vmem.vmem_test(0, iters=2, reps=1, passes=2)
    print(json.dumps({k: v for k, v in r.items() if k not in ("ops", "bounds", "ldsdma")}))
    _clean(r)
    cus = diag.device_info(0)["cus"]
    assert r["blocks"] == 2 * cus and r["simds"] == 4 * cus
    if cus == 256:
        assert r["simds"] == 1024 and r["xcds"] == 8


@pytest.mark.parametrize("op", HOOKED)
def test_an_injected_flip_is_one_wrong_word_in_that_op_only(vmem, op):
    r = vmem.vmem_test(0, ops=HOOKED, blocks=8, iters=3, reps=1, passes=2, inject_op=op, inject_block=5)
    print(op, r["detail"], r["ops"][op])
    assert r["pass"] is False and r["errors"] == 1
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    bad = r["ops"][op]["first_bad"]
    assert bad["lane"] == 0 and bad["chain"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert re.fullmatch(SIMD, bad["where"]), bad
    assert r["detail"] == f"1 wrong words in {op} on {bad['where']}" and r["bad_simds"] == [f"{bad['where']} (1)"]
    assert r["bounds"]["errors"] == r["l1"]["errors"] == r["ldsdma"]["errors"] == 0


@pytest.mark.parametrize("op", HOOKED)
def test_a_skipped_access_shows_in_that_op_only(vmem, op):
    r = vmem.vmem_test(0, ops=HOOKED, blocks=8, iters=3, reps=1, passes=2, inject_op=op, inject_block=5, inject_skip_iter=1)
    print(op, r["detail"], r["ops"][op])
    assert r["pass"] is False and r["errors"] > 0
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op}
    assert r["ops"][op]["first_bad"]["got"] != r["ops"][op]["first_bad"]["want"]
    assert len(r["bad_simds"]) == 1  # one wave's words, and for a store its own region's bytes


def test_a_flipped_table_word_shows_in_every_load_that_reads_it(vmem):
    iters, word = 3, None
    loads = ("global_load_ubyte", "global_load_dwordx4", "buffer_load_dwordx3", "flat_load_dword", "buffer_load_sshort")
    for w in range(0, 16384, 7):  # a word that some of these walks read and some do not
        reads = {op: vmem.walk_reads(op, w, iters) for op in loads}
        if 0 < sum(reads.values()) < len(loads):
            word = w
            break
    assert word is not None
    r = vmem.vmem_test(0, ops=loads + ("global_store_dword",), blocks=2, iters=iters, reps=1, passes=2, inject_table_word=word)
    print(word, reads, r["detail"])
    assert {k for k, row in r["ops"].items() if row["errors"]} == {op for op, hit in reads.items() if hit}
    assert r["bounds"]["errors"] == r["l1"]["errors"] == r["ldsdma"]["errors"] == 0
    _clean(vmem.vmem_test(0, ops=loads, blocks=2, iters=iters, reps=1, passes=2))  # and the word was restored


def test_a_flipped_slice_word_is_passes_times_four_wrong_reads_on_one_cu(vmem):
    r = vmem.vmem_test(0, ops=HOOKED[:1], blocks=8, iters=2, reps=1, slice_bytes=2048, passes=3, inject_l1_block=6,
                       inject_l1_word=77)
    print(r["detail"], r["l1"])
    assert r["pass"] is False and r["errors"] == r["l1"]["errors"] == 3 * 4
    bad = r["l1"]["first_bad"]
    assert bad["slice"] == 6 and bad["word"] == 77 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert r["bad_cus"] == [bad["where"]] and re.fullmatch(SIMD.rsplit("/", 1)[0], bad["where"])
    assert sum(int(s.split("(")[1][:-1]) for s in r["bad_simds"]) == 12
    assert r["bounds"]["errors"] == r["ldsdma"]["errors"] == 0 and r["ops"][HOOKED[0]]["errors"] == 0


def test_a_leaking_descriptor_shows_in_every_bounds_row(vmem):
    blocks, n = 2, 4096
    r = vmem.vmem_test(0, ops=HOOKED[:1], blocks=blocks, iters=2, reps=1, passes=2, inject_bounds_leak=True)
    print(r["detail"], {k: v["errors"] for k, v in r["bounds"]["rows"].items()})
    rows, waves = r["bounds"]["rows"], 4 * blocks
    # the 32 odd lanes of every wave are out of range in every round: n / 512 rounds, a raw dword row visits 4 dwords
    assert rows["load_raw_dword"]["errors"] == waves * 32 * (n // 512) * 4
    assert rows["load_raw_dwordx4"]["errors"] == rows["load_structured_dwordx4"]["errors"] == waves * 32 * (n // 512) * 4
    assert rows["load_structured_dword"]["errors"] == waves * 32 * (n // 512)
    for k, row in rows.items():
        assert row["errors"] > 0 and row["first_bad"]["byte"] >= n, (k, row)  # a leak lies in the second half
        if k.startswith("load"):
            assert int(row["first_bad"]["want"], 16) == 0 and int(row["first_bad"]["got"], 16) != 0
    assert r["errors"] == r["bounds"]["errors"] and r["l1"]["errors"] == r["ldsdma"]["errors"] == 0


def test_refused_calls(vmem):
    for kw in (dict(iters=0), dict(reps=0), dict(blocks=4, inject_op=vmem.OPS[0], inject_block=4),
               dict(iters=4, inject_op=vmem.OPS[0], inject_block=0, inject_skip_iter=4), dict(slice_bytes=3000),
               dict(slice_bytes=512), dict(passes=0), dict(bounds_bytes=512), dict(inject_table_word=1 << 14),
               dict(blocks=2, inject_l1_block=2), dict(blocks=8193)):
        with pytest.raises(RuntimeError, match=r"vmem failed \(-2\)"):
            vmem.vmem_test(0, ops=vmem.OPS[:1], **{"blocks": 2, "iters": 2, "reps": 1, "passes": 1, **kw})
    words = [0] * 64
    for op, offs, kw in (("global_load_dword", [256] * 64, {}), ("global_load_ushort", [1] * 64, {}),
                         ("global_load_dword_saddr_p4092", [0] * 64, {}), ("buffer_load_dword", [0] * 64, {"num_records": 257}),
                         ("buffer_load_dword", [0] * 64, {"stride": 16})):
        with pytest.raises(RuntimeError, match=r"vmem failed \(-2\)"):
            vmem.apply(op, words, offs, **kw)


def test_diag_run_carries_a_passing_vmem_result(vmem):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(0, 0, extra=("vmem",))
    assert list(res) == ["vmem"] and res["vmem"]["pass"] and res["vmem"]["errors"] == 0
    assert tuple(res["vmem"]["ops"]) == vmem.OPS and tuple(res["vmem"]["ldsdma"]["forms"]) == vmem.LDSDMA_FORMS


def test_the_cli_flag_carries_a_passing_vmem_result(repo):
    def run(*flags):
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag",
                            "--level", "1", "--device", "0", "--format", "json", *flags], capture_output=True, text=True,
                           timeout=300, cwd=repo)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    tests = run("--vmem")
    assert tests["vmem"]["pass"] and tests["vmem"]["errors"] == 0 and len(tests["vmem"]["ops"]) == 59
    assert "vmem" not in run()
