"""libmi355x_hbmscan.so on an MI355X: the three kernels on the smallest tested set at which they can go wrong, every
hook seen to fire, the classifier on what the kernels recorded, and the opt-in wiring up to ``mi355x-diag --hbmscan``.

Unless a test says otherwise the set is 5 MiB + 48 bytes in 1 MiB chunks: six chunks, a last chunk of three words, a
grid tail in every launch.  One test runs 2 GiB (the size from which a read is taken to come from HBM); none asks for
more, and none for all free memory.  The expected words come from the Python model of tests/test_hbmscan_cpu.py.

These tests plant wrong values in data; none provokes a GPU fault.  No rate is asserted: the rates are reported
(profiles/hbmscan_mi355x.json) and never judged."""
import json
import subprocess
import sys

import pytest

from test_hbmscan_cpu import model_bit, model_kind, model_steps, model_want

pytestmark = pytest.mark.gpu

MIB, GIB = 1 << 20, 1 << 30
LIMIT = 5 * MIB + 48
WORDS = LIMIT // 16                 # 327,683
CHUNK_WORDS = MIB // 16
SMALL = dict(gib=LIMIT / GIB, chunk_mib=1)   # (exact: an integer over 2^30)
PHASES = ("addr", "invert", "random", "fade")
LAST_WRITE = {"addr": 1, "invert": 14, "random": 2, "fade": 1}


@pytest.fixture(scope="module")
def hs():
    from k8s_gpu_node_checker_amd.ops import hbmscan as h
    assert h.device_count() >= 1
    return h


def _clean(r, tested=LIMIT, chunks=6, cached=True):
    assert r["pass"] and r["errors"] == 0 and r["records"] == [] and r["hist"] == {} and r["finding"] == {"kind": "none"}, r
    assert r["complete"] and r["cached"] is cached and r["reached"] == {"phase": "fade", "step": 2}, r
    assert r["tested_bytes"] == tested and r["chunks"] == chunks, r
    assert all(p["errors"] == 0 and p["ms"] > 0 for p in r["phases"].values()), r
    assert ("cells are not proven" in r["detail"]) is cached


def _int128(lanes):
    return sum(x << (32 * i) for i, x in enumerate(lanes))


def test_a_clean_run_tests_the_plan_to_the_byte(hs):
    r = hs.hbmscan_test(0, **SMALL)
    print(json.dumps(r))
    _clean(r)
    assert r["planned_bytes"] == LIMIT and r["halved"] == 0 and r["alloc_failures"] == 0
    assert r["coverage"] == round(LIMIT / (r["total_gib"] * GIB), 4) or r["coverage"] < 1e-3
    assert r["free_gib"] <= r["total_gib"] and r["tested_gib"] == round(LIMIT / GIB, 6)


def test_the_index_carries_into_its_high_half(hs):
    base = (1 << 32) - 100
    _clean(hs.hbmscan_test(0, index_base=base, **SMALL))
    word, bit = 150, 33  # beyond the carry: global word 2^32 + 50; bit 33 is bit 1 of the index's high half
    r = hs.hbmscan_test(0, index_base=base, inject_flip=("addr", 0, word, bit), **SMALL)
    print(json.dumps(r))
    rec = r["records"][0]
    assert r["errors"] == 1 and rec["global_word"] == (1 << 32) + 50 and rec["offset"] == word * 16, r
    want = model_want("addr", 0, base + word, hs.DEFAULT_SEED)
    assert want[1] == 1 and int(rec["want"], 16) == _int128(want) and int(rec["got"], 16) == _int128(want) ^ (1 << bit)


@pytest.mark.parametrize("word", (0, WORDS - 1, 3 * CHUNK_WORDS), ids=("first", "last", "middle_chunk"))
@pytest.mark.parametrize("last", (False, True), ids=("first_write", "last_write"))
@pytest.mark.parametrize("phase", PHASES)
def test_a_flipped_bit_is_found_where_it_was_planted(hs, phase, last, word):
    step = LAST_WRITE[phase] if last else 0
    bit = (7 + 37 * PHASES.index(phase) + 64 * last + word) % 128
    r = hs.hbmscan_test(0, inject_flip=(phase, step, word, bit), **SMALL)
    print(phase, step, word, bit, json.dumps(r))
    assert not r["pass"] and r["errors"] == 1 and len(r["records"]) == 1 and r["complete"], r
    assert {p: v["errors"] for p, v in r["phases"].items()} == {p: int(p == phase) for p in PHASES}
    rec = r["records"][0]
    # the step after the write verifies it
    assert (rec["phase"], rec["step"]) == (phase, step + 1) and model_kind(phase, step + 1) != "write"
    assert (rec["chunk"], rec["chunk_offset"], rec["offset"]) == (word // CHUNK_WORDS, word % CHUNK_WORDS * 16, word * 16)
    want = _int128(model_want(phase, step, word, hs.DEFAULT_SEED))
    assert int(rec["want"], 16) == want and int(rec["got"], 16) == want ^ (1 << bit), rec
    direction = 1 - ((want >> bit) & 1)  # a 0 that reads 1 is direction 1
    assert r["hist"] == {str(2 * bit + direction): 1} and rec["flipped"] == [[bit, hs.DIRECTIONS[direction]]]
    assert r["finding"] == {"kind": "stuck_bit", "bit": bit, "direction": hs.DIRECTIONS[direction]}  # 1 of 1 flipped bits
    assert r["detail"].startswith(f"1 wrong 16-byte words; stuck bit {bit} ({hs.DIRECTIONS[direction]}); first at "
                                  f"+0x{rec['chunk_offset']:x} of chunk {rec['chunk']}")


@pytest.mark.parametrize("value", (0, 1))
def test_a_stuck_bit_is_counted_in_every_step_that_expects_the_other_value(hs, value):
    word, bit, passes = CHUNK_WORDS + 4321, 37, 2
    r = hs.hbmscan_test(0, inject_stuck=(word, bit, value), random_passes=passes, **SMALL)
    print(json.dumps(r))
    expected = {p: sum(model_bit(p, s - 1, word, hs.DEFAULT_SEED, bit) != value for s in range(model_steps(p, passes))
                       if model_kind(p, s) != "write") for p in PHASES}
    assert {p: v["errors"] for p, v in r["phases"].items()} == expected and r["errors"] == sum(expected.values())
    # one of addr's two verifying steps; of invert's twelve, those that expect the other value in lane 1's bit 5
    assert expected["addr"] == 1 and expected["invert"] == (5, 7)[value]
    assert r["finding"] == {"kind": "stuck_bit", "bit": bit, "direction": hs.DIRECTIONS[value]}
    assert all(rec["chunk"] == 1 and rec["chunk_offset"] == 4321 * 16 and rec["flipped"] == [[bit, hs.DIRECTIONS[value]]]
               for rec in r["records"]) and len(r["records"]) == r["errors"]
    assert r["hist"] == {str(2 * bit + value): r["errors"]}


@pytest.mark.parametrize("a, b, bit", ((1029, 1029 + (1 << 16), 16), (1029 + (1 << 16), 1029, 16), (1029, 1029 ^ 0b110000, None)))
def test_an_alias_names_both_words(hs, a, b, bit):
    r = hs.hbmscan_test(0, inject_alias=(a, b), **SMALL)
    print(json.dumps(r))
    assert r["errors"] == 1 and r["phases"]["addr"]["errors"] == 1, r
    rec = r["records"][0]
    assert (rec["phase"], rec["step"], rec["offset"]) == ("addr", 1, b * 16)
    assert int(rec["got"], 16) == _int128(model_want("addr", 0, a, 0)) and int(rec["want"], 16) == _int128(model_want("addr", 0, b, 0))
    assert r["finding"] == {"kind": "alias", "word": b, "holds": a, "bit": bit}
    assert f"alias: word {b:#x} held the content of word {a:#x}" in r["detail"]
    assert ("index bit 16" in r["detail"]) is (bit == 16)


def test_two_flips_in_one_span_are_a_region_and_in_two_chunks_scattered(hs):
    w = 2 * CHUNK_WORDS
    r = hs.hbmscan_test(0, inject_flip=[("invert", 1, w + 5, 3), ("random", 0, w + 60000, 90)], **SMALL)
    print(json.dumps(r))
    assert r["errors"] == 2 and len(r["hist"]) == 2 and [x["chunk"] for x in r["records"]] == [2, 2]
    assert r["finding"] == {"kind": "region", "chunk": 2, "span": 0, "span_bytes": 2 * MIB}
    r = hs.hbmscan_test(0, inject_flip=[("invert", 1, CHUNK_WORDS + 5, 3), ("random", 0, 4 * CHUNK_WORDS + 5, 90)], **SMALL)
    assert r["errors"] == 2 and [x["chunk"] for x in r["records"]] == [1, 4] and r["finding"] == {"kind": "scattered"}
    assert "2 wrong 16-byte words; scattered; first at +0x50 of chunk 1 (invert step 2)" in r["detail"]


def test_a_failed_allocation_is_halved_and_never_a_finding(hs):
    r = hs.hbmscan_test(0, fail_alloc_at=1, min_chunk_mib=0.25, **SMALL)
    print(json.dumps(r))
    _clean(r, chunks=7)  # the first chunk as two halves: the same bytes
    assert r["halved"] == 1 and r["alloc_failures"] == 1
    # a flip in the second half of the split chunk is found in chunk 1, at its offset in the tested set
    r = hs.hbmscan_test(0, fail_alloc_at=1, min_chunk_mib=0.25, inject_flip=("fade", 1, CHUNK_WORDS // 2 + 9, 127), **SMALL)
    assert r["errors"] == 1 and (r["records"][0]["chunk"], r["records"][0]["chunk_offset"]) == (1, 9 * 16)
    assert r["records"][0]["offset"] == (CHUNK_WORDS // 2 + 9) * 16
    # the three-word chunk cannot be halved above the floor: the scan goes on with what it holds
    r = hs.hbmscan_test(0, fail_alloc_at=6, min_chunk_mib=0.25, **SMALL)
    _clean(r, tested=5 * MIB, chunks=5)
    assert r["planned_bytes"] == LIMIT and r["halved"] == 0 and r["alloc_failures"] == 1
    _clean(hs.hbmscan_test(0, **SMALL))  # and the pretended failure left no error behind


def test_the_fade_phase_holds_between_write_and_check(hs):
    r = hs.hbmscan_test(0, hold_ms=50, **SMALL)
    print(json.dumps(r["phases"]))
    _clean(r)
    fade = r["phases"]["fade"]
    assert fade["wall_ms"] >= 100 and fade["wall_ms"] - fade["ms"] >= 100  # two holds of 50 ms, outside the sweeps' time
    assert all(r["phases"][p]["wall_ms"] < 100 for p in ("addr", "invert", "random"))


def test_a_deadline_stops_the_scan_without_failing_it(hs):
    r = hs.hbmscan_test(0, deadline_s=1e-9, **SMALL)
    print(json.dumps(r))
    assert r["pass"] and r["errors"] == 0 and r["complete"] is False and r["reached"] == {"phase": "addr", "step": 0}
    assert "stopped by its deadline after addr step 0: incomplete, not failed" in r["detail"]
    assert r["phases"]["invert"]["ms"] == 0 and r["tested_bytes"] == LIMIT
    _clean(hs.hbmscan_test(0, deadline_s=300, **SMALL))


@pytest.mark.parametrize("kw, message", (
    (dict(device=99), "valid device"), (dict(chunk_mib=1 + 1 / (1 << 17)), "multiples of 16"),
    (dict(chunk_mib=16 * 1024 + 1), "up to 16 GiB"), (dict(min_chunk_mib=0), "min_chunk"),
    (dict(hold_ms=-1), "hold_ms 0..60000"), (dict(hold_ms=60001), "hold_ms 0..60000"),
    (dict(random_passes=0), "random_passes 1..64"), (dict(random_passes=65), "random_passes 1..64"),
    (dict(deadline_s=-1.0), "deadline_s >= 0"), (dict(deadline_s=float("nan")), "deadline_s >= 0"),
    (dict(index_base=(1 << 62) + 1), "index_base"), (dict(fail_alloc_at=-1), "fail_alloc_at"),
    (dict(gib=8 / GIB), "nothing to test"), (dict(reserve_mib=1 << 30), "nothing to test"),
    (dict(chunk_mib=1 / 1024), "4096 chunks"),
    (dict(inject_flip=[("addr", 0, 0, 0)] * 5), "at most 4 flips"),
    (dict(inject_flip=("addr", 2, 0, 0)), "a step of it that writes"), (dict(inject_flip=("invert", 3, 0, 0)), "that writes"),
    (dict(inject_flip=("random", 4, 0, 0)), "a step of it"), (dict(inject_flip=("fade", 0, 0, 128)), "bit 0..127"),
    (dict(inject_flip=("fade", 0, WORDS, 0)), "outside the tested set"), (dict(inject_flip=("fade", 0, -1, 0)), "word >= 0"),
    (dict(inject_stuck=(WORDS, 0, 0)), "outside the tested set"), (dict(inject_stuck=(0, 128, 0)), "stuck_bit 0..127"),
    (dict(inject_stuck=(0, 0, 2)), "stuck_value 0 or 1"), (dict(inject_alias=(5, 5)), "two different alias words"),
    (dict(inject_alias=(5, WORDS)), "outside the tested set"), (dict(inject_alias=(5, -1)), "alias"),
))
def test_arguments_out_of_range_are_refused(hs, kw, message):
    kw = {**SMALL, **kw}
    with pytest.raises(RuntimeError, match=r"hbmscan failed \(-2\)") as e:
        hs.hbmscan_test(**kw)
    assert message in str(e.value), str(e.value)


def test_nothing_refused_left_the_device_in_an_error_state(hs):
    with pytest.raises(RuntimeError, match=r"hbmscan failed \(-2\)"):
        hs.hbmscan_test(0, inject_flip=("fade", 0, WORDS, 0), **SMALL)  # refused after the chunks were allocated
    _clean(hs.hbmscan_test(0, **SMALL))


def test_two_gib_are_past_the_caches(hs):
    r = hs.hbmscan_test(0, gib=2, chunk_mib=512)
    print(json.dumps(r))
    _clean(r, tested=2 * GIB, chunks=4, cached=False)
    assert r["detail"] == "" and all(p["gbs"] > 0 for p in r["phases"].values())
    # two flips in one 2 MiB span that is not a chunk's first: the region is named by its chunk and offset
    span = 2 * MIB // 16
    w = (512 * MIB // 16) + 5 * span
    r = hs.hbmscan_test(0, gib=2, chunk_mib=512, inject_flip=[("addr", 1, w + 1, 0), ("fade", 0, w + span - 1, 64)])
    assert r["errors"] == 2 and r["finding"] == {"kind": "region", "chunk": 1, "span": 10 * MIB, "span_bytes": 2 * MIB}, r
    r = hs.hbmscan_test(0, gib=2, chunk_mib=512, inject_flip=[("addr", 1, w + 1, 0), ("fade", 0, w + span, 64)])
    assert r["errors"] == 2 and r["finding"] == {"kind": "scattered"}, r


def test_the_suite_runs_it_only_when_asked(repo):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(0, 0, extra=("hbmscan",), options={"hbmscan": {"gib": 0.0625}})
    assert list(res) == ["hbmscan"] and res["hbmscan"]["pass"] and res["hbmscan"]["tested_bytes"] == 64 * MIB, res
    assert diag.run(0, 0) == {}
    assert "cached: cells not proven" in diag._summary("hbmscan", res["hbmscan"])

    def cli(*flags):
        p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                            "--format", "json", *flags], capture_output=True, text=True, timeout=300, cwd=repo)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    on, off = cli("--hbmscan", "--hbmscan-gib", "0.0625"), cli()
    assert on["hbmscan"]["pass"] and on["hbmscan"]["tested_bytes"] == 64 * MIB and on["hbmscan"]["cached"]
    assert "hbmscan" not in off and set(off) == set(on) - {"hbmscan"}
