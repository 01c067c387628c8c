"""libmi355x_scratch.so on an MI355X: the isolate row clean at the least shape that puts several waves on a SIMD and
has a previous round, and once at the default grid of twice the device's wave slots; both frames rows; the three
self-check hooks; the refused calls; the opt-in wiring up to ``mi355x-diag --scratch``.

These tests plant wrong values in data only; no kernel waits on another wave, so none provokes a GPU fault or a hang.
No time and no co-residency figure is judged beyond "more than one frame was live"."""
import json
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ISO_BLOCKS, ROUNDS, BLOCKS = 64, 2, 8
SIMD = re.compile(r"^xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]$")


@pytest.fixture(scope="module")
def scratch():
    from k8s_gpu_node_checker_amd.ops import scratch as sc
    assert sc.device_count() >= 1
    return sc


@pytest.fixture(scope="module")
def small(scratch):
    """all three rows at the smallest shape: computed once and shared"""
    return scratch.scratch_test(0, blocks=BLOCKS, isolate_blocks=ISO_BLOCKS, rounds=ROUNDS, slots=True)


def test_isolate_is_clean_at_64_workgroups_and_2_rounds(scratch, small):
    r = small
    print(json.dumps({k: v for k, v in r.items() if k != "slots"}))
    row = r["rows"]["isolate/1k"]
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and "bad_simds" not in r
    assert row["errors"] == 0 and row["first_bad"] is None and row["launches"] == 2
    assert row["words_checked"] == 2 * scratch.words_per_launch("isolate/1k", ISO_BLOCKS, ROUNDS) == 2 * 64 * 256 * 256 * 2
    assert r["isolate_waves"] == 4 * ISO_BLOCKS and 1024 <= row["frame_bytes"] <= 1088 and row["ms"] > 0
    assert r["co_resident_waves"] >= 1 and r["frame_bytes"]["isolate"] == row["frame_bytes"]
    from k8s_gpu_node_checker_amd.ops.diag import simd_name
    assert r["simds"] == len(r["slots"]) >= 1 and all(SIMD.match(simd_name(s)) for s in r["slots"])


def test_both_frames_rows_are_clean_on_8_workgroups(scratch, small):
    for name in scratch.FRAMES_ROWS:
        row = small["rows"][name]
        assert row["errors"] == 0 and row["first_bad"] is None, (name, row)
        assert row["words_checked"] == 2 * scratch.words_per_launch(name, BLOCKS) == 2 * 8 * 256 * 17
        assert 0 < row["frame_bytes"] <= 1088


def test_isolate_at_the_default_grid_once(scratch):
    from k8s_gpu_node_checker_amd.ops import diag
    cus = int(diag.device_info(0)["cus"])
    r = scratch.scratch_test(0, rows=("isolate/1k",), rounds=ROUNDS)
    print(json.dumps(r))
    waves = min(2 * cus * 32, scratch.ISO_MAX_WAVES)
    assert r["pass"] and r["errors"] == 0 and r["isolate_waves"] == waves
    assert r["rows"]["isolate/1k"]["words_checked"] == 2 * waves * 64 * 256 * ROUNDS
    assert r["co_resident_waves"] > 1
    assert r["simds"] == 4 * cus  # every SIMD of the device ran a wave


def test_the_flip_hook_gives_one_corrupt_word(scratch):
    for row, kw in (("isolate/1k", {}), ("frames/index", {}), ("frames/calls", {})):
        r = scratch.scratch_test(0, blocks=BLOCKS, isolate_blocks=ISO_BLOCKS, rounds=ROUNDS, inject_row=row, inject_wave=5)
        bad = r["rows"][row]["first_bad"]
        print(row, r["detail"], bad)
        assert r["pass"] is False and r["errors"] == 1 and [k for k, v in r["rows"].items() if v["errors"]] == [row]
        assert bad["class"] == "corrupt" and bad["age"] == 0 and bad["writer"] is None
        assert int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
        assert (bad["wave"], bad["lane"], bad["word"], bad["launch"]) == (5, 0, 0, 0)
        assert SIMD.match(bad["where"]) and bad["where"] in r["detail"] and r["bad_simds"] == [f"{bad['where']} (1)"]


def test_the_alias_hook_names_the_writer(scratch):
    r = scratch.scratch_test(0, rows=("isolate/1k",), isolate_blocks=ISO_BLOCKS, rounds=ROUNDS, inject_row="isolate/1k",
                             inject_wave=5, inject_round=1, inject_alias=True, slots=True)
    bad = r["rows"]["isolate/1k"]["first_bad"]
    print(r["detail"], bad)
    assert r["pass"] is False and r["errors"] == 1 and bad["class"] == "alias" and bad["age"] == 0
    assert (bad["wave"], bad["lane"], bad["word"], bad["round"], bad["launch"]) == (5, 0, 0, 1, 0)
    assert bad["writer"]["wave"] == 6 and SIMD.match(bad["writer"]["where"])
    assert f"alias, written by wave 6 on {bad['writer']['where']}" in r["detail"]


@pytest.mark.parametrize("word", (0, 77, 255))
def test_the_stale_hook_gives_one_stale_word_of_age_one(scratch, word):
    r = scratch.scratch_test(0, rows=("isolate/1k",), isolate_blocks=ISO_BLOCKS, rounds=ROUNDS, inject_row="isolate/1k",
                             inject_wave=9, inject_stale_word=word)
    bad = r["rows"]["isolate/1k"]["first_bad"]
    print(r["detail"], bad)
    assert r["pass"] is False and r["errors"] == 1 and bad["class"] == "stale" and bad["age"] == 1
    assert (bad["wave"], bad["lane"], bad["word"], bad["round"], bad["launch"]) == (9, 0, word, 1, 0)
    assert bad["got"] != bad["want"] and "stale, 1 rounds old" in r["detail"]


def test_refused_calls(scratch):
    iso = dict(rows=("isolate/1k",), inject_row="isolate/1k")
    for kw in (dict(isolate_blocks=4097), dict(rounds=0), dict(rounds=17), dict(reps=0),
               dict(isolate_blocks=ISO_BLOCKS, inject_wave=4 * ISO_BLOCKS - 1, inject_alias=True, **iso),
               dict(inject_stale_word=3, inject_round=0, **iso), dict(inject_stale_word=256, **iso),
               dict(rows=("frames/index",), blocks=BLOCKS, inject_row="frames/index", inject_wave=4 * BLOCKS)):
        with pytest.raises(RuntimeError, match=r"scratch failed \(-2\)"):
            scratch.scratch_test(0, **kw)
    for kw in (dict(rows=("isolate/2k",)), dict(rows=()), dict(rows=("frames/index",), inject_row="frames/calls")):
        with pytest.raises(ValueError):
            scratch.scratch_test(0, **kw)


def test_the_cli_flag_carries_a_passing_scratch_result(repo):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                        "--format", "text", "--scratch"], capture_output=True, text=True, timeout=300, cwd=repo)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (line,) = [ln for ln in p.stdout.splitlines() if ln.split()[:1] == ["scratch"]]
    assert line.split()[1] == "pass" and "0 wrong words" in line, line
