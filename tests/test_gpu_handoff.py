"""libmi355x_handoff.so on an MI355X: all eight rows (four forms of an in-launch hand-off, across XCDs and inside
one) clean at the smallest grid and once at the default one, the three self-check hooks, the refused calls and the
opt-in wiring up to ``mi355x-diag --handoff``.

G = 16 is the least grid where ``w + 8`` differs from ``w``, with two workgroups per XCD; 8 rounds, one timed launch.
These tests plant wrong values in data and leave one signal out; every spin in the kernels is bounded, so the muted
launch ends by itself at its software deadline: none provokes a GPU fault or a hang.  No rate is asserted: the rates
are reported (profiles/handoff_mi355x.json) and never judged."""
import json
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

G, ROUNDS, REPS = 16, 8, 1
SIMD = re.compile(r"^xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]$")
CU = re.compile(r"^xcd[0-7]/se[0-3]/cu\d+(/sh1)?$")


@pytest.fixture(scope="module")
def handoff():
    from k8s_gpu_node_checker_amd.ops import handoff as ho
    assert ho.device_count() >= 1
    return ho


@pytest.fixture(scope="module")
def small(handoff):
    """all eight rows at the smallest shape: computed once and shared"""
    return handoff.handoff_test(0, blocks=G, rounds=ROUNDS, reps=REPS, slots=True)


def _rows_with_errors(r):
    return [k for k, v in r["rows"].items() if v["errors"]]


def test_all_eight_rows_are_clean_at_the_smallest_grid(handoff, small):
    r = small
    print(json.dumps({k: v for k, v in r.items() if k != "slots"}))
    assert r["pass"] and r["errors"] == 0 and r["complete"] and r["detail"] == "" and "bad_simds" not in r
    assert r["blocks"] == G and tuple(r["rows"]) == handoff.ROWS and len(r["rows"]) == 8
    # every launch places its 16 workgroups anew: the map adds up the SIMDs of all 16 launches
    assert r["simds"] == len(r["slots"]) >= G
    from k8s_gpu_node_checker_amd.ops.diag import simd_name
    assert all(SIMD.match(simd_name(s)) for s in r["slots"])
    for name, row in r["rows"].items():
        print(name, row["pairs_cross_xcd"], row["pairs_same_xcd"], row["pairs_same_cu"], row["us_per_round"])
        assert row["errors"] == 0 and row["timeouts"] == 0 and row["complete"] and row["first_bad"] is None
        assert row["launches"] == REPS + 1
        assert row["words_checked"] == G * ROUNDS * handoff.words_per_round(name) * (REPS + 1), name
        assert row["pairs_same_cu"] == 0
        assert row["pairs_cross_xcd"] + row["pairs_same_xcd"] == G
        assert row["ms"] > 0 and row["us_per_round"] > 0
        if r["xcds"] == 8:  # an unpartitioned device
            if name.endswith("/cross"):
                assert row["pairs_cross_xcd"] > 0, name
            else:
                assert row["pairs_same_xcd"] > 0, name


def test_the_default_grid_once(handoff):
    from k8s_gpu_node_checker_amd.ops import diag
    cus = int(diag.device_info(0)["cus"])
    r = handoff.handoff_test(0, reps=1)
    print(json.dumps(r))
    assert r["pass"] and r["complete"] and r["errors"] == 0
    assert r["blocks"] == cus - cus % 8 and r["rounds"] == handoff.DEFAULT_ROUNDS
    if cus == 256:
        assert r["blocks"] == cus and r["xcds"] == 8
    for name, row in r["rows"].items():
        assert row["words_checked"] == r["blocks"] * 64 * handoff.words_per_round(name) * 2 and row["pairs_same_cu"] == 0


@pytest.mark.parametrize("row", ("fence/cross", "wt/same", "wt_add/cross", "granule/same"))
def test_the_flip_hook_gives_one_corrupt_word_in_that_row_only(handoff, row):
    r = handoff.handoff_test(0, blocks=G, rounds=ROUNDS, reps=REPS, inject_row=row, inject_block=5, inject_round=3)
    print(row, r["detail"], r["rows"][row]["first_bad"])
    assert r["pass"] is False and r["errors"] == 1 and _rows_with_errors(r) == [row] and r["complete"]
    bad = r["rows"][row]["first_bad"]
    assert bad["class"] == "corrupt" and bad["age"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    stride = 8 if row.endswith("/same") else 1
    assert bad["lane"] == 0 and bad["word"] == 0 and bad["round"] == 3 and bad["launch"] == 0
    assert bad["producer_block"] == (5 + stride) % G and CU.match(bad["producer"])
    assert SIMD.match(bad["where"]) and bad["where"] in r["detail"] and r["bad_simds"] == [f"{bad['where']} (1)"]
    assert not bad["where"].startswith(bad["producer"] + "/")  # another CU


@pytest.mark.parametrize("rnd", (1, 7))
@pytest.mark.parametrize("row,word", (("fence/cross", 1023), ("granule/same", 300)))
def test_the_stale_hook_gives_one_stale_word_of_age_one(handoff, row, word, rnd):
    r = handoff.handoff_test(0, blocks=G, rounds=ROUNDS, reps=REPS, inject_row=row, inject_block=6, inject_round=rnd,
                             inject_stale_word=word)
    print(row, rnd, r["detail"], r["rows"][row]["first_bad"])
    assert r["pass"] is False and r["errors"] == 1 and _rows_with_errors(r) == [row] and r["complete"]
    bad = r["rows"][row]["first_bad"]
    assert bad["class"] == "stale" and bad["age"] == 1
    assert bad["producer_block"] == 6 and bad["round"] == rnd and bad["word"] == word and bad["launch"] == 0
    assert bad["got"] != bad["want"] and SIMD.match(bad["where"]) and CU.match(bad["producer"])
    assert "stale, 1 rounds old" in r["detail"]


def test_the_mute_hook_runs_the_give_up_path_once(handoff):
    """the muted workgroup leaves the last round's flag out: its consumer's bounded spin runs out after 2 ms, the
    launch returns by itself, and the row is incomplete, not failed"""
    row, muted = "wt/cross", 6
    r = handoff.handoff_test(0, rows=(row,), blocks=G, rounds=ROUNDS, reps=REPS, spin_ms=2, inject_row=row,
                             inject_block=muted, inject_round=ROUNDS - 1, inject_mute=True)
    print(json.dumps(r))
    got = r["rows"][row]
    assert got["timeouts"] >= 1 and got["complete"] is False and r["complete"] is False
    assert r["errors"] == 0 and got["errors"] == 0 and r["pass"] is True
    assert got["first_timeout"] == {"who": (muted - 1) % G, "for": "flag", "producer": muted, "round": ROUNDS - 1}
    assert "incomplete, not failed" in r["detail"] and "re-run on an idle device" in r["detail"]
    assert r["wall_s"] < 5
    assert got["words_checked"] < G * ROUNDS * 1024 * (REPS + 1)  # the muted round was not compared by its consumer


def test_refused_calls(handoff):
    from k8s_gpu_node_checker_amd.ops import diag
    cus = int(diag.device_info(0)["cus"])
    over = cus - cus % 8 + 8
    for kw in (dict(blocks=8), dict(blocks=20), dict(blocks=over), dict(rounds=0), dict(spin_ms=0), dict(reps=0),
               dict(blocks=G, inject_row="fence/cross", inject_block=1, inject_round=0, inject_stale_word=3),
               dict(blocks=G, inject_row="fence/cross", inject_block=G),
               dict(blocks=G, rounds=4, inject_row="fence/cross", inject_round=4),
               dict(blocks=G, inject_row="granule/cross", inject_round=1, inject_stale_word=512)):
        with pytest.raises(RuntimeError, match=r"handoff failed \(-2\)"):
            handoff.handoff_test(0, **kw)
    for kw in (dict(rows=("fence/diagonal",)), dict(rows=()), dict(rows=("wt/same",), inject_row="wt/cross")):
        with pytest.raises(ValueError):
            handoff.handoff_test(0, **kw)


def test_the_cli_flag_carries_a_passing_handoff_result(repo):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                        "--format", "json", "--handoff"], capture_output=True, text=True, timeout=300, cwd=repo)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(p.stdout)["devices"]["0"]["tests"]["handoff"]
    assert r["pass"] and r["errors"] == 0 and r["complete"] and len(r["rows"]) == 8
