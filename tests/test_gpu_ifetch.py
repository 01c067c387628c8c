"""libmi355x_ifetch.so on an MI355X: the map of the walk kernel's blocks, every block and every branch op applied
once and held against the model word for word, both parts clean at the smallest grid and at the default one, both
self-check hooks in each part, and the opt-in wiring up to ``mi355x-diag --ifetch``.

These tests plant wrong values in data and models only; none alters a branch target or provokes a GPU fault.  No rate
is asserted: the rates are reported (profiles/ifetch_mi355x.json) and never judged.

The model here is an independent Python implementation of csrc/ifetch/ifetch_ref.h's constant hash, block and branch
select (tests/test_ifetch_cpu.py holds the header against the same rules)."""
import json
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

M = 0xffffffff
M64 = (1 << 64) - 1
SMALL = 8  # blocks of the small footprint: a few KiB of code


def mix32(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x & M


def lit(block, j):
    return (mix32(((block + 1) << 32) | (j + 1)) & 0x7fffffff) | 0x00800001


def block_x(block, x):
    for s in range(16):
        r = 1 + mix32(((block + 1) << 32) | (3 * s + 1)) % 31
        x = (((((x << r) | (x >> (32 - r))) & M) ^ lit(block, 3 * s + 1)) + lit(block, 3 * s + 2)) & M
    return x


def block_p(block, p):
    v = (p ^ lit(block, 48)) * 0x9E3779B1 & M
    v ^= v >> 15
    v = v * 0x85EBCA6B & M
    return v ^ (v >> 13)


def branch(ifetch, op, w, cond):
    k = ifetch.NB + ifetch.OPS.index(op)
    taken = (cond == 0) if op in ("s_cbranch_scc0", "s_cbranch_vccz", "s_cbranch_execz") else (cond != 0)
    return (w + lit(k, 0)) & M if taken else w ^ lit(k, 1)


@pytest.fixture(scope="module")
def ifetch():
    from k8s_gpu_node_checker_amd.ops import ifetch as fe
    assert fe.device_count() >= 1
    return fe


@pytest.fixture(scope="module")
def small(ifetch):
    """both parts at 8 workgroups, the walk at 512 steps over the small and the full footprint, the branches at 64
    steps: computed once and shared"""
    return ifetch.ifetch_test(0, blocks=8, steps=512, nbs=(SMALL, ifetch.NB), iters=64, reps=1, slots=True)


def test_the_map_has_every_block_apart_and_spans_what_the_result_reports(ifetch, small):
    addrs = ifetch.block_map(0)
    assert len(addrs) == ifetch.NB == len(set(addrs)) and all(a % 4 == 0 and a > 0 for a in addrs)
    order = sorted(addrs)
    gaps = [b - a for a, b in zip(order, order[1:])]
    print("gaps", min(gaps), max(gaps), "span", order[-1] - order[0])
    assert min(gaps) >= ifetch.BLOCK_MIN_BYTES  # at least a block's literal bytes
    rows = small["parts"]["walk"]["rows"]
    full = rows[ifetch.row_name(ifetch.NB)]["footprint_bytes"]
    assert full >= ifetch.FLOOR_BYTES
    assert full == order[-1] + min(gaps) - order[0]  # the last block counted as long as the shortest other
    # the small footprint: from the lowest of its blocks to the next block above the highest of them
    mine = sorted(addrs[:SMALL])
    above = min(a for a in addrs if a > mine[-1])
    assert rows[ifetch.row_name(SMALL)]["footprint_bytes"] == above - mine[0] < 16 * 1024
    assert ifetch.block_map(0) == addrs  # the same kernel, loaded once


def test_every_block_applied_once_equals_the_model_word_for_word(ifetch):
    x = [mix32(0x51ED + 977 * i) for i in range(64)]
    x[0], x[1], x[63] = 0, M, 0x80000000
    p = 0xC0FFEE11
    got = ifetch.apply_blocks(list(range(ifetch.NB)), x, p)
    assert len(got) == ifetch.NB
    wrong = [b for b in range(ifetch.NB) if got[b][0] != [block_x(b, v) for v in x] or got[b][1] != block_p(b, p)]
    print("blocks checked:", ifetch.NB, "disagreeing:", wrong[:16])
    assert not wrong, wrong[:16]
    # a list in another order, with a block twice: every entry starts from the same words
    again = ifetch.apply_blocks([1023, 0, 1023, 512], x, p)
    assert again == [got[1023], got[0], got[1023], got[512]]


def test_every_branch_op_taken_and_not_taken_equals_the_model(ifetch):
    wrong = []
    for k, op in enumerate(ifetch.OPS):
        rows = [(mix32(77 * k + i), i & 1) for i in range(128)]
        rows += [(w, c) for w in (0, M, 0x80000000, 0xfc, 0x3) for c in (0, 1)]  # the bit VCC / EXEC keep: 63, 0
        got = ifetch.apply_many(op, rows)
        want = [branch(ifetch, op, w, c) for w, c in rows]
        wrong += [(op, hex(w), c, hex(g), hex(v)) for (w, c), g, v in zip(rows, got, want) if g != v]
        assert ifetch.apply(op, 5, 0) != ifetch.apply(op, 5, 1)
    print("ops checked:", len(ifetch.OPS), "disagreeing:", wrong[:8])
    assert not wrong, wrong[:8]


def test_both_parts_are_clean_at_eight_workgroups(ifetch, small):
    r = small
    print(json.dumps({k: v for k, v in r.items() if k != "slots"}))
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "" and "bad_simds" not in r, r
    assert r["blocks"] == {"walk": 8, "branch": 8}
    walk, br = r["parts"]["walk"], r["parts"]["branch"]
    assert walk["steps"] == 512 and list(walk["rows"]) == [ifetch.row_name(SMALL), ifetch.row_name(ifetch.NB)]
    for row in walk["rows"].values():
        assert row["errors"] == 0 and row["first_bad"] is None and row["blocks_visited"] == row["nb"], row
        assert row["ms"] > 0 and row["ns_per_block"] > 0 and row["footprint_bytes"] > 0
    assert br["iters"] == 64 and tuple(br["ops"]) == ifetch.OPS
    for op, row in br["ops"].items():
        assert row["errors"] == 0 and row["first_bad"] is None and row["ms"] > 0, (op, row)
    for slot in r["slots"]:
        assert re.fullmatch(r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]", ifetch.simd_name(slot)), slot
    assert r["simds"] == len(r["slots"]) >= 1


def test_the_default_grid_is_clean_on_every_xcd(ifetch):
    from k8s_gpu_node_checker_amd.ops import diag
    r = ifetch.ifetch_test(0, iters=64, reps=1)
    print(json.dumps(r))
    assert r["pass"] and r["errors"] == 0, r["detail"]
    cus = diag.device_info(0)["cus"]
    assert r["blocks"] == {"walk": 4 * cus, "branch": 4 * cus} and r["simds"] <= 4 * cus
    assert [v["blocks_visited"] for v in r["parts"]["walk"]["rows"].values()] == list(ifetch.DEFAULT_NBS)
    if cus == 256:
        assert r["xcds"] == 8 and r["simds"] == 1024


def _walk_rows_with_errors(r):
    return [k for k, v in r["parts"]["walk"]["rows"].items() if v["errors"]]


def _ops_with_errors(r):
    return [k for k, v in r["parts"]["branch"]["ops"].items() if v["errors"]]


@pytest.mark.parametrize("nb", (SMALL, 1024))
def test_an_injected_flip_is_one_wrong_word_in_that_walk_row_only(ifetch, nb):
    r = ifetch.ifetch_test(0, blocks=8, steps=512, nbs=(SMALL, ifetch.NB), iters=8, reps=1, inject_part="walk",
                           inject_row=nb, inject_block=5)
    name = ifetch.row_name(nb)
    print(r["detail"], r["parts"]["walk"]["rows"][name])
    assert r["pass"] is False and r["errors"] == 1
    assert _walk_rows_with_errors(r) == [name] and _ops_with_errors(r) == []
    bad = r["parts"]["walk"]["rows"][name]["first_bad"]
    assert bad["lane"] == 0 and bad["word"] == "x" and bad["path"] == 20 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert re.fullmatch(r"xcd[0-7]/se[0-3]/cu\d+(/sh1)?/simd[0-3]", bad["where"]), bad
    assert r["detail"] == f"1 wrong words in the walk over {nb} blocks on {bad['where']}"
    assert r["bad_simds"] == [f"{bad['where']} (1)"]


@pytest.mark.parametrize("step", (0, 511))
def test_a_block_that_was_not_executed_shows_in_that_walk_row_only(ifetch, step):
    r = ifetch.ifetch_test(0, blocks=8, steps=512, nbs=(SMALL, ifetch.NB), iters=8, reps=1, inject_part="walk",
                           inject_row=ifetch.NB, inject_block=5, inject_skip_step=step)
    name = ifetch.row_name(ifetch.NB)
    print(step, r["detail"], r["parts"]["walk"]["rows"][name])
    assert r["pass"] is False and 0 < r["errors"] <= 65  # one wave's lanes and its walker at the most
    assert _walk_rows_with_errors(r) == [name] and _ops_with_errors(r) == []
    bad = r["parts"]["walk"]["rows"][name]["first_bad"]
    assert bad["got"] != bad["want"] and bad["path"] == 20


@pytest.mark.parametrize("op", ("s_cbranch_scc1", "s_cbranch_execz", "s_swappc_b64"))
def test_the_hooks_of_the_branch_part_show_in_that_op_only(ifetch, op):
    kw = dict(blocks=8, parts=("branch",), ops=ifetch.OPS, iters=64, reps=1, inject_part="branch", inject_row=op,
              inject_block=5)
    r = ifetch.ifetch_test(0, **kw)
    print(op, r["detail"])
    assert r["pass"] is False and r["errors"] == 1 and _ops_with_errors(r) == [op]
    bad = r["parts"]["branch"]["ops"][op]["first_bad"]
    assert bad["chain"] == 0 and int(bad["got"], 16) == int(bad["want"], 16) ^ 0x10
    assert r["detail"] == f"1 wrong words in {op} on {bad['where']}" and r["bad_simds"] == [f"{bad['where']} (1)"]
    r = ifetch.ifetch_test(0, inject_skip_step=63, **kw)
    print(op, r["detail"])
    assert r["pass"] is False and 0 < r["errors"] <= 4 and _ops_with_errors(r) == [op]  # one wave's chains at the most


def test_refused_calls(ifetch):
    for kw in (dict(steps=0), dict(reps=0), dict(iters=0, parts=("branch",)),
               dict(blocks=4, inject_part="walk", inject_block=4),
               dict(steps=16, nbs=(4,), inject_part="walk", inject_block=0, inject_skip_step=16),
               dict(steps=64, nbs=(1024,))):  # 64 x 64 draws leave some of 1,024 blocks out: refused, not run
        with pytest.raises(RuntimeError, match=r"ifetch failed \(-2\)"):
            ifetch.ifetch_test(0, **kw)
    with pytest.raises(RuntimeError, match=r"visit \d+ of 1024 blocks in 64 steps"):
        ifetch.ifetch_test(0, steps=64, nbs=(1024,))


def test_the_cli_flag_carries_a_passing_ifetch_result(repo):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                        "--format", "json", "--ifetch"], capture_output=True, text=True, timeout=300, cwd=repo)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    tests = json.loads(p.stdout)["devices"]["0"]["tests"]
    r = tests["ifetch"]
    assert r["pass"] and r["errors"] == 0 and len(r["parts"]["branch"]["ops"]) == 10
    assert [v["nb"] for v in r["parts"]["walk"]["rows"].values()] == [8, 64, 256, 1024]
