"""libmi355x_atomics.so on an MI355X: every kind of atomic on small arrays whose sizes sit where the indexing can go
wrong, one run of the default size, both self-check hooks, and the opt-in wiring up to ``mi355x-diag --atomics``.

These tests plant wrong values in data; none provokes a GPU fault.  No rate is asserted: the rates are reported
(profiles/atomics_mi355x.json) and never judged.

The drop hook's reference: the library returns ``want_without`` -- atomics_expected() of csrc/atomics/atomics_ref.h
without the dropped operand, computed on the host -- and the tests read that field (the header itself is held
against the element types' own arithmetic, in any order, by tests/test_atomics_cpu.py)."""
import json
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

# below, at and across a wave; across a 256-thread workgroup; odd for the packed and the 64-bit kinds
WORDS = (1, 63, 64, 65, 1000, 4097)
ADDERS = (1, 8, 32)  # fewer than, equal to and more than the XCD count
TICKET_MAX_WORDS = 1 << 20  # atomics_ref.h ATOMICS_TICKET_MAX_WORDS


@pytest.fixture(scope="module")
def atomics():
    from k8s_gpu_node_checker_amd.ops import atomics as a
    assert a.device_count() >= 1
    return a


def _clean(a, r, words, adders):
    assert r["pass"] and r["errors"] == 0 and r["detail"] == "", r
    assert r["words"] == words and r["adders"] == adders and set(r["kinds"]) == set(a.KINDS)
    for kind, row in r["kinds"].items():
        assert row["errors"] == 0 and row["first_bad"] is None and row["got"] is None and row["want"] is None, (kind, row)
        # the kernel counts what it issued: one operation per element and adder; a ticket is two (the returning add on
        # its counter and the add on the hit word it was handed), and every one of them was handed out in range
        want_ops = 2 * min(words, TICKET_MAX_WORDS) * adders if kind == "ticket" else words * adders
        assert row["ops"] == want_ops, (kind, row)
        assert 1 <= row["xcds"] <= 8 and sum(row["waves"]) >= 1, (kind, row)


@pytest.mark.parametrize("adders", ADDERS)
@pytest.mark.parametrize("words", WORDS)
def test_small_shapes_are_exact_in_every_kind(atomics, words, adders):
    r = atomics.atomics_test(0, words=words, adders=adders, iters=1)
    print(words, adders, r)
    _clean(atomics, r, words, adders)


def test_default_size_runs_clean_on_every_xcd(atomics):
    from k8s_gpu_node_checker_amd.ops import diag
    r = atomics.atomics_test(0)
    print(json.dumps(r))
    _clean(atomics, r, 16 << 20, 8)
    cus = diag.device_info(0)["cus"]
    xcds = 8 if cus >= 256 else max(1, cus // 32)  # a partition: its share of the eight XCDs
    assert {k: row["xcds"] for k, row in r["kinds"].items()} == {k: xcds for k in atomics.KINDS}, r
    assert all(row["gbs"] > 0 and row["ms"] > 0 for row in r["kinds"].values())


@pytest.mark.parametrize("word", (0, 2048, 4096))
@pytest.mark.parametrize("kind", ("add_u32", "add_u64", "add_f32", "add_f64", "pk_bf16", "max_u32", "xor_u32", "ticket"))
def test_a_flipped_bit_is_found_in_its_kind_only(atomics, kind, word):
    r = atomics.atomics_test(0, words=4097, adders=8, iters=2, inject_kind=kind, inject_word=word)
    print(kind, word, r)
    assert not r["pass"] and r["errors"] == 1
    hit = r["kinds"][kind]
    assert hit["errors"] == 1 and hit["first_bad"] == word, hit
    assert int(hit["got"], 16) == int(hit["want"], 16) ^ 0x10, hit
    assert all(row["errors"] == 0 and row["first_bad"] is None for k, row in r["kinds"].items() if k != kind), r
    assert r["detail"] == (f"1 elements wrong in {kind} (first at +0x{word * atomics.elem_bytes(kind):x}: "
                           f"got {hit['got']}, want {hit['want']})")


@pytest.mark.parametrize("adders, drop", ((8, 3), (1, 0), (32, 31)))
@pytest.mark.parametrize("kind", ("add_u32", "add_f32", "pk_bf16", "xor_u32"))
def test_a_dropped_operation_leaves_the_value_without_it(atomics, kind, adders, drop):
    word = 1234
    r = atomics.atomics_test(0, words=4097, adders=adders, iters=2, kinds=(kind, "add_u64"), inject_kind=kind,
                             inject_word=word, inject_drop_adder=drop)
    print(kind, adders, drop, r)
    hit = r["kinds"][kind]
    assert not r["pass"] and r["errors"] == 1 and hit["errors"] == 1 and hit["first_bad"] == word, r
    assert hit["got"] == hit["want_without"] and hit["got"] != hit["want"], hit  # a lost add, not a flipped bit
    assert hit["ops"] == 4097 * adders - 1, hit
    assert r["kinds"]["add_u64"]["errors"] == 0 and "want_without" not in r["kinds"]["add_u64"]
    assert kind in r["detail"]


def test_arguments_outside_the_exactness_bounds_are_refused(atomics):
    for kw in (dict(adders=0), dict(adders=33), dict(words=0), dict(iters=0), dict(device=atomics.device_count()),
               dict(inject_kind="add_f32", inject_word=64), dict(inject_kind="add_f32", inject_word=-1),
               dict(inject_kind="add_f32", inject_drop_adder=8)):
        kw.setdefault("words", 64)
        with pytest.raises(RuntimeError, match=r"atomics failed \(-2\)"):
            atomics.atomics_test(**kw)
    with pytest.raises(ValueError):
        atomics.atomics_test(words=64, kinds=("add_f16",))
    _clean(atomics, atomics.atomics_test(words=64, iters=1), 64, 8)  # nothing above left the device in an error state


def test_the_suite_runs_it_only_when_asked(repo):
    from k8s_gpu_node_checker_amd.ops import diag
    res = diag.run(1, 0, extra=("atomics",))
    assert list(res)[-1] == "atomics" and res["atomics"]["pass"], res["atomics"]
    assert set(res) - {"atomics"} == {t.replace("_quick", "") for t in diag.LEVELS[1]}

    def cli(*flags):
        p = subprocess.run([sys.executable, "-m", "k8s_gpu_node_checker_amd.ops.diag", "--level", "1", "--device", "0",
                            "--format", "json", *flags], capture_output=True, text=True, timeout=300, cwd=repo)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        return json.loads(p.stdout)["devices"]["0"]["tests"]
    on, off = cli("--atomics"), cli()
    assert on["atomics"]["pass"] and on["atomics"]["kinds"]["ticket"]["errors"] == 0
    assert "atomics" not in off and set(off) == set(on) - {"atomics"}
