"""Level 3 on the GPU (MI355X only, ``pytest -m gpu``): the register-file pattern test and the vector-ALU burn-in,
each clean on a healthy device and each shown one planted fault that it must count once and locate.  Every case is
a few launches of well under a millisecond; no test depends on a rate."""
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _regfile_clean():
    from k8s_gpu_node_checker_amd.ops import diag
    return diag.regfile_test(0, rounds=1)


def test_regfile_covers_every_simd_with_registers_only(dev):
    """One workgroup per CU: its four 512-register waves sit on the CU's four SIMDs, so every SIMD of the device
    ran a wave; at least 500 of a lane's 512 registers hold a pattern at once, and none of it is scratch."""
    from k8s_gpu_node_checker_amd.ops import diag
    r = _regfile_clean()
    cus = diag.device_info(0)["cus"]
    print(f"regfile: {r['simds']} SIMDs, {r['waves']} waves, {r['regs_per_lane']} registers, {r['ms']} ms")
    assert r["pass"] and r["errors"] == 0 and r["by_file"] == {"vgpr": 0, "agpr": 0} and "bad_simds" not in r, r
    assert r["scratch_bytes"] == 0, r
    assert r["regs_per_lane"] >= 500, r
    assert r["simds"] == 4 * cus and r["waves"] == 4 * cus, r   # every SIMD ran at least (here: exactly) one wave
    assert r["bytes_per_simd"] == r["regs_per_lane"] * 256, r


@pytest.mark.parametrize("reg", ["vgpr_lo", "vgpr_hi", "agpr_lo", "agpr_hi"])
def test_regfile_counts_and_locates_one_flipped_bit(dev, reg):
    """One bit of one register of one lane flipped between the write and the check of the first pattern: one wrong
    word, in the right file, on one SIMD that ran a wave."""
    from k8s_gpu_node_checker_amd.ops import diag
    assert _regfile_clean()["errors"] == 0
    r = diag.regfile_test(0, rounds=1, inject_block=5, inject_reg=reg)
    file = reg.split("_")[0]
    assert r["errors"] == 1 and not r["pass"], r
    assert r["by_file"] == {"vgpr": int(file == "vgpr"), "agpr": int(file == "agpr")}, r
    m = r["simd_map"]
    wrong = {row: (m[3 * row + 1], m[3 * row + 2]) for row in range(len(m) // 3) if m[3 * row + 1] or m[3 * row + 2]}
    assert len(wrong) == 1 and sum(next(iter(wrong.values()))) == 1, wrong
    row = next(iter(wrong))
    assert m[3 * row] > 0, "the wrong word is on a SIMD that ran no wave"
    assert r["bad_simds"] == [f"{diag.simd_name(row)} ({file} 1)"] and r["bad_simds"][0].startswith("xcd"), r
    assert "1 register words wrong on " + r["bad_simds"][0] in r["detail"], r


def test_regfile_refuses_an_injection_outside_the_grid(dev):
    from k8s_gpu_node_checker_amd.ops import diag
    with pytest.raises(RuntimeError, match="outside the grid"):
        diag.regfile_test(0, rounds=1, inject_block=1 << 20)


@pytest.mark.parametrize("kind", ["f64", "pk_f32", "i32"])
def test_valu_burn_matches_the_host_and_locates_one_wrong_lane(dev, kind):
    """Clean: every lane's final values equal the host's correctly rounded ones bit for bit.  One lane of one wave
    made wrong in the warm-up launch: one wrong result, on one CU, named; the rate is still reported."""
    from k8s_gpu_node_checker_amd.ops import diag
    ok = diag.valu_burn(0, kinds=(kind,), iters=16, reps=1)
    assert ok["kinds"][kind]["errors"] == 0 and ok["numerics"] == "" and "bad_cus" not in ok["map"], ok
    r = diag.valu_burn(0, kinds=(kind,), iters=16, reps=1, inject_block=5)
    assert r["kinds"][kind]["errors"] == 1 and not r["pass"] and "1 wrong results" in r["numerics"], r
    flat = r["cu_maps"][kind]
    wrong = {s: flat[3 * s + 1] for s in range(len(flat) // 3) if flat[3 * s + 1]}
    assert len(wrong) == 1 and list(wrong.values()) == [1], wrong
    slot = next(iter(wrong))
    assert flat[3 * slot] > 0, "the wrong lane is on a slot that ran no wave"
    assert r["map"]["bad_cus"] == [f"{diag.slot_name(slot)} ({kind} 1)"], r["map"]
    assert r["kinds"][kind]["gops"] > 0 and r["rates"][kind] > 0, r
    # every wave of both launches (2 workgroups of 4 waves per CU each) is in the map
    assert sum(flat[0::3]) == 2 * 2 * 4 * diag.device_info(0)["cus"], sum(flat[0::3])
    with pytest.raises(RuntimeError, match="outside the grid"):
        diag.valu_burn(0, kinds=(kind,), iters=16, reps=1, inject_block=1 << 20)


@pytest.mark.parametrize("test", ["regfile", "valu"])
def test_the_level_three_tests_pass_on_a_healthy_device(dev, test):
    from k8s_gpu_node_checker_amd.ops import diag
    r = diag._one(test, 0, diag.device_scale(0))
    print(test, diag._summary(test, r))
    assert r["pass"], r
    assert r.get("errors", 0) == 0 and not r.get("numerics"), r
