"""The kernel-driven xGMI path on CPU: the C ABI of csrc/xgmi/xgmi.hip against ops/xgmi.py, and the attribution of
copy-path problems to the link or the copy engine (ops/diag.p2p_matrix(kernel=True)) through the fake C ABIs of
testing/fake_native.py, up to the CLI flag and a whole 8-GPU agent cycle.  The real library runs on an MI355X in
tests/test_gpu_xgmi.py."""
import ctypes
import json
import os

import pytest

from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.ops import amdsmi_probe, diag, fabric
from k8s_gpu_node_checker_amd.testing import fixtures
from k8s_gpu_node_checker_amd.testing.fake_native import FakeDiagLib, FakeFabricLib


@pytest.fixture
def fakes(monkeypatch):
    """install(diag_kw, xgmi_kw) -> (FakeDiagLib, FakeXgmiLib) for an 8-GPU node."""
    from k8s_gpu_node_checker_amd.ops import xgmi
    from k8s_gpu_node_checker_amd.testing.fake_native import FakeXgmiLib

    def install(diag_kw=None, xgmi_kw=None):
        lib, xlib = FakeDiagLib(n=8, **(diag_kw or {})), FakeXgmiLib(n=8, **(xgmi_kw or {}))
        monkeypatch.setattr(diag, "lib", lambda: lib)
        monkeypatch.setattr(xgmi, "lib", lambda: xlib)
        return lib, xlib
    return install


# --- 1. exports and signatures ------------------------------------------------------------------------------

def test_xgmi_exports_match_the_signature_table():
    from k8s_gpu_node_checker_amd.ops import xgmi
    from k8s_gpu_node_checker_amd.testing.fake_native import c_exports
    exports, sig = c_exports("xgmi"), xgmi._signatures()
    assert set(exports) == set(sig) == {"xgmi_last_error", "xgmi_device_count", "xgmi_kernel_fan"}
    pointers = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, params in exports.items():
        argtypes = sig[name][0]
        if not params:
            assert argtypes is None, name
            continue
        assert argtypes is not None and len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (isinstance(t, type) and issubclass(t, pointers)), (name, p, t)
    assert len(exports["xgmi_kernel_fan"]) == 14


def test_the_built_library_resolves_every_export(monkeypatch):
    from k8s_gpu_node_checker_amd.ops import native, xgmi
    if not os.path.exists(os.path.join(native.NATIVE_DIR, "libmi355x_xgmi.so")):
        pytest.skip("libmi355x_xgmi.so not built (no hipcc)")
    monkeypatch.setattr(xgmi, "_lib", None)  # the real library, whatever another test installed
    L = xgmi.lib()
    assert isinstance(L, ctypes.CDLL)
    for name, (argtypes, _) in xgmi._signatures().items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert argtypes is None or list(fn.argtypes) == argtypes


# --- 2-4. attribution ---------------------------------------------------------------------------------------

def test_a_pair_slow_for_the_kernel_too_is_the_link(fakes):
    lib, xlib = fakes({"slow_pairs": {(5, 3): 12.0}}, {"kernel_slow": {(5, 3, "store"): 11.4}})
    m = diag.p2p_matrix(kernel=True)
    assert not m["pass"]
    assert "5->3 12.0 GB/s (link: kernel stores 11.4 GB/s, median 55.0)" in m["detail"]
    assert [(s["src"], s["dst"], s["mode"], s["kind"]) for s in m["kernel"]["slow"]] == [(5, 3, "store", "pair")]
    # every source: 7 peers alone in both modes, then the fan in both modes; only distinct peers, never the source
    assert len(xlib.calls) == 8 * (7 * 2 + 2)
    assert xlib.calls[:3] == ["xkstore0->1", "xkload0->1", "xkstore0->2"]
    assert "xkstore5->0,1,2,3,4,6,7" in xlib.calls and "xkload5->0,1,2,3,4,6,7" in xlib.calls
    assert len(m["kernel"]["pairs"]) == 112 and len(m["kernel"]["fan"]) == 112


def test_a_pair_the_kernel_moves_at_full_rate_is_the_copy_engine(fakes):
    fakes({"slow_pairs": {(5, 3): 12.0}})
    m = diag.p2p_matrix(kernel=True)
    assert not m["pass"]
    assert "5->3 12.0 GB/s (copy engine: kernel stores 55.0 GB/s, median 55.0)" in m["detail"]
    assert m["kernel"]["slow"] == [] and m["kernel"]["bad"] == []


def test_a_fan_destination_is_attributed_from_the_kernel_fan_row(fakes):
    # slow only with every link of gpu 2 busy; the kernel's pair-alone row is fine both times
    fakes({"fan_slow": {(2, 6): 9.0}}, {"kernel_slow": {(2, 6, "fan_store"): 8.5}})
    m = diag.p2p_matrix(kernel=True)
    assert not m["pass"]
    assert ("fan 2->6 9.0 GB/s with every link of 2 busy (link: kernel stores 8.5 GB/s, median 55.0)"
            in m["detail"])
    fakes({"fan_slow": {(2, 6): 9.0}}, {"kernel_slow": {(2, 6, "store"): 8.5}})  # slow alone, not under the fan
    m = diag.p2p_matrix(kernel=True)
    assert ("fan 2->6 9.0 GB/s with every link of 2 busy (copy engine: kernel stores 55.0 GB/s, median 55.0)"
            in m["detail"])


# --- 5-7. what the kernel path itself changes ----------------------------------------------------------------

def test_a_slow_kernel_row_alone_does_not_fail_the_node(fakes):
    fakes(None, {"kernel_slow": {(1, 4, "load"): 20.0, (6, 0, "fan_store"): 10.0}})
    m = diag.p2p_matrix(kernel=True)
    assert m["pass"] and m["detail"] == ""
    assert sorted((s["src"], s["dst"], s["kind"], s["mode"], s["gbps"]) for s in m["kernel"]["slow"]) == [
        (1, 4, "pair", "load", 20.0), (6, 0, "fan", "store", 10.0)]
    assert m["kernel"]["min_gbps"] == {"pair_store": 55.0, "pair_load": 20.0, "fan_store": 10.0, "fan_load": 55.0}
    assert set(m["kernel"]["median_gbps"].values()) == {55.0}


def test_kernel_bad_words_fail_with_the_pair_named(fakes):
    fakes(None, {"kernel_errors": {(2, 5, "store"): 3, (7, 1, "fan_load"): 2}})
    m = diag.p2p_matrix(kernel=True)
    assert not m["pass"]
    assert "kernel store 2->5 3 bad words" in m["detail"] and "kernel load fan 7->1 2 bad words" in m["detail"]
    assert len(m["kernel"]["bad"]) == 2


def test_a_hung_kernel_launch_stops_the_matrix(fakes):
    lib, xlib = fakes(None, {"hung": ((3, 4),)})
    m = diag.p2p_matrix(kernel=True, timeout_s=0.3)
    assert not m["pass"]
    assert m["stopped"].startswith("kernel store 3->4 hung: xgmi kernel store 3->4: the launches did not complete")
    assert m["stopped"] in m["detail"] and m["kernel"]["stopped"] == m["stopped"]
    assert xlib.calls[-1] == "xkstore3->4"  # nothing is launched behind a hung kernel
    assert all(0 < t <= 300.0 for t in xlib.timeouts_ms)  # each launch gets what is left of the one deadline


def test_a_single_gpu_has_no_kernel_matrix(fakes):
    from k8s_gpu_node_checker_amd.ops import xgmi
    lib, xlib = fakes()
    assert "skipped" in xgmi.kernel_matrix([0]) and xlib.calls == []


# --- 8. default off ------------------------------------------------------------------------------------------

def test_off_by_default_nothing_new_is_called_or_reported(fakes):
    kw = {"slow_pairs": {(5, 3): 12.0}, "fan_slow": {(2, 6): 9.0}, "fan_errors": {(1, 0): 4}}
    lib, xlib = fakes(kw)
    off = diag.p2p_matrix()
    assert xlib.calls == [] and "kernel" not in off
    assert off["detail"] == ("5->3 12.0 GB/s; fan 2->6 9.0 GB/s with every link of 2 busy; "
                             "fan 5->3 12.0 GB/s with every link of 5 busy; fan 1->0 4 bad words")
    lib, xlib = fakes(kw)
    on = diag.p2p_matrix(kernel=True)
    assert {k: v for k, v in on.items() if k not in ("kernel", "detail", "wall_s")} == \
        {k: v for k, v in off.items() if k not in ("detail", "wall_s")}
    assert "fan 1->0 4 bad words (copy engine: kernel stores clean)" in on["detail"]
    assert diag.fabric_tests(list(range(8)), rccl=False)["p2p"]["detail"] == off["detail"] and xlib.calls != []


# --- 9. CLI and agent ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv, expect", [
    (["--level", "2"], {}), (["--level", "2", "--xgmi-kernel"], {"kernel": True}),
    (["--level", "2", "--xgmi-kernel", "--duration", "0.001"], {"kernel": True}),
    (["--level", "2", "--duration", "0.001"], {})])
def test_the_cli_flag_reaches_fabric_tests(monkeypatch, capsys, argv, expect):
    seen = []
    monkeypatch.setattr(diag, "device_count", lambda: 2)
    monkeypatch.setattr(diag, "device_info", lambda d: {"name": "fake"})
    monkeypatch.setattr(diag, "run_devices", lambda level, devices, parallel=8: {d: {} for d in devices})
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: {"pass": True, "rounds": 1})
    monkeypatch.setattr(diag, "fabric_tests", lambda *a, **k: seen.append(k) or {"p2p": {"pass": True}})
    assert diag.main(argv) == 0
    assert seen == [expect]
    assert json.loads(capsys.readouterr().out)["fabric"] == {"p2p": {"pass": True}}


def _cycle(monkeypatch, xgmi_kw=None, **agent_kw):
    from k8s_gpu_node_checker_amd.ops import xgmi
    from k8s_gpu_node_checker_amd.testing.fake_native import FakeXgmiLib
    lib, xlib = FakeDiagLib(n=8, slow_pairs={(5, 3): 12.0}), FakeXgmiLib(n=8, **(xgmi_kw or {}))
    monkeypatch.setattr(diag, "lib", lambda: lib)
    monkeypatch.setattr(xgmi, "lib", lambda: xlib)
    monkeypatch.setattr(fabric, "_lib", FakeFabricLib())
    monkeypatch.setattr(amdsmi_probe, "probe", lambda node, src, fx: fixtures.mi355x_probe_report(node, gpus=8))
    rep = A.Agent("n8", source="fake", diag_level=2, expect_gpus=8, diag_timeout=60, **agent_kw).probe_once()
    return rep, xlib


def test_an_agent_cycle_with_the_flag_publishes_the_kernel_summary(monkeypatch):
    rep, xlib = _cycle(monkeypatch, {"kernel_slow": {(5, 3, "store"): 11.4}}, diag_xgmi_kernel=True)
    p2p = rep["fabric"]["p2p"]
    assert not p2p["pass"] and "5->3 12.0 GB/s (link: kernel stores 11.4 GB/s, median 55.0)" in p2p["detail"]
    k = p2p["kernel"]
    assert "pairs" not in k and "fan" not in k  # the per-row lists stay with mi355x-diag, as the fan's do
    assert k["median_gbps"]["pair_store"] == 55.0 and k["min_gbps"]["pair_store"] == 11.4
    assert [(s["src"], s["dst"]) for s in k["slow"]] == [(5, 3)] and k["bad"] == []
    json.dumps(rep)
    args = A.build_parser().parse_args(["--node", "n", "--diag-xgmi-kernel"])
    assert args.diag_xgmi_kernel is True
    assert A.build_parser().parse_args(["--node", "n"]).diag_xgmi_kernel is False


def test_an_agent_cycle_without_the_flag_is_todays_report(monkeypatch):
    rep, xlib = _cycle(monkeypatch)
    p2p = rep["fabric"]["p2p"]
    assert xlib.calls == []
    assert set(p2p) == {"pass", "median_gbps", "min_gbps", "floor_gbps", "link_gbps", "detail", "wall_s", "fan"}
    assert p2p["detail"] == "5->3 12.0 GB/s; fan 5->3 12.0 GB/s with every link of 5 busy"
    # a three-argument stand-in for the suite, as existing tests install, still works without the flag
    calls = []
    monkeypatch.setattr(A, "_fabric_suite", lambda devices, timeout_s=None, link=None: calls.append(link) or {
        "p2p": {"pass": True, "detail": ""}, "rccl": {"pass": True, "detail": ""}})
    _cycle(monkeypatch)
    assert len(calls) == 1
