"""The table of opt-in diagnostics (ops/optin.py) against everything derived from it: the module, the dispatcher and
tables of ops/diag.py, the build target, the three command lines and the stand-in's C ABI, per entry; then the order
of the chosen names and the agent's two ways of asking for one."""
import argparse
import contextlib
import importlib.util
import io
import os
import types

import pytest

from k8s_gpu_node_checker_amd import build as B
from k8s_gpu_node_checker_amd.agent import agent as A
from k8s_gpu_node_checker_amd.agent import node_cycle
from k8s_gpu_node_checker_amd.ops import diag, native
from k8s_gpu_node_checker_amd.ops.optin import OPT_IN, add_flags, chosen
from k8s_gpu_node_checker_amd.testing import fake_native
from k8s_gpu_node_checker_amd.testing.fake_native import c_exports


def test_the_order_is_the_order_of_the_results():
    assert list(OPT_IN) == ["atomics", "lanes", "scalar", "matrix", "vmem", "cvt", "hbmscan", "ifetch", "handoff",
                            "scratch"]


@pytest.fixture(scope="module")
def helps():
    """``--help`` of mi355x-diag, node_cycle and the agent, printed once."""
    out = {}
    for main in (diag.main, node_cycle.main, A.main):
        text = io.StringIO()
        with contextlib.redirect_stdout(text), pytest.raises(SystemExit):
            main(["--help"])
        out[main] = text.getvalue()
    return out


@pytest.mark.parametrize("name", list(OPT_IN))
def test_everything_derived_from_an_entry(name, helps, monkeypatch):
    # a second copy of the module, run where no library exists: one loaded at import would raise NativeUnavailable
    monkeypatch.setattr(native, "NATIVE_DIR", "/nonexistent")
    monkeypatch.setattr(native, "_cache", {})
    spec = importlib.util.spec_from_file_location(f"{diag.__package__}.{name}_again",
                                                  os.path.join(os.path.dirname(diag.__file__), f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod._lib is None
    for attr in (f"{name}_test", "summary", "_signatures", "lib"):
        assert callable(getattr(mod, attr)), attr
    assert diag._TESTS[name] == (f"{name}_test", {}) and f"{name}_test" in diag._UNSCALED
    assert callable(getattr(diag, f"{name}_test")) and name in diag.KERNEL_REVISION
    t = B._targets()
    assert t[name]["cmd"] == t["xgmi"]["cmd"] and f"libmi355x_{name}.so" in B.__doc__
    assert f"--{name}" in helps[diag.main] and f"--{name}" in helps[node_cycle.main]
    assert f"--diag-{name}" in helps[A.main]
    exports = c_exports(name)
    assert exports and set(exports) == set(mod._signatures())
    assert getattr(fake_native, f"{name}_c_exports")() == exports  # the per-library spelling of earlier tests


def test_a_replaced_module_function_is_the_one_the_dispatcher_runs(monkeypatch):
    from k8s_gpu_node_checker_amd.ops import lanes
    monkeypatch.setattr(lanes, "lanes_test", lambda device, **kw: {"pass": True, "device": device, **kw})
    assert diag.lanes_test(3, iters=1) == {"pass": True, "device": 3, "iters": 1}
    assert diag._one("lanes", 2, diag.FULL) == {"pass": True, "device": 2}
    monkeypatch.setattr(diag, "lanes_test", lambda device, **kw: {"pass": True, "replaced": True})
    assert diag._one("lanes", 2, diag.FULL) == {"pass": True, "replaced": True}


def test_chosen_follows_the_table_not_the_command_line():
    ap = argparse.ArgumentParser()
    add_flags(ap, "", "also run the {name} diagnostic")
    assert chosen(ap.parse_args(["--scratch", "--lanes"])) == ("lanes", "scratch")
    assert chosen(ap.parse_args([])) == ()
    ap = argparse.ArgumentParser()
    add_flags(ap, "diag-", "also run the {name} test")
    assert chosen(ap.parse_args(["--diag-scratch", "--diag-atomics"]), "diag_") == ("atomics", "scratch")


def test_node_cycle_and_diag_pass_the_names_in_table_order(monkeypatch):
    seen = []
    monkeypatch.setattr(node_cycle, "run", lambda *a: seen.append(a[-1]) or {})
    assert node_cycle.main(["--devices", "0", "--scratch", "--lanes"]) == 0
    monkeypatch.setattr(diag, "device_count", lambda: 1)
    monkeypatch.setattr(diag, "burn_in", lambda *a, **k: seen.append(k.get("extra")) or {"pass": True, "rounds": 1})
    assert diag.main(["--scratch", "--lanes", "--duration", "0.001"]) == 0
    assert seen == [("lanes", "scratch"), ("lanes", "scratch")]


def _jobs(**kw):
    """What ``Agent(**kw)`` hands its workers for device 0: (level, device, keyword arguments but the deadline)."""
    ag = A.Agent("n", source="fake", diag_level=1, diag_timeout=60, **kw)
    seen = []

    def device(level, d, k, *a):
        seen.append((level, d, {x: v for x, v in k.items() if x != "deadline"}))
        return types.SimpleNamespace(box={})
    ag.workers.device = device
    ag._start_diag(0, "NPS1", None)
    return ag.diag_extra, seen


def test_the_agent_takes_a_name_either_way_and_refuses_an_unknown_keyword():
    assert _jobs(diag_lanes=True) == _jobs(diag_extra=("lanes",))
    assert _jobs(diag_lanes=True)[1] == [(1, 0, {"memory_partition": "NPS1", "extra": ("lanes",)})]
    assert _jobs(diag_scratch=True, diag_extra=("lanes", "atomics"))[0] == ("atomics", "lanes", "scratch")
    assert _jobs(diag_lanes=False) == _jobs() and "extra" not in _jobs()[1][0][2]
    with pytest.raises(TypeError, match=r"__init__\(\) got an unexpected keyword argument 'diag_bogus'"):
        A.Agent("n", source="fake", diag_bogus=True)
    with pytest.raises(TypeError, match="unexpected keyword argument 'lanes'"):
        A.Agent("n", source="fake", lanes=True)
    with pytest.raises(ValueError, match="bogus"):
        A.Agent("n", source="fake", diag_extra=("bogus",))
