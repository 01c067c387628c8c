"""Kernel-driven xGMI test: ``libmi355x_xgmi.so`` (csrc/xgmi/xgmi.hip) from Python.

The copy-engine path of the pair matrix (``ops/diag.p2p_copy`` / ``p2p_fan``) cannot tell a slow link from a busy
SDMA engine.  Here the bytes are moved by the source GPU's CUs, with stores into and loads from a peer's memory,
the way RCCL loads the links; ``diag.p2p_matrix(kernel=True)`` sets these rates next to the copy path's.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`; nothing falls back to a copy.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Tuple

from .native import bind_cdll

MODES = ("store", "load")  # the native `mode` argument: index into this
HUNG = -4                  # xgmi_kernel_fan: the launches (or the verification) missed the deadline

# No absolute floor for a kernel rate: the kernel path has never run with a peer GPU (every rate measured so far is a
# one-GPU self-peer rate, that is local HBM: profiles/xgmi_kernel_selfpeer_mi355x.json), so peer rates are "not
# measured" and no number could anchor one.  Kernel rows are judged against their own mode's median only
# (``diag.P2P_MIN_FRACTION_OF_MEDIAN``), and even that only attributes a copy-path problem: it never fails a node.
KERNEL_MIN_GBPS: Optional[float] = None

_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/xgmi/xgmi.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_xgmi_kernel_cpu.py holds it against the C source."""
    I, Z, D, LL = ctypes.c_int, ctypes.c_size_t, ctypes.c_double, ctypes.c_longlong
    pI, pD, pU = (ctypes.POINTER(t) for t in (I, D, ctypes.c_ulonglong))
    return {
        "xgmi_last_error": (None, ctypes.c_char_p),
        "xgmi_device_count": (None, I),
        "xgmi_kernel_fan": ([I, pI, I, Z, I, I, D, I, LL, pD, pU, pU, pI, pD], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_xgmi.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x xgmi failed ({rc}): {lib().xgmi_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().xgmi_device_count())


def kernel_fan(src: int, dsts: List[int], mib: int = 256, iters: int = 5, mode: str = "store",
               timeout_s: Optional[float] = None, nbytes: Optional[int] = None, inject_dst: int = -1,
               inject_word: int = 0) -> Dict[str, Any]:
    """One kernel on ``src`` storing to (``mode="store"``) or loading from (``"load"``) a buffer of ``mib`` MiB
    (``nbytes`` overrides it) on every device of ``dsts`` at once; one destination is the pair test.  ``src`` itself
    and repeated devices are allowed (a one-GPU box: local-HBM rates, not link rates).  Per destination: the GB/s it
    saw, bad 16-byte elements, the lowest bad element (None: none) and peer access; ``total_gbps`` for the source.
    ``inject_dst`` / ``inject_word``: the verifier's self-check (one bit of that 32-bit word flipped from the host).
    ``{"hung": True, ...}`` at the deadline ``timeout_s``."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
    n = len(dsts)  # 0 or more than 64: refused by the native side before it reads an array
    arr = (ctypes.c_int * n)(*dsts)
    gbps, errs, first = (ctypes.c_double * n)(), (ctypes.c_ulonglong * n)(), (ctypes.c_ulonglong * n)()
    peer = (ctypes.c_int * n)()
    total = ctypes.c_double()
    ms = 0.0 if not timeout_s else max(1.0, 1000.0 * timeout_s)
    size = (mib << 20) if nbytes is None else int(nbytes)
    rc = lib().xgmi_kernel_fan(src, arr, n, size, iters, MODES.index(mode), ms, inject_dst, inject_word, gbps, errs,
                               first, peer, ctypes.byref(total))
    if rc == HUNG:
        return {"src": src, "mode": mode, "hung": True,
                "detail": lib().xgmi_last_error().decode(errors="replace"), "to": []}
    _check(rc)
    none = (1 << 64) - 1

    def sig4(x: float) -> float:  # 4 significant digits: a 16-byte self-test moves at a rate far below 0.1 GB/s
        return float(f"{x:.4g}")
    return {"src": src, "mode": mode, "total_gbps": sig4(total.value),
            "to": [{"dst": d, "gbps": sig4(gbps[i]), "errors": errs[i],
                    "first_bad": None if first[i] == none else first[i], "peer": bool(peer[i])}
                   for i, d in enumerate(dsts)]}


def kernel_matrix(devices: Optional[list] = None, mib: int = 256, iters: int = 5,
                  timeout_s: Optional[float] = None) -> Dict[str, Any]:
    """For every source of ``devices`` (default: all): each peer alone, store then load (``pairs``), then the fan to
    all its peers at once, store then load (``fan``).  Only distinct peers are passed, never the source.

    Rows are ``{"src", "dst", "mode", "gbps", "errors", "first_bad", "peer"}``.  ``median_gbps`` / ``min_gbps`` are per
    ``pair_store`` / ``pair_load`` / ``fan_store`` / ``fan_load``; ``bad`` = the rows with errors, ``slow`` = the rows
    under ``diag.P2P_MIN_FRACTION_OF_MEDIAN`` of the median of their own kind and mode (no absolute floor:
    ``KERNEL_MIN_GBPS``).  ``timeout_s`` bounds the whole matrix: each launch gets what is left of it, and the first
    that hangs, or a deadline passing between launches, ends it (``stopped``); a launch the library refused or that
    errored is named in ``failed`` and the matrix goes on."""
    from .diag import P2P_MIN_FRACTION_OF_MEDIAN
    devs = list(range(device_count())) if devices is None else list(devices)
    if len(devs) < 2:
        return {"skipped": f"{len(devs)} GPU(s): no pairs", "pairs": [], "fan": [], "bad": [], "slow": []}
    t0 = time.perf_counter()
    rows: Dict[str, List[Dict[str, Any]]] = {"pair": [], "fan": []}
    stopped = ""
    failed: List[str] = []

    def run(kind: str, src: int, peers: List[int], mode: str) -> bool:
        nonlocal stopped
        rest = None if not timeout_s else timeout_s - (time.perf_counter() - t0)
        name = f"kernel {mode} {src}->{peers[0]}" if kind == "pair" else f"kernel {mode} fan from {src}"
        if rest is not None and rest <= 0:
            stopped = f"deadline of {timeout_s:g} s passed before {name}"
            return False
        try:
            f = kernel_fan(src, peers, mib, iters, mode) if rest is None else \
                kernel_fan(src, peers, mib, iters, mode, timeout_s=rest)
        except RuntimeError as e:  # refused or errored (a pair without peer access): named, and the matrix goes on
            failed.append(f"{name}: {e}"[:200])
            return True
        if f.get("hung"):
            stopped = f"{name} hung: {f['detail']}"
            return False
        rows[kind] += [dict(t, src=src, mode=mode) for t in f["to"]]
        return True

    for a in devs:
        peers = [b for b in devs if b != a]
        jobs = [("pair", [b], m) for b in peers for m in MODES] + [("fan", peers, m) for m in MODES]
        if not all(run(kind, a, p, m) for kind, p, m in jobs):  # all() stops at the first that did not run
            break
    median: Dict[str, float] = {}
    lowest: Dict[str, float] = {}
    slow: List[Dict[str, Any]] = []
    for kind in ("pair", "fan"):
        for mode in MODES:
            of = [r for r in rows[kind] if r["mode"] == mode]
            rates = sorted(r["gbps"] for r in of) or [0.0]
            median[f"{kind}_{mode}"] = rates[len(rates) // 2]
            lowest[f"{kind}_{mode}"] = rates[0]
            slow += [dict(r, kind=kind) for r in of if r["gbps"] < P2P_MIN_FRACTION_OF_MEDIAN * rates[len(rates) // 2]]
    out: Dict[str, Any] = {"pairs": rows["pair"], "fan": rows["fan"], "median_gbps": median, "min_gbps": lowest,
                           "bad": [dict(r, kind=k) for k in ("pair", "fan") for r in rows[k] if r["errors"]],
                           "slow": slow, "wall_s": round(time.perf_counter() - t0, 3)}
    if failed:
        out["failed"] = failed
    if stopped:
        out["stopped"] = stopped
    return out
