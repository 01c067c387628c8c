"""Atomics diagnostic: ``libmi355x_atomics.so`` (csrc/atomics/atomics.hip) from Python.

On gfx950 a global atomic executes at the memory side, past the CU and the L2, so none of the other diagnostics can
show a broken atomic adder, an add lost when several XCDs hit one address, or a wrong returned value.  Here every
element of an array in ordinary device memory receives ``adders`` atomic operations from workgroups spread over the
XCDs, and every element is then held, bit for bit, against a value that does not depend on the order of arrival
(csrc/atomics/atomics_ref.h; tests/test_atomics_cpu.py proves the order-independence on the CPU).

Opt-in: no level runs it; ``ops/diag.run(extra=("atomics",))``, ``mi355x-diag --atomics``, ``node_cycle --atomics``
and the agent's ``--diag-atomics`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, Optional, Sequence, Tuple

from .native import bind_cdll

# the native kind index (AtomicsKind of atomics_ref.h): index into this
KINDS = ("add_u32", "add_u64", "add_f32", "add_f64", "pk_bf16", "max_u32", "xor_u32", "ticket")
ELEM_BYTES = {"add_u64": 8, "add_f64": 8}  # every other kind: 4
MAX_ADDERS = 32   # beyond it the float kinds' partial sums are no longer exact: refused by the library
XCDS = 8
DEFAULT_SEED = 0xA70C5

_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/atomics/atomics.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_atomics_cpu.py holds it against the C source."""
    I, Z, D, LL, U, U64 = (ctypes.c_int, ctypes.c_size_t, ctypes.c_double, ctypes.c_longlong, ctypes.c_uint,
                           ctypes.c_uint64)
    pD, pU = ctypes.POINTER(D), ctypes.POINTER(ctypes.c_ulonglong)
    return {
        "atomics_last_error": (None, ctypes.c_char_p),
        "atomics_device_count": (None, I),
        "atomics_test": ([I, Z, I, U, U64, I, I, LL, I] + [pU] * 7 + [pD], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_atomics.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x atomics failed ({rc}): {lib().atomics_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().atomics_device_count())


def elem_bytes(kind: str) -> int:
    return ELEM_BYTES.get(kind, 4)


def atomics_test(device: int = 0, words: int = 16 << 20, adders: int = 8, kinds: Sequence[str] = KINDS,
                 seed: int = DEFAULT_SEED, iters: int = 3, inject_kind: Optional[str] = None, inject_word: int = 0,
                 inject_drop_adder: int = -1) -> Dict[str, Any]:
    """Every kind of ``kinds`` on ``words`` elements with ``adders`` atomic operations each (1..32), ``iters``
    times: fill, atomics, verify.  A wrong element fails the test.

    Per kind: ``errors`` (wrong elements over all iterations), ``first_bad`` (the lowest wrong element, None: none)
    with ``got`` / ``want`` as hex strings, ``ops`` (atomic operations one launch issued, counted by the kernel),
    ``xcds`` (how many XCDs' waves took part, from ``XCC_ID``; ``waves`` has the count per XCD) and ``gbs`` (bytes of
    operands applied per second, in GB/s, from ``ms``, the mean time of a timed launch).  The ``ticket`` kind draws
    tickets with returning adds on at most 2^20 elements; its elements are its hit words, then its counters.

    The rate is reported and never judged: the project has measured no reference rate for these kernels on a second
    device (profiles/atomics_mi355x.json is one box).

    A wrong element is located by address only -- ``detail`` gives its byte offset into the test's array.  The
    project has no map from an address to an HBM stack or channel, so no unit is named.

    Self-check hooks (off by default), on element ``inject_word`` of ``inject_kind`` in the last iteration: with
    ``inject_drop_adder`` < 0 the host flips one bit of it between the atomics and the verify launch; with an adder
    given, the one lane that would apply that adder's operation skips it, and the kind's ``want_without`` is the
    reference value without that operand (computed by the library from atomics_ref.h), which ``got`` must equal: a lost
    add, told from a flipped bit."""
    unknown = [k for k in kinds if k not in KINDS]
    if unknown or (inject_kind is not None and inject_kind not in kinds):
        raise ValueError(f"kinds must be of {KINDS} and inject_kind one of them, not {unknown or inject_kind!r}")
    mask = 0
    for k in kinds:
        mask |= 1 << KINDS.index(k)
    n = len(KINDS)
    arr = ctypes.c_ulonglong * n
    errs, first, got, want, without, ops = arr(), arr(), arr(), arr(), arr(), arr()
    waves = (ctypes.c_ulonglong * (XCDS * n))()
    ms = (ctypes.c_double * n)()
    t0 = time.perf_counter()
    _check(lib().atomics_test(device, int(words), int(adders), mask, seed & ((1 << 64) - 1), int(iters),
                              -1 if inject_kind is None else KINDS.index(inject_kind), int(inject_word),
                              int(inject_drop_adder), errs, first, got, want, without, ops, waves, ms))
    none = (1 << 64) - 1
    rows: Dict[str, Dict[str, Any]] = {}
    problems = []
    for k in kinds:
        i = KINDS.index(k)
        per_xcd = [int(waves[XCDS * i + x]) for x in range(XCDS)]
        bad = None if first[i] == none else int(first[i])
        width = 2 * elem_bytes(k)
        row: Dict[str, Any] = {"errors": int(errs[i]), "first_bad": bad,
                               "got": None if bad is None else f"0x{got[i]:0{width}x}",
                               "want": None if bad is None else f"0x{want[i]:0{width}x}",
                               "ops": int(ops[i]), "xcds": sum(1 for w in per_xcd if w), "waves": per_xcd,
                               "ms": round(ms[i], 4),
                               "gbs": float(f"{ops[i] * elem_bytes(k) / (ms[i] * 1e-3) / 1e9:.4g}") if ms[i] > 0 else 0.0}
        if k == inject_kind and inject_drop_adder >= 0:
            row["want_without"] = f"0x{without[i]:0{width}x}"
        rows[k] = row
        if errs[i]:
            where = (f" (first at +0x{bad * elem_bytes(k):x}: got {row['got']}, want {row['want']})" if bad is not None
                     else " (tickets returned out of range)")
            problems.append(f"{errs[i]} elements wrong in {k}{where}")
    total = sum(r["errors"] for r in rows.values())
    return {"pass": total == 0, "errors": total, "kinds": rows, "words": int(words), "adders": int(adders),
            "ms": {k: r["ms"] for k, r in rows.items()}, "wall_s": round(time.perf_counter() - t0, 3),
            "detail": "; ".join(problems)}


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    kinds = r.get("kinds") or {}
    xcds = sorted({v.get("xcds") for v in kinds.values()} - {None})
    rates = " · ".join(f"{k} {v.get('gbs', 0):.0f}" for k, v in kinds.items())
    return (f"{r.get('words', '?')} elements x {r.get('adders', '?')} adders from "
            f"{'/'.join(map(str, xcds)) or '?'} XCDs, {r.get('errors', 0)} wrong; {rates} GB/s")
