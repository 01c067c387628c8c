"""Lanes diagnostic: ``libmi355x_lanes.so`` (csrc/lanes/lanes.hip) from Python.

Every other compute diagnostic keeps each lane's data in its own lane.  This one tests the hardware that moves a
value from one lane of a wave to another -- the DPP operand network of each SIMD, the gfx950 half exchanges
``v_permlane16_swap`` / ``v_permlane32_swap``, the LDS crossbar used without memory (``ds_bpermute``, ``ds_permute``,
``ds_swizzle``) and the VGPR <-> SGPR lane port (``v_readlane``, ``v_readfirstlane``) -- one native instruction per
op, in chains whose every step depends on the previous crossing.  A crossing only moves bits, so the words every wave
must end with come from the host's model of each instruction (csrc/lanes/lanes_ref.h; tests/test_lanes_cpu.py holds
the model against hand-worked tables), and every lane compares bit for bit.

Opt-in: no level runs it; ``ops/diag.run(extra=("lanes",))``, ``mi355x-diag --lanes``, ``node_cycle --lanes`` and the
agent's ``--diag-lanes`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name  # noqa: F401  (simd_name: part of this module's interface)
from .native import bind_cdll

# the native op index (LanesOp of lanes_ref.h): index into this
OPS = (
    "dpp_quad_perm_1032", "dpp_quad_perm_2301", "dpp_quad_perm_3210", "dpp_quad_perm_0000", "dpp_row_shl1",
    "dpp_row_shr1", "dpp_row_shr2", "dpp_row_shr3", "dpp_row_shr8", "dpp_row_ror1", "dpp_row_ror4", "dpp_wave_shl1",
    "dpp_wave_shr1", "dpp_wave_rol1", "dpp_wave_ror1", "dpp_row_mirror", "dpp_row_half_mirror", "dpp_row_bcast15",
    "dpp_row_bcast31", "dpp_row_shr1_bound_ctrl", "dpp_row_shr1_masked",
    "swizzle_xor1", "swizzle_xor2", "swizzle_xor4", "swizzle_xor8", "swizzle_xor16", "swizzle_reverse32",
    "swizzle_bcast0", "swizzle_quad_2031",
    "bpermute_xor32", "bpermute_rot1", "bpermute_seeded", "bpermute_gather", "permute_rot17", "permute_seeded",
    "permlane32_swap", "permlane16_swap", "readlane", "readfirstlane",
)
BPERMUTE_Y = "bpermute_y"  # apply() only (one past the table): ds_bpermute with ``y`` as the address register
CHAINS = 4         # independent chains per lane
WAVE = 64
THREADS = 256      # of a workgroup: 4 waves
BLOCKS_PER_CU = 4  # the default grid
DEFAULT_SEED = 0x1A7E5

_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/lanes/lanes.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_lanes_cpu.py holds it against the C source."""
    I, U, D, ULL, U64 = ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64
    pD, pU, pI, pW = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(ctypes.c_uint32)
    return {
        "lanes_last_error": (None, ctypes.c_char_p),
        "lanes_device_count": (None, I),
        "lanes_slots": (None, I),
        "lanes_test": ([I, I, I, I, ULL, U64, I, I, I, pU, pU, pU, pU, pD, pU, pI], None),
        "lanes_apply": ([I, I, U, pW, pW, pW, pW], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_lanes.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x lanes failed ({rc}): {lib().lanes_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().lanes_device_count())


def lanes_test(device: int = 0, ops: Sequence[str] = OPS, iters: int = 2000, reps: int = 5,
               blocks: Optional[int] = None, seed: int = DEFAULT_SEED, inject_op: Optional[str] = None,
               inject_block: int = -1, inject_skip_iter: int = -1, slots: bool = False) -> Dict[str, Any]:
    """Every op of ``ops`` on ``blocks`` workgroups of four waves (default: 4 per CU): a checked warm-up launch and
    ``reps`` timed, checked launches of ``iters`` steps of 4 chains per lane.  A wrong lane fails the test.

    ``errors`` counts wrong lanes over all launches; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs
    they lie on (``slots=True`` adds ``slots``, the map rows seen, for :func:`simd_name`).  Per op: ``errors``,
    ``first_bad`` (``where`` names the SIMD of one wrong lane as ``xcd5/se1/cu8/simd2``, with its ``lane``,
    ``chain``, ``got`` and ``want``; None when clean),
    ``ms`` (the mean time of a timed launch) and ``gops`` (crossings per second, in G/s).  ``bad_simds`` lists the
    SIMDs with wrong lanes, over all ops.

    The rates are reported and never judged: the project has measured them on one box
    (profiles/lanes_mi355x.json), which gives no reference.

    Self-check hooks (off by default), in the warm-up launch of ``inject_op`` on wave 0 of workgroup
    ``inject_block``: with ``inject_skip_iter`` < 0 one bit of lane 0's final chain-0 word is flipped before the
    compare (1 wrong lane, ``got == want ^ 0x10``); with a step given, the wave leaves the crossing out of that one
    step -- a crossing that did not happen (wrong lanes > 0)."""
    unknown = [k for k in ops if k not in OPS]
    if unknown or not ops or (inject_op is not None and inject_op not in ops):
        raise ValueError(f"ops must be of lanes.OPS and inject_op one of them, not {unknown or inject_op!r}")
    mask = 0
    for k in ops:
        mask |= 1 << OPS.index(k)
    L = lib()
    n, nrows = len(OPS), int(L.lanes_slots())
    arr = ctypes.c_ulonglong * n
    errs, first, got, want = arr(), arr(), arr(), arr()
    ms = (ctypes.c_double * n)()
    m = (ctypes.c_ulonglong * (3 * nrows))()
    ran = ctypes.c_int()
    t0 = time.perf_counter()
    _check(L.lanes_test(device, int(blocks or 0), int(iters), int(reps), mask, seed & ((1 << 64) - 1),
                        -1 if inject_op is None else OPS.index(inject_op), int(inject_block), int(inject_skip_iter),
                        errs, first, got, want, ms, m, ctypes.byref(ran)))
    none = (1 << 64) - 1
    rows: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    crossings = ran.value * THREADS * CHAINS * int(iters)
    for k in ops:
        i = OPS.index(k)
        bad = None
        if first[i] != none:
            bad = {"where": simd_name(int(first[i]) >> 16), "lane": (int(first[i]) >> 8) & 0xff,
                   "chain": int(first[i]) & 0xff, "got": f"0x{got[i]:08x}", "want": f"0x{want[i]:08x}"}
        rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4),
                   "gops": float(f"{crossings / (ms[i] * 1e-3) / 1e9:.4g}") if ms[i] > 0 else 0.0}
        if errs[i]:
            problems.append(f"{errs[i]} wrong lanes in {k}" + (f" on {bad['where']}" if bad else ""))
    seen, xcds, bad_simds = simd_map_summary(m, nrows)
    total = sum(r["errors"] for r in rows.values())
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen),
                           "xcds": xcds, "blocks": ran.value, "iters": int(iters),
                           "ops": rows, "ms": round(sum(r["ms"] for r in rows.values()), 4),
                           "wall_s": round(time.perf_counter() - t0, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    rows = r.get("ops") or {}
    rate = sum(v.get("gops", 0) for v in rows.values()) / len(rows) if rows else 0.0
    return (f"{len(rows)} ops x {r.get('iters', '?')} steps on {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} "
            f"XCDs, {r.get('errors', 0)} wrong lanes; {r.get('ms', 0):.1f} ms, mean {rate:.0f} G crossings/s")


def apply(op: str, x: Sequence[int], y: Optional[Sequence[int]] = None, iter: int = 0,
          device: int = 0) -> Tuple[List[int], List[int]]:
    """One application of ``op`` at step ``iter`` by one wave, returned raw: the two registers' 64 lanes after the
    instruction on ``x`` and ``y`` (default ``~x``, as in the chains).  ``op`` may also be :data:`BPERMUTE_Y`:
    ``ds_bpermute`` with ``y`` as the address register (lane i reads lane ``(y[i] >> 2) & 63``)."""
    if op != BPERMUTE_Y and op not in OPS:
        raise ValueError(f"op must be of lanes.OPS or {BPERMUTE_Y!r}, not {op!r}")
    if len(x) != WAVE or (y is not None and len(y) != WAVE):
        raise ValueError("x and y hold one word per lane of a 64-lane wave")
    words = ctypes.c_uint32 * WAVE
    xi = words(*[v & 0xffffffff for v in x])
    yi = words(*[(~v if y is None else y[i]) & 0xffffffff for i, v in enumerate(x)])
    xo, yo = words(), words()
    _check(lib().lanes_apply(device, len(OPS) if op == BPERMUTE_Y else OPS.index(op), int(iter) & 0xffffffff, xi, yi,
                             xo, yo))
    return list(xo), list(yo)
