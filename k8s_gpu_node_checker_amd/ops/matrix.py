"""Matrix diagnostic: ``libmi355x_matrix.so`` (csrc/matrix/matrix.hip) from Python.

The matrix-core burn-in runs four encodings of one 16x16 shape on ``{-1, 0, +1}`` operands and checks a lane sum, and
the GEMMs sample their outputs against a tolerance.  This one issues the MFMA families the MI355X has -- fp32, fp16, bf16,
int8 and fp64 inputs, the gfx94x-era bf8 instructions, the bf8 / fp6 / bf6 / fp4 formats of ``f8f6f4`` with and
without block scales in both shapes, and the gfx94x-era sparse ``v_smfmac_*`` (34 ops; matrix_ref.h names the ones
left out because the device disagreed with the model) -- one native instruction per op, four dependent steps per
round, and compares every element of the accumulator bit for bit with the host's model (csrc/matrix/matrix_ref.h;
tests/test_matrix_cpu.py holds the model against an independent exact matmul).  The operands obey the header's
exactness rule (every partial sum in any order is exactly representable), so the result has one value.

Opt-in: no level runs it; ``ops/diag.run(extra=("matrix",))``, ``mi355x-diag --matrix``, ``node_cycle --matrix`` and
the agent's ``--diag-matrix`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary
from .lanes import simd_name
from .native import bind_cdll

# the native op index (MATRIX_OP_TABLE of matrix_ref.h): index into this
OPS = (
    "f32_32x32x2_f32", "f32_16x16x4_f32",
    "f32_32x32x8_f16", "f32_16x16x16_f16", "f32_32x32x16_f16", "f32_16x16x32_f16",
    "f32_32x32x8_bf16_1k", "f32_16x16x16_bf16_1k", "f32_32x32x16_bf16", "f32_16x16x32_bf16",
    "i32_16x16x32_i8", "i32_16x16x64_i8",
    "f64_16x16x4_f64",
    "f32_16x16x32_bf8_bf8",
    "f32_32x32x16_bf8_bf8",
    "f8f6f4_16x16x128_bf8", "f8f6f4_16x16x128_fp6", "f8f6f4_16x16x128_bf6",
    "f8f6f4_16x16x128_fp4", 
    "f8f6f4_16x16x128_scale_fp6", "f8f6f4_16x16x128_scale_fp4",
    "f8f6f4_32x32x64_bf8", "f8f6f4_32x32x64_fp6", "f8f6f4_32x32x64_bf6",
    "f8f6f4_32x32x64_fp4", 
    "f8f6f4_32x32x64_scale_fp6", "f8f6f4_32x32x64_scale_fp4",
    "smfmac_f32_16x16x32_f16", "smfmac_f32_32x32x16_f16", 
    "smfmac_f32_16x16x32_bf16", "smfmac_f32_32x32x16_bf16", 
    "smfmac_i32_16x16x64_i8", 
    
    
    "smfmac_f32_16x16x64_bf8_bf8", "smfmac_f32_32x32x32_bf8_bf8", 
    
)
STEPS = 4          # dependent instructions per round
WAVE = 64
THREADS = 256      # of a workgroup: 4 waves
BLOCKS_PER_CU = 2  # the default grid
AW, CW = 8, 16     # words per lane of apply()'s A / B and C / D register blocks
DEFAULT_ITERS = 8000  # the whole test then costs about what the lanes test costs (profiles/matrix_mi355x.json)
DEFAULT_SEED = 0x3A7121

_lib: Optional[ctypes.CDLL] = None


def shape(op: str) -> Tuple[int, int, int]:
    """(M, N, K) of an op, read from its name; K is the dense K, for the sparse ops too."""
    m, n, k = next(f for f in op.split("_") if f[0].isdigit() and "x" in f).split("x")
    return int(m), int(n), int(k)


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/matrix/matrix.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_matrix_cpu.py holds it against the C source."""
    I, D, ULL, U64 = ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64
    pD, pU, pI, pW = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(ctypes.c_uint32)
    return {
        "matrix_last_error": (None, ctypes.c_char_p),
        "matrix_device_count": (None, I),
        "matrix_slots": (None, I),
        "matrix_test": ([I, I, I, I, pI, I, U64, I, I, I, pU, pU, pU, pU, pD, pU, pI], None),
        "matrix_apply": ([I, I, pW, pW, pW, pW, pW, pW, pW], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_matrix.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x matrix failed ({rc}): {lib().matrix_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().matrix_device_count())


def matrix_test(device: int = 0, ops: Sequence[str] = OPS, iters: int = DEFAULT_ITERS, reps: int = 3,
                blocks: Optional[int] = None, seed: int = DEFAULT_SEED, inject_op: Optional[str] = None,
                inject_block: int = -1, inject_skip_step: int = -1, slots: bool = False) -> Dict[str, Any]:
    """Every op of ``ops`` on ``blocks`` workgroups of four waves (default: 2 per CU): a checked warm-up launch and
    ``reps`` timed, checked launches of ``iters`` rounds of 4 dependent instructions, every element of the
    accumulator compared with the model after every round.  A wrong element fails the test.

    ``errors`` counts wrong elements over all launches; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many
    XCDs they lie on (``slots=True`` adds ``slots``, the map rows seen, for :func:`simd_name`).  Per op: ``errors``,
    ``first_bad`` (``where`` names the SIMD of one wrong element as ``xcd5/se1/cu8/simd2``, with its ``lane``,
    ``reg``, ``got`` and ``want``; None when clean), ``ms`` (the mean time of a timed launch) and ``tops``
    (2 * M * N * K operations per instruction, in TFLOP/s or, for int8, TOP/s; the sparse ops are counted on the
    dense K, as the vendor's figures are).  ``bad_simds`` lists the SIMDs with wrong elements, over all ops.

    The rates are reported and never judged: the project has measured them on one box
    (profiles/matrix_mi355x.json), which gives no reference, and a round's four dependent instructions on one
    accumulator measure latency as much as throughput.

    Self-check hooks (off by default), in the warm-up launch of ``inject_op`` on wave 0 of workgroup
    ``inject_block``: with ``inject_skip_step`` < 0 one bit of lane 0's register 0 of the last round's accumulator
    is flipped before the compare (1 wrong element, ``got == want ^ 0x10``); with a step 0..3 given, the wave leaves
    that one instruction out of its last round (wrong elements > 0)."""
    unknown = [k for k in ops if k not in OPS]
    if unknown or not ops or len(set(ops)) != len(ops) or (inject_op is not None and inject_op not in ops):
        raise ValueError(f"ops must be distinct names of matrix.OPS and inject_op one of them, not {unknown or inject_op!r}")
    L = lib()
    n, nrows = len(OPS), int(L.matrix_slots())
    chosen = (ctypes.c_int * len(ops))(*[OPS.index(k) for k in ops])
    arr = ctypes.c_ulonglong * n
    errs, first, got, want = arr(), arr(), arr(), arr()
    ms = (ctypes.c_double * n)()
    m = (ctypes.c_ulonglong * (3 * nrows))()
    ran = ctypes.c_int()
    t0 = time.perf_counter()
    _check(L.matrix_test(device, int(blocks or 0), int(iters), int(reps), chosen, len(ops), seed & ((1 << 64) - 1),
                         -1 if inject_op is None else OPS.index(inject_op), int(inject_block), int(inject_skip_step),
                         errs, first, got, want, ms, m, ctypes.byref(ran)))
    none = (1 << 64) - 1
    rows: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    for k in ops:
        i = OPS.index(k)
        bad = None
        if first[i] != none:
            width = 16 if k.startswith("f64") else 8
            bad = {"where": simd_name(int(first[i]) >> 16), "lane": (int(first[i]) >> 8) & 0xff,
                   "reg": int(first[i]) & 0xff, "got": f"0x{got[i]:0{width}x}", "want": f"0x{want[i]:0{width}x}"}
        M, N, K = shape(k)
        work = 2.0 * M * N * K * STEPS * int(iters) * ran.value * (THREADS // WAVE)
        rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4),
                   "tops": float(f"{work / (ms[i] * 1e-3) / 1e12:.4g}") if ms[i] > 0 else 0.0}
        if errs[i]:
            problems.append(f"{errs[i]} wrong elements in {k}" + (f" on {bad['where']}" if bad else ""))
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
    return (f"{len(rows)} ops x {r.get('iters', '?')} rounds on {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} "
            f"XCDs, {r.get('errors', 0)} wrong elements; {r.get('ms', 0):.1f} ms")


def apply(op: str, a: Sequence[int], b: Sequence[int], c: Sequence[int], idx: Optional[Sequence[int]] = None,
          scale_a: Optional[Sequence[int]] = None, scale_b: Optional[Sequence[int]] = None,
          device: int = 0) -> List[int]:
    """One application of ``op`` by one wave on raw per-lane registers, returned raw: ``a`` and ``b`` hold 8 words
    per lane (lane l's block at ``8 * l``; the words past the op's own are ignored), ``c`` and the result 16 words per
    lane; ``idx`` (sparse ops) and the scales (scaled ops: byte 0 is the E8M0 code) one word per lane."""
    if op not in OPS:
        raise ValueError(f"op must be of matrix.OPS, not {op!r}")
    if len(a) != WAVE * AW or len(b) != WAVE * AW or len(c) != WAVE * CW:
        raise ValueError("a and b hold 8 words per lane of a 64-lane wave, c holds 16")
    per_lane = [[0] * WAVE if v is None else list(v) for v in (idx, scale_a, scale_b)]
    if any(len(v) != WAVE for v in per_lane):
        raise ValueError("idx and the scales hold one word per lane")
    words = lambda v: (ctypes.c_uint32 * len(v))(*[int(x) & 0xffffffff for x in v])
    d = (ctypes.c_uint32 * (WAVE * CW))()
    _check(lib().matrix_apply(device, OPS.index(op), words(a), words(b), words(c), *[words(v) for v in per_lane], d))
    return list(d)

