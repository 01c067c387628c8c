"""Cvt diagnostic: ``libmi355x_cvt.so`` (csrc/cvt/cvt.hip) from Python.

Every quantised workload narrows its activations through the vector ALU's format converters and widens them back, and
no other diagnostic executes one.  This one runs every conversion of :data:`OPS` -- the classic ones (f16 / f32 / f64 /
integers, ``pkrtz``, ``pknorm``, ``pk_u8``, ``rpi``, ``flr``, ``off_i4``), bf16, fp8 / bf8 with every byte and word
select, and the gfx950 ``scalef32`` forms of fp8, bf8, fp4, fp6 and bf6 from and to f32, f16 and bf16 -- one native
instruction per op, in chains whose every
step's operands are shaped from the previous result towards ties, the largest finite result, subnormals and +-0.  An
in-range conversion has one correct result, so the words every wave must end with come from the host's model
(csrc/cvt/cvt_ref.h, which states the operand domain; tests/test_cvt_cpu.py holds the model against an exact referee),
and every lane compares bit for bit.

Not built: the stochastic-rounding group (cvt_ref.h).  NaN, Inf and overflowing sources lie outside the model's domain;
:func:`apply_many` returns what the device makes of them.

Opt-in: no level runs it; ``ops/diag.run(extra=("cvt",))``, ``mi355x-diag --cvt``, ``node_cycle --cvt`` and the
agent's ``--diag-cvt`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name  # noqa: F401  (simd_name: part of this module's interface)
from .native import bind_cdll

# the native op index (CvtOp of cvt_ref.h): index into OPS
CLASSIC = ("f16_f32", "f32_f16", "f32_f64", "f64_f32", "i32_f32", "u32_f32", "i32_f64", "u32_f64", "f32_i32", "f32_u32",
           "f64_i32", "f64_u32", "f32_ubyte0", "f32_ubyte1", "f32_ubyte2", "f32_ubyte3", "pkrtz_f16_f32", "pknorm_i16_f32",
           "pknorm_u16_f32", "pk_u8_f32", "rpi_i32_f32", "flr_i32_f32", "off_f32_i4", "f16_u16", "f16_i16", "u16_f16",
           "i16_f16")
BF16 = ("pk_bf16_f32", "f32_bf16")
FP8 = tuple(f"f32_{f}_b{b}" for f in ("fp8", "bf8") for b in range(4)) + tuple(
    f"pk_f32_{f}_{h}" for f in ("fp8", "bf8") for h in ("lo", "hi")) + tuple(
    f"pk_{f}_f32_{h}" for f in ("fp8", "bf8") for h in ("lo", "hi"))
SCALEF32 = tuple(f"scalef32_pk_{f}_f32_{h}" for f in ("fp8", "bf8") for h in ("lo", "hi")) + tuple(
    f"scalef32_pk_f32_{f}_{h}" for f in ("fp8", "bf8") for h in ("lo", "hi")) + tuple(
    f"scalef32_f32_{f}_b{b}" for f in ("fp8", "bf8") for b in range(4)) + tuple(
    f"scalef32_pk_fp4_f32_b{b}" for b in range(4)) + tuple(f"scalef32_pk_f32_fp4_b{b}" for b in range(4)) + tuple(
    f"scalef32_pk_{f}_{t}_{h}" for f in ("fp8", "bf8") for t in ("f16", "bf16") for h in ("lo", "hi")) + tuple(
    f"scalef32_pk_{t}_{f}_{h}" for f in ("fp8", "bf8") for t in ("f16", "bf16") for h in ("lo", "hi")) + tuple(
    f"scalef32_f16_{f}_b{b}_{h}" for f in ("fp8", "bf8") for h in ("lo", "hi") for b in range(4)) + tuple(
    f"scalef32_pk_fp4_{t}_b{b}" for t in ("f16", "bf16") for b in range(4)) + tuple(
    f"scalef32_pk_{t}_fp4_b{b}" for t in ("f16", "bf16") for b in range(4)) + tuple(
    f"scalef32_2xpk16_{f}_f32" for f in ("fp6", "bf6")) + tuple(
    f"scalef32_pk32_{f}_{t}" for f in ("fp6", "bf6") for t in ("f16", "bf16")) + tuple(
    f"scalef32_pk32_{t}_{f}" for f in ("fp6", "bf6") for t in ("f32", "f16", "bf16"))
GROUPS = {"classic": CLASSIC, "bf16": BF16, "fp8": FP8, "scalef32": SCALEF32}
OPS = CLASSIC + BF16 + FP8 + SCALEF32
CHAINS = 4         # independent chains per lane
WAVE = 64
THREADS = 256      # of a workgroup: 4 waves
BLOCKS_PER_CU = 4  # the default grid
DEFAULT_SEED = 0xC0A7E5
# the default shape: chosen so the whole test costs per GPU and cycle no more than the lanes test does
# (profiles/cvt_mi355x.json)
DEFAULT_ITERS = 32
MODE_ROUND_NEAREST_EVEN, MODE_DENORM_KEPT = 0, 15  # the float mode the model holds for

_lib: Optional[ctypes.CDLL] = None
_NONE = (1 << 64) - 1


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/cvt/cvt.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_cvt_cpu.py holds it against the C source."""
    I, D, ULL, U64 = ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64
    pD, pU, pI, pW, pB = (ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(ctypes.c_uint),
                          ctypes.POINTER(ctypes.c_ubyte))
    return {
        "cvt_last_error": (None, ctypes.c_char_p),
        "cvt_device_count": (None, I),
        "cvt_slots": (None, I),
        "cvt_ops": (None, I),
        "cvt_row_words": ([I, pI, pI], None),
        "cvt_shape_rows": ([I, U64, I, pW], None),
        "cvt_model_rows": ([I, pW, I, pW, pB], None),
        "cvt_test": ([I, I, I, I, pI, I, U64, I, I, I, pU, pU, pD, pW, pU, pI], None),
        "cvt_apply_many": ([I, I, pW, I, pW], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_cvt.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x cvt failed ({rc}): {lib().cvt_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().cvt_device_count())


def cvt_test(device: int = 0, ops: Sequence[str] = OPS, iters: int = DEFAULT_ITERS, reps: int = 3,
             blocks: Optional[int] = None, seed: int = DEFAULT_SEED, inject_op: Optional[str] = None,
             inject_block: int = -1, inject_skip_iter: int = -1, slots: bool = False) -> Dict[str, Any]:
    """Every op of ``ops`` on ``blocks`` workgroups of four waves (default: 4 per CU): a checked warm-up launch and
    ``reps`` timed, checked launches of ``iters`` steps of 4 chains per lane.  A wrong word fails the test.

    ``errors`` counts wrong chain words over all launches; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many
    XCDs they lie on (``slots=True`` adds ``slots``, the map rows seen, for :func:`simd_name`).  Per op: ``errors``,
    ``first_bad`` (``where`` names the SIMD of one wrong word as ``xcd5/se1/cu8/simd2``, with its ``lane``, ``chain``,
    ``got`` and ``want``; None when clean), ``ms`` (the mean time of a timed launch) and ``gops`` (conversion
    instructions per second over all lanes, in G/s).  ``bad_simds`` lists the SIMDs with wrong words, over all ops.
    ``mode`` is the float mode the waves ran in (``round`` and ``denorm``: MODE.FP_ROUND and MODE.FP_DENORM, with
    ``nearest_even`` and ``denormals_kept`` true when they are what the model holds for; under another mode the
    library refuses to judge and this raises).

    The rates are reported and never judged: the project has measured them on one box (profiles/cvt_mi355x.json),
    which gives no reference.

    Self-check hooks (off by default), in the warm-up launch of ``inject_op`` on wave 0 of workgroup
    ``inject_block``: with ``inject_skip_iter`` < 0 one bit of lane 0's final chain-0 word is flipped before the
    compare (1 wrong word, ``got == want ^ 0x10``); with a step given, the wave leaves the conversion out of that one
    step (wrong words > 0, in that op only)."""
    unknown = [k for k in ops if k not in OPS]
    if unknown or not ops or len(set(ops)) != len(ops) or (inject_op is not None and inject_op not in ops):
        raise ValueError(f"ops must be distinct names of cvt.OPS and inject_op one of them, not {unknown or inject_op!r}")
    L = lib()
    n, nrows = len(OPS), int(L.cvt_slots())
    chosen = (ctypes.c_int * len(ops))(*[OPS.index(k) for k in ops])
    errs, first, ms = (ctypes.c_ulonglong * n)(), (ctypes.c_ulonglong * (4 * n))(), (ctypes.c_double * n)()
    m = (ctypes.c_ulonglong * (3 * nrows))()
    mode, ran = ctypes.c_uint(), ctypes.c_int()
    t0 = time.perf_counter()
    _check(L.cvt_test(device, int(blocks or 0), int(iters), int(reps), chosen, len(ops), seed & _NONE,
                      -1 if inject_op is None else OPS.index(inject_op), int(inject_block), int(inject_skip_iter),
                      errs, first, ms, ctypes.byref(mode), m, ctypes.byref(ran)))
    rows: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    count = ran.value * THREADS * CHAINS * int(iters)
    for k in ops:
        i = OPS.index(k)
        bad = None
        where = int(first[4 * i])
        if where != _NONE:
            bad = {"where": simd_name(where >> 16), "lane": (where >> 8) & 0xff, "chain": where & 0xff,
                   "got": f"0x{first[4 * i + 2]:08x}", "want": f"0x{first[4 * i + 3]:08x}"}
        rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4),
                   "gops": float(f"{count / (ms[i] * 1e-3) / 1e9:.4g}") if ms[i] > 0 else 0.0}
        if errs[i]:
            problems.append(f"{errs[i]} wrong words in {k}" + (f" on {bad['where']}" if bad else ""))
    seen, xcds, bad_simds = simd_map_summary(m, nrows)
    total = sum(r["errors"] for r in rows.values())
    rnd, den = mode.value & 0xf, (mode.value >> 4) & 0xf
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen), "xcds": xcds, "blocks": ran.value,
                           "iters": int(iters), "ops": rows,
                           "mode": {"round": rnd, "denorm": den, "nearest_even": rnd == MODE_ROUND_NEAREST_EVEN,
                                    "denormals_kept": den == MODE_DENORM_KEPT},
                           "ms": round(sum(r["ms"] for r in rows.values()), 4),
                           "wall_s": round(time.perf_counter() - t0, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    rows, mode = r.get("ops") or {}, r.get("mode") or {}
    rate = sum(v.get("gops", 0) for v in rows.values()) / len(rows) if rows else 0.0
    return (f"{len(rows)} ops x {r.get('iters', '?')} steps on {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} "
            f"XCDs, round {mode.get('round', '?')} denorm {mode.get('denorm', '?')}, {r.get('errors', 0)} wrong words; "
            f"{r.get('ms', 0):.1f} ms, mean {rate:.0f} G conversions/s")


Row = Tuple[int, ...]
WIDE = 32  # values per lane of a wide form


def row_words_of(op: str) -> Tuple[int, int]:
    """:func:`row_words` from the op's name alone (no library needed)."""
    if op not in OPS:
        raise ValueError(f"op must be of cvt.OPS, not {op!r}")
    return (WIDE + 1, WIDE) if "_2xpk16_" in op or "_pk32_" in op else (4, 2)


def row_words(op: str) -> Tuple[int, int]:
    """The words of one operand row and of one result row of ``op``: 4 (``a, b, c, s``) and 2 (the result registers),
    or, for the wide forms (fp6 / bf6: 32 values per lane), 33 (32 words of values, then the scale's fp32 bits) and
    32.  32 fp32 values take a word each (``2xpk16``: the first source's 16, then the second's); 32 f16 / bf16 values
    take words 0..15, value j in half ``j % 2`` of word ``j // 2``; 32 six-bit codes take words 0..5, code j in bits
    ``6 j .. 6 j + 5`` of the 192.  Words an op does not use are 0."""
    if op not in OPS:
        raise ValueError(f"op must be of cvt.OPS, not {op!r}")
    a, b = ctypes.c_int(), ctypes.c_int()
    _check(lib().cvt_row_words(OPS.index(op), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def _rows_array(rows: Sequence[Sequence[int]]) -> Any:
    flat = [int(v) & 0xffffffff for r in rows for v in r]
    return (ctypes.c_uint * len(flat))(*flat)


def _checked_rows(op: str, rows: Sequence[Sequence[int]]) -> Tuple[int, int]:
    iw, ow = row_words(op)
    if not rows or any(len(r) != iw for r in rows):
        raise ValueError(f"every operand row of {op} holds {iw} words (cvt.row_words)")
    return iw, ow


def shaped_rows(op: str, n: int, seed: int = DEFAULT_SEED) -> List[Row]:
    """The operand rows (:func:`row_words`) the chains' shape gives ``n`` chain words drawn from ``seed`` (host only).
    A row of four is ``(a, b, c, s)``: two sources (a 64-bit source: low, high), the destination before the
    instruction, the scale's fp32 bits."""
    iw, _ = row_words(op)
    out = (ctypes.c_uint * (iw * n))()
    _check(lib().cvt_shape_rows(OPS.index(op), seed & _NONE, int(n), out))
    return [tuple(out[iw * i:iw * (i + 1)]) for i in range(n)]


def model(op: str, rows: Sequence[Sequence[int]]) -> List[Optional[Row]]:
    """The host model's result row per operand row; None where the operands lie outside the model's domain
    (cvt_ref.h).  Host only."""
    _, ow = _checked_rows(op, rows)
    n = len(rows)
    out, ok = (ctypes.c_uint * (ow * n))(), (ctypes.c_ubyte * n)()
    _check(lib().cvt_model_rows(OPS.index(op), _rows_array(rows), n, out, ok))
    return [tuple(out[ow * i:ow * (i + 1)]) if ok[i] else None for i in range(n)]


def apply_many(op: str, rows: Sequence[Sequence[int]], device: int = 0) -> List[Row]:
    """Single applications of ``op`` by one wave, returned raw: per operand row (as :func:`shaped_rows`) the result
    registers after the instruction (:func:`row_words`; a register the op does not write is 0; a 16-bit result is the
    first word's low half).  Lane ``i % 64`` of wave-row ``i // 64`` applies row ``i``; the last wave-row is padded
    with its own last row.  Any operand may be given: NaN, Inf and overflowing sources are probed this way."""
    _, ow = _checked_rows(op, rows)
    n = len(rows)
    padded = list(rows) + [rows[-1]] * (-n % WAVE)
    nrows = len(padded) // WAVE
    out = (ctypes.c_uint * (ow * len(padded)))()
    _check(lib().cvt_apply_many(device, OPS.index(op), _rows_array(padded), nrows, out))
    return [tuple(out[ow * i:ow * (i + 1)]) for i in range(n)]
