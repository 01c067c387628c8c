"""Scratch diagnostic: ``libmi355x_scratch.so`` (csrc/scratch/scratch.hip) from Python.

Every other diagnostic is built to have no private (scratch) memory, and every other library refuses a build that has
some.  This one tests it: the frame base the dispatcher hands every wave slot, the compiler's own scratch accesses,
generic pointers into private memory at call depth and the backing store the runtime hands out.  Every kernel that
spills, indexes a local array at run time or passes a local by pointer rests on these.  Two parts, every row selectable
by name (:data:`ROWS`):

``isolate/1k``    no two resident waves share a frame: a grid of twice the device's wave slots, each wave writing a
                  1 KiB-per-lane frame, dwelling a constant time and reading it back, round after round; the written
                  word is a bijection of (round, wave, lane, word), so a wrong word is classified ``alias`` (another
                  wave's, lane's or word's: the writer is named), ``stale`` (the same cell of an earlier round, with its
                  age) or ``corrupt``
``frames/index``, ``frames/calls``  what the compiler does with locals: a runtime-indexed local array, and a chain of
                  four functions with a buffer each and the caller's by pointer, run on both sides, compared bit for bit

A third part, a table of the ``scratch_*`` instruction forms, is not here: csrc/scratch/scratch_ref.h says why.

Opt-in: no level runs it; ``ops/diag.run(extra=("scratch",))``, ``mi355x-diag --scratch``, ``node_cycle --scratch``
and the agent's ``--diag-scratch`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name
from .native import bind_cdll

ISOLATE_ROW = "isolate/1k"
FRAMES_ROWS = ("frames/index", "frames/calls")
ROWS = (ISOLATE_ROW,) + FRAMES_ROWS  # the native row index is the position here
CLASSES = (None, "alias", "stale", "corrupt")  # ScratchClass
THREADS = 256
ISO_WORDS = 256        # the isolate frame: 1 KiB per lane
ISO_MAX_WAVES = 16384  # the wave's field of the written word: 14 bits
ISO_MAX_ROUNDS = 16
FRAMES_OUT = 17
DEFAULT_ROUNDS = 4
DEFAULT_REPS = 1
DEFAULT_SEED = 0x5C7A7C11

_NONE = (1 << 64) - 1
_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/scratch/scratch.hip: name -> (argtypes, restype); None leaves ctypes' default (no
    declared arguments / an int result).  tests/test_scratch_cpu.py holds it against the C source."""
    I, D, ULL, U32 = ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint32
    pD, pU, pI = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I)
    return {
        "scratch_last_error": (None, ctypes.c_char_p),
        "scratch_device_count": (None, I),
        "scratch_slots": (None, I),
        "scratch_rows": (None, I),
        "scratch_test": ([I, pI, I, I, I, I, I, U32, I, I, I, I, I, pU, pU, pD, pU, pI, pU, pU], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_scratch.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x scratch failed ({rc}): {lib().scratch_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().scratch_device_count())


def words_per_launch(row: str, blocks: int, rounds: int = DEFAULT_ROUNDS) -> int:
    """What one launch of ``row`` compares on ``blocks`` workgroups (for ``isolate/1k``: of the isolate grid)."""
    lanes = blocks * THREADS
    if row == ISOLATE_ROW:
        return lanes * ISO_WORDS * rounds
    return lanes * FRAMES_OUT


def scratch_test(device: int = 0, rows: Sequence[str] = ROWS, blocks: Optional[int] = None,
                 isolate_blocks: Optional[int] = None, rounds: int = DEFAULT_ROUNDS, reps: int = DEFAULT_REPS,
                 seed: int = DEFAULT_SEED, inject_row: Optional[str] = None,
                 inject_wave: int = 0, inject_round: Optional[int] = None, inject_alias: bool = False,
                 inject_stale_word: Optional[int] = None, slots: bool = False) -> Dict[str, Any]:
    """The rows named in ``rows``, each with a checked warm-up launch and ``reps`` timed, checked launches.  The
    ``frames`` rows run ``blocks`` workgroups of 256 threads (default: one per CU); ``isolate/1k`` runs
    ``isolate_blocks`` workgroups (default: twice the device's wave slots, 2 x CUs x 32 waves; more than 16,384 waves are
    refused) for ``rounds`` rounds.  Any wrong word fails the test.

    ``errors`` counts wrong words over all rows; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs they lie
    on (``slots=True`` adds ``slots``, the map rows seen).  ``rows`` holds per row ``errors``, ``words_checked`` over its
    ``launches`` (``reps`` + 1), ``ms`` (the mean time of a timed launch), ``frame_bytes`` (the kernel's private segment
    per lane) and ``first_bad``: None when clean, else ``where`` (the SIMD that read the word, ``xcd5/se1/cu8/simd2``),
    ``lane``, ``wave``, ``word`` (isolate: the cell's word, with its ``round``; frames: the output word), ``got``, ``want``,
    ``class`` (``alias``, ``stale`` or ``corrupt``; a word the host's model disagrees with is ``corrupt``), ``age``
    (rounds), ``writer`` (an alias: ``{"wave", "where"}`` of the wave whose word it is and the SIMD that one ran on)
    and ``launch`` (0: the warm-up).

    ``frame_bytes`` is the private segment per kernel part, ``co_resident_waves`` the most isolate frames that were
    live at one time by the waves' own clocks, ``backing_bytes`` / ``backing_peak_bytes`` the free device memory the
    first isolate launch of the call took and still held afterwards / held at most while it ran (0 when the process
    already held it).  These and the times are reported and never judged.

    Self-check hooks (off by default), in the warm-up launch of row ``inject_row`` on wave ``inject_wave``: by default
    a flipped bit before the compare (exactly 1 wrong word, ``got == want ^ 0x10``, ``corrupt``); on ``isolate/1k``
    also ``inject_alias=True`` (the compare is given the word that wave + 1 wrote to the same cell: 1 wrong word,
    ``alias``, that writer named) and ``inject_stale_word=i`` in ``inject_round`` >= 1 (default 1; lane 0 skips writing
    word ``i``, so it reads the round before: 1 wrong word, ``stale``, ``age`` 1 -- real, not substituted)."""
    rows = list(rows)
    unknown = [k for k in rows if k not in ROWS]
    if unknown or not rows or len(set(rows)) != len(rows) or (inject_row is not None and inject_row not in rows):
        raise ValueError(f"rows must be distinct rows of scratch.ROWS and inject_row one of them, not {unknown or inject_row!r}")
    L = lib()
    nslots, nr = int(L.scratch_slots()), len(ROWS)
    errs, words = (ctypes.c_ulonglong * nr)(), (ctypes.c_ulonglong * nr)()
    ms, first = (ctypes.c_double * nr)(), (ctypes.c_ulonglong * (10 * nr))()
    fbytes, info = (ctypes.c_int * nr)(), (ctypes.c_ulonglong * 8)()
    m = (ctypes.c_ulonglong * (3 * nslots))()
    idx = (ctypes.c_int * len(rows))(*[ROWS.index(k) for k in rows])
    hooked = inject_row is not None
    stale = int(inject_stale_word) if hooked and inject_stale_word is not None else -1
    rnd = int(inject_round) if inject_round is not None else (1 if stale >= 0 else 0)
    t0 = time.perf_counter()
    _check(L.scratch_test(device, idx, len(rows), int(blocks or 0), int(isolate_blocks or 0),
                          int(rounds), int(reps), seed & 0xffffffff, ROWS.index(inject_row) if hooked else -1,
                          int(inject_wave) if hooked else -1, rnd if hooked else 0, 1 if hooked and inject_alias else 0,
                          stale, errs, words, ms, first, fbytes, info, m))
    wall = time.perf_counter() - t0
    out: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    for k in rows:
        i = ROWS.index(k)
        f = [int(v) for v in first[10 * i:10 * i + 10]]
        bad = None
        if f[0] != _NONE:
            bad = {"where": simd_name(f[0] >> 16), "lane": f[0] & 0xff, "wave": f[1], "word": f[2], "got": f"0x{f[3]:08x}",
                   "want": f"0x{f[4]:08x}", "class": CLASSES[f[5]], "age": f[6],
                   "writer": None if f[7] == _NONE else {"wave": f[7], "where": simd_name(f[8])}, "launch": f[9]}
            if k == ISOLATE_ROW:  # the cell: round:4 | wave:14 | lane:6 | word:8
                bad["round"], bad["word"] = f[2] >> 28, f[2] & 0xff
        out[k] = {"errors": int(errs[i]), "words_checked": int(words[i]), "launches": int(reps) + 1, "ms": round(ms[i], 4),
                  "frame_bytes": int(fbytes[i]), "first_bad": bad}
        if errs[i]:
            note = ""
            if bad:
                note = f" on {bad['where']} ({bad['class']}" + (f", {bad['age']} rounds old" if bad["age"] else "") + (
                    f", written by wave {bad['writer']['wave']} on {bad['writer']['where']}" if bad["writer"] else "") + ")"
            problems.append(f"{errs[i]} wrong words in {k}{note}")
    seen, xcds, bad_simds = simd_map_summary(m, nslots)
    total = sum(r["errors"] for r in out.values())
    part = {p: max((r["frame_bytes"] for k, r in out.items() if k.startswith(p + "/")), default=0)
            for p in ("isolate", "frames")}
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen), "xcds": xcds, "blocks": int(info[4]),
                           "isolate_blocks": int(info[5]), "isolate_waves": int(info[3]), "rounds": int(rounds),
                           "rows": out, "frame_bytes": part,
                           "co_resident_waves": int(info[0]), "backing_bytes": int(info[1]),
                           "backing_peak_bytes": int(info[2]), "ms": round(sum(r["ms"] for r in out.values()), 4),
                           "wall_s": round(wall, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    rows = r.get("rows") or {}
    return (f"{len(rows)} rows ({', '.join(rows)}) on {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} XCDs, "
            f"{r.get('isolate_waves', '?')} isolate waves x {r.get('rounds', '?')} rounds ({r.get('co_resident_waves', '?')} "
            f"frames live at once), {r.get('errors', 0)} wrong words; {r.get('ms', 0):.1f} ms")
