"""Handoff diagnostic: ``libmi355x_handoff.so`` (csrc/handoff/handoff.hip) from Python.

Every other diagnostic lets data cross from one workgroup to another only at a kernel boundary.  This one hands data
from one CU to another *inside* a launch, which is what the L2 write-back (``buffer_wbl2 sc1``), the L1 invalidate
(``buffer_inv sc1``), write-through ``sc1`` stores, L1-bypassing ``sc1`` loads and agent-scope flags and atomic adds
exist for: the eight per-XCD L2s of an MI355X are not coherent with each other, and a CU's vector L1 is never
refreshed by another CU's stores.  RCCL's kernels, every split-K and stream-K GEMM and every persistent or fused kernel
rest on exactly these instructions.

``G`` workgroups form a ring of ping-pong hand-offs: workgroup ``w`` owns a 4 KiB slab, writes it in every round and
consumes the slab of ``w + 1`` (placement ``cross``: observed on another XCD) or ``w + 8`` (``same``: observed on the
same one), in four forms:

fence    plain stores, an agent release fence, a flag; a relaxed poll, an agent acquire fence, plain loads
wt       write-through ``sc1`` stores and an ``sc1`` flag; an ``sc1`` poll and ``sc1`` loads, no fence
wt_add   as ``wt``, the signal an agent-scope atomic add to a counter
granule  512 8-byte ``{tag, value}`` granules, one agent store each; swept until every tag is the round's

A hand-off only moves bits, so the expected word is a hash (csrc/handoff/handoff_ref.h; tests/test_handoff_cpu.py
holds it against an independent implementation) and every lane compares every word bit for bit.  A wrong word is
classified by the host: ``stale`` with its age when it is the producer's word of one of the eight rounds before (the
release or the acquire let an old copy through), ``corrupt`` otherwise.  Every spin in the kernels is bounded
(``spin_ms``): HIP promises no co-residency and another tenant may hold CUs, so a wait that ran out is reported
(``timeouts``, ``complete: false``, ``first_timeout``) and does not fail the GPU; a wrong word does.

Opt-in: no level runs it; ``ops/diag.run(extra=("handoff",))``, ``mi355x-diag --handoff``, ``node_cycle --handoff``
and the agent's ``--diag-handoff`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name, slot_name
from .native import bind_cdll

# the native row index is FORMS.index(form) * 2 + PLACEMENTS.index(placement) (handoff_ref.h)
FORMS = ("fence", "wt", "wt_add", "granule")
PLACEMENTS = ("cross", "same")
ROWS = tuple(f"{f}/{p}" for f in FORMS for p in PLACEMENTS)
WAITS = (None, "flag", "ack", "granule")     # HandoffWait
CLASSES = (None, "stale", "corrupt")         # HandoffClass
THREADS = 256          # of a workgroup: 4 waves
SLAB_WORDS = 1024      # a slab: 4 KiB
GRANULES = 512         # the granule form's slab
MIN_BLOCKS = 16        # the least grid where w + 8 differs from w, two workgroups per XCD
STALE_ROUNDS = 8       # how far back the classifier looks
LDS_BYTES = 81 * 1024  # what every kernel declares: more than half of a CU's LDS, one workgroup per CU
DEFAULT_ROUNDS = 64
DEFAULT_REPS = 2
DEFAULT_SPIN_MS = 50   # three orders above the dearest hop measured (44.5 us), far under every caller's timeout
DEFAULT_SEED = 0x4A2D0FF

_NONE = (1 << 64) - 1
_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/handoff/handoff.hip: name -> (argtypes, restype); None leaves ctypes' default (no
    declared arguments / an int result).  tests/test_handoff_cpu.py holds it against the C source."""
    I, D, ULL, U64 = ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64
    pD, pU, pI = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I)
    return {
        "handoff_last_error": (None, ctypes.c_char_p),
        "handoff_device_count": (None, I),
        "handoff_slots": (None, I),
        "handoff_lds_bytes": (None, I),
        "handoff_test": ([I, I, I, I, pI, I, U64, I, I, I, I, I, I, I, pU, pU, pU, pU, pU, pI, pD, pU, pI], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_handoff.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x handoff failed ({rc}): {lib().handoff_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().handoff_device_count())


def words_per_round(row: str) -> int:
    """What one workgroup compares in one round of ``row``: 1,024 words, or the granule form's 512 values."""
    return GRANULES if row.split("/")[0] == "granule" else SLAB_WORDS


def handoff_test(device: int = 0, rows: Sequence[str] = ROWS, rounds: int = DEFAULT_ROUNDS, reps: int = DEFAULT_REPS,
                 blocks: Optional[int] = None, spin_ms: int = DEFAULT_SPIN_MS, jitter: bool = True,
                 seed: int = DEFAULT_SEED, inject_row: Optional[str] = None, inject_block: int = 0,
                 inject_round: int = 0, inject_stale_word: Optional[int] = None, inject_mute: bool = False,
                 slots: bool = False) -> Dict[str, Any]:
    """The rows named in ``rows`` (``form/placement``) on ``blocks`` workgroups (default: one per CU; otherwise a
    multiple of 8 from 16 to the CU count), ``rounds`` hand-offs per workgroup and launch: every row gets a checked
    warm-up launch and ``reps`` timed, checked launches.  Any wrong word fails the test; a timeout does not.

    ``errors`` counts wrong words over all rows, ``complete`` is false when a wait ran out in any launch (``detail``
    says so: re-run on an idle device); ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs they lie on,
    ``blocks`` the grid (``slots=True`` adds ``slots``, the map rows seen).  ``rows`` holds per row:

    ``errors``          wrong 32-bit words over its launches (``granule``: wrong values)
    ``words_checked``   words compared over its ``launches`` (``reps`` + 1): per launch blocks x rounds x 1,024
                        (``granule``: x 512) when complete
    ``timeouts``        waits that ran out; ``complete`` is false when there was one, and ``first_timeout`` then holds
                        who waited (``who``: the workgroup), for what (``for``: ``flag``, ``ack`` or ``granule``), on
                        which ``producer`` and in which ``round``
    ``pairs_cross_xcd`` consumer/producer pairs observed on different XCDs in the row's last launch,
    ``pairs_same_xcd``  on one XCD, and ``pairs_same_cu`` on one CU (0: the library refuses a complete launch that
                        shows one); placement is only observed, from every workgroup's ``XCC_ID`` / ``HW_ID``
    ``ms``              the mean time of a timed launch, ``us_per_round`` that time over ``rounds``
    ``first_bad``       None when clean; else ``where`` (the consuming SIMD, ``xcd5/se1/cu8/simd2``), ``lane``,
                        ``producer`` (the producing CU's name), ``producer_block``, ``round``, ``word``, ``got``,
                        ``want``, ``class`` (``stale`` or ``corrupt``), ``age`` (rounds, 0 for ``corrupt``) and
                        ``launch`` (0: the warm-up)

    ``bad_simds`` lists the consuming SIMDs with wrong words.  The rates are reported and never judged: the project
    has measured them on one box (profiles/handoff_mi355x.json), which gives no reference.

    Self-check hooks (off by default), in the warm-up launch of row ``inject_row`` on workgroup ``inject_block`` in
    round ``inject_round``: by default one bit of lane 0's first loaded word is flipped before the compare (exactly 1
    wrong word, ``got == want ^ 0x10``, ``corrupt``); with ``inject_stale_word=i`` (round >= 1) that workgroup writes
    word ``i`` with its value of the round before (``granule``: the right tag, the old value): exactly 1 wrong word at
    its consumer, ``stale``, ``age`` 1; with ``inject_mute=True`` it leaves that round's signal out, so with a small
    ``spin_ms`` its consumer gives up: ``timeouts`` >= 1, ``complete: false``, ``errors`` 0.  (Muted in the last round,
    the first timeout is its consumer's for certain; earlier, the muted workgroup's own wait for its ack may run out
    first.)"""
    rows = list(rows)
    unknown = [k for k in rows if k not in ROWS]
    if unknown or not rows or len(set(rows)) != len(rows) or (inject_row is not None and inject_row not in rows):
        raise ValueError(f"rows must be distinct rows of handoff.ROWS and inject_row one of them, not {unknown or inject_row!r}")
    L = lib()
    nslots = int(L.handoff_slots())
    nr = len(ROWS)
    errs, words, tmos = (ctypes.c_ulonglong * nr)(), (ctypes.c_ulonglong * nr)(), (ctypes.c_ulonglong * nr)()
    first, tmo = (ctypes.c_ulonglong * (8 * nr))(), (ctypes.c_ulonglong * (4 * nr))()
    pairs, ms = (ctypes.c_int * (3 * nr))(), (ctypes.c_double * nr)()
    m = (ctypes.c_ulonglong * (3 * nslots))()
    ran = ctypes.c_int()
    idx = (ctypes.c_int * len(rows))(*[ROWS.index(k) for k in rows])
    hooked = inject_row is not None
    t0 = time.perf_counter()
    _check(L.handoff_test(device, int(blocks or 0), int(rounds), int(reps), idx, len(rows), seed & _NONE, int(spin_ms),
                          1 if jitter else 0, ROWS.index(inject_row) if hooked else -1,
                          int(inject_block) if hooked else -1, int(inject_round) if hooked else -1,
                          int(inject_stale_word) if hooked and inject_stale_word is not None else -1,
                          1 if hooked and inject_mute else 0, errs, words, tmos, first, tmo, pairs, ms, m,
                          ctypes.byref(ran)))
    wall = time.perf_counter() - t0
    out: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    waited: List[str] = []
    for k in rows:
        i = ROWS.index(k)
        bad = None
        if first[8 * i] != _NONE:
            w, index = int(first[8 * i]), int(first[8 * i + 1])
            bad = {"where": simd_name(w >> 16), "lane": w & 0xff, "producer": slot_name(int(first[8 * i + 4])),
                   "producer_block": index >> 32, "round": (index >> 16) & 0xffff, "word": index & 0xffff,
                   "got": f"0x{first[8 * i + 2]:08x}", "want": f"0x{first[8 * i + 3]:08x}",
                   "class": CLASSES[int(first[8 * i + 5])], "age": int(first[8 * i + 6]), "launch": int(first[8 * i + 7])}
        gave_up = None
        if tmos[i]:
            gave_up = {"who": int(tmo[4 * i]), "for": WAITS[int(tmo[4 * i + 1])], "producer": int(tmo[4 * i + 2]),
                       "round": int(tmo[4 * i + 3])}
            waited.append(f"{k}: {tmos[i]} waits ran out, first workgroup {gave_up['who']} for the {gave_up['for']} of "
                          f"{gave_up['producer']} in round {gave_up['round']}")
        out[k] = {"errors": int(errs[i]), "words_checked": int(words[i]), "launches": int(reps) + 1,
                  "timeouts": int(tmos[i]), "complete": tmos[i] == 0, "first_timeout": gave_up,
                  "pairs_cross_xcd": int(pairs[3 * i]), "pairs_same_xcd": int(pairs[3 * i + 1]),
                  "pairs_same_cu": int(pairs[3 * i + 2]), "ms": round(ms[i], 4),
                  "us_per_round": float(f"{ms[i] * 1e3 / int(rounds):.4g}"), "first_bad": bad}
        if errs[i]:
            problems.append(f"{errs[i]} wrong words in {k}" + (
                f" on {bad['where']} ({bad['class']}" + (f", {bad['age']} rounds old" if bad["age"] else "") +
                f", from {bad['producer']})" if bad else ""))
    if waited:
        problems.append("incomplete, not failed (" + "; ".join(waited[:2]) + (" ..." if len(waited) > 2 else "") +
                        "): the workgroups were not all resident; re-run on an idle device")
    seen, xcds, bad_simds = simd_map_summary(m, nslots)
    total = sum(r["errors"] for r in out.values())
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "complete": all(r["complete"] for r in out.values()),
                           "simds": len(seen), "xcds": xcds, "blocks": ran.value, "rounds": int(rounds), "rows": out,
                           "ms": round(sum(r["ms"] for r in out.values()), 4), "wall_s": round(wall, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    rows = r.get("rows") or {}
    per = "/".join(f"{v.get('us_per_round', 0):.1f}" for v in rows.values())
    waits = sum(v.get("timeouts", 0) for v in rows.values())
    state = "" if r.get("complete", True) else f", incomplete ({waits} waits ran out: re-run on an idle device)"
    return (f"{len(rows)} rows x {r.get('rounds', '?')} rounds on {r.get('blocks', '?')} workgroups, {r.get('simds', '?')} "
            f"SIMDs of {r.get('xcds', '?')} XCDs ({per} us per round), {r.get('errors', 0)} wrong words{state}; "
            f"{r.get('ms', 0):.1f} ms")
