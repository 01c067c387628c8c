"""hbmscan diagnostic: ``libmi355x_hbmscan.so`` (csrc/hbmscan/hbmscan.hip) from Python.

The probe reads what the hardware has already caught (ECC counters, retired pages), and the levels' ``memtest`` writes
one address hash and its inverse over 8 GiB, under 3 % of an MI355X.  This test takes every byte ``hipMalloc`` will
give it, minus a reserve, in chunks; runs four phases over all of them (own address, moving inversions over fixed
patterns, moving inversions over an address hash, a write-hold-verify) with every word checked in every verifying
step; and names what it found: ``stuck_bit``, ``alias``, ``region`` or ``scattered``
(csrc/hbmscan/hbmscan_ref.h holds the expected word, the plan and the classifier; tests/test_hbmscan_cpu.py holds them
against an independent model on the CPU).

Opt-in: no level runs it; ``ops/diag.run(extra=("hbmscan",))``, ``mi355x-diag --hbmscan``, ``node_cycle --hbmscan``
and the agent's ``--diag-hbmscan`` do.  While it runs it holds all of the GPU's free memory.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .native import bind_cdll

# the native indices (HbmscanPhase, HbmscanFindingKind of hbmscan_ref.h): index into these
PHASES = ("addr", "invert", "random", "fade")
FINDINGS = ("none", "stuck_bit", "alias", "region", "scattered")
DIRECTIONS = ("1->0", "0->1")   # a flipped bit: what was written -> what was read
MAX_RECORDS = 64
HIST = 256                      # 128 bit positions x 2 directions
MAX_CHUNKS = 4096
WORD = 16
REGION_BYTES = 2 << 20
CACHED_BELOW = 2 << 30          # under it the L2s and the Infinity Cache may have answered the reads
DEFAULT_SEED = 0x5CA9
MIB, GIB = 1 << 20, 1 << 30

_lib: Optional[ctypes.CDLL] = None


class Record(ctypes.Structure):
    """HbmscanRecord of hbmscan_ref.h: one wrong word."""
    _fields_ = [("phase", ctypes.c_uint32), ("step", ctypes.c_uint32), ("chunk", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("word", ctypes.c_uint64), ("global_word", ctypes.c_uint64),
                ("got", ctypes.c_uint32 * 4), ("want", ctypes.c_uint32 * 4)]


class Finding(ctypes.Structure):
    """HbmscanFinding of hbmscan_ref.h."""
    _fields_ = [("kind", ctypes.c_int32), ("bit", ctypes.c_int32), ("direction", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("victim", ctypes.c_uint64), ("source", ctypes.c_uint64),
                ("span", ctypes.c_uint64)]


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/hbmscan/hbmscan.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_hbmscan_cpu.py holds it against the C source."""
    I, D, LL, U64 = ctypes.c_int, ctypes.c_double, ctypes.c_longlong, ctypes.c_uint64
    ULL = ctypes.c_ulonglong
    pD, pU, pLL = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(LL)
    pR, pF = ctypes.POINTER(Record), ctypes.POINTER(Finding)
    return {
        "hbmscan_last_error": (None, ctypes.c_char_p),
        "hbmscan_device_count": (None, I),
        "hbmscan_plan": ([ULL] * 5 + [pU], None),
        "hbmscan_want": ([I, I, ULL, U64, ctypes.POINTER(ctypes.c_uint)], None),
        "hbmscan_classify": ([pR, I, pU, ULL, ULL, pF], None),
        "hbmscan_test": ([I, ULL, ULL, ULL, ULL, I, I, U64, D, ULL, pLL, I, LL, I, I, LL, LL, I, pU, pU, pD, pD, pD, pR, pU,
                          pF], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_hbmscan.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x hbmscan failed ({rc}): {lib().hbmscan_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().hbmscan_device_count())


def steps(phase: str, random_passes: int = 1) -> int:
    """Steps of a phase (hbmscan_ref.h hbmscan_steps)."""
    return {"addr": 3, "invert": 16, "random": 4 * random_passes, "fade": 3}[phase]


def step_kind(phase: str, step: int) -> str:
    """``write``, ``verify_write`` or ``verify`` (hbmscan_ref.h hbmscan_step_kind): a verifying step compares against
    what the step before left, and one that writes too leaves the inverse of what it verified."""
    sub = step if phase in ("addr", "fade") else (0, 1, 1, 2)[step & 3]
    return ("write", "verify_write", "verify")[sub]


def plan(free: int, total: int, reserve: int = 2 * GIB, limit: int = 0, chunk: int = 4 * GIB) -> List[int]:
    """The chunk sizes (bytes) for ``hipMemGetInfo``'s numbers: ``min(limit, free - reserve)`` rounded down to 16 bytes
    (``limit`` 0: no limit), all of ``chunk`` bytes but a ragged last one.  Nothing to test: RuntimeError (-2)."""
    out = (ctypes.c_ulonglong * MAX_CHUNKS)()
    n = int(lib().hbmscan_plan(int(free), int(total), int(reserve), int(limit), int(chunk), out))
    if n < 0:
        _check(n)
    return [int(out[i]) for i in range(n)]


def want(phase: str, step: int, global_word: int, seed: int = DEFAULT_SEED) -> Tuple[int, int, int, int]:
    """The four 32-bit lanes that global word ``global_word`` holds once ``step`` of ``phase`` has run."""
    out = (ctypes.c_uint * 4)()
    _check(lib().hbmscan_want(PHASES.index(phase), int(step), int(global_word), seed & ((1 << 64) - 1), out))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def _finding(f: Any) -> Dict[str, Any]:
    kind = FINDINGS[int(f.kind)]
    out: Dict[str, Any] = {"kind": kind}
    if kind == "stuck_bit":
        out.update(bit=int(f.bit), direction=DIRECTIONS[int(f.direction)])
    elif kind == "alias":
        out.update(word=int(f.victim), holds=int(f.source), bit=None if f.bit < 0 else int(f.bit))
    elif kind == "region":
        out.update(chunk=int(f.chunk), span=int(f.span), span_bytes=REGION_BYTES)
    return out


def finding_text(f: Dict[str, Any]) -> str:
    kind = f.get("kind")
    if kind == "stuck_bit":
        return f"stuck bit {f['bit']} ({f['direction']})"
    if kind == "alias":
        line = "" if f.get("bit") is None else f", index bit {f['bit']}"
        return f"alias: word {f['word']:#x} held the content of word {f['holds']:#x}{line}"
    if kind == "region":
        return f"one region: +{f['span']:#x}..+{f['span'] + REGION_BYTES:#x} of chunk {f['chunk']}"
    return str(kind)


def classify(records: Sequence[Dict[str, Any]], hist: Sequence[int], index_base: int = 0,
             tested_words: int = 0) -> Dict[str, Any]:
    """The finding for ``records`` (dicts of ``phase`` (name), ``step``, ``chunk``, ``word``, ``global_word``, ``got``
    and ``want`` as four ints each) and the 256-entry bit histogram (``[2 * bit + direction]``)."""
    arr = (Record * max(1, len(records)))()
    for r, rec in zip(arr, records):
        r.phase, r.step, r.chunk = PHASES.index(rec["phase"]), int(rec["step"]), int(rec["chunk"])
        r.word, r.global_word = int(rec["word"]), int(rec["global_word"])
        r.got[:], r.want[:] = list(rec["got"]), list(rec["want"])
    h = (ctypes.c_ulonglong * HIST)(*[int(x) for x in hist])
    f = Finding()
    _check(lib().hbmscan_classify(arr, len(records), h, int(index_base), int(tested_words), ctypes.byref(f)))
    return _finding(f)


def _hex128(lanes: Any) -> str:
    return f"0x{sum(int(lanes[i]) << (32 * i) for i in range(4)):032x}"


def hbmscan_test(device: int = 0, gib: Optional[float] = None, reserve_mib: float = 2048, chunk_mib: float = 4096,
                 hold_ms: int = 0, random_passes: int = 1, seed: int = DEFAULT_SEED, deadline_s: float = 0.0,
                 min_chunk_mib: float = 256, index_base: int = 0,
                 inject_flip: Optional[Sequence[Any]] = None, inject_stuck: Optional[Tuple[int, int, int]] = None,
                 inject_alias: Optional[Tuple[int, int]] = None, fail_alloc_at: int = 0) -> Dict[str, Any]:
    """Test ``gib`` of the device's free memory (None: all of it but ``reserve_mib``) in chunks of ``chunk_mib``, every
    16-byte word, in four phases (``addr``, ``invert``, ``random`` x ``random_passes``, ``fade`` with ``hold_ms``
    between a write and its check).  Any wrong word fails the test.

    The result: ``pass``, ``errors``; ``total_gib`` / ``free_gib`` / ``tested_gib`` and ``coverage`` (tested / total);
    ``chunks`` (``halved``: how many failed to allocate and were split; an allocation failure is never a finding, it
    only lowers ``tested_gib``); ``cached`` (under 2 GiB tested: verified word for word, but the L2s and the Infinity
    Cache may have answered, so the cells are not proven); ``complete`` (False: ``deadline_s`` ran out, after ``reached``
    -- reported, not failed); per phase ``errors``, ``ms``, ``wall_ms`` and ``gbs`` (traffic per second; a step that
    verifies and writes counts twice); ``records`` (the first 64 wrong words: byte ``offset`` in the tested set,
    ``chunk`` and ``chunk_offset``, ``got`` / ``want`` as 128-bit hex, ``flipped`` bits with their direction);
    ``finding`` (``none``, ``stuck_bit`` with ``bit`` and ``direction``, ``alias`` with both words, ``region`` with its
    2 MiB span, ``scattered``), a description that never changes ``pass``.

    Offsets are virtual, into this process's allocations: the project has no map from an address to an HBM stack or
    channel.  Rates are reported and never judged (profiles/hbmscan_mi355x.json is one box).

    Self-check hooks (off by default; words are indices into the tested set): ``inject_flip`` = ``(phase, step, word,
    bit)`` or up to four of them: the bit is flipped once after that (writing) step, and the next step reports it;
    ``inject_stuck`` = ``(word, bit, value)``: forced after every writing step; ``inject_alias`` = ``(a, b)``: in
    ``addr``, word ``a`` copied over word ``b`` after the first write; ``index_base``: the global index starts there;
    ``fail_alloc_at`` = k: the k-th allocation is taken as failed, so the halving path (down to ``min_chunk_mib``) runs."""
    flips = list(inject_flip or ())
    if flips and not isinstance(flips[0], (tuple, list)):
        flips = [tuple(flips)]
    flat = (ctypes.c_longlong * max(4, 4 * len(flips)))()
    for k, (ph, st, word, bit) in enumerate(flips):
        flat[4 * k:4 * k + 4] = [PHASES.index(ph), int(st), int(word), int(bit)]
    sw, sb, sv = inject_stuck if inject_stuck is not None else (-1, 0, 0)
    aa, ab = inject_alias if inject_alias is not None else (-1, -1)
    totals = (ctypes.c_ulonglong * 16)()
    perr = (ctypes.c_ulonglong * len(PHASES))()
    pms, pwall, pbytes = ((ctypes.c_double * len(PHASES))() for _ in range(3))
    recs = (Record * MAX_RECORDS)()
    hist = (ctypes.c_ulonglong * HIST)()
    f = Finding()
    t0 = time.perf_counter()
    _check(lib().hbmscan_test(device, 0 if gib is None else int(gib * GIB), int(reserve_mib * MIB), int(chunk_mib * MIB),
                              int(min_chunk_mib * MIB), int(hold_ms), int(random_passes), seed & ((1 << 64) - 1),
                              float(deadline_s), int(index_base), flat, len(flips), int(sw), int(sb), int(sv), int(aa),
                              int(ab), int(fail_alloc_at), totals, perr, pms, pwall, pbytes, recs, hist,
                              ctypes.byref(f)))
    total, free, planned, tested, chunks, errors, nrec, complete, cached, rph, rst, halved, failed = (
        int(totals[i]) for i in range(13))
    phases = {}
    for i, name in enumerate(PHASES):
        gbs = pbytes[i] / (pms[i] * 1e-3) / 1e9 if pms[i] > 0 else 0.0
        phases[name] = {"errors": int(perr[i]), "ms": round(pms[i], 3), "wall_ms": round(pwall[i], 3),
                        "gbs": float(f"{gbs:.4g}")}
    records = []
    for r in recs[:nrec]:
        flipped = [[32 * lane + b, DIRECTIONS[(r.got[lane] >> b) & 1]] for lane in range(4) for b in range(32)
                   if ((r.got[lane] ^ r.want[lane]) >> b) & 1]
        records.append({"offset": (int(r.global_word) - int(index_base)) * WORD, "chunk": int(r.chunk),
                        "chunk_offset": int(r.word) * WORD, "global_word": int(r.global_word),
                        "phase": PHASES[r.phase], "step": int(r.step), "got": _hex128(r.got), "want": _hex128(r.want),
                        "flipped": flipped})
    finding = _finding(f)
    said = []
    if errors:
        first = records[0]
        said.append(f"{errors} wrong 16-byte words; {finding_text(finding)}; first at +0x{first['chunk_offset']:x} of "
                    f"chunk {first['chunk']} ({first['phase']} step {first['step']})")
    if not complete:
        said.append(f"stopped by its deadline after {PHASES[rph]} step {rst}: incomplete, not failed")
    if cached:
        said.append(f"{tested / GIB:.3g} GiB tested, under 2 GiB: verified word for word, but the caches may have "
                    "answered, so the cells are not proven")
    return {"pass": errors == 0, "errors": errors,
            "total_gib": round(total / GIB, 3), "free_gib": round(free / GIB, 3), "tested_gib": round(tested / GIB, 6),
            "total_bytes": total, "free_bytes": free, "tested_bytes": tested, "planned_bytes": planned, "coverage": round(tested / total, 4) if total else 0.0,
            "chunks": chunks, "halved": halved, "alloc_failures": failed, "cached": bool(cached),
            "complete": bool(complete), "reached": {"phase": PHASES[rph], "step": rst},
            "phases": phases, "records": records, "hist": {str(i): int(hist[i]) for i in range(HIST) if hist[i]},
            "finding": finding, "wall_s": round(time.perf_counter() - t0, 3), "detail": "; ".join(said)}


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    state = ("" if r.get("complete", True) else ", incomplete") + (", cached: cells not proven" if r.get("cached") else "")
    return (f"{r.get('tested_gib', 0):.4g} of {r.get('total_gib', 0):.4g} GiB ({r.get('coverage', 0):.1%}) in "
            f"{r.get('chunks', '?')} chunks{state}, {r.get('errors', 0)} wrong words, finding "
            f"{finding_text(r.get('finding') or {'kind': 'none'})}; {r.get('wall_s', 0):.1f} s")
