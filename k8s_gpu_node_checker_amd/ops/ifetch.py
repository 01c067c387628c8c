"""Ifetch diagnostic: ``libmi355x_ifetch.so`` (csrc/ifetch/ifetch.hip) from Python.

Every other diagnostic runs a few hundred bytes to a few KiB of code in a tight loop, fetched once and then served
from the instruction buffer or a handful of I-cache lines.  This one tests the front end of a CU -- the instruction
cache, the fetch path from memory to a wave's instruction buffer and the branch unit -- in two parts of one result:

walk    one kernel of 1,024 straight-line basic blocks (more than 400 KiB of code), each 16 steps of a rotate, an xor
        with a 32-bit literal and an add of a 32-bit literal on a per-lane word, ended by an update of a wave-uniform
        walker word that chooses the next block (``p % nb``): a data-dependent walk over a code footprint that
        ``nb`` sets, from a few KiB to all of it.  Every constant is a literal of the instruction stream, so a wrongly
        fetched dword changes a word, and a wrongly resolved branch derails the rest of the walk.
branch  ``s_branch``, ``s_cbranch_scc0/1``, ``s_cbranch_vccz/nz``, ``s_cbranch_execz/nz``, ``s_setpc_b64``,
        ``s_swappc_b64`` and ``s_call_b64``, one native instruction per op in 4 scalar chains whose every step's
        condition comes from the previous word.

Executing code only computes, so the words every wave must end with come from the host's model
(csrc/ifetch/ifetch_ref.h; tests/test_ifetch_cpu.py holds it against an independent implementation), and every lane
compares bit for bit.  Wrong words are located to the SIMD that executed.  The instruction cache is shared between
CUs and the project has no map of which CUs share one: a wrong word names the CU that executed, not the cache that
served it.

Opt-in: no level runs it; ``ops/diag.run(extra=("ifetch",))``, ``mi355x-diag --ifetch``, ``node_cycle --ifetch`` and
the agent's ``--diag-ifetch`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name  # noqa: F401  (simd_name: part of this module's interface)
from .native import bind_cdll

PARTS = ("walk", "branch")
# the native op index (IfetchBranchOp of ifetch_ref.h): index into this
OPS = (
    "s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz",
    "s_cbranch_execnz", "s_setpc_b64", "s_swappc_b64", "s_call_b64",
)
NB = 1024          # basic blocks of the walk kernel
ST = 16            # steps of a block
PATHS = 64         # distinct paths of a launch: wave_in_grid % 64
CHAINS = 4         # scalar chains of a branch op
WAVE = 64
THREADS = 256      # of a workgroup: 4 waves
BLOCKS_PER_CU = 4  # the default grid
BLOCK_MIN_BYTES = ST * 8   # a block's literal instructions: the least two blocks lie apart
FLOOR_BYTES = 256 * 1024   # the least all blocks span
DEFAULT_NBS = (8, 64, 256, NB)  # a few KiB, two in between, all of it
DEFAULT_STEPS = 512        # 64 paths x 512 steps: 32 draws per block of 1,024 (64 steps leave some unvisited: refused)
DEFAULT_ITERS = 1024
DEFAULT_REPS = 2
DEFAULT_SEED = 0x1FE7C4

_NONE = (1 << 64) - 1
_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/ifetch/ifetch.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_ifetch_cpu.py holds it against the C source."""
    I, U32, D, ULL, U64 = ctypes.c_int, ctypes.c_uint32, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64
    pD, pU, pI, pW = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(U32)
    return {
        "ifetch_last_error": (None, ctypes.c_char_p),
        "ifetch_device_count": (None, I),
        "ifetch_slots": (None, I),
        "ifetch_blocks": (None, I),
        "ifetch_block_map": ([I, pU], None),
        "ifetch_walk_test": ([I, I, I, I, pI, I, U64, I, I, I, pU, pU, pD, pU, pI, pU, pI], None),
        "ifetch_branch_test": ([I, I, I, I, pI, I, U64, I, I, I, pU, pU, pD, pU, pI], None),
        "ifetch_apply_blocks": ([I, pI, I, pW, U32, pW, pW], None),
        "ifetch_apply": ([I, I, I, pW, pW, pW], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_ifetch.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x ifetch failed ({rc}): {lib().ifetch_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().ifetch_device_count())


def row_name(nb: int) -> str:
    """The key of the walk row over blocks [0, nb)."""
    return f"nb{int(nb)}"


def ifetch_test(device: int = 0, parts: Sequence[str] = PARTS, nbs: Sequence[int] = DEFAULT_NBS,
                steps: int = DEFAULT_STEPS, ops: Sequence[str] = OPS, iters: int = DEFAULT_ITERS,
                reps: int = DEFAULT_REPS, blocks: Optional[int] = None, seed: int = DEFAULT_SEED,
                inject_part: Optional[str] = None, inject_row: Any = None, inject_block: int = -1,
                inject_skip_step: int = -1, slots: bool = False) -> Dict[str, Any]:
    """The parts named in ``parts`` on ``blocks`` workgroups of four waves (default: 4 per CU): every row gets a
    checked warm-up launch and ``reps`` timed, checked launches.  A wrong word fails the test.

    ``errors`` counts wrong words over all parts; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs they
    lie on, ``blocks`` the grid of each part (``slots=True`` adds ``slots``, the map rows seen).  ``parts`` holds per
    part its ``errors`` and ``ms`` and:

    walk    ``steps`` blocks per wave over blocks [0, nb) for every nb of ``nbs``; per row (``nb8`` ...) ``nb``,
            ``footprint_bytes`` (the code span of those blocks, derived from the addresses the blocks record for
            themselves in a map launch -- not nb times a nominal size), ``blocks_visited`` (the distinct blocks the
            model's 64 paths run: the library refuses a walk that leaves one of [0, nb) out), ``errors`` (wrong
            words: every lane's final word, and on lane 0 the walker), ``first_bad`` (``where`` names the SIMD that
            executed as ``xcd5/se1/cu8/simd2``, with ``lane``, ``word`` -- ``x`` or ``p`` --, ``path``, ``got``,
            ``want``; None when clean), ``ms`` (the mean time of a timed launch) and ``ns_per_block`` (that time over
            ``steps``: what one block costs a wave while the whole grid runs)
    branch  ``iters`` steps of 4 chains per wave for every op of ``ops``; per op ``errors`` (wrong wave-words),
            ``first_bad`` (``where``, ``chain``, ``got``, ``want``), ``ms`` and ``gops`` (branches per second, G/s)

    ``bad_simds`` lists the SIMDs with wrong words, over all parts.  The instruction cache is shared between CUs and
    the project has no map of which CUs share one: a wrong word names the CU that executed, not the cache that
    served it.  The rates are reported and never judged: the project has measured them on one box
    (profiles/ifetch_mi355x.json), which gives no reference.

    Self-check hooks (off by default), in the warm-up launch of one row of ``inject_part`` (``inject_row``: an nb of
    ``nbs`` or an op of ``ops``; default the part's first row) on wave 0 of workgroup ``inject_block``: with
    ``inject_skip_step`` < 0 one bit of lane 0's final word (the branch part: of chain 0's) is flipped before the
    compare (1 wrong word, ``got == want ^ 0x10``); with a step given, the wave skips the block (the branch part: the
    branch) of that step (wrong words > 0, in that row only)."""
    nbs = [int(v) for v in nbs]
    unknown = [k for k in parts if k not in PARTS] + [k for k in ops if k not in OPS] + \
              [v for v in nbs if not 1 <= v <= NB]
    if unknown or not parts or not ops or not nbs or len(set(nbs)) != len(nbs) or inject_part not in (None,) + tuple(parts):
        raise ValueError(f"parts and ops must be of ifetch.PARTS / OPS, nbs distinct values in 1..{NB} and inject_part "
                         f"one of parts, not {unknown or inject_part!r}")
    hook_row = -1
    if inject_part == "walk":
        if inject_row is not None and int(inject_row) not in nbs:
            raise ValueError(f"inject_row must be one of nbs, not {inject_row!r}")
        hook_row = 0 if inject_row is None else nbs.index(int(inject_row))
    elif inject_part == "branch":
        if inject_row is not None and inject_row not in ops:
            raise ValueError(f"inject_row must be one of ops, not {inject_row!r}")
        hook_row = OPS.index(ops[0] if inject_row is None else inject_row)
    L = lib()
    nrows = int(L.ifetch_slots())
    seed &= _NONE
    total_map = [0] * (3 * nrows)
    out_parts: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    grids: Dict[str, int] = {}
    t0 = time.perf_counter()

    if "walk" in parts:
        n = len(nbs)
        errs, first, foot = (ctypes.c_ulonglong * n)(), (ctypes.c_ulonglong * (4 * n))(), (ctypes.c_ulonglong * n)()
        ms, visited = (ctypes.c_double * n)(), (ctypes.c_int * n)()
        m = (ctypes.c_ulonglong * (3 * nrows))()
        ran = ctypes.c_int()
        hooked = inject_part == "walk"
        _check(L.ifetch_walk_test(device, int(blocks or 0), int(steps), int(reps), (ctypes.c_int * n)(*nbs), n, seed,
                                  hook_row if hooked else -1, int(inject_block) if hooked else -1,
                                  int(inject_skip_step) if hooked else -1, errs, first, ms, foot, visited, m,
                                  ctypes.byref(ran)))
        for i in range(3 * nrows):
            total_map[i] += m[i]
        grids["walk"] = ran.value
        rows: Dict[str, Dict[str, Any]] = {}
        for i, nb in enumerate(nbs):
            bad = None
            if first[4 * i] != _NONE:
                w = int(first[4 * i])
                bad = {"where": simd_name(w >> 16), "lane": (w >> 8) & 0xff, "word": "p" if w & 0xff else "x",
                       "path": int(first[4 * i + 1]), "got": f"0x{first[4 * i + 2]:08x}", "want": f"0x{first[4 * i + 3]:08x}"}
            rows[row_name(nb)] = {"nb": nb, "footprint_bytes": int(foot[i]), "blocks_visited": int(visited[i]),
                                  "errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4),
                                  "ns_per_block": float(f"{ms[i] * 1e6 / int(steps):.4g}")}
            if errs[i]:
                problems.append(f"{errs[i]} wrong words in the walk over {nb} blocks" + (f" on {bad['where']}" if bad else ""))
        out_parts["walk"] = {"errors": sum(r["errors"] for r in rows.values()),
                             "ms": round(sum(r["ms"] for r in rows.values()), 4), "steps": int(steps), "rows": rows}

    if "branch" in parts:
        n = len(OPS)
        errs, first = (ctypes.c_ulonglong * n)(), (ctypes.c_ulonglong * (4 * n))()
        ms = (ctypes.c_double * n)()
        m = (ctypes.c_ulonglong * (3 * nrows))()
        ran = ctypes.c_int()
        hooked = inject_part == "branch"
        idx = (ctypes.c_int * len(ops))(*[OPS.index(k) for k in ops])
        _check(L.ifetch_branch_test(device, int(blocks or 0), int(iters), int(reps), idx, len(ops), seed,
                                    hook_row if hooked else -1, int(inject_block) if hooked else -1,
                                    int(inject_skip_step) if hooked else -1, errs, first, ms, m, ctypes.byref(ran)))
        for i in range(3 * nrows):
            total_map[i] += m[i]
        grids["branch"] = ran.value
        count = ran.value * (THREADS // 64) * CHAINS * int(iters)
        rows = {}
        for k in ops:
            i = OPS.index(k)
            bad = None
            if first[4 * i] != _NONE:
                w = int(first[4 * i])
                bad = {"where": simd_name(w >> 16), "chain": w & 0xff, "got": f"0x{first[4 * i + 2]:08x}",
                       "want": f"0x{first[4 * i + 3]:08x}"}
            rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4),
                       "gops": float(f"{count / (ms[i] * 1e-3) / 1e9:.4g}") if ms[i] > 0 else 0.0}
            if errs[i]:
                problems.append(f"{errs[i]} wrong words in {k}" + (f" on {bad['where']}" if bad else ""))
        out_parts["branch"] = {"errors": sum(r["errors"] for r in rows.values()),
                               "ms": round(sum(r["ms"] for r in rows.values()), 4), "iters": int(iters), "ops": rows}

    seen, xcds, bad_simds = simd_map_summary(total_map, nrows)
    total = sum(p["errors"] for p in out_parts.values())
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen), "xcds": xcds,
                           "blocks": grids, "parts": out_parts, "ms": round(sum(p["ms"] for p in out_parts.values()), 4),
                           "wall_s": round(time.perf_counter() - t0, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    p = r.get("parts") or {}
    walk, br = p.get("walk") or {}, p.get("branch") or {}
    rows = walk.get("rows") or {}
    feet = [v.get("footprint_bytes", 0) for v in rows.values()]
    span = f"{min(feet) / 1024:.0f}-{max(feet) / 1024:.0f} KiB of code" if feet else "no rows"
    per = "/".join(f"{v.get('ns_per_block', 0):.0f}" for v in rows.values())
    return (f"walk {len(rows)} footprints ({span}) x {walk.get('steps', '?')} blocks per wave ({per} ns per block), "
            f"{len(br.get('ops') or {})} branch ops x {br.get('iters', '?')} steps on {r.get('simds', '?')} SIMDs of "
            f"{r.get('xcds', '?')} XCDs, {r.get('errors', 0)} wrong words; {r.get('ms', 0):.1f} ms")


def block_map(device: int = 0) -> List[int]:
    """The address every one of the :data:`NB` blocks of the walk kernel recorded for itself on ``device``
    (``s_getpc_b64`` inside the block, in a launch that runs every block once), as read: :func:`ifetch_test` judges
    it (distinct, at least :data:`BLOCK_MIN_BYTES` apart, all of them spanning :data:`FLOOR_BYTES` or more)."""
    L = lib()
    n = int(L.ifetch_blocks())
    addrs = (ctypes.c_ulonglong * n)()
    _check(L.ifetch_block_map(device, addrs))
    return [int(a) for a in addrs]


def apply_blocks(blocks: Sequence[int], x: Sequence[int], p: int, device: int = 0) -> List[Tuple[List[int], int]]:
    """Each block of ``blocks`` run once from the lanes' words ``x`` (64) and the walker ``p``, returned raw: a list
    of ``(x_out, p_out)``, one per listed block.  A few waves share the list; no compare is made."""
    if len(x) != WAVE or not blocks or any(not 0 <= int(b) < NB for b in blocks):
        raise ValueError(f"x holds one word per lane of a 64-lane wave and blocks lie in 0..{NB - 1}")
    n = len(blocks)
    xo, po = (ctypes.c_uint32 * (WAVE * n))(), (ctypes.c_uint32 * n)()
    _check(lib().ifetch_apply_blocks(device, (ctypes.c_int * n)(*[int(b) for b in blocks]), n,
                                     (ctypes.c_uint32 * WAVE)(*[v & 0xffffffff for v in x]), p & 0xffffffff, xo, po))
    return [(list(xo[WAVE * i:WAVE * (i + 1)]), int(po[i])) for i in range(n)]


def apply_many(op: str, rows: Sequence[Tuple[int, int]], device: int = 0) -> List[int]:
    """The word after branch op ``op`` for every ``(w, cond)`` of ``rows``, applied one after the other by one wave
    and returned raw.  ``cond`` is what the op looks at: SCC, VCC != 0, EXEC != 0 (narrowed inside the statement and
    restored); for the unconditional ops, whether the jump to the taken arm is reached."""
    if op not in OPS:
        raise ValueError(f"op must be of ifetch.OPS, not {op!r}")
    n = len(rows)
    if n == 0:
        return []
    w = (ctypes.c_uint32 * n)(*[r[0] & 0xffffffff for r in rows])
    cond = (ctypes.c_uint32 * n)(*[1 if r[1] else 0 for r in rows])
    out = (ctypes.c_uint32 * n)()
    _check(lib().ifetch_apply(device, OPS.index(op), n, w, cond, out))
    return [int(v) for v in out]


def apply(op: str, w: int, cond: int, device: int = 0) -> int:
    """One application of branch op ``op`` by one wave, returned raw (:func:`apply_many` of one row)."""
    return apply_many(op, [(w, cond)], device)[0]
