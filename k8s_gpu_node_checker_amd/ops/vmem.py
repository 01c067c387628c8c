"""Vmem diagnostic: ``libmi355x_vmem.so`` (csrc/vmem/vmem.hip) from Python.

Every byte a kernel reads or writes goes through the vector memory path of its CU, and the other diagnostics use
16-byte global accesses only.  This one tests that path, in four parts reported in one result:

``ops``     every load and store form as one native instruction (global, saddr with immediates, the ``sc0`` / ``sc1`` /
            ``nt`` policies, flat, buffer with ``offen`` / ``idxen`` / ``soffset``; sub-dword and multi-dword widths,
            D16 stores) in walks whose every address depends on the previous step's data.  A memory instruction only
            moves bytes, so the words every wave must end with, and the bytes a store walk must leave, come from the
            host's model (csrc/vmem/vmem_ref.h; tests/test_vmem_cpu.py holds it against an independent one).
``bounds``  the buffer descriptor's range check: a lane at or past ``num_records`` must read 0 and its store must be
            dropped, while its neighbours in the same wave-instruction are served.
``l1``      the 32 KiB vector L1 of every CU: co-resident workgroups read a small slice each again and again, every
            word compared; timed a second time with ``sc1`` loads, which bypass the L1.
``ldsdma``  the LDS-DMA loads (``global_load_lds_dword`` / ``x4`` and the buffer forms), read back from the LDS by
            other lanes.

Left out (vmem_ref.h): the twelve D16 loads (the device did not keep the other half of the destination as the model
did; cause unsettled), the LDS-DMA ``dwordx3`` forms (their bytes did not land at M0 + 12 x lane; cause unsettled),
the typed buffer formats, misaligned accesses, a multi-dword access that straddles
``num_records`` (probe it with :func:`apply`), an ``soffset`` that crosses it, the LDS-DMA sub-dword forms.

Opt-in: no level runs it; ``ops/diag.run(extra=("vmem",))``, ``mi355x-diag --vmem``, ``node_cycle --vmem`` and the
agent's ``--diag-vmem`` do.

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

_WIDTHS = ("ubyte", "sbyte", "ushort", "sshort", "dword", "dwordx2", "dwordx3", "dwordx4")
_STORE_WIDTHS = ("byte", "byte_d16_hi", "short", "short_d16_hi", "dword", "dwordx2", "dwordx3", "dwordx4")
# the native op index (VmemOp of vmem_ref.h): index into OPS; the loads come first
LOADS = tuple(f"global_load_{w}" for w in _WIDTHS) + tuple(
    f"global_load_{w}_{v}" for w in ("dword", "dwordx4") for v in ("saddr", "saddr_p4092", "saddr_m4096")) + tuple(
    f"global_load_{w}_{v}" for w in ("dword", "dwordx4") for v in ("sc0", "sc1", "sc0_sc1", "nt")) + (
    "flat_load_dword", "flat_load_dwordx4_p4095") + tuple(f"buffer_load_{w}" for w in _WIDTHS) + (
    "buffer_load_dword_idxen", "buffer_load_dword_idxen_offen", "buffer_load_dword_soffset",
    "buffer_load_dword_offen_soffset_p4095")
STORES = tuple(f"global_store_{w}" for w in _STORE_WIDTHS) + (
    "global_store_dword_saddr_m8", "global_store_dword_nt", "global_store_dword_sc0_sc1", "global_store_dwordx4_nt",
    "global_store_dwordx4_sc0_sc1", "flat_store_dword") + tuple(f"buffer_store_{w}" for w in _STORE_WIDTHS) + (
    "buffer_store_dword_idxen",)
OPS = LOADS + STORES
BOUNDS_ROWS = tuple(f"{k}_{d}_{w}" for k in ("load", "store") for d in ("raw", "structured") for w in ("dword", "dwordx4"))
LDSDMA_FORMS = ("global_load_lds_dword", "global_load_lds_dwordx4", "buffer_load_dword_lds", "buffer_load_dwordx4_lds")
WAVE = 64
CHAINS = 4         # independent chains per lane
THREADS = 256      # of a workgroup: 4 waves
BLOCKS_PER_CU = 2  # the default grid
TABLE_BYTES = 64 * 1024
STRIDE = 16        # of the structured descriptors
DEFAULT_SEED = 0x7E3E3
# the default shape: chosen so the whole test costs about what the lanes test does (profiles/vmem_mi355x.json)
DEFAULT_ITERS = 256
DEFAULT_PASSES = 128
DEFAULT_SLICE_BYTES = 8192
DEFAULT_BOUNDS_BYTES = 4096

_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/vmem/vmem.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_vmem_cpu.py holds it against the C source."""
    I, U, D, ULL, U64, LL = (ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64,
                             ctypes.c_longlong)
    pD, pU, pI, pW = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(U)
    return {
        "vmem_last_error": (None, ctypes.c_char_p),
        "vmem_device_count": (None, I),
        "vmem_slots": (None, I),
        "vmem_ops": (None, I),
        "vmem_loads": (None, I),
        "vmem_walk_reads": ([I, U64, I, U], None),
        "vmem_walks": ([I, I, I, I, pI, I, U64, I, I, I, LL, pU, pU, pD, pU, pI], None),
        "vmem_bounds": ([I, I, U, U64, I, pU, pU, pD, pU, pI], None),
        "vmem_l1": ([I, I, I, U, I, U64, I, LL, pU, pU, pD, pD, pU, pI], None),
        "vmem_ldsdma_forms": (None, I),
        "vmem_ldsdma_name": ([I], ctypes.c_char_p),
        "vmem_ldsdma": ([I, I, I, I, U64, pU, pU, pD, pU, pI], None),
        "vmem_apply": ([I, I, I, pW, U, pW, pW, U, U, pW], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_vmem.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x vmem failed ({rc}): {lib().vmem_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().vmem_device_count())


def cu_name(row: int) -> str:
    """``xcd3/se1/cu5`` of a SIMD map row: the CU the row's SIMD belongs to."""
    return simd_name(row).rsplit("/", 1)[0]


def walk_reads(op: str, word: int, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED) -> bool:
    """Whether the walk of load ``op`` reads byte 0 of table word ``word`` (the byte ``inject_table_word`` flips a bit
    of), from the host's model: no GPU is used."""
    rc = int(lib().vmem_walk_reads(OPS.index(op), seed & _NONE, int(iters), int(word)))
    if rc < 0:
        _check(rc)
    return bool(rc)


_NONE = (1 << 64) - 1


def _g(count: float, ms: float) -> float:
    return float(f"{count / (ms * 1e-3) / 1e9:.4g}") if ms > 0 else 0.0


def _first(rec: Any, at: int, **index: Any) -> Optional[Dict[str, Any]]:
    if rec[at] == _NONE:
        return None
    return {**index, "got": f"0x{rec[at + 2]:08x}", "want": f"0x{rec[at + 3]:08x}"}


def vmem_test(device: int = 0, ops: Sequence[str] = OPS, iters: int = DEFAULT_ITERS, reps: int = 3,
              blocks: Optional[int] = None, seed: int = DEFAULT_SEED, slice_bytes: int = DEFAULT_SLICE_BYTES,
              passes: int = DEFAULT_PASSES, bounds_bytes: int = DEFAULT_BOUNDS_BYTES, inject_op: Optional[str] = None,
              inject_block: int = -1, inject_skip_iter: int = -1, inject_table_word: Optional[int] = None,
              inject_l1_block: int = -1, inject_l1_word: int = 0, inject_bounds_leak: bool = False,
              slots: bool = False) -> Dict[str, Any]:
    """The four parts on ``blocks`` workgroups of four waves (default: 2 per CU): each launch shape gets a checked
    warm-up launch and ``reps`` timed, checked launches (the bounds rows: one).  A wrong word or byte fails the test.

    ``errors`` counts them over all parts; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs they lie
    on, ``blocks`` the grid (``slots=True`` adds ``slots``, the map rows seen).

    ops     per op of ``ops``, ``iters`` steps of 4 chains per lane: ``errors`` (wrong final words; a store's also
            the wrong bytes of every wave's region, guard cells included), ``first_bad`` (``where`` names the SIMD as
            ``xcd5/se1/cu8/simd2``, with ``lane``, ``chain``, ``got``, ``want``; a wrong byte of a region has
            ``wave`` and ``byte`` instead; None when clean), ``ms`` (the mean time of a timed launch) and ``gops``
            (instructions of the op per second, G lane-accesses/s)
    bounds  over a buffer of 2 x ``bounds_bytes`` whose descriptors cover the first half: per row of
            ``BOUNDS_ROWS`` ``errors`` (a load row: wrong words; a store row: wrong bytes, all 2 N of every wave
            compared on the host), ``first_bad`` and ``ms``
    l1      ``slice_bytes`` per workgroup read ``passes`` times by each of its 4 waves: ``errors`` (wrong reads),
            ``first_bad`` (``where`` the CU, ``slice``, ``word``, ``got``, ``want``), ``ms`` / ``ms_sc1`` (plain
            loads; ``sc1`` loads, which bypass the L1), ``ns_per_load`` / ``ns_per_load_sc1`` (per wave-instruction
            of one wave) and their ratio ``l1_gain``.  Nothing proves that a read was served by the L1: the ratio is
            reported and never judged
    ldsdma  per form of ``LDSDMA_FORMS``, ``iters`` steps: ``errors`` (wrong LDS words), ``first_bad``, ``ms``

    ``bad_simds`` lists the SIMDs with wrong words, ``bad_cus`` their CUs.  The rates are reported and never judged:
    the project has measured them on one box (profiles/vmem_mi355x.json), which gives no reference.

    Self-check hooks (off by default), each in a warm-up launch only: ``inject_op`` with ``inject_block`` flips one
    bit of lane 0's final chain-0 word on wave 0 of that workgroup (1 wrong word, ``got == want ^ 0x10``); with
    ``inject_skip_iter`` that wave leaves chain 0's load or store out of that step instead (wrong words > 0, in that
    op only); ``inject_table_word`` has the host flip one bit of that table word for every load op's warm-up (every
    op for which :func:`walk_reads` is true reports it); ``inject_l1_block`` with ``inject_l1_word`` flips one bit of
    that word of that workgroup's slice (``passes`` x 4 wrong reads on one CU); ``inject_bounds_leak`` passes
    descriptors of twice the ``num_records`` (every bounds row reports the lanes that were served)."""
    unknown = [k for k in ops if k not in OPS]
    if unknown or not ops or len(set(ops)) != len(ops) or (inject_op is not None and inject_op not in ops):
        raise ValueError(f"ops must be distinct names of vmem.OPS and inject_op one of them, not {unknown or inject_op!r}")
    L = lib()
    n, nrows = len(OPS), int(L.vmem_slots())
    seed &= _NONE
    total_map = [0] * (3 * nrows)
    problems: List[str] = []
    ran = ctypes.c_int()
    t0 = time.perf_counter()

    def merge(m: Any) -> None:
        for i in range(3 * nrows):
            total_map[i] += m[i]

    def new_map() -> Any:
        return (ctypes.c_ulonglong * (3 * nrows))()

    # ops
    chosen = (ctypes.c_int * len(ops))(*[OPS.index(k) for k in ops])
    errs, first, ms, m = (ctypes.c_ulonglong * n)(), (ctypes.c_ulonglong * (4 * n))(), (ctypes.c_double * n)(), new_map()
    _check(L.vmem_walks(device, int(blocks or 0), int(iters), int(reps), chosen, len(ops), seed,
                        -1 if inject_op is None else OPS.index(inject_op), int(inject_block), int(inject_skip_iter),
                        -1 if inject_table_word is None else int(inject_table_word), errs, first, ms, m, ctypes.byref(ran)))
    merge(m)
    grid = ran.value
    count = grid * THREADS * CHAINS * int(iters)
    rows: Dict[str, Dict[str, Any]] = {}
    for k in ops:
        i = OPS.index(k)
        where, index = int(first[4 * i]), int(first[4 * i + 1])
        if where != _NONE and (where >> 8) & 0xff == 0xff:
            bad = _first(first, 4 * i, where=simd_name(where >> 32), wave=index >> 32, byte=index & 0xffffffff)
        else:
            bad = _first(first, 4 * i, where=simd_name(where >> 32), lane=(where >> 8) & 0xff, chain=where & 0xff)
        rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4), "gops": _g(count, ms[i])}
        if errs[i]:
            problems.append(f"{errs[i]} wrong words in {k}" + (f" on {bad['where']}" if bad else ""))

    # bounds
    nb = len(BOUNDS_ROWS)
    errs, first, ms, m = (ctypes.c_ulonglong * nb)(), (ctypes.c_ulonglong * (4 * nb))(), (ctypes.c_double * nb)(), new_map()
    _check(L.vmem_bounds(device, int(blocks or 0), int(bounds_bytes), seed, 1 if inject_bounds_leak else 0, errs, first, ms,
                         m, ctypes.byref(ran)))
    merge(m)
    brows: Dict[str, Dict[str, Any]] = {}
    for i, k in enumerate(BOUNDS_ROWS):
        where, index = int(first[4 * i]), int(first[4 * i + 1])
        if k.startswith("store"):
            bad = _first(first, 4 * i, wave=index >> 32, byte=index & 0xffffffff)
        else:
            bad = _first(first, 4 * i, where=simd_name(where >> 32), lane=(where >> 8) & 0xff, byte=index)
        brows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4)}
        if errs[i]:
            problems.append(f"{errs[i]} wrong {'bytes' if k.startswith('store') else 'words'} in bounds {k}"
                            + (f" on {bad['where']}" if bad and "where" in bad else ""))
    bounds = {"errors": sum(r["errors"] for r in brows.values()), "ms": round(sum(r["ms"] for r in brows.values()), 4),
              "num_records_bytes": int(bounds_bytes), "buffer_bytes": 2 * int(bounds_bytes), "rows": brows}

    # l1
    one = ctypes.c_ulonglong
    e1, f1, plain, sc1, m = one(), (one * 4)(), ctypes.c_double(), ctypes.c_double(), new_map()
    _check(L.vmem_l1(device, int(blocks or 0), int(reps), int(slice_bytes), int(passes), seed, int(inject_l1_block),
                     int(inject_l1_word), ctypes.byref(e1), f1, ctypes.byref(plain), ctypes.byref(sc1), m, ctypes.byref(ran)))
    merge(m)
    loads_per_wave = int(passes) * (int(slice_bytes) // 1024)
    bad = _first(f1, 0, where=cu_name(int(f1[0]) >> 32), slice=int(f1[1]) >> 32, word=int(f1[1]) & 0xffffffff)
    l1 = {"errors": int(e1.value), "first_bad": bad, "slice_bytes": int(slice_bytes), "passes": int(passes),
          "ms": round(plain.value, 4), "ms_sc1": round(sc1.value, 4),
          "ns_per_load": float(f"{plain.value * 1e6 / loads_per_wave:.4g}"),
          "ns_per_load_sc1": float(f"{sc1.value * 1e6 / loads_per_wave:.4g}"),
          "l1_gain": float(f"{sc1.value / plain.value:.4g}") if plain.value > 0 else 0.0}
    if e1.value:
        problems.append(f"{e1.value} wrong reads of the L1 slices" + (f", first word {bad['word']} of slice {bad['slice']} "
                                                                        f"on {bad['where']}" if bad else ""))

    # ldsdma
    nf = len(LDSDMA_FORMS)
    errs, first, ms, m = (ctypes.c_ulonglong * nf)(), (ctypes.c_ulonglong * (4 * nf))(), (ctypes.c_double * nf)(), new_map()
    _check(L.vmem_ldsdma(device, int(blocks or 0), int(iters), int(reps), seed, errs, first, ms, m, ctypes.byref(ran)))
    merge(m)
    frows: Dict[str, Dict[str, Any]] = {}
    for i, k in enumerate(LDSDMA_FORMS):
        where, index = int(first[4 * i]), int(first[4 * i + 1])
        bad = _first(first, 4 * i, where=simd_name(where >> 32), lane=(where >> 8) & 0xff, step=index >> 8,
                     lds_word=index & 0xff)
        frows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4)}
        if errs[i]:
            problems.append(f"{errs[i]} wrong LDS words after {k}" + (f" on {bad['where']}" if bad else ""))
    ldsdma = {"errors": sum(r["errors"] for r in frows.values()), "ms": round(sum(r["ms"] for r in frows.values()), 4),
              "iters": int(iters), "forms": frows}

    seen, xcds, bad_simds = simd_map_summary(total_map, nrows)
    total = sum(r["errors"] for r in rows.values()) + bounds["errors"] + l1["errors"] + ldsdma["errors"]
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen), "xcds": xcds,
                           "blocks": grid, "iters": int(iters), "ops": rows, "bounds": bounds, "l1": l1, "ldsdma": ldsdma,
                           "ms": round(sum(r["ms"] for r in rows.values()) + bounds["ms"] + l1["ms"] + l1["ms_sc1"]
                                       + ldsdma["ms"], 4),
                           "wall_s": round(time.perf_counter() - t0, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots,
                              {"bad_cus": sorted({cu_name(r) for r in seen if total_map[3 * r + 1]})})


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    rows, b, l1, dma = r.get("ops") or {}, r.get("bounds") or {}, r.get("l1") or {}, r.get("ldsdma") or {}
    return (f"{len(rows)} ops x {r.get('iters', '?')} steps on {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} XCDs, "
            f"{len(b.get('rows') or {})} bounds rows, L1 {l1.get('slice_bytes', '?')} B x {l1.get('passes', '?')} passes "
            f"(sc1 / plain {l1.get('l1_gain', 0):.2f}), {len(dma.get('forms') or {})} LDS-DMA forms, "
            f"{r.get('errors', 0)} wrong words; {r.get('ms', 0):.1f} ms")


def apply(op: str, table_words: Sequence[int], offsets: Sequence[int], preset: Optional[Sequence[int]] = None,
          num_records: Optional[int] = None, stride: Optional[int] = None, device: int = 0) -> List[int]:
    """Applications of ``op`` by one wave, returned raw, one per 64 entries of ``offsets`` (the byte offset each lane
    accesses inside ``table_words``; several rows are applied one after the other).  ``preset`` holds 4 words per lane
    and row: a load's destination registers before it, a store's data; zeros when None.

    A load returns 4 words per lane and row: the registers it wrote, the rest 0.  A store returns the words of the
    memory after all rows.  The buffer forms go through a descriptor of ``num_records`` (default: all of the memory;
    in bytes, or in elements of 16 bytes for the ``idxen`` forms) -- giving less probes the range check, straddling
    accesses included -- and ``stride`` (default: the form's own, 16 for ``idxen``, else 0)."""
    if op not in OPS:
        raise ValueError(f"op must be of vmem.OPS, not {op!r}")
    if not offsets or len(offsets) % WAVE:
        raise ValueError("offsets holds one byte offset per lane of a 64-lane wave, for one or more rows")
    rows = len(offsets)
    regs = [0] * (4 * rows) if preset is None else list(preset)
    if len(regs) != 4 * rows:
        raise ValueError("preset holds 4 words per lane and row")
    if stride is None:
        stride = STRIDE if "idxen" in op else 0
    if num_records is None:
        num_records = len(table_words) * 4 // (stride or 1)
    words = lambda v: (ctypes.c_uint * len(v))(*[int(x) & 0xffffffff for x in v])
    store = op in STORES
    out = (ctypes.c_uint * (len(table_words) if store else 4 * rows))()
    _check(lib().vmem_apply(device, OPS.index(op), rows // WAVE, words(table_words), len(table_words), words(offsets),
                            words(regs), int(stride), int(num_records), out))
    return list(out)
