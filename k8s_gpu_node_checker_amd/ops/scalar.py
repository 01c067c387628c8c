"""Scalar diagnostic: ``libmi355x_scalar.so`` (csrc/scalar/scalar.hip) from Python.

Every other compute diagnostic runs on the vector side of a CU.  This one tests the scalar side, in three parts
reported in one result:

``salu``  the scalar ALU -- one native instruction per op through inline asm on SGPR operands, SCC set before it and
          read after it, in chains whose every step depends on the previous result and on SCC.  An instruction only
          computes bits, so the words every wave must end with come from the host's model of each instruction
          (csrc/scalar/scalar_ref.h; tests/test_scalar_cpu.py holds the model against an independent one and
          hand-worked rows).
``sgpr``  the SGPR file of each SIMD -- the explicitly named registers ``s20``..``s95`` (without the reserved
          ``s32``) of every wave under four patterns, written whole, held, then checked one by one.
``smem``  scalar loads through the scalar data cache -- every width of ``s_load`` and ``s_buffer_load`` over a table
          filled with an index hash, small (hits) and large (misses), every word compared in scalar registers.

Opt-in: no level runs it; ``ops/diag.run(extra=("scalar",))``, ``mi355x-diag --scalar``, ``node_cycle --scalar`` and
the agent's ``--diag-scalar`` do.

The library is *required* once this module is asked for it: a missing build raises
:class:`~k8s_gpu_node_checker_amd.ops.native.NativeUnavailable`.
"""

from __future__ import annotations

import ctypes
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .diag import finish_simd_result, simd_map_summary, simd_name
from .native import bind_cdll

# the native op index (ScalarOp of scalar_ref.h): index into this
OPS = (
    "s_add_u32", "s_addc_u32", "s_sub_u32", "s_subb_u32", "s_add_i32", "s_sub_i32", "s_absdiff_i32",
    "s_lshl1_add_u32", "s_lshl2_add_u32", "s_lshl3_add_u32", "s_lshl4_add_u32", "s_addk_i32",
    "s_mul_i32", "s_mul_hi_u32", "s_mul_hi_i32", "s_mulk_i32",
    "s_and_b32", "s_or_b32", "s_xor_b32", "s_andn2_b32", "s_orn2_b32", "s_nand_b32", "s_nor_b32", "s_xnor_b32",
    "s_not_b32",
    "s_and_b64", "s_or_b64", "s_xor_b64", "s_andn2_b64", "s_orn2_b64", "s_nand_b64", "s_nor_b64", "s_xnor_b64",
    "s_not_b64",
    "s_lshl_b32", "s_lshr_b32", "s_ashr_i32", "s_lshl_b64", "s_lshr_b64", "s_ashr_i64", "s_bfm_b32", "s_bfm_b64",
    "s_bfe_u32", "s_bfe_i32", "s_bfe_u64", "s_bfe_i64",
    "s_bcnt0_i32_b32", "s_bcnt1_i32_b64", "s_ff0_i32_b32", "s_ff1_i32_b64", "s_flbit_i32_b32", "s_flbit_i32",
    "s_flbit_i32_i64", "s_brev_b32", "s_brev_b64", "s_bitset0_b32", "s_bitset1_b32", "s_wqm_b64", "s_quadmask_b64",
    "s_bitreplicate_b64_b32",
    "s_min_i32", "s_min_u32", "s_max_i32", "s_max_u32", "s_cselect_b32", "s_cselect_b64", "s_cmov_b32",
    "s_sext_i32_i8", "s_sext_i32_i16", "s_abs_i32", "s_pack_ll_b32_b16", "s_pack_lh_b32_b16", "s_pack_hh_b32_b16",
    "s_cmp_eq_i32", "s_cmp_lg_u32", "s_cmp_gt_i32", "s_cmp_ge_u32", "s_cmp_lt_u32", "s_cmp_lt_i32", "s_cmp_le_i32",
    "s_cmp_eq_u64", "s_bitcmp0_b32", "s_bitcmp1_b32",
)
# the scalar-load kinds (ScalarSmemKind of scalar_ref.h) and the dwords one load of each returns
SMEM_KINDS = ("s_load_dword", "s_load_dwordx2", "s_load_dwordx4", "s_load_dwordx8", "s_load_dwordx16",
              "s_buffer_load_dword", "s_buffer_load_dwordx4")
SMEM_WORDS = (1, 2, 4, 8, 16, 1, 4)
PARTS = ("salu", "sgpr", "smem")
SGPR_PATTERNS = ("hash", "inverse", "0x55555555", "0xaaaaaaaa")
CHAINS = 4         # independent chains per wave
THREADS = 256      # of a workgroup: 4 waves
DEFAULT_SEED = 0x5CA1A
# the default shape: chosen so the whole test costs about what the lanes test does (profiles/scalar_mi355x.json)
DEFAULT_ITERS = 1024
DEFAULT_REPS = 2
DEFAULT_HOLD = 64          # x s_sleep 8 between a pattern's write and its check
DEFAULT_SMALL_BYTES = 4096
DEFAULT_LARGE_BYTES = 256 * 1024
DEFAULT_PASSES = 8         # walks of the small table per wave and launch
DEFAULT_LOADS = 1024       # loads of the large table per wave and launch

_lib: Optional[ctypes.CDLL] = None


def _signatures() -> Dict[str, Tuple[Optional[list], Any]]:
    """Every export of csrc/scalar/scalar.hip: name -> (argtypes, restype); None leaves ctypes' default (no declared
    arguments / an int result).  tests/test_scalar_cpu.py holds it against the C source."""
    I, U, D, ULL, U64, LL = (ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_ulonglong, ctypes.c_uint64,
                             ctypes.c_longlong)
    pD, pU, pI, pU64 = ctypes.POINTER(D), ctypes.POINTER(ULL), ctypes.POINTER(I), ctypes.POINTER(U64)
    return {
        "scalar_last_error": (None, ctypes.c_char_p),
        "scalar_device_count": (None, I),
        "scalar_slots": (None, I),
        "scalar_sgpr_lo": (None, I),
        "scalar_sgpr_hi": (None, I),
        "scalar_sgpr_regs": (None, I),
        "scalar_salu": ([I, I, I, I, pI, I, U64, I, I, I, pU, pU, pU, pU, pD, pU, pI], None),
        "scalar_sgpr": ([I, I, I, I, U64, I, I, pU, pU, pU, pU, pD, pU, pI], None),
        "scalar_smem": ([I, I, I, U, U, I, I, U, U64, LL, pU, pU, pU, pU, pD, pD, pU, pI], None),
        "scalar_apply": ([I, I, I, pU64, pU64, ctypes.POINTER(U), pU64, ctypes.POINTER(U)], None),
    }


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind_cdll("libmi355x_scalar.so", _signatures())
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"mi355x scalar failed ({rc}): {lib().scalar_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(lib().scalar_device_count())


def sgpr_range() -> Dict[str, Any]:
    """The SGPRs of a wave the ``sgpr`` part covers: ``lo``..``hi`` and how many (the reserved ``s32`` is skipped)."""
    L = lib()
    return {"lo": int(L.scalar_sgpr_lo()), "hi": int(L.scalar_sgpr_hi()), "regs": int(L.scalar_sgpr_regs())}


_NONE = (1 << 64) - 1


def _g(count: float, ms: float) -> float:
    return float(f"{count / (ms * 1e-3) / 1e9:.4g}") if ms > 0 else 0.0


def _merge(total: List[int], m: Any, nrows: int) -> None:
    for i in range(3 * nrows):
        total[i] += m[i]


def scalar_test(device: int = 0, parts: Sequence[str] = PARTS, ops: Sequence[str] = OPS, iters: int = DEFAULT_ITERS,
                reps: int = DEFAULT_REPS, blocks: Optional[int] = None, seed: int = DEFAULT_SEED,
                hold: int = DEFAULT_HOLD, kinds: Sequence[str] = SMEM_KINDS, small_bytes: int = DEFAULT_SMALL_BYTES,
                large_bytes: int = DEFAULT_LARGE_BYTES, passes: int = DEFAULT_PASSES, loads: int = DEFAULT_LOADS,
                inject_op: Optional[str] = None, inject_block: int = -1, inject_skip_iter: int = -1,
                inject_reg: Optional[str] = None, inject_word: Optional[int] = None,
                slots: bool = False) -> Dict[str, Any]:
    """The parts named in ``parts`` on ``blocks`` workgroups of four waves (default: 4 per CU, the SGPR part 7 per
    CU): each launch shape gets a checked warm-up launch and ``reps`` timed, checked launches.  A wrong word fails
    the test.

    ``errors`` counts wrong words over all parts; ``simds`` is how many SIMDs ran a wave, ``xcds`` how many XCDs they
    lie on, ``blocks`` the grid of each part (``slots=True`` adds ``slots``, the map rows seen).  ``parts`` holds per
    part its ``errors`` and ``ms`` and:

    salu  ``iters`` steps of 4 chains per wave for every op of ``ops``; per op ``errors`` (wrong wave-words),
          ``first_bad`` (``where`` names the SIMD as ``xcd5/se1/cu8/simd2``, with ``chain``, ``got``, ``want``; None
          when clean), ``ms`` (the mean time of a timed launch) and ``gops`` (instructions of the op per second, G/s)
    sgpr  ``regs_per_wave`` registers ``range`` under 4 patterns held ``hold`` x ``s_sleep 8``; ``errors`` (wrong
          registers), ``first_bad`` (``where``, ``reg``, ``pattern``, ``got``, ``want``), ``waves_per_simd`` (min and
          max over the SIMDs, per launch, from the map) and ``bytes_per_simd`` those waves' registers held at once
          *if* they were resident together, which the test does not assert
    smem  per kind of ``kinds``: ``errors`` (wrong words), ``first_bad`` (``where``, ``word`` -- the table index --
          ``got``, ``want``), ``ms`` (hit + miss launch), ``ms_hit`` / ``ms_miss`` and ``gwords_hit`` /
          ``gwords_miss`` (words loaded per second over the ``small_bytes`` table walked ``passes`` times in order,
          and over ``loads`` scattered loads of the ``large_bytes`` table)

    ``bad_simds`` lists the SIMDs with wrong words, over all parts.  The rates are reported and never judged: the
    project has measured them on one box (profiles/scalar_mi355x.json), which gives no reference.

    Self-check hooks (off by default), each in the warm-up launch on wave 0 of workgroup ``inject_block``:
    ``inject_op`` flips one bit of chain 0's final word before the compare (1 wrong word, ``got == want ^ 0x10``);
    with ``inject_skip_iter`` the wave leaves the instruction out of that one step instead (wrong words > 0, in that
    op only); ``inject_reg`` (``"lo"`` / ``"hi"``) flips one bit of the lowest / highest tested SGPR between the first
    pattern's write and its check (1 wrong register); ``inject_word`` has the host flip one bit of that word of the
    small table after the fill (every kind that reads it reports it)."""
    unknown = [k for k in parts if k not in PARTS] + [k for k in ops if k not in OPS] + \
              [k for k in kinds if k not in SMEM_KINDS]
    if unknown or not parts or not ops or not kinds or (inject_op is not None and inject_op not in ops) \
            or inject_reg not in (None, "lo", "hi"):
        raise ValueError(f"parts, ops and kinds must be of scalar.PARTS / OPS / SMEM_KINDS, inject_op one of ops and "
                         f"inject_reg 'lo' or 'hi', not {unknown or inject_op or inject_reg!r}")
    L = lib()
    nrows = int(L.scalar_slots())
    seed &= (1 << 64) - 1
    total_map = [0] * (3 * nrows)
    out_parts: Dict[str, Dict[str, Any]] = {}
    problems: List[str] = []
    grids: Dict[str, int] = {}
    t0 = time.perf_counter()

    def first_bad(where: int, **index: Any) -> Dict[str, Any]:
        return {"where": simd_name(where >> 32), **index}

    if "salu" in parts:
        n = len(OPS)
        arr = ctypes.c_ulonglong * n
        errs, first, got, want = arr(), arr(), arr(), arr()
        ms = (ctypes.c_double * n)()
        m = (ctypes.c_ulonglong * (3 * nrows))()
        ran = ctypes.c_int()
        idx = (ctypes.c_int * len(ops))(*[OPS.index(k) for k in ops])
        _check(L.scalar_salu(device, int(blocks or 0), int(iters), int(reps), idx, len(ops), seed,
                             -1 if inject_op is None else OPS.index(inject_op), int(inject_block),
                             int(inject_skip_iter), errs, first, got, want, ms, m, ctypes.byref(ran)))
        _merge(total_map, m, nrows)
        grids["salu"] = ran.value
        count = ran.value * (THREADS // 64) * CHAINS * int(iters)
        rows: Dict[str, Dict[str, Any]] = {}
        for k in ops:
            i = OPS.index(k)
            bad = None
            if first[i] != _NONE:
                bad = first_bad(int(first[i]), chain=int(first[i]) & 0xff, got=f"0x{got[i]:08x}", want=f"0x{want[i]:08x}")
            rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(ms[i], 4), "gops": _g(count, ms[i])}
            if errs[i]:
                problems.append(f"{errs[i]} wrong words in {k}" + (f" on {bad['where']}" if bad else ""))
        out_parts["salu"] = {"errors": sum(r["errors"] for r in rows.values()),
                             "ms": round(sum(r["ms"] for r in rows.values()), 4), "iters": int(iters), "ops": rows}

    if "sgpr" in parts:
        one = ctypes.c_ulonglong
        errs1, first1, got1, want1 = one(), one(), one(), one()
        ms1 = ctypes.c_double()
        m = (ctypes.c_ulonglong * (3 * nrows))()
        ran = ctypes.c_int()
        _check(L.scalar_sgpr(device, int(blocks or 0), int(reps), int(hold), seed, int(inject_block),
                             -1 if inject_reg is None else ("lo", "hi").index(inject_reg), ctypes.byref(errs1),
                             ctypes.byref(first1), ctypes.byref(got1), ctypes.byref(want1), ctypes.byref(ms1), m,
                             ctypes.byref(ran)))
        _merge(total_map, m, nrows)
        grids["sgpr"] = ran.value
        rng = sgpr_range()
        bad = None
        if first1.value != _NONE:
            code = int(first1.value) & 0xffffffff
            bad = first_bad(int(first1.value), reg=f"s{code & 0xff}", pattern=SGPR_PATTERNS[(code >> 8) & 3],
                            got=f"0x{got1.value:08x}", want=f"0x{want1.value:08x}")
        per_simd = [round(m[3 * r] / (int(reps) + 1), 2) for r in range(nrows) if m[3 * r]]
        waves = {"min": min(per_simd), "max": max(per_simd)} if per_simd else {"min": 0, "max": 0}
        out_parts["sgpr"] = {"errors": int(errs1.value), "ms": round(ms1.value, 4), "first_bad": bad,
                             "regs_per_wave": rng["regs"],
                             "range": f"s{rng['lo']}-s{rng['hi']}" + ("" if rng["hi"] - rng["lo"] + 1 == rng["regs"]
                                                                     else " without s32"),
                             "hold": int(hold), "waves_per_simd": waves,
                             "bytes_per_simd": {k: int(v * rng["regs"] * 4) for k, v in waves.items()}}
        if errs1.value:
            problems.append(f"{errs1.value} wrong SGPRs" + (f", first {bad['reg']} under {bad['pattern']} on {bad['where']}"
                                                             if bad else ""))

    if "smem" in parts:
        n = len(SMEM_KINDS)
        arr = ctypes.c_ulonglong * n
        errs, first, got, want = arr(), arr(), arr(), arr()
        hit, miss = (ctypes.c_double * n)(), (ctypes.c_double * n)()
        m = (ctypes.c_ulonglong * (3 * nrows))()
        ran = ctypes.c_int()
        mask = 0
        for k in kinds:
            mask |= 1 << SMEM_KINDS.index(k)
        _check(L.scalar_smem(device, int(blocks or 0), int(reps), int(small_bytes), int(large_bytes), int(passes),
                             int(loads), mask, seed, -1 if inject_word is None else int(inject_word), errs, first, got,
                             want, hit, miss, m, ctypes.byref(ran)))
        _merge(total_map, m, nrows)
        grids["smem"] = ran.value
        waves_run = ran.value * (THREADS // 64)
        rows = {}
        for k in kinds:
            i = SMEM_KINDS.index(k)
            bad = None
            if first[i] != _NONE:
                bad = first_bad(int(first[i]), word=int(first[i]) & 0xffffffff, got=f"0x{got[i]:08x}",
                                want=f"0x{want[i]:08x}")
            rows[k] = {"errors": int(errs[i]), "first_bad": bad, "ms": round(hit[i] + miss[i], 4),
                       "ms_hit": round(hit[i], 4), "ms_miss": round(miss[i], 4),
                       "gwords_hit": _g(waves_run * int(passes) * (int(small_bytes) // 4), hit[i]),
                       "gwords_miss": _g(waves_run * int(loads) * SMEM_WORDS[i], miss[i])}
            if errs[i]:
                problems.append(f"{errs[i]} wrong words from {k}" + (f", first word {bad['word']} on {bad['where']}"
                                                                      if bad else ""))
        out_parts["smem"] = {"errors": sum(r["errors"] for r in rows.values()),
                             "ms": round(sum(r["ms"] for r in rows.values()), 4), "small_bytes": int(small_bytes),
                             "large_bytes": int(large_bytes), "passes": int(passes), "loads": int(loads), "kinds": rows}

    seen, xcds, bad_simds = simd_map_summary(total_map, nrows)
    total = sum(p["errors"] for p in out_parts.values())
    res: Dict[str, Any] = {"pass": total == 0, "errors": total, "simds": len(seen), "xcds": xcds,
                           "blocks": grids, "parts": out_parts, "ms": round(sum(p["ms"] for p in out_parts.values()), 4),
                           "wall_s": round(time.perf_counter() - t0, 3)}
    return finish_simd_result(res, problems, seen, bad_simds, slots)


def summary(r: Dict[str, Any]) -> str:
    """One line of numbers for a result (``diag.render_text``)."""
    p = r.get("parts") or {}
    salu, sgpr, smem = p.get("salu") or {}, p.get("sgpr") or {}, p.get("smem") or {}
    said = []
    if salu:
        said.append(f"{len(salu.get('ops') or {})} ops x {salu.get('iters', '?')} steps {salu.get('errors', 0)} wrong")
    if sgpr:
        said.append(f"{sgpr.get('regs_per_wave', '?')} SGPRs x {(sgpr.get('waves_per_simd') or {}).get('max', 0):g} "
                    f"waves per SIMD {sgpr.get('errors', 0)} wrong")
    if smem:
        said.append(f"{len(smem.get('kinds') or {})} load kinds {smem.get('errors', 0)} wrong")
    return (f"{'; '.join(said) or 'no part'}; {r.get('simds', '?')} SIMDs of {r.get('xcds', '?')} XCDs, "
            f"{r.get('ms', 0):.1f} ms")


def apply_many(op: str, rows: Sequence[Tuple[int, int, int]], device: int = 0) -> List[Tuple[int, int]]:
    """``(result, scc_out)`` of ``op`` for every ``(a, b, scc_in)`` of ``rows``, applied one after the other by one
    wave and returned raw: S0 = ``a`` and S1 = ``b`` (64-bit; the 32-bit instructions read the low halves) with
    SCC = ``scc_in`` before the instruction.  The result is the destination zero-extended, 0 for a compare."""
    if op not in OPS:
        raise ValueError(f"op must be of scalar.OPS, not {op!r}")
    n = len(rows)
    if n == 0:
        return []
    a = (ctypes.c_uint64 * n)(*[r[0] & _NONE for r in rows])
    b = (ctypes.c_uint64 * n)(*[r[1] & _NONE for r in rows])
    scc_in = (ctypes.c_uint * n)(*[1 if r[2] else 0 for r in rows])
    result, scc_out = (ctypes.c_uint64 * n)(), (ctypes.c_uint * n)()
    _check(lib().scalar_apply(device, OPS.index(op), n, a, b, scc_in, result, scc_out))
    return [(int(result[i]), int(scc_out[i])) for i in range(n)]


def apply(op: str, a: int, b: int, scc_in: int = 0, device: int = 0) -> Tuple[int, int]:
    """One application of ``op`` by one wave, returned raw (:func:`apply_many` of one row)."""
    return apply_many(op, [(a, b, scc_in)], device)[0]
