#!/usr/bin/env python3
"""Rates of the scalar diagnostic (``ops/scalar.scalar_test``) at its default shape, and what it adds to a cycle.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per part the min, median
and max ms, per salu op the median G instructions/s, per scalar-load kind the median G words/s over the small table
(hits) and the large one (misses), the registers per wave and waves per SIMD of the SGPR part, the SIMDs and XCDs seen.
``cache_steps``: the per-load time of one kind over tables from 1 KiB to 1 MiB walked in order, to show where the
scalar data cache stops holding the table.  Reported only: no rate verdict exists for these kernels (one box gives
no reference).  ``added_wall_s``: the level-1 suite of ``ops/diag.run`` with and without ``extra=("scalar",)``.

    python tools/scalar_rates.py --runs 24 --out profiles/scalar_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, scalar  # noqa: E402


def _row(r):
    p = r["parts"]
    return {"part_ms": {k: v["ms"] for k, v in p.items()},
            "gops": {k: v["gops"] for k, v in p["salu"]["ops"].items()},
            "gwords_hit": {k: v["gwords_hit"] for k, v in p["smem"]["kinds"].items()},
            "gwords_miss": {k: v["gwords_miss"] for k, v in p["smem"]["kinds"].items()},
            "waves_per_simd": p["sgpr"]["waves_per_simd"], "total_ms": r["ms"], "errors": r["errors"],
            "simds": r["simds"], "xcds": r["xcds"], "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/scalar_mi355x.json")
    args = ap.parse_args()
    cold = scalar.scalar_test(args.device)
    scalar.scalar_test(args.device)
    runs = [_row(scalar.scalar_test(args.device)) for _ in range(max(1, args.runs))]
    steps = {}
    for kib in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024):  # one kind, in order: ns per load as the table grows
        kind, width = "s_load_dwordx4", 4
        r = scalar.scalar_test(args.device, parts=("smem",), kinds=(kind,), small_bytes=kib * 1024, passes=4,
                               large_bytes=4096, loads=1, reps=3)
        row = r["parts"]["smem"]["kinds"][kind]
        loads_per_wave = 4 * (kib * 1024 // 4 // width)
        steps[f"{kib}KiB"] = {"ms": row["ms_hit"], "ns_per_load_per_wave": round(row["ms_hit"] * 1e6 / loads_per_wave, 2),
                              "errors": row["errors"]}
    walls = {"without": [], "with": []}
    for _ in range(3):  # the suite as a cycle runs it, alternated
        for key, extra in (("without", ()), ("with", ("scalar",))):
            t0 = time.perf_counter()
            diag.run(1, args.device, extra=extra)
            walls[key].append(round(time.perf_counter() - t0, 3))
    sgpr = cold["parts"]["sgpr"]
    out = {"what": "ops/scalar.scalar_test on one MI355X at its default shape: the first (cold) run of the process, "
                   "one discarded warm-up, then the runs; ms = mean of the timed launches of a run",
           "device": diag.device_info(args.device), "blocks": cold["blocks"], "iters": scalar.DEFAULT_ITERS,
           "reps": scalar.DEFAULT_REPS, "hold": scalar.DEFAULT_HOLD, "small_bytes": scalar.DEFAULT_SMALL_BYTES,
           "large_bytes": scalar.DEFAULT_LARGE_BYTES, "passes": scalar.DEFAULT_PASSES, "loads": scalar.DEFAULT_LOADS,
           "chains": scalar.CHAINS, "runs": len(runs), "cold": _row(cold),
           "part_ms": {k: _spread(x["part_ms"][k] for x in runs) for k in scalar.PARTS},
           "salu_gops_median": {k: statistics.median(x["gops"][k] for x in runs) for k in scalar.OPS},
           "salu_gops_all_ops": _spread(statistics.median(x["gops"][k] for x in runs) for k in scalar.OPS),
           "smem_gwords_hit_median": {k: statistics.median(x["gwords_hit"][k] for x in runs) for k in scalar.SMEM_KINDS},
           "smem_gwords_miss_median": {k: statistics.median(x["gwords_miss"][k] for x in runs) for k in scalar.SMEM_KINDS},
           "sgpr": {"regs_per_wave": sgpr["regs_per_wave"], "range": sgpr["range"],
                    "waves_per_simd": _spread(x["waves_per_simd"]["max"] for x in runs),
                    "waves_per_simd_min": _spread(x["waves_per_simd"]["min"] for x in runs),
                    "share_of_800_entry_file_if_resident_together":
                        round(statistics.median(x["waves_per_simd"]["max"] for x in runs) * sgpr["regs_per_wave"] / 800, 3)},
           "cache_steps": steps,
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs), "test_wall_s": _spread(x["wall_s"] for x in runs),
           "level1_wall_s": walls,
           "added_wall_s": round(statistics.median(walls["with"]) - statistics.median(walls["without"]), 3),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0
                        and all(s["errors"] == 0 for s in steps.values()),
           "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "salu_gops_median", "cold")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
