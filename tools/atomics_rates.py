#!/usr/bin/env python3
"""Rates of the atomics diagnostic (``ops/atomics.atomics_test``) at its default shape, and what it adds to a cycle.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per kind the min, median
and max GB/s of operand bytes applied.  Reported only: no rate verdict exists for these kernels (one box, no second
device).  ``added_wall_s``: the level-1 suite of ``ops/diag.run`` with and without ``extra=("atomics",)``.

    python tools/atomics_rates.py --runs 24 --out profiles/atomics_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import atomics, diag  # noqa: E402


def _row(r):
    return {"gbs": {k: v["gbs"] for k, v in r["kinds"].items()}, "ms": r["ms"], "errors": r["errors"],
            "xcds": sorted({v["xcds"] for v in r["kinds"].values()}), "wall_s": r["wall_s"]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/atomics_mi355x.json")
    args = ap.parse_args()
    cold = atomics.atomics_test(args.device)
    atomics.atomics_test(args.device)
    runs = [_row(atomics.atomics_test(args.device)) for _ in range(max(1, args.runs))]
    walls = {"without": [], "with": []}
    for _ in range(3):  # the suite as a cycle runs it, alternated
        for key, extra in (("without", ()), ("with", ("atomics",))):
            t0 = time.perf_counter()
            diag.run(1, args.device, extra=extra)
            walls[key].append(round(time.perf_counter() - t0, 3))
    out = {"what": "ops/atomics.atomics_test on one MI355X at its default shape: the first (cold) run of the process, one "
                   "discarded warm-up, then the runs; GB/s of operand bytes applied, mean of the timed launches of a run",
           "device": diag.device_info(args.device), "words": cold["words"], "adders": cold["adders"], "iters": 3,
           "runs": len(runs), "unit": "GB/s", "cold": _row(cold),
           "kinds": {k: {"min": min(x["gbs"][k] for x in runs), "median": statistics.median(x["gbs"][k] for x in runs),
                         "max": max(x["gbs"][k] for x in runs)} for k in atomics.KINDS},
           "test_wall_s": {"min": min(x["wall_s"] for x in runs), "median": statistics.median(x["wall_s"] for x in runs),
                           "max": max(x["wall_s"] for x in runs)},
           "level1_wall_s": walls,
           "added_wall_s": round(statistics.median(walls["with"]) - statistics.median(walls["without"]), 3),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
