#!/usr/bin/env python3
"""Rates of the lanes diagnostic (``ops/lanes.lanes_test``) at its default shape, and what it adds to a cycle.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per op the min, median and
max ms of a timed launch and the median G crossings/s, the SIMDs and XCDs seen at the default grid, and the total ms
of a cycle's launches.  Reported only: no rate verdict exists for these kernels (one box gives no reference).
``added_wall_s``: the level-1 suite of ``ops/diag.run`` with and without ``extra=("lanes",)``.

    python tools/lanes_rates.py --runs 24 --out profiles/lanes_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, lanes  # noqa: E402


def _row(r):
    return {"ms": {k: v["ms"] for k, v in r["ops"].items()}, "gops": {k: v["gops"] for k, v in r["ops"].items()},
            "total_ms": r["ms"], "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"], "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/lanes_mi355x.json")
    args = ap.parse_args()
    cold = lanes.lanes_test(args.device)
    lanes.lanes_test(args.device)
    runs = [_row(lanes.lanes_test(args.device)) for _ in range(max(1, args.runs))]
    walls = {"without": [], "with": []}
    for _ in range(3):  # the suite as a cycle runs it, alternated
        for key, extra in (("without", ()), ("with", ("lanes",))):
            t0 = time.perf_counter()
            diag.run(1, args.device, extra=extra)
            walls[key].append(round(time.perf_counter() - t0, 3))
    out = {"what": "ops/lanes.lanes_test on one MI355X at its default shape: the first (cold) run of the process, one "
                   "discarded warm-up, then the runs; ms = mean of the timed launches of a run, gops = G crossings/s",
           "device": diag.device_info(args.device), "blocks": cold["blocks"], "iters": cold["iters"], "reps": 5,
           "chains": lanes.CHAINS, "runs": len(runs), "cold": _row(cold),
           "ops": {k: {"ms": _spread(x["ms"][k] for x in runs),
                       "gops_median": statistics.median(x["gops"][k] for x in runs)} for k in lanes.OPS},
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "test_wall_s": _spread(x["wall_s"] for x in runs),
           "level1_wall_s": walls,
           "added_wall_s": round(statistics.median(walls["with"]) - statistics.median(walls["without"]), 3),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "ops", "cold")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
