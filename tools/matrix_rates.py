#!/usr/bin/env python3
"""Rates of the matrix diagnostic (``ops/matrix.matrix_test``) at its default shape, and what it costs beside lanes.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per op the min, median and
max ms of a timed launch and the median TFLOP/s (TOP/s for int8; sparse ops counted on the dense K), the SIMDs and
XCDs seen at the default grid, and the seconds one GPU spends in the test per cycle -- with the lanes diagnostic
measured the same way in the same process, since the default ``iters`` was chosen against it.  Reported only: no rate
verdict exists for these kernels (one box gives no reference).

    python tools/matrix_rates.py --runs 24 --out profiles/matrix_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, lanes, matrix  # noqa: E402


def _row(r):
    return {"ms": {k: v["ms"] for k, v in r["ops"].items()}, "tops": {k: v["tops"] for k, v in r["ops"].items()},
            "total_ms": r["ms"], "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"], "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/matrix_mi355x.json")
    args = ap.parse_args()
    cold = matrix.matrix_test(args.device)
    matrix.matrix_test(args.device)
    runs = [_row(matrix.matrix_test(args.device)) for _ in range(max(1, args.runs))]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    info = diag.device_info(args.device)
    out = {"what": "ops/matrix.matrix_test on one MI355X at its default shape: the first (cold) run of the process, one "
                   "discarded warm-up, then the runs; ms = mean of the timed launches of a run, tops = TFLOP/s (TOP/s "
                   "for int8, sparse ops on the dense K) of four dependent instructions per round",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "blocks": cold["blocks"],
           "iters": cold["iters"], "reps": 3, "steps": matrix.STEPS, "runs": len(runs), "cold": _row(cold),
           "ops": {k: {"ms": _spread(x["ms"][k] for x in runs),
                       "tops_median": statistics.median(x["tops"][k] for x in runs)} for k in matrix.OPS},
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "ops", "cold")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
