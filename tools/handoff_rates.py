#!/usr/bin/env python3
"""Rates of the handoff diagnostic (``ops/handoff.handoff_test``) at its default shape, and its cost beside lanes.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per row the min, median and
max ms of a timed launch and microseconds per round, the pairs observed across XCDs and inside one, the timeouts, the
SIMDs and XCDs seen, and the seconds one GPU spends in the test per cycle -- with the lanes diagnostic measured the
same way in the same process.  Reported only: one box gives no reference.

    python tools/handoff_rates.py --runs 24 --out profiles/handoff_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, handoff, lanes  # noqa: E402


def _row(r):
    rows = r["rows"]
    return {"ms": {k: v["ms"] for k, v in rows.items()}, "us_per_round": {k: v["us_per_round"] for k, v in rows.items()},
            "pairs": {k: [v["pairs_cross_xcd"], v["pairs_same_xcd"], v["pairs_same_cu"]] for k, v in rows.items()},
            "timeouts": sum(v["timeouts"] for v in rows.values()), "complete": r["complete"], "total_ms": r["ms"],
            "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"], "blocks": r["blocks"], "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/handoff_mi355x.json")
    args = ap.parse_args()
    cold = handoff.handoff_test(args.device)
    handoff.handoff_test(args.device)
    runs = [_row(handoff.handoff_test(args.device)) for _ in range(max(1, args.runs))]
    even = [_row(handoff.handoff_test(args.device, jitter=False)) for _ in range(5)]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    info = diag.device_info(args.device)
    out = {"what": "ops/handoff.handoff_test on one MI355X at its default shape: the first (cold) run of the process, one "
                   "discarded warm-up, then the runs; ms = mean of the timed launches of a run, us_per_round = ms / rounds; "
                   "without_jitter: 5 runs with the uneven load off",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "blocks": cold["blocks"],
           "rounds": cold["rounds"], "reps": handoff.DEFAULT_REPS, "spin_ms": handoff.DEFAULT_SPIN_MS, "runs": len(runs),
           "cold": _row(cold),
           "ms": {k: _spread(x["ms"][k] for x in runs) for k in handoff.ROWS},
           "us_per_round": {k: _spread(x["us_per_round"][k] for x in runs) for k in handoff.ROWS},
           "us_per_round_without_jitter": {k: _spread(x["us_per_round"][k] for x in even) for k in handoff.ROWS},
           "pairs_cross_same_xcd_same_cu": cold and _row(cold)["pairs"],
           "timeouts": sum(x["timeouts"] for x in runs), "simds_seen": _spread(x["simds"] for x in runs),
           "xcds_seen": _spread(x["xcds"] for x in runs), "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls),
           "all_clean": all(x["errors"] == 0 for x in runs + even) and cold["errors"] == 0,
           "all_complete": all(x["complete"] for x in runs + even) and cold["complete"], "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "cold", "device")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
