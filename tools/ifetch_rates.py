#!/usr/bin/env python3
"""Rates of the ifetch diagnostic (``ops/ifetch.ifetch_test``) at its default shape, the sweep of its walk over the code footprint, and its cost beside lanes.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per walk row and branch op
the min, median and max ms of a timed launch, the SIMDs and XCDs seen at the default grid, and the seconds one GPU
spends in the test per cycle -- with the lanes diagnostic measured the same way in the same process.  Then the sweep:
the walk alone over ``--nbs`` footprints at the default grid and at one workgroup per CU, with ``footprint_bytes``
from the kernel's own map and ``ns_per_block``; where that time steps is where the walk no longer fits the
instruction cache.  Reported only: one box gives no reference.

    python tools/ifetch_rates.py --runs 24 --out profiles/ifetch_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, ifetch, lanes  # noqa: E402

SWEEP = (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 160, 192, 224, 256, 320, 384, 512, 640, 768, 896, 1024)


def _row(r):
    walk, br = r["parts"]["walk"], r["parts"]["branch"]
    return {"walk_ms": {k: v["ms"] for k, v in walk["rows"].items()},
            "ns_per_block": {k: v["ns_per_block"] for k, v in walk["rows"].items()},
            "branch_ms": {k: v["ms"] for k, v in br["ops"].items()}, "walk_total_ms": walk["ms"], "branch_total_ms": br["ms"],
            "total_ms": r["ms"], "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"], "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def _sweep(device, nbs, steps, blocks, runs):
    out = []
    for nb in nbs:
        rs = [ifetch.ifetch_test(device, parts=("walk",), nbs=(nb,), steps=steps, reps=3, blocks=blocks)
              for _ in range(runs)]
        row = rs[0]["parts"]["walk"]["rows"][ifetch.row_name(nb)]
        out.append({"nb": nb, "footprint_bytes": row["footprint_bytes"],
                    "ns_per_block": _spread(r["parts"]["walk"]["rows"][ifetch.row_name(nb)]["ns_per_block"] for r in rs),
                    "errors": sum(r["errors"] for r in rs)})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--nbs", type=int, nargs="*", default=list(SWEEP))
    ap.add_argument("--sweep-steps", type=int, default=2048)
    ap.add_argument("--out", default="profiles/ifetch_mi355x.json")
    args = ap.parse_args()
    cold = ifetch.ifetch_test(args.device)
    ifetch.ifetch_test(args.device)
    runs = [_row(ifetch.ifetch_test(args.device)) for _ in range(max(1, args.runs))]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    info = diag.device_info(args.device)
    cus = int(info.get("cus") or 256)
    addrs = ifetch.block_map(args.device)
    order = sorted(range(ifetch.NB), key=lambda b: addrs[b])
    gaps = [addrs[order[i + 1]] - addrs[order[i]] for i in range(ifetch.NB - 1)]
    out = {"what": "ops/ifetch.ifetch_test on one MI355X at its default shape: the first (cold) run of the process, one "
                   "discarded warm-up, then the runs; ms = mean of the timed launches of a run; wall_s includes the host's "
                   "model of every path; sweep: the walk alone, median of 5 runs of 3 timed launches per footprint, "
                   "ns_per_block = launch time / steps",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "blocks": cold["blocks"],
           "steps": cold["parts"]["walk"]["steps"], "iters": cold["parts"]["branch"]["iters"], "reps": ifetch.DEFAULT_REPS,
           "runs": len(runs), "cold": _row(cold),
           "footprint_bytes": {k: v["footprint_bytes"] for k, v in cold["parts"]["walk"]["rows"].items()},
           "map": {"blocks": ifetch.NB, "span_bytes": max(addrs) - min(addrs), "gap_bytes": _spread(gaps),
                   "order_first": order[:8], "order_last": order[-8:]},
           "walk_ms": {k: _spread(x["walk_ms"][k] for x in runs) for k in runs[0]["walk_ms"]},
           "ns_per_block": {k: _spread(x["ns_per_block"][k] for x in runs) for k in runs[0]["ns_per_block"]},
           "branch_ms": {k: _spread(x["branch_ms"][k] for x in runs) for k in ifetch.OPS},
           "walk_total_ms": _spread(x["walk_total_ms"] for x in runs),
           "branch_total_ms": _spread(x["branch_total_ms"] for x in runs),
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls),
           "sweep_steps": args.sweep_steps,
           "sweep_default_grid": _sweep(args.device, args.nbs, args.sweep_steps, None, 5),
           "sweep_one_workgroup_per_cu": _sweep(args.device, args.nbs, args.sweep_steps, cus, 5),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    out["all_clean"] = out["all_clean"] and all(r["errors"] == 0 for r in out["sweep_default_grid"] + out["sweep_one_workgroup_per_cu"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "cold", "device")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
