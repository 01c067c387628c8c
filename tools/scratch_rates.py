#!/usr/bin/env python3
"""What the scratch diagnostic (``ops/scratch.scratch_test``) reports at its default shape, and its cost beside lanes.

The first run of the process measures the backing store (free device memory before and after the first isolate
launch); one warm-up is discarded, then N runs: wrong words, ms per row, the most frames live at once, the SIMDs and
XCDs seen, and the seconds one GPU spends in the test per cycle -- with the lanes diagnostic measured the same way in
the same process.  Reported only: one box gives no reference.

    python tools/scratch_rates.py --runs 12 --out profiles/scratch_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, lanes, scratch  # noqa: E402


def _row(r):
    return {"ms": {k: v["ms"] for k, v in r["rows"].items()}, "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"],
            "co_resident_waves": r["co_resident_waves"], "backing_bytes": r["backing_bytes"],
            "backing_peak_bytes": r["backing_peak_bytes"], "wall_s": r["wall_s"], "total_ms": r["ms"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out", default="profiles/scratch_mi355x.json")
    args = ap.parse_args()
    cold = scratch.scratch_test(args.device)  # the process's first private segment of 1 KiB per lane
    scratch.scratch_test(args.device)
    runs = [_row(scratch.scratch_test(args.device)) for _ in range(max(1, args.runs))]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    info = diag.device_info(args.device)
    out = {"what": "ops/scratch.scratch_test on one MI355X at its default shape: the first (cold) run of the process, which "
                   "measures the backing store, one discarded warm-up, then the runs; ms = mean of the timed launches of a run",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "isolate_waves": cold["isolate_waves"],
           "isolate_blocks": cold["isolate_blocks"], "blocks": cold["blocks"], "rounds": cold["rounds"],
           "frame_bytes": cold["frame_bytes"], "runs": len(runs), "cold": _row(cold),
           "backing_bytes": cold["backing_bytes"], "backing_peak_bytes": cold["backing_peak_bytes"],
           "backing_bytes_derived": int(info.get("cus", 256)) * 32 * 64 * cold["frame_bytes"]["isolate"],
           "ms": {k: _spread(x["ms"][k] for x in runs) for k in scratch.ROWS},
           "co_resident_waves": _spread(x["co_resident_waves"] for x in runs + [_row(cold)]),
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "cold", "device")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
