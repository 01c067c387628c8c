#!/usr/bin/env python3
"""Rates of the vmem diagnostic (``ops/vmem.vmem_test``) at its default shape, the L1 slice sweep, and its cost beside lanes.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per op the min, median and
max ms of a timed launch, the per-part times, the SIMDs and XCDs seen at the default grid, and the seconds one GPU
spends in the test per cycle -- with the lanes diagnostic measured the same way in the same process, since the default
``iters`` / ``passes`` were chosen against it.  Then ``slice_bytes`` from 1 KiB to 1 MiB: the time of one
wave-instruction of one wave with plain loads and with ``sc1`` loads (which bypass the L1), to see whether it steps
near 32 KiB per CU (two workgroups per CU: 16 KiB slices).  Last, what the device returns for a multi-dword buffer
load that straddles ``num_records`` (not judged anywhere).  Reported only: one box gives no reference.

    python tools/vmem_rates.py --runs 24 --out profiles/vmem_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, lanes, vmem  # noqa: E402


def _row(r):
    return {"ms": {k: v["ms"] for k, v in r["ops"].items()}, "ops_ms": round(sum(v["ms"] for v in r["ops"].values()), 4),
            "bounds_ms": r["bounds"]["ms"], "l1_ms": r["l1"]["ms"], "l1_ms_sc1": r["l1"]["ms_sc1"], "l1_gain": r["l1"]["l1_gain"],
            "ldsdma_ms": r["ldsdma"]["ms"], "total_ms": r["ms"], "errors": r["errors"], "simds": r["simds"], "xcds": r["xcds"],
            "wall_s": r["wall_s"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def _straddle(device):
    """A dwordx4 buffer load and store whose 16 bytes begin 8 bytes below num_records = 256: what comes back."""
    words = [0x11110000 + i for i in range(128)]
    got = vmem.apply("buffer_load_dwordx4", words, [248] * 64, None, num_records=256, device=device)[:4]
    after = vmem.apply("buffer_store_dwordx4", words, [248] * 64, [0xAAAA0000 + j for _ in range(64) for j in range(4)],
                       num_records=256, device=device)[62:66]
    return {"load_dwordx4_at_248_of_256": [f"0x{w:08x}" for w in got], "memory_words_62_65": [f"0x{w:08x}" for w in words[62:66]],
            "store_dwordx4_at_248_of_256_leaves_words_62_65": [f"0x{w:08x}" for w in after]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/vmem_mi355x.json")
    args = ap.parse_args()
    cold = vmem.vmem_test(args.device)
    vmem.vmem_test(args.device)
    runs = [_row(vmem.vmem_test(args.device)) for _ in range(max(1, args.runs))]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    sweep = {}
    for kib in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        rs = [vmem.vmem_test(args.device, ops=vmem.OPS[:1], iters=1, reps=3, slice_bytes=kib * 1024,
                             passes=max(2, 256 // kib))["l1"] for _ in range(5)]
        sweep[f"{kib}KiB"] = {"ns_per_load": statistics.median(r["ns_per_load"] for r in rs),
                              "ns_per_load_sc1": statistics.median(r["ns_per_load_sc1"] for r in rs),
                              "l1_gain": statistics.median(r["l1_gain"] for r in rs), "errors": sum(r["errors"] for r in rs)}
    info = diag.device_info(args.device)
    out = {"what": "ops/vmem.vmem_test on one MI355X at its default shape: the first (cold) run of the process, one discarded "
                   "warm-up, then the runs; ms = mean of the timed launches of a run; the L1 sweep: ns per wave-instruction "
                   "of one wave (two workgroups of 4 waves per CU, each on its own slice), plain and sc1",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "blocks": cold["blocks"], "iters": cold["iters"],
           "passes": cold["l1"]["passes"], "slice_bytes": cold["l1"]["slice_bytes"], "reps": 3, "runs": len(runs),
           "cold": _row(cold), "ops": {k: {"ms": _spread(x["ms"][k] for x in runs)} for k in vmem.OPS},
           "parts_ms": {k: _spread(x[k] for x in runs) for k in ("ops_ms", "bounds_ms", "l1_ms", "l1_ms_sc1", "ldsdma_ms")},
           "l1_gain": _spread(x["l1_gain"] for x in runs), "l1_sweep": sweep, "straddle": _straddle(args.device),
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "ops", "cold", "device")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
