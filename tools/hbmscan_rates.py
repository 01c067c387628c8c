#!/usr/bin/env python3
"""Rates and wall time of the hbmscan diagnostic (``ops/hbmscan.hbmscan_test``) at 2, 16 and 64 GiB, beside the
levels' ``memtest`` and the ``hbm`` streams in the same process, and one whole-device scan if the device is unused.

Per size: the per-phase GB/s of traffic (a step that verifies and writes counts twice) and the wall time.  Reported
only: no rate verdict exists for these kernels (one box, no second device).

The whole-device scan (``gib=None``: all free memory minus the 2 GiB reserve) is taken once, and only when
``hipMemGetInfo`` shows the device otherwise unused -- free at least 95 % of total.  These GPUs are shared: the tool
does not take all memory from a device that something else is using, and writes that it did not.

    python tools/hbmscan_rates.py --out profiles/hbmscan_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag, hbmscan  # noqa: E402

UNUSED_FRACTION = 0.95


def _row(r):
    return {"tested_gib": r["tested_gib"], "chunks": r["chunks"], "halved": r["halved"],
            "alloc_failures": r["alloc_failures"], "coverage": r["coverage"], "cached": r["cached"],
            "complete": r["complete"], "errors": r["errors"], "finding": r["finding"]["kind"], "wall_s": r["wall_s"],
            "sweep_s": round(sum(p["ms"] for p in r["phases"].values()) / 1e3, 3),
            "gbs": {k: p["gbs"] for k, p in r["phases"].items()}, "ms": {k: p["ms"] for k, p in r["phases"].items()}}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="2,16,64", help="comma list of GiB")
    ap.add_argument("--no-whole", dest="whole", action="store_false", help="never take the whole-device scan")
    ap.add_argument("--out", default="profiles/hbmscan_mi355x.json")
    args = ap.parse_args()
    first = hbmscan.hbmscan_test(args.device, gib=0.0625)  # loads the kernels; its free / total are the device's
    total_b, free_b = first["total_gib"], first["free_gib"]
    sizes = {}
    for gib in (float(x) for x in args.sizes.split(",") if x.strip()):
        if gib + 2 > free_b:
            sizes[f"{gib:g}"] = {"measured": False, "why": f"{free_b} GiB free: not enough beside the 2 GiB reserve"}
            continue
        hbmscan.hbmscan_test(args.device, gib=gib)  # one discarded run: first touch of the pages
        sizes[f"{gib:g}"] = _row(hbmscan.hbmscan_test(args.device, gib=gib))
    mt = diag.memtest(args.device)
    hbm = diag.hbm(args.device)
    unused = free_b >= UNUSED_FRACTION * total_b
    if args.whole and unused:
        r = hbmscan.hbmscan_test(args.device, gib=None)
        whole = dict(_row(r), measured=True, reserve_gib=2.0, total_gib=r["total_gib"], free_gib=r["free_gib"],
                     total_bytes=r["total_bytes"], free_bytes=r["free_bytes"],
                     tested_bytes=r["tested_bytes"], planned_bytes=r["planned_bytes"],
                     reserve_held=r["tested_bytes"] == r["planned_bytes"])
    else:
        whole = {"measured": False,
                 "why": "--no-whole" if not args.whole else
                        f"{free_b} of {total_b} GiB free, under {UNUSED_FRACTION:.0%}: the device is in use by something else"}
    out = {"what": "ops/hbmscan.hbmscan_test on one MI355X: per size one discarded run, then one run; GB/s of traffic per "
                   "phase (a step that verifies and writes counts twice), wall_s of the call, sweep_s of its launches; "
                   "memtest and the hbm streams of ops/diag in the same process; whole_device: gib=None, once, only on "
                   "an otherwise unused device",
           "device": diag.device_info(args.device), "unit": "GB/s", "free_gib": free_b, "total_gib": total_b,
           "free_bytes": first["free_bytes"], "total_bytes": first["total_bytes"],
           "sizes": sizes,
           "memtest": {k: mt[k] for k in ("gib", "passes", "gbps", "errors", "wall_s")},
           "hbm": {k: hbm[k] for k in ("copy_tbs", "read_tbs", "write_tbs", "errors", "gib", "wall_s")},
           "whole_device": whole,
           "all_clean": all(s.get("errors", 0) == 0 for s in sizes.values()) and not mt["errors"] and not hbm["errors"]
           and whole.get("errors", 0) == 0 and first["errors"] == 0}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
