#!/usr/bin/env python3
"""Rates of the cvt diagnostic (``ops/cvt.cvt_test``) at its default shape, its cost beside lanes, and the device's decode of the special codes.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; per op the min, median and
max ms of a timed launch, the SIMDs and XCDs seen at the default grid, the float mode, and the seconds one GPU spends
in the test per cycle -- with the lanes diagnostic measured the same way in the same process, since the default
``iters`` is chosen against it: ``--iters`` gives further step counts to time, so the largest that stays below lanes
can be read off.  Last, what the device returns for sources outside the model's domain (not judged anywhere): the
Inf and NaN codes of fp8 and bf8, an fp32 NaN, Inf and an overflowing value into f16, bf16, fp8, bf8 and fp4.
Reported only: one box gives no reference.

    python tools/cvt_rates.py --runs 24 --out profiles/cvt_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import cvt, diag, lanes  # noqa: E402

ONE = 0x3f800000


def _row(r):
    return {"ms": {k: v["ms"] for k, v in r["ops"].items()}, "total_ms": r["ms"], "errors": r["errors"], "simds": r["simds"],
            "xcds": r["xcds"], "wall_s": r["wall_s"], "mode": r["mode"]}


def _spread(values):
    values = list(values)
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def _outside(device):
    """Single applications on sources the model refuses: what the device makes of them."""
    h = lambda pairs: [[f"0x{a:08x}", f"0x{b:08x}"] for a, b in pairs]
    nan, inf, big = 0x7fc00000, 0x7f800000, 0x7f7fffff
    out = {
        "f32_fp8_b0 of 0x7f, 0xff": h(cvt.apply_many("f32_fp8_b0", [(0x7f, 0, 0, ONE), (0xff, 0, 0, ONE)], device)),
        "f32_bf8_b0 of 0x7c, 0x7d, 0xfc, 0xff": h(cvt.apply_many("f32_bf8_b0", [(c, 0, 0, ONE) for c in (0x7c, 0x7d, 0xfc, 0xff)],
                                                                  device)),
    }
    for op in ("f16_f32", "pk_bf16_f32", "pk_fp8_f32_lo", "pk_bf8_f32_lo", "scalef32_pk_fp8_f32_lo", "scalef32_pk_bf8_f32_lo",
               "scalef32_pk_fp4_f32_b0", "i32_f32", "u32_f32"):
        out[f"{op} of NaN, +Inf, -Inf, 3.4e38, -3.4e38 (both sources)"] = h(cvt.apply_many(
            op, [(v, v, 0, ONE) for v in (nan, inf, inf | 1 << 31, big, big | 1 << 31)], device))
    out["pk_fp8_f32_lo of 464 (the tie above 448), 465, 480"] = h(cvt.apply_many(
        "pk_fp8_f32_lo", [(v, v, 0, ONE) for v in (0x43e80000, 0x43e88000, 0x43f00000)], device))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--iters", type=int, nargs="*", default=[16, 32, 40, 48, 64, 128])
    ap.add_argument("--out", default="profiles/cvt_mi355x.json")
    args = ap.parse_args()
    cold = cvt.cvt_test(args.device)
    cvt.cvt_test(args.device)
    runs = [_row(cvt.cvt_test(args.device)) for _ in range(max(1, args.runs))]
    lanes.lanes_test(args.device)
    lanes_walls = [lanes.lanes_test(args.device)["wall_s"] for _ in range(max(1, args.runs))]
    by_iters = {}
    for it in args.iters:
        rs = [cvt.cvt_test(args.device, iters=it) for _ in range(5)]
        by_iters[str(it)] = {"wall_s": statistics.median(r["wall_s"] for r in rs), "ms": statistics.median(r["ms"] for r in rs),
                             "errors": sum(r["errors"] for r in rs)}
    info = diag.device_info(args.device)
    out = {"what": "ops/cvt.cvt_test on one MI355X at its default shape: the first (cold) run of the process, one discarded "
                   "warm-up, then the runs; ms = mean of the timed launches of a run; wall_s includes the host's model of "
                   "every op's chains; by_iters: the median of 5 runs at other step counts",
           "device": info, "bdf": info.get("pci_bus_id") or info.get("bdf"), "blocks": cold["blocks"], "iters": cold["iters"],
           "reps": 3, "runs": len(runs), "ops_count": len(cvt.OPS), "mode": cold["mode"], "cold": _row(cold),
           "ops": {k: {"ms": _spread(x["ms"][k] for x in runs)} for k in cvt.OPS},
           "simds_seen": _spread(x["simds"] for x in runs), "xcds_seen": _spread(x["xcds"] for x in runs),
           "total_ms": _spread(x["total_ms"] for x in runs),
           "seconds_per_gpu_and_cycle": _spread(x["wall_s"] for x in runs),
           "lanes_seconds_per_gpu_and_cycle": _spread(lanes_walls), "by_iters": by_iters,
           "outside_the_domain": _outside(args.device),
           "all_clean": all(x["errors"] == 0 for x in runs) and cold["errors"] == 0, "samples": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("samples", "ops", "cold", "device")}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
