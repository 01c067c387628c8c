#!/usr/bin/env python3
"""Rates and exactness of the vector-ALU burn-in (``ops/diag.valu_burn``) and the register-file test's times.

The first (cold) run of the process is kept apart, one warm-up is discarded, then N runs; ``REFERENCE_RATES["valu"]``
is the slowest healthy run / 0.97 (``ops/diag.py``):

    python tools/valu_rates.py --runs 24 --out profiles/valu_burn_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k8s_gpu_node_checker_amd.ops import diag  # noqa: E402


def _errors(r):
    return {k: v["errors"] for k, v in r["kinds"].items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--out", default="profiles/valu_burn_mi355x.json")
    args = ap.parse_args()
    cold = diag.valu_burn(args.device)
    diag.valu_burn(args.device)
    runs = []
    for _ in range(max(1, args.runs)):
        r = diag.valu_burn(args.device)
        runs.append({"rates": r["rates"], "errors": _errors(r), "pass": r["pass"], "degraded": r.get("degraded", False),
                     "slowest_rel": r["map"].get("slowest_rel"), "slowest_cu_rel": r["map"].get("slowest_cu_rel"),
                     "wall_s": r["wall_s"]})
    out = {"what": "ops/diag.valu_burn on one MI355X: the first (cold) run of the process, one discarded warm-up, "
                   "then the runs; regfile_test timings at 1, 2 and 4 rounds",
           "device": diag.device_info(args.device), "iters": 2000, "reps": 5, "runs": len(runs), "unit": "GOP/s",
           "cold": {"rates": cold["rates"], "wall_s": cold["wall_s"], "errors": _errors(cold)},
           "kinds": {k: {"min": round(min(x["rates"][k] for x in runs), 1),
                         "median": round(statistics.median(x["rates"][k] for x in runs), 1),
                         "max": round(max(x["rates"][k] for x in runs), 1)} for k in diag.VALU_KINDS},
           "all_clean": all(not any(x["errors"].values()) for x in runs), "samples": runs, "regfile": []}
    for rounds in (1, 2, 4):
        for _ in range(3):
            r = diag.regfile_test(args.device, rounds=rounds)
            out["regfile"].append({k: r[k] for k in ("ms", "wall_s", "simds", "waves", "errors")} | {"rounds": rounds})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}, indent=1))
    return 0 if out["all_clean"] else 1


if __name__ == "__main__":
    sys.exit(main())
