"""One node-level agent cycle over several local GPUs, as a standalone process: the multi-device paths of the
node agent on real hardware.

``bench.py --full`` runs it (untimed, rank 0, in a child process with a time limit) whenever it has more than one
GPU: the agent's per-device diagnostic threads on every GPU at once (``--diag-parallel``, the thread-local GEMM
knobs, the per-device dynamic-LDS attribute, the host-link lock), then the node-level xGMI pair matrix and the
in-process RCCL suite under its deadline.  Prints one JSON line.

    python -m k8s_gpu_node_checker_amd.agent.node_cycle --devices 0,1,2,3,4,5,6,7 --level 1 --timeout 150
"""

from __future__ import annotations

import argparse
import json
import sys
import threading
import time
from typing import Any, Dict, List, Optional


def run(devices: List[int], level: int = 1, timeout_s: float = 150.0, parallel: int = 8,
        fabric: bool = True, xgmi_kernel: bool = False, atomics: bool = False, lanes: bool = False,
        scalar: bool = False, matrix: bool = False, vmem: bool = False, cvt: bool = False,
        hbmscan: bool = False, ifetch: bool = False, handoff: bool = False,
        scratch: bool = False) -> Dict[str, Any]:
    """The cycle; returns the summary (never raises for a failed test: failures are in the result)."""
    from ..ops import diag
    from .agent import Agent
    t0 = time.monotonic()
    out: Dict[str, Any] = {"devices": devices, "level": level, "parallel": parallel}
    live = [0]
    peak = [0]
    lock = threading.Lock()
    real_run = diag.run

    def counted(lvl: int, d: int, **kw: Any) -> Dict[str, Any]:
        with lock:
            live[0] += 1
            peak[0] = max(peak[0], live[0])
        try:
            return real_run(lvl, d, **kw)
        finally:
            with lock:
                live[0] -= 1
    diag.run = counted  # type: ignore[assignment]
    try:
        ag = Agent("node-cycle", source="auto", diag_level=level, devices=list(devices), diag_when="always",
                   diag_timeout=timeout_s, diag_parallel=parallel, **({"diag_atomics": True} if atomics else {}), **({"diag_lanes": True} if lanes else {}),
                   **({"diag_scalar": True} if scalar else {}), **({"diag_matrix": True} if matrix else {}),
                   **({"diag_vmem": True} if vmem else {}), **({"diag_cvt": True} if cvt else {}),
                   **({"diag_hbmscan": True} if hbmscan else {}), **({"diag_ifetch": True} if ifetch else {}),
                   **({"diag_handoff": True} if handoff else {}), **({"diag_scratch": True} if scratch else {}))
        rep = ag.probe_once()
    finally:
        diag.run = real_run  # type: ignore[assignment]
    per: Dict[str, Any] = {}
    for d in devices:
        res = ag._diag_cache.get(d)
        if res is None:
            per[str(d)] = {"skipped": ag._diag_skipped.get(d, "no result")}
            continue
        per[str(d)] = {"pass": all(r.get("pass") is not False for r in res.values() if isinstance(r, dict)),
                       "failed": sorted(k for k, r in res.items() if isinstance(r, dict) and r.get("pass") is False),
                       "degraded": sorted(k for k, r in res.items() if isinstance(r, dict) and r.get("degraded")),
                       "gemm_tflops": (res.get("gemm") or {}).get("tflops"),
                       "hbm_read_tbs": (res.get("hbm") or {}).get("read_tbs"),
                       # every rate test as a share of its single-GPU reference: with all GPUs of the node running
                       # the suite at once, this is the measurement the lone-GPU calibration lacks
                       "fractions": {k: r["fraction"] for k, r in res.items()
                                     if isinstance(r, dict) and isinstance(r.get("fraction"), (int, float))}}
    out["per_device"] = per
    out["peak_threads"] = peak[0]
    out["diag_wall_s"] = round(time.monotonic() - t0, 2)
    out["probe_gpus"] = len(rep.get("gpus") or [])
    out["verdict"] = rep.get("state")
    if fabric and len(devices) >= 2:
        t1 = time.monotonic()
        extra = {"kernel": True} if xgmi_kernel else {}  # the kernel-driven xGMI passes and their attribution
        out["fabric"] = Agent._fabric_suite(list(devices), timeout_s, **extra)
        out["fabric_wall_s"] = round(time.monotonic() - t1, 2)
    out["wall_s"] = round(time.monotonic() - t0, 2)
    return out


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="mi355x-node-cycle", description=__doc__.splitlines()[0])
    ap.add_argument("--devices", required=True, help="comma list of HIP ordinals")
    ap.add_argument("--level", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--timeout", type=float, default=150.0, help="per-device watchdog and RCCL deadline (s)")
    ap.add_argument("--parallel", type=int, default=8)
    ap.add_argument("--no-fabric", dest="fabric", action="store_false")
    ap.add_argument("--xgmi-kernel", dest="xgmi_kernel", action="store_true",
                    help="also load the xGMI links from a kernel and attribute slow copies to link or copy engine")
    ap.add_argument("--atomics", action="store_true",
                    help="also run the atomics diagnostic on every device (ops/atomics.py)")
    ap.add_argument("--lanes", action="store_true",
                    help="also run the lanes diagnostic on every device (ops/lanes.py)")
    ap.add_argument("--scalar", action="store_true",
                    help="also run the scalar diagnostic on every device (ops/scalar.py)")
    ap.add_argument("--matrix", action="store_true",
                    help="also run the matrix diagnostic on every device (ops/matrix.py)")
    ap.add_argument("--vmem", action="store_true",
                    help="also run the vmem diagnostic on every device (ops/vmem.py)")
    ap.add_argument("--cvt", action="store_true",
                    help="also run the cvt diagnostic on every device (ops/cvt.py)")
    ap.add_argument("--hbmscan", action="store_true",
                    help="also run the hbmscan diagnostic on every device (ops/hbmscan.py)")
    ap.add_argument("--ifetch", action="store_true",
                    help="also run the ifetch diagnostic on every device (ops/ifetch.py)")
    ap.add_argument("--handoff", action="store_true",
                    help="also run the handoff diagnostic on every device (ops/handoff.py)")
    ap.add_argument("--scratch", action="store_true",
                    help="also run the scratch diagnostic on every device (ops/scratch.py)")
    args = ap.parse_args(argv)
    devices = [int(x) for x in args.devices.split(",") if x.strip()]
    res = run(devices, args.level, args.timeout, args.parallel, args.fabric, args.xgmi_kernel, args.atomics, args.lanes,
              args.scalar, args.matrix, args.vmem, args.cvt, args.hbmscan, args.ifetch, args.handoff, args.scratch)
    print(json.dumps(res, separators=(",", ":"), default=str), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
