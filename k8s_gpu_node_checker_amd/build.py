"""Build every native component in-tree (``k8s_gpu_node_checker_amd/_native/``).

``python -m k8s_gpu_node_checker_amd.build [--only {targets}] [--force]``

=====================  ==================================================  ==========================
artefact               source                                              toolchain
=====================  ==================================================  ==========================
``_fastpath*.so``      ``csrc/fastpath/fastpath.cpp`` (CPython ext)        g++ -O3
``libmi355x_probe.so`` ``csrc/probe/probe.cpp`` (C ABI over libamd_smi)     g++ + /opt/rocm/lib/libamd_smi
``mi355x-probe``       ``csrc/probe/probe_main.cpp`` (standalone CLI)       g++ + libamd_smi
``libmi355x_diag.so``  ``csrc/diag/diag.hip`` + ``csrc/diag/*.h`` (kernels)   hipcc --offload-arch=gfx950
``libmi355x_xgmi.so``  ``csrc/xgmi/xgmi.hip`` (kernel-driven xGMI test)      hipcc --offload-arch=gfx950
{opt_in_rows}
``libmi355x_fabric.so`` ``csrc/fabric/fabric.hip`` (RCCL over xGMI)         hipcc + /opt/rocm/lib/librccl
=====================  ==================================================  ==========================

The HIP libraries share ``csrc/common/hip_host.h`` (one build line for all; includes are relative, no ``-I``);
{simd_located} also share ``csrc/common/simd_report.h``, and the instruction-level ones among them
``csrc/common/op_list.h``.
The opt-in diagnostics' targets and their rows above are generated from ``ops/optin.OPT_IN``.
Every header a source reaches is listed in its target's ``headers``, so a change to one rebuilds the library.
The ifetch library's one large kernel (more than 400 KiB of code) takes about 40 s to compile, the longest of all.

Outputs are rebuilt only when a source or header is newer or the build command changed (``--force`` to override).
No JIT cache, nothing outside the tree: the ``.so`` files travel with the
source snapshot to the GPU box.
"""

from __future__ import annotations

import argparse
import os
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

from .ops.optin import OPT_IN

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
OUT = os.path.join(PKG, "_native")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _ext_suffix() -> str:
    return sysconfig.get_config_var("EXT_SUFFIX") or ".so"


def _targets() -> Dict[str, Dict[str, object]]:
    py_inc = sysconfig.get_paths()["include"]
    cxx = os.environ.get("CXX", "g++")
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    smi = ["-I", os.path.join(ROCM, "include"), "-L", os.path.join(ROCM, "lib"), "-lamd_smi",
           f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"]
    # every HIP library is built by the same line (fabric adds RCCL after its sources); includes are relative, no -I
    hip_cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-result"]
    hip_host = os.path.join(CSRC, "common", "hip_host.h")  # the host helpers every HIP library shares
    simd_report = os.path.join(CSRC, "common", "simd_report.h")  # the report of the SIMD-located diagnostics
    op_list = os.path.join(CSRC, "common", "op_list.h")  # the op-list and self-check hook decisions ...
    op_list_users = ("lanes", "scalar", "matrix", "vmem", "cvt", "ifetch")  # ... of the instruction-level diagnostics
    return {
        "fastpath": {
            "sources": [os.path.join(CSRC, "fastpath", "fastpath.cpp")],
            "out": os.path.join(OUT, "_fastpath" + _ext_suffix()),
            # libstdc++ linked in statically: loading the shared one cost ~1.2 ms of a 1-node cold start
            "cmd": [cxx, "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wextra",
                    "-Wno-missing-field-initializers", "-Wno-cast-function-type", "-ffunction-sections",
                    "-fdata-sections", "-I", py_inc],
            "post": ["-static-libstdc++", "-static-libgcc", "-Wl,--gc-sections"],
        },
        "probe": {
            "sources": [os.path.join(CSRC, "probe", "probe.cpp")],
            "headers": [os.path.join(CSRC, "probe", "probe.h")],
            "out": os.path.join(OUT, "libmi355x_probe.so"),
            "cmd": [cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra"],
            "post": smi,
        },
        "probe_cli": {
            "sources": [os.path.join(CSRC, "probe", "probe_main.cpp"), os.path.join(CSRC, "probe", "probe.cpp")],
            "headers": [os.path.join(CSRC, "probe", "probe.h")],
            "out": os.path.join(OUT, "mi355x-probe"),
            "cmd": [cxx, "-O2", "-std=c++17", "-Wall", "-Wextra"],
            "post": smi,
        },
        "diag": {
            "sources": [os.path.join(CSRC, "diag", "diag.hip")],
            "headers": [os.path.join(CSRC, "diag", h) for h in (
                "types.h", "tile_order.h", "gemm_epilogue.h", "gemm_kernels.h", "gemm_common.h", "gemm_v1.h", "gemm_v2.h",
                "gemm_v3.h", "gemm_v4.h", "v4_plan.h", "gemm_check.h", "mem_kernels.h", "burn_kernels.h",
                "valu_ref.h", "xcd_kernels.h", "gemm_host.h", "gemm_verdict.h")] + [hip_host],
            "out": os.path.join(OUT, "libmi355x_diag.so"),
            "cmd": hip_cmd,
            "requires": hipcc,
        },
        "xgmi": {
            "sources": [os.path.join(CSRC, "xgmi", "xgmi.hip")],
            "headers": [hip_host],
            "out": os.path.join(OUT, "libmi355x_xgmi.so"),
            "cmd": hip_cmd,
            "requires": hipcc,
        },
        **{name: {  # the opt-in diagnostics (ops/optin.py), one library each
            "sources": [os.path.join(CSRC, name, f"{name}.hip")],
            "headers": [os.path.join(CSRC, name, f"{name}_ref.h"), hip_host]
            + ([simd_report] if entry.simd_report else []) + ([op_list] if name in op_list_users else []),
            "out": os.path.join(OUT, f"libmi355x_{name}.so"),
            "cmd": hip_cmd,
            "requires": hipcc,
        } for name, entry in OPT_IN.items()},
        "fabric": {
            "sources": [os.path.join(CSRC, "fabric", "fabric.hip")],
            "headers": [hip_host],
            "out": os.path.join(OUT, "libmi355x_fabric.so"),
            "cmd": hip_cmd,
            "post": ["-L", os.path.join(ROCM, "lib"), "-lrccl", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"],
            "requires": hipcc,
        },
    }


__doc__ = __doc__.format(
    targets=",".join(_targets()),
    opt_in_rows="\n".join(f"{f'``libmi355x_{n}.so``':<22} {f'``csrc/{n}/{n}.hip`` ({n} diagnostic)':<51} "
                          f"hipcc --offload-arch={ARCH}" for n in OPT_IN),
    simd_located=", ".join(n for n, entry in OPT_IN.items() if entry.simd_report))


def _stale(out: str, deps: Sequence[str], cmd: str = "") -> bool:
    """Rebuild when the output is missing, older than a source, or was built by a different command."""
    if not os.path.exists(out):
        return True
    try:
        with open(out + ".cmd") as f:
            if f.read() != cmd:
                return True
    except OSError:
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_one(name: str, spec: Dict[str, object], force: bool = False, verbose: bool = False) -> Optional[str]:
    sources: List[str] = list(spec["sources"])  # type: ignore[arg-type]
    out = str(spec["out"])
    deps = sources + list(spec.get("headers", []))  # type: ignore[arg-type]
    req = spec.get("requires")
    if req and not os.path.exists(str(req)):
        return f"{name}: skipped ({req} not found)"
    cmd = list(spec["cmd"]) + sources + ["-o", out + ".tmp"] + list(spec.get("post", []))  # type: ignore[arg-type]
    stamp = " ".join(cmd)
    if not force and not _stale(out, deps, stamp):
        return None
    os.makedirs(OUT, exist_ok=True)
    tmp = out + ".tmp"
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"build of {name} failed:\n{' '.join(cmd)}\n{proc.stdout}")
    os.replace(tmp, out)
    with open(out + ".cmd", "w") as f:
        f.write(stamp)
    return f"{name}: built {os.path.relpath(out, os.path.dirname(PKG))}"


def build(only: Optional[Sequence[str]] = None, force: bool = False, verbose: bool = False) -> List[str]:
    targets = _targets()
    names = [n for n in targets if not only or n in only or (n == "probe_cli" and "probe" in only)]
    msgs: List[str] = []
    with ThreadPoolExecutor(max_workers=min(4, len(names) or 1)) as ex:
        futs = {n: ex.submit(build_one, n, targets[n], force, verbose) for n in names}
        errors = []
        for n, f in futs.items():
            try:
                m = f.result()
                if m:
                    msgs.append(m)
            except Exception as e:  # collect all failures, then raise once
                errors.append(str(e))
    if errors:
        raise RuntimeError("\n\n".join(errors))
    return msgs


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", help="comma list of " + ",".join(_targets()))
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-v", "--verbose", action="store_true")
    args = ap.parse_args(argv)
    only = args.only.split(",") if args.only else None
    for m in build(only, args.force, args.verbose):
        print(m)
    return 0


if __name__ == "__main__":
    sys.exit(main())
