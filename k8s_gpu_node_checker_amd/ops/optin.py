"""The opt-in diagnostics, declared once: no level of ``ops/diag.LEVELS`` runs them, ``diag.run(extra=...)`` does.

Everything that wires a diagnostic in is derived from its name ``X`` here: the module ``ops/X.py`` with ``X_test``
and ``summary``, the library ``libmi355x_X.so`` built from ``csrc/X/X.hip`` with the header ``X_ref.h``, the flag
``--X`` of ``mi355x-diag`` and ``node_cycle`` and ``--diag-X`` of the agent.  A new one adds its entry here, those
files, its stand-in (``testing/fake_native.py``) and tests, and its ``diag.KERNEL_REVISION`` stamp.

Imports nothing, so the build and the argument parsers can read it without loading ctypes.
"""


class OptIn:
    __slots__ = ("description", "simd_report")

    def __init__(self, description, simd_report=True):
        self.description = description  # one clause, for the help texts and the docstring of diag.X_test
        self.simd_report = simd_report  # the library locates wrong results to a SIMD: csrc/common/simd_report.h


# in the order the results appear in: `extra` is normalised to it (chosen)
OPT_IN = {
    "atomics": OptIn("atomic adds, max, xor and returning adds from every XCD onto one array, every element checked",
                     simd_report=False),
    "lanes": OptIn("every lane-crossing instruction of a wave (DPP, permlane swaps, ds_swizzle / ds_bpermute / "
                   "ds_permute, readlane) checked bit for bit against the host's model, wrong lanes located to their SIMD"),
    "scalar": OptIn("every scalar-ALU instruction against the host's model, the SGPR file of every SIMD under patterns, "
                    "every width of scalar load through the scalar data cache"),
    "matrix": OptIn("every MFMA family of the matrix cores (fp32, fp16, bf16, int8, fp64, bf8, f8f6f4, sparse) on exact "
                    "operands, every accumulator element checked bit for bit against the host's model"),
    "vmem": OptIn("every vector load and store form against the host's model, the buffer descriptor's range check, the "
                  "vector L1 of every CU and the LDS-DMA loads"),
    "cvt": OptIn("every format conversion of the vector ALU (classic, bf16, fp8 / bf8, the scalef32 forms) checked bit "
                 "for bit against the host's model, wrong words located to their SIMD"),
    "hbmscan": OptIn("every free byte of its memory but a 2 GiB reserve through four phases, every 16-byte word checked, "
                     "and a named finding (stuck bit, alias, region, scattered); holds the GPU's free memory while it "
                     "runs and, given a deadline, stops by itself at half of what is left of it (reported incomplete, "
                     "not failed)", simd_report=False),
    "ifetch": OptIn("a data-dependent walk over more code than the instruction cache holds and every branch instruction, "
                    "checked bit for bit against the host's model, wrong words located to the SIMD that executed"),
    "handoff": OptIn("a ring of hand-offs between workgroups inside one launch, across XCDs and inside one, in four forms "
                     "(release / acquire fences, write-through stores, an atomic counter, tagged granules), every word "
                     "checked bit for bit, a wrong one classified stale or corrupt, every spin bounded"),
    "scratch": OptIn("private memory -- twice the device's wave slots of 1 KiB-per-lane frames written, held and read "
                     "back, a wrong word classified alias, stale or corrupt; the compiler's own locals and call frames, "
                     "compared bit for bit with the host's run"),
}


def add_flags(ap, prefix, help_prefix):
    """One ``store_true`` flag ``--<prefix>X`` per diagnostic on the argparse parser ``ap``; ``help_prefix`` names the
    diagnostic as ``{name}`` and is followed by its description."""
    for name, entry in OPT_IN.items():
        ap.add_argument(f"--{prefix}{name}", action="store_true",
                        help=f"{help_prefix.format(name=name)}: {entry.description} (ops/{name}.py)")


def chosen(args, prefix=""):
    """The diagnostics whose flag (dest ``<prefix>X``) is set in the parsed ``args``, in table order."""
    return tuple(name for name in OPT_IN if getattr(args, prefix + name))
