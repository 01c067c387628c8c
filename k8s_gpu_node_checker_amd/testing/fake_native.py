"""CPU stand-ins for the C ABIs of ``libmi355x_diag.so``, ``libmi355x_xgmi.so``, ``libmi355x_atomics.so``,
``libmi355x_lanes.so``, ``libmi355x_scalar.so``, ``libmi355x_matrix.so``, ``libmi355x_vmem.so``, ``libmi355x_cvt.so``,
``libmi355x_hbmscan.so``, ``libmi355x_ifetch.so``, ``libmi355x_handoff.so``, ``libmi355x_scratch.so`` and
``libmi355x_fabric.so``.

They implement the same calls with the same out-parameter protocol (values written through ctypes
pointers), so ``ops/diag.py``, ``ops/xgmi.py`` and ``ops/fabric.py`` run unchanged on CPU with scripted results: a node of
N healthy MI355X by default, with per-GPU rate factors, wrong-result counts, slow or peer-less GPU pairs
and RCCL failures injectable.  Used by the CPU tests of the verdict logic and of whole 8-GPU agent
cycles; the real libraries run under ``tests/test_gpu.py`` on an MI355X.
"""

from __future__ import annotations

import ctypes
import inspect
import threading
import time
from typing import Dict, List, Optional, Tuple


def c_exports(name: str, prefix: Optional[str] = None) -> Dict[str, List[str]]:
    """The C ABI that the stand-in of ``libmi355x_<name>.so`` stands in for, read from csrc/<name>/<name>.hip: every
    function ``<prefix>...`` (default ``<name>_``) defined at the top level of its ``extern "C"`` blocks -> its parameter
    declarations (``(void)``: none).  Exports of diagnostic builds only (inside an ``#ifdef``) are left out."""
    import os
    import re
    with open(os.path.join(os.path.dirname(__file__), "..", "csrc", name, name + ".hip")) as f:
        source = re.sub(r"^#ifdef .*?^#endif", "", f.read(), flags=re.M | re.S)
    defined = r"^\w[\w ]*[ *]+(%s\w+)\(([^)]*)\)\s*\{" % re.escape(prefix or name + "_")
    out: Dict[str, List[str]] = {}
    for block in re.findall(r'^extern "C" \{$(.*?)^\}  // extern "C"$', source, re.M | re.S):
        for fn, params in re.findall(defined, block, re.M):
            out[fn] = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
    return out


def __getattr__(attr: str):
    """``<name>_c_exports()``, the per-library spelling that tests written before :func:`c_exports` import: the same
    call with the name bound."""
    if attr.endswith("_c_exports"):
        import functools
        return functools.partial(c_exports, attr[:-len("_c_exports")])
    raise AttributeError(f"module {__name__!r} has no attribute {attr!r}")


def _put(ptr, ctype, value) -> None:
    ctypes.cast(ptr, ctypes.POINTER(ctype))[0] = value


class FakeDiagLib:
    """``libmi355x_diag.so`` for a node of ``n`` GPUs.

    rate:        every GEMM / HBM / MFMA / host-link rate = rate x the full-GPU reference (per GPU:
                 ``gpu_rate[d]``; a list ``rates`` overrides it call by call)
    cus/mem_gib: what HIP reports per device (a CPX partition: 32 CUs)
    mfma_errors: ``{(device, kind index): wrong results}``
    p2p_gbps:    rate of every GPU pair; ``slow_pairs[(src, dst)]`` / ``nopeer`` override pairs; a pair in
                 ``hung_pairs`` never completes (with a deadline: returns -4 at it; without: blocks until
                 ``release`` is set); ``p2p_wall_s`` = wall time of each completed pair
    delay_s:     wall time of each GEMM call (the agent's per-GPU threads overlap them)
    gemm_bad_tiles: ``{(device, "gemm" | "gemm_fp8"): {xcd: tiles}}`` failing the GEMM's output checksums
    slow_xcd:    ``{xcd: factor}`` on the burn-in's per-XCD wave time; ``bad_cu[(device, kind)]`` = the CU
                 slot its ``mfma_errors`` come from
    """

    def __init__(self, n: int = 1, rate: float = 1.0, gpu_rate: Optional[Dict[int, float]] = None,
                 rates: Optional[List[float]] = None, cus: int = 256, mem_gib: int = 288, gemm_err: float = 2e-5,
                 mfma: Optional[Dict[int, Tuple[float, int]]] = None,
                 mfma_errors: Optional[Dict[Tuple[int, int], int]] = None, link: Optional[Tuple[float, float]] = None,
                 p2p_gbps: float = 48.0, slow_pairs: Optional[Dict[Tuple[int, int], float]] = None,
                 nopeer: Tuple[Tuple[int, int], ...] = (), rc: int = 0, err: bytes = b"boom", delay_s: float = 0.0,
                 slow_xcd: Optional[Dict[int, float]] = None, bad_cu: Optional[Dict[Tuple[int, int], int]] = None,
                 lds_bad: Optional[Dict[Tuple[int, int], int]] = None,
                 l2_bad: Optional[Dict[Tuple[int, int], int]] = None, slow_cu: Optional[Dict[int, float]] = None,
                 hbm_xcd_slow: Optional[Dict[int, float]] = None, hbm_bad: Optional[Dict[Tuple[int, int], int]] = None,
                 compute_rate: Optional[Dict[int, float]] = None,
                 hung_pairs: Tuple[Tuple[int, int], ...] = (), p2p_wall_s: float = 0.0,
                 gemm_bad_tiles: Optional[Dict[Tuple[int, str], Dict[int, int]]] = None,
                 hang_devices: Tuple[int, ...] = (), abort_devices: Tuple[int, ...] = (),
                 fan_slow: Optional[Dict[Tuple[int, int], float]] = None,
                 fan_errors: Optional[Dict[Tuple[int, int], int]] = None,
                 regfile_bad: Optional[Dict[Tuple[int, int], Tuple[int, int]]] = None,
                 valu_errors: Optional[Dict[Tuple[int, int], int]] = None,
                 valu_bad_cu: Optional[Dict[Tuple[int, int], int]] = None,
                 valu_slow_xcd: Optional[Dict[int, float]] = None):
        from ..ops import diag
        # the fan pass (diag_p2p_fan): fan_slow[(src, dst)] = that pair's rate while every link of src is busy,
        # fan_errors[(src, dst)] = bad words it delivers then
        self.fan_slow = dict(fan_slow or {})
        self.fan_errors = dict(fan_errors or {})
        # hang_devices: a GEMM call on that device never returns (a hung queue: no deadline ends it);
        # abort_devices: it ends the process with SIGABRT, as the HIP runtime does on a GPU memory fault
        self.hang_devices = set(hang_devices)
        self.abort_devices = set(abort_devices)
        self.ref = diag.REFERENCE_RATES
        self.kinds = diag.MFMA_KINDS
        self.n = n
        self.rate = rate
        self.gpu_rate = dict(gpu_rate or {})
        # compute_rate[d]: an extra factor on device d's matrix-core tests only (GEMM, burn-in) -- a lowered
        # power cap slows the core clock, not HBM or the host link
        self.compute_rate = dict(compute_rate or {})
        self.rates = list(rates or [])
        self.cus = cus
        self.mem_gib = mem_gib
        self.gemm_err = gemm_err
        self.gemm_bad_tiles = dict(gemm_bad_tiles or {})
        self.mfma = mfma
        self.mfma_errors = dict(mfma_errors or {})
        self.link = link
        self.p2p_gbps = p2p_gbps
        self.slow_pairs = dict(slow_pairs or {})
        self.nopeer = set(nopeer)
        self.hung_pairs = set(hung_pairs)
        self.p2p_wall_s = p2p_wall_s
        self.p2p_timeouts_ms: List[float] = []
        self.release = threading.Event()
        self.rc = rc
        self.err = err
        self.delay_s = delay_s
        self.slow_xcd = dict(slow_xcd or {})
        self.bad_cu = dict(bad_cu or {})
        self.lds_bad = dict(lds_bad or {})
        # per-XCD HBM: hbm_xcd_slow[xcd] = that XCD's alone rate as a share of the reference; hbm_bad[(device,
        # slot)] = wrong words read there
        self.hbm_xcd_slow = dict(hbm_xcd_slow or {})
        self.hbm_bad = dict(hbm_bad or {})
        self.l2_bad = dict(l2_bad or {})
        self.slow_cu = dict(slow_cu or {})
        # level 3: regfile_bad[(device, row)] = (wrong VGPR words, wrong AGPR words) on SIMD row (slot << 2 | simd);
        # valu_errors[(device, kind)] = wrong lanes, on CU slot valu_bad_cu[(device, kind)]; valu_slow_xcd {xcd: time
        # factor} lags the vector-ALU waves of an XCD only
        self.regfile_bad = dict(regfile_bad or {})
        self.valu_errors = dict(valu_errors or {})
        self.valu_bad_cu = dict(valu_bad_cu or {})
        self.valu_slow_xcd = dict(valu_slow_xcd or {})
        self.calls: List[str] = []
        self.threads: Dict[int, set] = {}
        self.lock = threading.Lock()
        # shared host link: with link_shared, concurrent host_link calls split the host's bandwidth (each gets
        # 1/k of it while k run at once, for link_delay_s); in_flight / peak_* record the overlap
        self.link_shared = False
        self.link_delay_s = 0.0
        self.in_flight: Dict[str, int] = {}
        self.peak: Dict[str, int] = {}

    def _enter(self, what: str) -> int:
        with self.lock:
            k = self.in_flight.get(what, 0) + 1
            self.in_flight[what] = k
            self.peak[what] = max(self.peak.get(what, 0), k)
            return k

    def _leave(self, what: str) -> None:
        with self.lock:
            self.in_flight[what] -= 1

    def _rate(self, device: int) -> float:
        with self.lock:
            if self.rates:
                return self.rates.pop(0)
        return self.gpu_rate.get(device, self.rate)

    def _slots(self):
        """(xcd, slot) of every CU of the device: 8 XCDs (a partition: its share of them) x 4 SEs x 8 CUs."""
        for xcd in range(8 if self.cus >= 256 else max(1, self.cus // 32)):
            for se in range(4):
                for cu in range(8):
                    yield xcd, (xcd << 7) | (se << 5) | cu

    def _log(self, device: int, what: str) -> None:
        with self.lock:
            self.calls.append(what)
            self.threads.setdefault(device, set()).add(threading.current_thread().name)

    # --- C ABI ------------------------------------------------------------------------------------------
    def diag_last_error(self) -> bytes:
        return self.err

    def diag_device_count(self) -> int:
        return self.n

    def diag_device_arch(self, device, buf, size):
        if not 0 <= device < self.n:
            self.err = b"hipSetDevice: invalid device ordinal"
            return -1
        v = f"gfx950:sramecc+:xnack-|AMD Instinct MI355X|{self.cus}|{self.mem_gib << 30}|0000:{0x05 + 0x10 * device:02x}:00.0"
        ctypes.memmove(buf, v.encode() + b"\0", min(size, len(v) + 1))
        return 0

    def _gemm(self, test, device, size, tflops, err, ms):
        self._log(device, test)
        if device in self.abort_devices:
            import os
            import resource
            resource.setrlimit(resource.RLIMIT_CORE, (0, 0))  # no core file from a scripted abort
            os.abort()
        if device in self.hang_devices:
            while True:
                time.sleep(3600)
        self._enter("gemm")
        if self.delay_s:
            time.sleep(self.delay_s)
        self._leave("gemm")
        table = self.ref[test]
        key = size if size in table else min(table, key=lambda k: abs(k - size))
        _put(tflops, ctypes.c_double, self._rate(device) * self.compute_rate.get(device, 1.0) * table[key])
        _put(err, ctypes.c_double, self.gemm_err)
        _put(ms, ctypes.c_double, 0.1)
        return self.rc

    def _checksums(self, test, device, inject, ck_err, out):
        """Tile checksums: ``gemm_bad_tiles[(device, test)] = {xcd: tiles}``; an injected element = one bad
        tile on XCD 0, as on the GPU (workgroup 0 computes tile (0, 0) on XCD 0)."""
        bad = dict(self.gemm_bad_tiles.get((device, test), {}))
        if inject >= 0:
            bad[0] = bad.get(0, 0) + 1
        vals = [0] * 12
        vals[0] = sum(bad.values())
        vals[1] = 256 * vals[0]
        for x, t in bad.items():
            vals[2 + x] = t
        vals[10], vals[11] = (0, 0) if vals[0] else (-1, -1)
        for i, v in enumerate(vals):
            out[i] = v
        _put(ck_err, ctypes.c_double, 0.4 if vals[0] else 3e-8)

    def _checked(self, test, device, size, inject, tol, tflops, err, ms, ck_err, out, floor):
        rc = self._gemm(test, device, size, tflops, err, ms)
        if floor:
            _put(floor, ctypes.c_double, max(tol, 0.0) * 5.2e5)  # tol x the largest column sum|a*b|
        if rc == 0 and tol >= 0:
            self._checksums(test, device, inject, ck_err, out)
        return rc

    def diag_gemm_bf16(self, device, m, n, k, warmup, iters, samples, inject, delta, tol, tflops, err, ms, ck_err, out,
                       floor):
        return self._checked("gemm", device, m, inject, tol, tflops, err, ms, ck_err, out, floor)

    def diag_gemm_fp8(self, device, m, n, k, warmup, iters, samples, inject, delta, tol, tflops, err, ms, ck_err, out,
                      floor):
        return self._checked("gemm_fp8", device, m, inject, tol, tflops, err, ms, ck_err, out, floor)

    def diag_hbm_bandwidth(self, device, nbytes, iters, inject_word, inject_phase, c, r, w, errs):
        self._log(device, "hbm")
        f = self._rate(device)
        _put(errs, ctypes.c_ulonglong, 1 if inject_word >= 0 else 0)
        _put(c, ctypes.c_double, f * self.ref["hbm"]["copy_tbs"])
        _put(r, ctypes.c_double, f * self.ref["hbm"]["read_tbs"])
        _put(w, ctypes.c_double, f * 6.9)
        return self.rc

    def diag_memtest(self, device, nbytes, seed, passes, inject_word, inject_word2, inject_pass, inject_invert, errs,
                     first, gbps):
        self._log(device, "memtest")
        _put(errs, ctypes.c_ulonglong, 0)
        _put(gbps, ctypes.c_double, 5400.0)
        return self.rc

    def diag_mfma_burn_slots(self):
        return 1024

    def diag_mfma_burn(self, device, kind, iters, reps, inject_block, tflops, errors, cu_map):
        """The rate and wrong results of one kind and, with ``cu_map``, the per-CU table: 8 XCDs x 32 CUs (4 SEs x
        8), 8 waves per CU and launch; ``slow_xcd`` {xcd: time factor} and ``bad_cu`` {(device, kind): slot} shape
        it."""
        self._log(device, "mfma")
        if self.rc:
            return self.rc
        if self.mfma is not None:
            tf, e = self.mfma[kind]
        else:
            tf, e = (self.gpu_rate.get(device, self.rate) * self.compute_rate.get(device, 1.0)
                     * self.ref["mfma"][self.kinds[kind]], 0)
        _put(tflops, ctypes.c_double, tf)
        _put(errors, ctypes.c_ulonglong, self.mfma_errors.get((device, kind), e))
        if not cu_map:
            return 0
        nerr = self.mfma_errors.get((device, kind), 0)
        bad_slot = self.bad_cu.get((device, kind))
        for xcd, slot in self._slots():
            waves = 8 * (reps + 1)
            cu_map[3 * slot] = waves
            cu_map[3 * slot + 2] = int(waves * 40000 * self.slow_xcd.get(xcd, 1.0) * self.slow_cu.get(slot, 1.0))
        if bad_slot is not None and nerr:
            cu_map[3 * bad_slot + 1] = nerr
        return 0

    def diag_l2_bandwidth(self, device, slice_bytes, passes, blocks_per_cu, seed, inject_xcd, inject_word, tbs, errors,
                          cu_map):
        """Aggregate rate = rate x reference; per-CU table shaped like the burn-in's (``slow_xcd`` applies,
        ``l2_bad[(device, slot)]`` = wrong words read there)."""
        self._log(device, "l2")
        if self.rc:
            return self.rc
        _put(tbs, ctypes.c_double, self._rate(device) * self.ref["l2"]["read_tbs"])
        total = 0
        for xcd, slot in self._slots():
            waves = 4 * blocks_per_cu
            cu_map[3 * slot] = waves
            cu_map[3 * slot + 2] = int(waves * 90000 * self.slow_xcd.get(xcd, 1.0))
            bad = self.l2_bad.get((device, slot), 0)
            cu_map[3 * slot + 1] = bad
            total += bad
        _put(errors, ctypes.c_ulonglong, total)
        return 0

    def diag_hbm_xcd(self, device, slice_bytes, passes, blocks_per_cu, seed, inject_xcd, inject_word, tbs, errors,
                     cu_map, xcd_tbs):
        """All XCDs together at rate x reference; each XCD alone at rate x reference x ``hbm_xcd_slow``."""
        self._log(device, "hbm_xcd")
        if self.rc:
            return self.rc
        r = self._rate(device)
        _put(tbs, ctypes.c_double, r * self.ref["hbm_xcd"]["read_tbs"])
        total = 0
        nx = 8 if self.cus >= 256 else max(1, self.cus // 32)
        for xcd in range(8):
            # an XCD alone reads at its own path's rate whatever the partition: the device's rate share
            # (rate) is normalised by its CU share
            share = min(1.0, self.cus / 256)
            xcd_tbs[xcd] = r / share * 1.31 * self.hbm_xcd_slow.get(xcd, 1.0) if xcd < nx else 0.0
        for _, slot in self._slots():
            waves = 4 * blocks_per_cu
            cu_map[3 * slot] = waves
            cu_map[3 * slot + 2] = waves * 50000
            bad = self.hbm_bad.get((device, slot), 0)
            cu_map[3 * slot + 1] = bad
            total += bad
        _put(errors, ctypes.c_ulonglong, total)
        return 0

    def diag_lds_test(self, device, rounds, seed, inject_block, errors, cu_map, lds_bytes, ms):
        """Every CU of the device runs `rounds` workgroups; ``lds_bad[(device, slot)]`` = bad words there."""
        self._log(device, "lds")
        if self.rc:
            return self.rc
        total = 0
        for xcd, slot in self._slots():
            cu_map[2 * slot] = rounds
            bad = self.lds_bad.get((device, slot), 0) + (1 if inject_block >= 0 and slot == 0 else 0)
            cu_map[2 * slot + 1] = bad
            total += bad
        _put(errors, ctypes.c_ulonglong, total)
        _put(lds_bytes, ctypes.c_int, 163840 - 16)
        _put(ms, ctypes.c_double, 0.2)
        return 0

    def diag_regfile_slots(self):
        return 4096

    def diag_regfile_test(self, device, rounds, seed, hold, inject_block, inject_reg, errors, simd_map, regs, scratch, ms):
        """Every SIMD of the device runs `rounds` waves; ``regfile_bad[(device, row)]`` = (VGPR, AGPR) bad words."""
        self._log(device, "regfile")
        if self.rc:
            return self.rc
        total = 0
        for _, slot in self._slots():
            for simd in range(4):
                row = (slot << 2) | simd
                simd_map[3 * row] = rounds
                bv, ba = self.regfile_bad.get((device, row), (0, 0))
                if inject_block >= 0 and row == 0:
                    bv, ba = bv + (inject_reg < 2), ba + (inject_reg >= 2)
                simd_map[3 * row + 1], simd_map[3 * row + 2] = bv, ba
                total += bv + ba
        _put(errors, ctypes.c_ulonglong, total)
        _put(regs, ctypes.c_int, 504)
        _put(scratch, ctypes.c_int, 0)
        _put(ms, ctypes.c_double, 0.3)
        return 0

    VALU_RATES = (48000.0, 105000.0, 50000.0)  # G(FL)OP/s of a kind that ops/diag.REFERENCE_RATES does not list

    def diag_valu_burn(self, device, kind, iters, reps, inject_block, gops, errors, cu_map):
        """The vector-ALU burn-in, shaped like diag_mfma_burn (``valu_slow_xcd``, ``valu_errors``,
        ``valu_bad_cu``)."""
        self._log(device, "valu")
        if self.rc:
            return self.rc
        ref = (self.ref.get("valu") or {}).get(("f64", "pk_f32", "i32")[kind], self.VALU_RATES[kind])
        _put(gops, ctypes.c_double, self.gpu_rate.get(device, self.rate) * self.compute_rate.get(device, 1.0) * ref)
        nerr = self.valu_errors.get((device, kind), 0)
        for xcd, slot in self._slots():
            waves = 8 * (reps + 1)
            cu_map[3 * slot] = waves
            cu_map[3 * slot + 2] = int(waves * 60000 * self.valu_slow_xcd.get(xcd, 1.0))
        if nerr:
            cu_map[3 * self.valu_bad_cu.get((device, kind), 0) + 1] = nerr
        if inject_block >= 0:
            cu_map[1] += 1
            nerr += 1
        _put(errors, ctypes.c_ulonglong, nerr)
        return 0

    def diag_host_link(self, device, nbytes, iters, h2d, d2h):
        self._log(device, "host_link")
        f = self.gpu_rate.get(device, self.rate)
        k = self._enter("host_link")
        if self.link_delay_s:
            time.sleep(self.link_delay_s)
        k = max(k, self.in_flight.get("host_link", 1))
        self._leave("host_link")
        if self.link_shared:
            f /= k
        h, d = self.link or (f * self.ref["host_link"]["h2d_gbps"], f * self.ref["host_link"]["d2h_gbps"])
        _put(h2d, ctypes.c_double, h)
        _put(d2h, ctypes.c_double, d)
        return self.rc

    def diag_p2p_copy(self, src, dst, nbytes, iters, timeout_ms, gbps, errors, peer):
        with self.lock:  # node-level: runs on the agent's main thread, after the per-GPU threads
            self.calls.append(f"p2p{src}->{dst}")
            self.p2p_timeouts_ms.append(float(timeout_ms))
        if not (0 <= src < self.n and 0 <= dst < self.n) or src == dst:
            self.err = b"p2p: invalid device pair"
            return -1
        if (src, dst) in self.hung_pairs:
            if timeout_ms > 0 and not self.release.wait(timeout_ms / 1000.0):
                self.err = b"p2p %d->%d: copies did not complete within %d ms (xGMI link or engine hung)" % (
                    src, dst, int(timeout_ms))
                return -4
            self.release.wait()
        elif self.p2p_wall_s:
            time.sleep(self.p2p_wall_s)
        _put(gbps, ctypes.c_double, self.slow_pairs.get((src, dst), self.p2p_gbps))
        _put(errors, ctypes.c_ulonglong, 0)
        _put(peer, ctypes.c_int, 0 if (src, dst) in self.nopeer else 1)
        return 0

    def diag_p2p_fan(self, src, dsts, ndst, nbytes, iters, timeout_ms, gbps, errors, peer, total):
        """Every peer of ``src`` at once: a pair's rate is ``fan_slow[(src, dst)]`` when given (a link that holds up
        alone but not under load), else its pair rate (``slow_pairs`` / ``p2p_gbps``)."""
        with self.lock:
            self.calls.append(f"fan{src}")
            self.p2p_timeouts_ms.append(float(timeout_ms))
        peers = [dsts[i] for i in range(ndst)]
        if not 0 <= src < self.n or not peers or any(not 0 <= d < self.n or d == src for d in peers):
            self.err = b"p2p fan: every peer must be a device other than the source"
            return -2
        for d in peers:
            if (src, d) in self.hung_pairs and timeout_ms > 0 and not self.release.wait(timeout_ms / 1000.0):
                self.err = b"p2p fan %d->%d: copies did not complete within %d ms (xGMI link or engine hung)" % (
                    src, d, int(timeout_ms))
                return -4
        for i, d in enumerate(peers):
            gbps[i] = self.fan_slow.get((src, d), self.slow_pairs.get((src, d), self.p2p_gbps))
            errors[i] = self.fan_errors.get((src, d), 0)
            peer[i] = 0 if (src, d) in self.nopeer else 1
        _put(total, ctypes.c_double, float(sum(gbps[i] for i in range(ndst))))
        return 0


class FakeXgmiLib:
    """``libmi355x_xgmi.so`` for a node of ``n`` GPUs.

    kernel_gbps:   rate of every destination, alone or under the fan, in both modes
    kernel_slow:   ``{(src, dst, mode): rate}`` overrides it (``mode``: "store" | "load" for the pair-alone launch,
                   "fan_store" | "fan_load" for that destination under the fan)
    kernel_errors: ``{(src, dst, mode): bad elements}``, keyed the same way
    hung:          ``(src, dst)`` pairs whose launch never completes: -4 at the deadline (it is waited out)
    Calls are logged as ``xk{mode}{src}->{dsts}``."""

    def __init__(self, n: int = 8, kernel_gbps: float = 55.0,
                 kernel_slow: Optional[Dict[Tuple[int, int, str], float]] = None,
                 kernel_errors: Optional[Dict[Tuple[int, int, str], int]] = None,
                 hung: Tuple[Tuple[int, int], ...] = ()):
        self.n, self.kernel_gbps = n, kernel_gbps
        self.kernel_slow = dict(kernel_slow or {})
        self.kernel_errors = dict(kernel_errors or {})
        self.hung = set(hung)
        self.release = threading.Event()
        self.calls: List[str] = []
        self.timeouts_ms: List[float] = []
        self.err = b"boom"

    def xgmi_last_error(self) -> bytes:
        return self.err

    def xgmi_device_count(self) -> int:
        return self.n

    def xgmi_kernel_fan(self, src, dsts, ndst, nbytes, iters, mode, timeout_ms, inject_dst, inject_word, gbps, errors,
                        first_bad, peer, total):
        name = ("store", "load")[mode]
        peers = [dsts[i] for i in range(ndst)]
        self.calls.append(f"xk{name}{src}->{','.join(map(str, peers))}")
        self.timeouts_ms.append(float(timeout_ms))
        if not 0 <= src < self.n or not 1 <= ndst <= 64 or any(not 0 <= d < self.n for d in peers) or nbytes < 16:
            self.err = b"xgmi kernel fan: need a valid source, 1..64 destinations, iters >= 1, bytes >= 16"
            return -2
        for d in peers:
            if (src, d) in self.hung:
                if timeout_ms > 0:
                    self.release.wait(timeout_ms / 1000.0)
                else:
                    self.release.wait()
                if not self.release.is_set():
                    self.err = b"xgmi kernel %s %d->%d: the launches did not complete within %d ms (xGMI link hung)" % (
                        name.encode(), src, d, int(timeout_ms))
                    return -4
        key = name if ndst == 1 else "fan_" + name
        for i, d in enumerate(peers):
            gbps[i] = self.kernel_slow.get((src, d, key), self.kernel_gbps)
            errors[i] = self.kernel_errors.get((src, d, key), 0)
            first_bad[i] = 0 if errors[i] else (1 << 64) - 1
            peer[i] = 1
        _put(total, ctypes.c_double, float(sum(gbps[i] for i in range(ndst))))
        return 0


class FakeAtomicsLib:
    """``libmi355x_atomics.so`` for a node of ``n`` GPUs: every kind clean on all ``xcds`` XCDs.

    wrong:    ``{(device, kind index): wrong elements}``; the first of them is element ``first_bad``, read back as
              ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``atomics{device}`` in ``calls``: empty = never called."""

    KINDS = 8
    WANT = 0x47800100

    def __init__(self, n: int = 8, wrong: Optional[Dict[Tuple[int, int], int]] = None, first_bad: int = 0x690,
                 xcds: int = 8, ms: float = 0.4, physical: Optional[int] = None):
        self.n, self.wrong, self.first_bad, self.xcds, self.ms = n, dict(wrong or {}), first_bad, xcds, ms
        self.physical = physical
        self.calls: List[str] = []
        self.err = b"boom"

    def atomics_last_error(self) -> bytes:
        return self.err

    def atomics_device_count(self) -> int:
        return self.n if self.physical is None else 1

    def atomics_test(self, device, words, adders, kind_mask, seed, iters, inject_kind, inject_word, inject_drop_adder,
                     errors, first_bad, got, want, want_without, ops, xcd_waves, ms):
        if self.physical is not None:
            if device != 0:
                self.err = b"hipSetDevice(device): invalid device ordinal"
                return -1
            device = self.physical
        self.calls.append(f"atomics{device}")
        if not 0 <= device < self.n or words < 1 or not 1 <= adders <= 32 or iters < 1 or not kind_mask \
                or kind_mask >> self.KINDS:
            self.err = b"atomics test: need a valid device, words 1..2^31, adders 1..32, iters >= 1 and a mask of known kinds"
            return -2
        for k in range(self.KINDS):
            on = bool((kind_mask >> k) & 1)
            bad = self.wrong.get((device, k), 0) if on else 0
            if on and k == inject_kind:
                bad += 1
            errors[k] = bad
            first_bad[k] = (inject_word if k == inject_kind else self.first_bad) if bad else (1 << 64) - 1
            want[k] = self.WANT if bad else 0
            got[k] = self.WANT ^ 0x100 if bad else 0
            want_without[k] = got[k] if k == inject_kind and inject_drop_adder >= 0 else 0
            ops[k] = words * adders if on else 0
            ms[k] = self.ms if on else 0.0
            for x in range(8):
                xcd_waves[8 * k + x] = max(1, -(-words // 64) * adders // self.xcds) if on and x < self.xcds else 0
        return 0


class FakeHbmscanLib:
    """``libmi355x_hbmscan.so`` for a node of ``n`` GPUs of 288 GiB with ``free_gib`` free: every word clean.

    bad:        ``{device: wrong words}``, all bit 37 read as 1 where 0 was written, the first at +0x1a2b3c40 of
                chunk 5 in the ``invert`` phase: finding ``stuck_bit``
    incomplete: the devices whose scan runs out of its deadline after ``random`` step 1 (whatever ``deadline_s`` is)
    physical:   the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``hbmscan{device}`` in ``calls`` (empty = never called), their deadlines in ``deadlines``."""

    TOTAL = 309220868096  # hipMemGetInfo's total on an MI355X

    def __init__(self, n: int = 8, bad: Optional[Dict[int, int]] = None, incomplete: Tuple[int, ...] = (),
                 free_gib: float = 287.0, gbs: float = 5000.0, physical: Optional[int] = None):
        self.n, self.bad, self.incomplete = n, dict(bad or {}), set(incomplete)
        self.free, self.gbs, self.physical = int(free_gib * (1 << 30)), gbs, physical
        self.calls: List[str] = []
        self.deadlines: List[float] = []
        self.err = b"boom"

    def hbmscan_last_error(self) -> bytes:
        return self.err

    def hbmscan_device_count(self) -> int:
        return self.n if self.physical is None else 1

    def hbmscan_plan(self, free_bytes, total_bytes, reserve, limit, chunk, plan_out):
        target = max(0, free_bytes - reserve)
        target = min(target, limit) if limit else target
        target -= target % 16
        count = -(-target // chunk) if chunk >= 16 and chunk % 16 == 0 else 0
        if free_bytes > total_bytes or target < 16 or not 1 <= count <= 4096:
            self.err = b"hbmscan plan: need free <= total, a target of at least 16 bytes and at most 4096 chunks"
            return -2
        for i in range(count):
            plan_out[i] = chunk if i + 1 < count else target - i * chunk
        return count

    def hbmscan_want(self, phase, step, global_word, seed, out):
        if not 0 <= phase < 4 or not 0 <= step < (3, 16, 256, 3)[phase]:
            self.err = b"hbmscan want: no such phase or step"
            return -2
        out[0] = out[1] = out[2] = out[3] = 0  # (the fake models no content: tests/test_hbmscan_cpu.py has the model)
        return 0

    def hbmscan_classify(self, records, n, hist, index_base, tested_words, finding_out):
        f = finding_out._obj if hasattr(finding_out, "_obj") else finding_out
        f.kind, f.bit, f.direction, f.chunk = (1, 37, 1, -1) if n else (0, -1, -1, -1)
        return 0

    def hbmscan_test(self, device, limit, reserve, chunk, min_chunk, hold_ms, random_passes, seed, deadline_s,
                     index_base, flips, n_flips, stuck_word, stuck_bit, stuck_value, alias_a, alias_b, fail_alloc_at,
                     totals, phase_errors, phase_ms, phase_wall_ms, phase_bytes, records, hist, finding):
        if self.physical is not None:
            if device != 0:
                self.err = b"hipSetDevice(device): invalid device ordinal"
                return -1
            device = self.physical
        self.calls.append(f"hbmscan{device}")
        self.deadlines.append(float(deadline_s))
        plan = (ctypes.c_ulonglong * 4096)()
        count = self.hbmscan_plan(self.free, self.TOTAL, reserve, limit, chunk, plan) if 0 <= device < self.n else -2
        if count < 0 or not 1 <= random_passes <= 64 or not 0 <= hold_ms <= 60000 or deadline_s < 0:
            self.err = (b"hbmscan test: need a valid device, chunk and min_chunk multiples of 16 (chunk up to 16 GiB), "
                        b"hold_ms 0..60000, random_passes 1..64, deadline_s >= 0")
            return -2
        tested = sum(plan[i] for i in range(count))
        bad = self.bad.get(device, 0)
        stopped = device in self.incomplete
        for i, v in enumerate((self.TOTAL, self.free, tested, tested, count, bad, min(bad, 64), 0 if stopped else 1,
                               1 if tested < 2 << 30 else 0, 2 if stopped else 3, 1 if stopped else 2, 0, 0, 0, 0, 0)):
            totals[i] = v
        sweeps = (4, 24, 6 * random_passes, 4)
        for ph in range(4):
            ran = ph < 2 or not stopped
            phase_errors[ph] = bad if ph == 1 else 0
            phase_bytes[ph] = float(tested * sweeps[ph]) if ran else 0.0
            phase_ms[ph] = phase_bytes[ph] / (self.gbs * 1e9) * 1e3
            phase_wall_ms[ph] = phase_ms[ph] + (2 * hold_ms if ph == 3 and ran else 0)
        for i in range(256):
            hist[i] = 0
        hist[2 * 37 + 1] = min(bad, 4096)
        for i in range(min(bad, 64)):
            r = records[i]
            r.phase, r.step, r.chunk, r.word = 1, 1, 5 if count > 5 else 0, (0x1a2b3c40 >> 4) + i
            r.global_word = r.chunk * (chunk // 16) + r.word
            for lane in range(4):
                r.want[lane], r.got[lane] = 0, (1 << 5) if lane == 1 else 0
        f = finding._obj if hasattr(finding, "_obj") else finding
        f.kind, f.bit, f.direction, f.chunk, f.victim, f.source, f.span = (1, 37, 1, -1, 0, 0, 0) if bad else (0, -1, -1, -1, 0, 0, 0)
        return 0


class _SimdFake:
    """What the stand-ins of the SIMD-located libraries share: the node (``n`` GPUs of ``xcds`` x 32 CUs, a launch
    ``ms`` long), the wrong results asked for (``bad``, all on SIMD map row ``bad_row``), the one GPU a narrowed process
    sees (``physical``), the ``calls`` log and the last error."""

    SLOTS = 4096
    BAD_ROW = (((5 << 7) | (1 << 5) | 7) << 2) | 2  # xcd5/se1/cu7/simd2

    def __init__(self, n, bad, bad_row, xcds, ms, physical):
        self.n, self.bad, self.bad_row, self.xcds, self.ms, self.physical = n, dict(bad or {}), bad_row, xcds, ms, physical
        self.calls: List[str] = []
        self.err = b"boom"

    def _count(self) -> int:
        return self.n if self.physical is None else 1

    def _device(self, device: int, log: Optional[str] = None) -> Optional[int]:
        """The node's ordinal of ``device`` (logged as ``{log}{ordinal}``), None with the error set when a narrowed
        process asks for another than its own."""
        if self.physical is not None:
            if device != 0:
                self.err = b"hipSetDevice(device): invalid device ordinal"
                return None
            device = self.physical
        if log is not None:
            self.calls.append(f"{log}{device}")
        return device

    def _fill_map(self, simd_map, grid: int, launches: int, ticks: int) -> None:
        """``launches`` launches of ``grid`` workgroups, ``ticks`` long each, and nothing wrong."""
        for r in range(3 * self.SLOTS):
            simd_map[r] = 0
        rows = [(((x << 7) | (se << 5) | cu) << 2) | simd for x in range(self.xcds) for se in range(4)
                for cu in range(8) for simd in range(4)][:4 * grid]  # a workgroup's 4 waves: one per SIMD of a CU
        for r in rows:
            simd_map[3 * r] = max(1, 4 * grid // len(rows)) * launches
            simd_map[3 * r + 2] = ticks * launches

    def _blame(self, simd_map, wrong: int) -> None:
        """``wrong`` (> 0) wrong words on ``bad_row``."""
        simd_map[3 * self.bad_row] = max(1, simd_map[3 * self.bad_row])
        simd_map[3 * self.bad_row + 1] += wrong


class FakeLanesLib(_SimdFake):
    """``libmi355x_lanes.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every op clean on every SIMD.

    bad:      ``{(device, op index): wrong lanes}``, all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the
              first of them lane 9, chain 1, read as ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``lanes{device}`` in ``calls``: empty = never called."""

    OPS = 39
    WANT = 0x5EED1A9E

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.2,
                 physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)

    def lanes_last_error(self) -> bytes:
        return self.err

    def lanes_device_count(self) -> int:
        return self._count()

    def lanes_slots(self) -> int:
        return self.SLOTS

    def lanes_test(self, device, blocks, iters, reps, op_mask, seed, inject_op, inject_block, inject_skip_iter,
                   errors, first_where, got, want, ms, simd_map, blocks_run):
        device = self._device(device, "lanes")
        if device is None:
            return -1
        if not 0 <= device < self.n or blocks < 0 or not 1 <= iters <= 1 << 20 or reps < 1 or not op_mask \
                or op_mask >> self.OPS:
            self.err = (b"lanes test: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a "
                        b"mask of known ops")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, (reps + 1) * bin(op_mask).count("1"), 1000 * iters)
        for k in range(self.OPS):
            on = bool((op_mask >> k) & 1)
            wrong = self.bad.get((device, k), 0) if on else 0
            if on and k == inject_op:
                wrong += 1
            errors[k] = wrong
            first_where[k] = ((self.bad_row << 16) | (9 << 8) | 1) if wrong else (1 << 64) - 1
            want[k] = self.WANT if wrong else 0
            got[k] = self.WANT ^ 0x100 if wrong else 0
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def lanes_apply(self, device, op, iter, x_in, y_in, x_out, y_out):
        self.err = b"lanes apply: the stand-in has no wave to apply an instruction on"
        return -1


def cvt_c_ops() -> List[str]:
    """The op names of csrc/cvt/cvt_ref.h's table, in order."""
    import os
    import re
    with open(os.path.join(os.path.dirname(__file__), "..", "csrc", "cvt", "cvt_ref.h")) as f:
        return re.findall(r'^\s*X\((\w+), "v_cvt_\w+", CG_', f.read(), re.M)


class FakeCvtLib(_SimdFake):
    """``libmi355x_cvt.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every op clean on every SIMD, the waves in
    float mode ``mode`` (MODE bits 7:0; 0xf0: round-to-nearest-even, denormals kept).

    bad:      ``{(device, op index): wrong words}``, all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the
              first of them lane 9, chain 1, read as ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``cvt{device}`` in ``calls``: empty = never called."""

    OPS = len(cvt_c_ops())  # the op table's length, read from cvt_ref.h: nothing repeats the count
    WANT = 0x5EEDC0A7

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.05,
                 mode: int = 0xf0, physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)
        self.float_mode = mode

    def cvt_last_error(self) -> bytes:
        return self.err

    def cvt_device_count(self) -> int:
        return self._count()

    def cvt_slots(self) -> int:
        return self.SLOTS

    def cvt_ops(self) -> int:
        return self.OPS

    def cvt_row_words(self, op, operand_words, result_words):
        self.err = b"cvt row_words: the stand-in has no model"
        return -1

    def cvt_shape_rows(self, op, seed, n, rows):
        self.err = b"cvt shape_rows: the stand-in has no model"
        return -1

    def cvt_model_rows(self, op, rows, n, out, ok):
        self.err = b"cvt model_rows: the stand-in has no model"
        return -1

    def cvt_test(self, device, blocks, iters, reps, ops, nops, seed, inject_op, inject_block, inject_skip_iter,
                 errors, first, ms, mode, simd_map, blocks_run):
        device = self._device(device, "cvt")
        if device is None:
            return -1
        chosen = [ops[i] for i in range(nops)] if 1 <= nops <= self.OPS else []
        if not 0 <= device < self.n or blocks < 0 or not 1 <= iters <= 1 << 16 or reps < 1 or not chosen \
                or len(set(chosen)) != len(chosen) or not all(0 <= k < self.OPS for k in chosen):
            self.err = (b"cvt test: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^16, reps >= 1 and a list "
                        b"of distinct known ops")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        if (inject_op >= 0 and (inject_op not in chosen or not 0 <= inject_block < grid or inject_skip_iter >= iters)):
            self.err = b"cvt test: inject_op must be in the list, inject_block inside the grid and inject_skip_iter below iters"
            return -2
        _put(mode, ctypes.c_uint, self.float_mode)
        if self.float_mode & 0xff != 0xf0:
            field = b"FP_ROUND" if self.float_mode & 0xf else b"FP_DENORM"
            self.err = b"cvt test: the waves run with MODE." + field + b": the model holds for another"
            return -3
        self._fill_map(simd_map, grid, (reps + 1) * len(chosen), 1000 * iters)
        for k in range(self.OPS):
            on = k in chosen
            wrong = self.bad.get((device, k), 0) if on else 0
            if on and k == inject_op:
                wrong += 1
            errors[k] = wrong
            first[4 * k] = ((self.bad_row << 16) | (9 << 8) | 1) if wrong else (1 << 64) - 1
            first[4 * k + 1] = 0
            first[4 * k + 2] = self.WANT ^ 0x100 if wrong else 0
            first[4 * k + 3] = self.WANT if wrong else 0
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def cvt_apply_many(self, device, op, rows, nrows, out):
        self.err = b"cvt apply: the stand-in has no wave to apply an instruction on"
        return -1


class FakeIfetchLib(_SimdFake):
    """``libmi355x_ifetch.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every row of both parts clean on every
    SIMD, the walk kernel's blocks ``BLOCK_BYTES`` apart.

    bad:      ``{(device, part, row): wrong words}`` with part ``"walk"`` (row: an nb) or ``"branch"`` (row: an op
              index), all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the first of them lane 9 (the walk) /
              chain 1 (a branch op), read as ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``ifetch_walk{device}`` / ``ifetch_branch{device}`` in ``calls``: empty = never called."""

    OPS = 10
    NB = 1024
    BLOCK_BYTES = 456
    WANT = 0x1FE7C4ED

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, str, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.05,
                 physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)

    def ifetch_last_error(self) -> bytes:
        return self.err

    def ifetch_device_count(self) -> int:
        return self._count()

    def ifetch_slots(self) -> int:
        return self.SLOTS

    def ifetch_blocks(self) -> int:
        return self.NB

    def ifetch_block_map(self, device, addrs):
        for b in range(self.NB):
            addrs[b] = 0x7f0000100000 + self.BLOCK_BYTES * (self.NB - 1 - b)
        return 0

    def _record(self, first, k, wrong, where):
        first[4 * k] = where if wrong else (1 << 64) - 1
        first[4 * k + 1] = 0
        first[4 * k + 2] = self.WANT ^ 0x100 if wrong else 0
        first[4 * k + 3] = self.WANT if wrong else 0

    def ifetch_walk_test(self, device, blocks, steps, reps, nbs, nrows, seed, inject_row, inject_block, inject_skip_step,
                         errors, first, ms, footprint, visited, simd_map, blocks_run):
        device = self._device(device, "ifetch_walk")
        if device is None:
            return -1
        rows = [nbs[i] for i in range(nrows)] if 1 <= nrows <= 64 else []
        if not 0 <= device < self.n or blocks < 0 or not 1 <= steps <= 1 << 16 or reps < 1 or not rows \
                or not all(1 <= v <= self.NB for v in rows):
            self.err = (b"ifetch walk: need a valid device, blocks >= 0 (0: 4 per CU), steps 1..2^16, reps >= 1 and 1..64 "
                        b"rows of nb 1..1024")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        if inject_row >= 0 and (inject_row >= nrows or not 0 <= inject_block < grid or inject_skip_step >= steps):
            self.err = (b"ifetch walk: inject_row must be one of the rows, inject_block inside the grid and "
                        b"inject_skip_step below steps")
            return -2
        for nb in rows:  # 64 paths x steps draws: the stand-in refuses what cannot cover nb blocks on average
            if 64 * steps < 4 * nb:
                self.err = b"ifetch walk: the 64 paths of seed %d visit fewer than %d blocks in %d steps" % (seed, nb, steps)
                return -2
        self._fill_map(simd_map, grid, (reps + 1) * len(rows), 1000 * steps)
        for k, nb in enumerate(rows):
            wrong = self.bad.get((device, "walk", nb), 0) + (1 if k == inject_row else 0)
            errors[k] = wrong
            self._record(first, k, wrong, (self.bad_row << 16) | (9 << 8))
            ms[k] = self.ms
            footprint[k] = self.BLOCK_BYTES * nb
            visited[k] = nb
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def ifetch_branch_test(self, device, blocks, iters, reps, ops, nops, seed, inject_op, inject_block, inject_skip_iter,
                           errors, first, ms, simd_map, blocks_run):
        device = self._device(device, "ifetch_branch")
        if device is None:
            return -1
        chosen = [ops[i] for i in range(nops)] if 1 <= nops <= self.OPS else []
        if not 0 <= device < self.n or blocks < 0 or not 1 <= iters <= 1 << 20 or reps < 1 or not chosen \
                or not all(0 <= k < self.OPS for k in chosen):
            self.err = (b"ifetch branch: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a "
                        b"list of known ops")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        if inject_op >= 0 and (inject_op not in chosen or not 0 <= inject_block < grid or inject_skip_iter >= iters):
            self.err = (b"ifetch branch: inject_op must be in the list, inject_block inside the grid and inject_skip_iter "
                        b"below iters")
            return -2
        self._fill_map(simd_map, grid, (reps + 1) * len(chosen), 100 * iters)
        for k in range(self.OPS):
            on = k in chosen
            wrong = (self.bad.get((device, "branch", k), 0) + (1 if k == inject_op else 0)) if on else 0
            errors[k] = wrong
            self._record(first, k, wrong, (self.bad_row << 16) | 1)
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def ifetch_apply_blocks(self, device, blocks, n, x, p, x_out, p_out):
        self.err = b"ifetch apply_blocks: the stand-in has no wave to run a block on"
        return -1

    def ifetch_apply(self, device, op, n, w, cond, out):
        self.err = b"ifetch apply: the stand-in has no wave to apply an instruction on"
        return -1


class FakeHandoffLib(_SimdFake):
    """``libmi355x_handoff.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every row clean and complete, block b on
    CU ``b // xcds`` of XCD ``b % xcds`` (so ``cross`` pairs lie on different XCDs and ``same`` pairs on one).

    bad:      ``{(device, row): wrong words}`` (row: the native index, form * 2 + placement), all on SIMD map row
              ``bad_row`` (xcd5/se1/cu7/simd2), the first of them lane 9, word 37 of block 3's slab in round 5 of the
              first timed launch, read as that word of round 4 (``stale``: ``STALE``) or, for a row listed in
              ``corrupt``, as ``want ^ 0x100``
    timeout:  ``{(device, row): waits}`` that ran out, the first workgroup 2's for the flag of block 3 in round 5
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    The hooks act as the library's do: the flip gives 1 ``corrupt`` word at ``inject_block``, the stale word 1 ``stale``
    word at its consumer, the mute 1 timeout of its consumer and no launch completes that round.
    Calls are logged as ``handoff{device}`` in ``calls``: empty = never called."""

    ROWS = 8
    LDS = 81 * 1024
    WANT = 0x4A2D0FF1
    STALE = 0x0DD0FF1C

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None, corrupt: Tuple[int, ...] = (),
                 timeout: Optional[Dict[Tuple[int, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.4,
                 physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)
        self.corrupt, self.timeout = set(corrupt), dict(timeout or {})

    def handoff_last_error(self) -> bytes:
        return self.err

    def handoff_device_count(self) -> int:
        return self._count()

    def handoff_slots(self) -> int:
        return self.SLOTS

    def handoff_lds_bytes(self) -> int:
        return self.LDS

    def _slot(self, block: int) -> int:
        cu = block // self.xcds
        return ((block % self.xcds) << 7) | ((cu // 8) << 5) | (cu % 8)

    def handoff_test(self, device, blocks, rounds, reps, rows, nrows, seed, spin_ms, jitter, inject_row, inject_block,
                     inject_round, inject_stale_word, inject_mute, errors, words, timeouts, first, tmo, pairs, ms,
                     simd_map, blocks_run):
        device = self._device(device, "handoff")
        if device is None:
            return -1
        chosen = [rows[i] for i in range(nrows)] if 1 <= nrows <= self.ROWS else []
        if not 0 <= device < self.n or not 1 <= rounds <= 1 << 15 or reps < 1 or not 1 <= spin_ms <= 1000 or not chosen \
                or not all(0 <= k < self.ROWS for k in chosen):
            self.err = b"handoff: need a valid device, rounds 1..2^15, reps >= 1, spin_ms 1..1000 and a list of known rows"
            return -2
        cus = self.xcds * 32
        grid = blocks or cus
        if grid < 16 or grid > cus or grid % 8:
            self.err = (b"handoff: blocks must be 0 (one per CU) or a multiple of 8 from 16 to the CU count %d, not %d: "
                        b"a larger grid is not co-resident, a smaller one pairs a workgroup with itself" % (cus, grid))
            return -2
        _put(blocks_run, ctypes.c_int, grid)
        if inject_row >= 0 and inject_row not in chosen:
            self.err = b"handoff: inject_row must be in the list"
            return -2
        if inject_row >= 0:
            limit = 512 if inject_row // 2 == 3 else 1024
            if not 0 <= inject_block < grid or not 0 <= inject_round < rounds or inject_stale_word >= limit \
                    or (inject_stale_word >= 0 and (inject_round < 1 or inject_mute)):
                self.err = (b"handoff: inject_block must lie inside the grid, inject_round inside the rounds, "
                            b"inject_stale_word inside the slab and in a round >= 1 (round 0 has no round before), and "
                            b"one hook at a time")
                return -2
        for r in range(3 * self.SLOTS):
            simd_map[r] = 0
        launches = (reps + 1) * len(chosen)
        for b in range(grid):
            for simd in range(4):
                simd_map[3 * ((self._slot(b) << 2) | simd)] = launches
                simd_map[3 * ((self._slot(b) << 2) | simd) + 2] = 1000 * rounds * launches
        for k in range(self.ROWS):
            on = k in chosen
            stride, per = (8 if k % 2 else 1), (512 if k // 2 == 3 else 1024)
            errors[k] = timeouts[k] = 0
            words[k] = grid * rounds * per * (reps + 1) if on else 0
            for j in range(8):
                first[8 * k + j] = 0
            first[8 * k] = (1 << 64) - 1
            for j in range(4):
                tmo[4 * k + j] = 0
            same = sum(1 for b in range(grid) if self._slot(b) >> 7 == self._slot((b + stride) % grid) >> 7)
            pairs[3 * k], pairs[3 * k + 1], pairs[3 * k + 2] = (grid - same, same, 0) if on else (0, 0, 0)
            ms[k] = self.ms if on else 0.0
            if not on:
                continue
            record = None  # where, producer, round, word, got, want, class, age, launch
            wrong = self.bad.get((device, k), 0)
            if wrong:
                cls = 2 if k in self.corrupt else 1
                record = ((self.bad_row << 16) | 9, 3, 5, 37, self.WANT ^ 0x100 if cls == 2 else self.STALE, self.WANT,
                          cls, 0 if cls == 2 else 1, 1)
                self._blame(simd_map, wrong)
            waits = self.timeout.get((device, k), 0)
            gave_up = (2, 1, 3, 5) if waits else None
            if k == inject_row:
                consumer = (inject_block - stride) % grid
                if inject_mute:
                    waits += 1
                    gave_up = (consumer, 4 - 1 if k // 2 == 3 else 1, inject_block, inject_round)
                    words[k] -= grid * (rounds - inject_round) * per  # nobody finishes that round
                else:
                    at = consumer if inject_stale_word >= 0 else inject_block
                    row = (self._slot(at) << 2) | 0
                    producer = inject_block if inject_stale_word >= 0 else (inject_block + stride) % grid
                    record = ((row << 16) | (inject_stale_word // 4 % 64 if inject_stale_word >= 0 else 0), producer,
                              inject_round, max(inject_stale_word, 0),
                              self.STALE if inject_stale_word >= 0 else self.WANT ^ 0x10, self.WANT,
                              1 if inject_stale_word >= 0 else 2, 1 if inject_stale_word >= 0 else 0, 0)
                    wrong += 1
                    simd_map[3 * row + 1] += 1
            errors[k] = wrong
            if record:
                where, producer, rnd, word, got, want, cls, age, launch = record
                for j, v in enumerate((where, (producer << 32) | (rnd << 16) | word, got, want, self._slot(producer), cls,
                                       age, launch)):
                    first[8 * k + j] = v
            timeouts[k] = waits
            if gave_up:
                for j, v in enumerate(gave_up):
                    tmo[4 * k + j] = v
        return 0


class FakeScratchLib(_SimdFake):
    """``libmi355x_scratch.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every row clean, wave w on SIMD ``w % 4``
    of CU ``(w // 4) // xcds % 32`` of XCD ``(w // 4) % xcds``.

    bad:      ``{(device, row): wrong words}`` (row: the native index, the position in ``ops.scratch.ROWS``), all on
              SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the first of them lane 9 of wave 3 in the first timed
              launch; on the isolate row it is classified as listed in ``classes`` (``{row: "alias" | "stale" |
              "corrupt"}``, default ``corrupt``; an alias is written by wave 4)
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    The hooks act as the library's do: exactly one wrong word of the hook's class in the warm-up launch.
    Calls are logged as ``scratch{device}`` in ``calls``: empty = never called."""

    WANT = 0x5C7A7C11
    FRAME = {"isolate": 1040, "index": 272, "calls": 400}

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None,
                 classes: Optional[Dict[int, str]] = None, bad_row: int = _SimdFake.BAD_ROW,
                 xcds: int = 8, ms: float = 0.05, physical: Optional[int] = None):
        from ..ops import scratch as ops_scratch
        self.rows = len(ops_scratch.ROWS)
        self.iso, self.index, self.calls_row = self.rows - 3, self.rows - 2, self.rows - 1
        super().__init__(n, bad, bad_row, xcds, ms, physical)
        self.classes = dict(classes or {})

    def scratch_last_error(self) -> bytes:
        return self.err

    def scratch_device_count(self) -> int:
        return self._count()

    def scratch_slots(self) -> int:
        return self.SLOTS

    def scratch_rows(self) -> int:
        return self.rows

    def _simd(self, wave: int) -> int:
        block = wave // 4
        cu = block // self.xcds % 32
        return ((((block % self.xcds) << 7) | ((cu // 8) << 5) | (cu % 8)) << 2) | (wave % 4)

    def scratch_test(self, device, rows, nrows, blocks, iso_blocks, rounds, reps, seed, inject_row,
                     inject_wave, inject_round, inject_alias, inject_stale_word, errors, words, ms, first, frame_bytes,
                     info, simd_map):
        device = self._device(device, "scratch")
        if device is None:
            return -1
        chosen = [rows[i] for i in range(nrows)] if 1 <= nrows <= self.rows else []
        if not 0 <= device < self.n or not 1 <= rounds <= 16 or reps < 1 \
                or blocks < 0 or iso_blocks < 0 or not chosen or not all(0 <= k < self.rows for k in chosen):
            self.err = (b"scratch: need a valid device, rounds 1..16, reps >= 1 and a list of known rows")
            return -2
        cus = self.xcds * 32
        grid = blocks or cus
        iso_grid = iso_blocks or min(2 * cus * 32 // 4, 4096)
        if iso_grid * 4 > 16384 or grid > 4096:
            self.err = (b"scratch: the isolate grid may have at most 16384 waves (4096 workgroups: the wave's field of the "
                        b"written word has 14 bits), not %d workgroups; the frames grid at most 4096 workgroups"
                        % iso_grid)
            return -2
        if inject_row >= 0 and inject_row not in chosen:
            self.err = b"scratch: inject_row must be in the list"
            return -2
        if inject_row >= 0:
            iso = inject_row == self.iso
            waves = (iso_grid if iso else grid) * 4
            if not 0 <= inject_wave < waves or (not iso and (inject_alias or inject_stale_word >= 0 or inject_round != 0)) \
                    or not 0 <= inject_round < rounds or (inject_alias and inject_wave + 1 >= waves) \
                    or inject_stale_word >= 256 or (inject_stale_word >= 0 and inject_round < 1) \
                    or (inject_alias and inject_stale_word >= 0):
                self.err = (b"scratch: inject_wave must lie inside the row's grid (an alias needs wave + 1 there too), "
                            b"inject_round inside the rounds, inject_stale_word inside the frame and in a round >= 1 (round 0 "
                            b"has no round before), one hook at a time, and only the isolate row has the alias and stale "
                            b"hooks and rounds")
                return -2
        for r in range(3 * self.SLOTS):
            simd_map[r] = 0
        for j in range(8):
            info[j] = 0
        info[3], info[4], info[5] = iso_grid * 4, grid, iso_grid
        classes = {"alias": 1, "stale": 2, "corrupt": 3}
        for k in range(self.rows):
            on = k in chosen
            errors[k] = words[k] = 0
            for j in range(10):
                first[10 * k + j] = 0
            first[10 * k] = (1 << 64) - 1
            frame_bytes[k] = 0
            ms[k] = self.ms if on else 0.0
            if not on:
                continue
            waves = (iso_grid if k == self.iso else grid) * 4
            for w in range(waves):
                simd_map[3 * self._simd(w)] += reps + 1
                simd_map[3 * self._simd(w) + 2] += 1000 * (reps + 1)
            if k == self.iso:
                per, frame_bytes[k] = waves * 64 * 256 * rounds, self.FRAME["isolate"]
                info[0] = min(waves, cus * 32 // 2)  # half the slots: a 1 KiB frame halves nothing, the fake just says so
                info[1] = info[2] = cus * 32 * 64 * 1040
            else:
                per, frame_bytes[k] = waves * 64 * 17, self.FRAME["index" if k == self.index else "calls"]
            words[k] = per * (reps + 1)
            record = None  # where, wave, word, got, want, class, age, writer wave, writer row, launch
            wrong = self.bad.get((device, k), 0)
            if wrong:
                cls = classes[self.classes.get(k, "corrupt")] if k == self.iso else 3
                cell = (1 << 28) | (3 << 14) | (9 << 8) | 37 if k == self.iso else 37
                record = ((self.bad_row << 16) | 9, 3, cell, self.WANT ^ 0x100, self.WANT, cls, 1 if cls == 2 else 0,
                          4 if cls == 1 else (1 << 64) - 1, self._simd(4) if cls == 1 else 0, 1)
                self._blame(simd_map, wrong)
            if k == inject_row:
                row = self._simd(inject_wave)
                if inject_alias:
                    cls, age, writer, wrow = 1, 0, inject_wave + 1, self._simd(inject_wave + 1)
                elif inject_stale_word >= 0:
                    cls, age, writer, wrow = 2, 1, (1 << 64) - 1, 0
                else:
                    cls, age, writer, wrow = 3, 0, (1 << 64) - 1, 0
                word = max(inject_stale_word, 0)
                cell = (inject_round << 28) | (inject_wave << 14) | word if k == self.iso else 0
                got = self.WANT ^ 0x10 if cls == 3 else self.WANT ^ 0x5A5A5A5A
                record = ((row << 16) | 0, inject_wave, cell, got, self.WANT, cls, age, writer, wrow, 0)
                wrong += 1
                simd_map[3 * row + 1] += 1
            errors[k] = wrong
            if record:
                for j, v in enumerate(record):
                    first[10 * k + j] = v
        return 0


class FakeMatrixLib(_SimdFake):
    """``libmi355x_matrix.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every op clean on every SIMD.

    bad:      ``{(device, op index): wrong elements}``, all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the
              first of them lane 9, register 1, read as ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``matrix{device}`` in ``calls``: empty = never called."""

    OPS = 34
    WANT = 0x4A82C64E

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.2,
                 physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)

    def matrix_last_error(self) -> bytes:
        return self.err

    def matrix_device_count(self) -> int:
        return self._count()

    def matrix_slots(self) -> int:
        return self.SLOTS

    def matrix_test(self, device, blocks, iters, reps, ops, n_ops, seed, inject_op, inject_block, inject_skip_step,
                    errors, first_where, got, want, ms, simd_map, blocks_run):
        device = self._device(device, "matrix")
        if device is None:
            return -1
        chosen = [int(ops[i]) for i in range(n_ops)]
        if not 0 <= device < self.n or blocks < 0 or not 1 <= iters <= 1 << 20 or reps < 1 or not chosen \
                or len(set(chosen)) != len(chosen) or not all(0 <= k < self.OPS for k in chosen):
            self.err = (b"matrix test: need a valid device, blocks >= 0 (0: 2 per CU), iters 1..2^20, reps >= 1 and a "
                        b"list of distinct known ops")
            return -2
        grid = blocks or self.xcds * 32 * 2
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, (reps + 1) * len(chosen), 1000 * iters)
        for k in range(self.OPS):
            on = k in chosen
            wrong = self.bad.get((device, k), 0) if on else 0
            if on and k == inject_op:
                wrong += 1
            errors[k] = wrong
            first_where[k] = ((self.bad_row << 16) | (9 << 8) | 1) if wrong else (1 << 64) - 1
            want[k] = self.WANT if wrong else 0
            got[k] = self.WANT ^ 0x100 if wrong else 0
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def matrix_apply(self, device, op, a, b, c, idx, scale_a, scale_b, d):
        self.err = b"matrix apply: the stand-in has no wave to apply an instruction on"
        return -1


class FakeVmemLib(_SimdFake):
    """``libmi355x_vmem.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every part clean on every SIMD.

    bad:      ``{(device, op index): wrong words}``, all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2), the first
              of them lane 9, chain 1, read as ``want ^ 0x100``
    bad_l1:   ``{device: wrong reads}`` of word 33 of slice 3, on the same row's CU
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``vmem{device}`` (once per test: by the walks) in ``calls``: empty = never called."""

    OPS = 59
    LOADS = 36
    WANT = 0x4A82C64E
    FORMS = (b"global_load_lds_dword", b"global_load_lds_dwordx4", b"buffer_load_dword_lds", b"buffer_load_dwordx4_lds")

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, int], int]] = None,
                 bad_l1: Optional[Dict[int, int]] = None, bad_row: int = _SimdFake.BAD_ROW,
                 xcds: int = 8, ms: float = 0.2, physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)
        self.bad_l1 = dict(bad_l1 or {})

    def vmem_last_error(self) -> bytes:
        return self.err

    def vmem_device_count(self) -> int:
        return self._count()

    def vmem_slots(self) -> int:
        return self.SLOTS

    def vmem_ops(self) -> int:
        return self.OPS

    def vmem_loads(self) -> int:
        return self.LOADS

    def vmem_walk_reads(self, op, seed, iters, word) -> int:
        if not 0 <= op < self.LOADS or not 1 <= iters <= 1 << 16 or not 0 <= word < 16384:
            self.err = b"vmem walk_reads: need a load op, iters 1..2^16 and a word of the table"
            return -2
        return (op + word) & 1

    def _grid(self, blocks, blocks_run, simd_map, launches, ticks) -> int:
        grid = blocks or self.xcds * 32 * 2
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, launches, ticks)
        return grid

    def vmem_walks(self, device, blocks, iters, reps, ops, nops, seed, inject_op, inject_block, inject_skip_iter,
                   inject_table_word, errors, first, ms, simd_map, blocks_run):
        device = self._device(device, "vmem")
        if device is None:
            return -1
        chosen = [int(ops[i]) for i in range(nops)]
        if not 0 <= device < self.n or not 0 <= blocks <= 8192 or not 1 <= iters <= 1 << 16 or reps < 1 or not chosen \
                or len(set(chosen)) != len(chosen) or not all(0 <= k < self.OPS for k in chosen):
            self.err = (b"vmem walks: need a valid device, blocks 0..8192 (0: 2 per CU), iters 1..2^16, reps >= 1 and a "
                        b"list of distinct known ops")
            return -2
        self._grid(blocks, blocks_run, simd_map, (reps + 1) * len(chosen), 1000 * iters)
        for k in range(self.OPS):
            on = k in chosen
            wrong = self.bad.get((device, k), 0) if on else 0
            if on and k == inject_op:
                wrong += 1
            if on and k < self.LOADS and inject_table_word >= 0 and self.vmem_walk_reads(k, seed, iters, inject_table_word):
                wrong += 4 * (blocks or self.xcds * 64)
            errors[k] = wrong
            first[4 * k] = ((self.bad_row << 32) | (9 << 8) | 1) if wrong else (1 << 64) - 1
            first[4 * k + 1] = 0
            first[4 * k + 2] = self.WANT ^ 0x100 if wrong else 0
            first[4 * k + 3] = self.WANT if wrong else 0
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def vmem_bounds(self, device, blocks, n, seed, leak, errors, first, ms, simd_map, blocks_run):
        device = self._device(device)
        if device is None:
            return -1
        if not 0 <= device < self.n or not 0 <= blocks <= 8192 or not 1024 <= n <= 65536 or n & (n - 1):
            self.err = (b"vmem bounds: need a valid device, blocks 0..8192 (0: 2 per CU) and n a power of two from 1 KiB "
                        b"to 64 KiB")
            return -2
        grid = self._grid(blocks, blocks_run, simd_map, 16, 100 * n)
        for k in range(8):
            wrong = 4 * grid * (n // 32) * (4 if k & 1 else 1) if leak else 0  # the out-of-range half of every wave
            errors[k] = wrong
            first[4 * k] = (0 if k >= 4 else (self.bad_row << 32) | (1 << 8)) if wrong else (1 << 64) - 1
            first[4 * k + 1] = n if wrong else 0
            first[4 * k + 2] = self.WANT if wrong else 0
            first[4 * k + 3] = 0
            ms[k] = self.ms / 4
            if wrong and k < 4:
                self._blame(simd_map, wrong)
        return 0

    def vmem_l1(self, device, blocks, reps, slice_bytes, passes, seed, inject_block, inject_word, errors, first, ms_plain,
                ms_sc1, simd_map, blocks_run):
        device = self._device(device)
        if device is None:
            return -1
        if not 0 <= device < self.n or not 0 <= blocks <= 8192 or reps < 1 or not 1024 <= slice_bytes <= 1 << 20 \
                or slice_bytes & (slice_bytes - 1) or not 1 <= passes <= 65536:
            self.err = (b"vmem l1: need a valid device, blocks 0..8192 (0: 2 per CU), reps >= 1, slice_bytes a power of two "
                        b"from 1 KiB to 1 MiB and passes 1..65536")
            return -2
        grid = self._grid(blocks, blocks_run, simd_map, 2 * reps + 1, 100 * passes)
        if inject_block >= grid or (inject_block >= 0 and not 0 <= inject_word < slice_bytes // 4):
            self.err = b"vmem l1: at most 8192 workgroups, inject_block inside the grid and inject_word inside the slice"
            return -2
        wrong = self.bad_l1.get(device, 0) + (4 * passes if inject_block >= 0 else 0)
        _put(errors, ctypes.c_ulonglong, wrong)
        first[0] = (self.bad_row << 32) | (3 << 8) if wrong else (1 << 64) - 1
        first[1] = ((max(inject_block, 0) if inject_block >= 0 else 3) << 32) | (inject_word if inject_block >= 0 else 33) \
            if wrong else 0
        first[2] = self.WANT ^ 0x10 if wrong else 0
        first[3] = self.WANT if wrong else 0
        _put(ms_plain, ctypes.c_double, self.ms)
        _put(ms_sc1, ctypes.c_double, 2 * self.ms)
        if wrong:
            self._blame(simd_map, wrong)
        return 0

    def vmem_ldsdma_forms(self) -> int:
        return len(self.FORMS)

    def vmem_ldsdma_name(self, form) -> bytes:
        return self.FORMS[form] if 0 <= form < len(self.FORMS) else b""

    def vmem_ldsdma(self, device, blocks, iters, reps, seed, errors, first, ms, simd_map, blocks_run):
        device = self._device(device)
        if device is None:
            return -1
        if not 0 <= device < self.n or not 0 <= blocks <= 8192 or not 1 <= iters <= 1 << 16 or reps < 1:
            self.err = b"vmem ldsdma: need a valid device, blocks 0..8192 (0: 2 per CU), iters 1..2^16 and reps >= 1"
            return -2
        self._grid(blocks, blocks_run, simd_map, (reps + 1) * len(self.FORMS), 1000 * iters)
        for f in range(len(self.FORMS)):
            errors[f] = 0
            first[4 * f] = (1 << 64) - 1
            first[4 * f + 1] = first[4 * f + 2] = first[4 * f + 3] = 0
            ms[f] = self.ms
        return 0

    def vmem_apply(self, device, op, n, mem_words, nwords, offsets, regs, stride, num_records, out):
        self.err = b"vmem apply: the stand-in has no wave to apply an instruction on"
        return -1


_M32, _M64 = 0xffffffff, (1 << 64) - 1


def _s32(v: int) -> int:
    return v - (1 << 32) if v & 0x80000000 else v


def _s64(v: int) -> int:
    return v - (1 << 64) if v >> 63 else v


def _bfe(s0: int, s1: int, bits: int, signed: bool) -> int:
    off, w, full = s1 & (bits - 1), (s1 >> 16) & 0x7f, (1 << bits) - 1
    if w == 0:
        return 0
    val = ((_s64(s0) if bits == 64 else _s32(s0)) if signed else s0) >> off
    if off + w < bits:
        val &= (1 << w) - 1
        if signed and val >> (w - 1):
            val -= 1 << w
    return val & full


def _ffs(v: int) -> int:
    return (v & -v).bit_length() - 1 if v else _M32


def _lead(v: int, bits: int) -> int:
    return bits - v.bit_length() if v else _M32


def _spread(v: int, each) -> int:
    return sum(each(q) for q in range(16) if (v >> (4 * q)) & 0xf)


# the ops whose destination is a register pair
_SCALAR_WIDE = frozenset(
    [f"s_{k}_b64" for k in ("and", "or", "xor", "andn2", "orn2", "nand", "nor", "xnor", "not", "lshl", "lshr", "bfm", "brev",
                            "wqm", "quadmask", "cselect")]
    + ["s_ashr_i64", "s_bfe_u64", "s_bfe_i64", "s_bitreplicate_b64_b32"])


def scalar_model(op: str, a: int, b: int, scc: int) -> Tuple[int, int]:
    """csrc/scalar/scalar_ref.h's scalar_apply() in Python: ``(result, scc_out)`` of instruction ``op`` on S0 = a,
    S1 = b (64-bit; the 32-bit ops read the low halves) with SCC = ``scc`` before it."""
    a32, b32, ai, bi = a & _M32, b & _M32, _s32(a & _M32), _s32(b & _M32)
    ovf = lambda v: int(not -(1 << 31) <= v < (1 << 31))  # noqa: E731
    keep, nz = "keep", "nz"
    addk, mulk = 0x6b35, -0x2c4b
    table = {
        "s_add_u32": lambda: (a32 + b32, (a32 + b32) >> 32), "s_addc_u32": lambda: (a32 + b32 + scc, (a32 + b32 + scc) >> 32),
        "s_sub_u32": lambda: (a32 - b32, int(b32 > a32)), "s_subb_u32": lambda: (a32 - b32 - scc, int(b32 + scc > a32)),
        "s_add_i32": lambda: (ai + bi, ovf(ai + bi)), "s_sub_i32": lambda: (ai - bi, ovf(ai - bi)),
        "s_absdiff_i32": lambda: (abs(_s32((a32 - b32) & _M32)), nz),
        "s_lshl1_add_u32": lambda: ((a32 << 1) + b32, ((a32 << 1) + b32) >> 32 != 0),
        "s_lshl2_add_u32": lambda: ((a32 << 2) + b32, ((a32 << 2) + b32) >> 32 != 0),
        "s_lshl3_add_u32": lambda: ((a32 << 3) + b32, ((a32 << 3) + b32) >> 32 != 0),
        "s_lshl4_add_u32": lambda: ((a32 << 4) + b32, ((a32 << 4) + b32) >> 32 != 0),
        "s_addk_i32": lambda: (ai + addk, ovf(ai + addk)),
        "s_mul_i32": lambda: (a32 * b32, keep), "s_mul_hi_u32": lambda: ((a32 * b32) >> 32, keep),
        "s_mul_hi_i32": lambda: ((ai * bi) >> 32, keep), "s_mulk_i32": lambda: (ai * mulk, keep),
        "s_and": lambda x, y: x & y, "s_or": lambda x, y: x | y, "s_xor": lambda x, y: x ^ y,
        "s_andn2": lambda x, y: x & ~y, "s_orn2": lambda x, y: x | ~y, "s_nand": lambda x, y: ~(x & y),
        "s_nor": lambda x, y: ~(x | y), "s_xnor": lambda x, y: ~(x ^ y), "s_not": lambda x, y: ~x,
        "s_lshl_b32": lambda: (a32 << (b32 & 31), nz), "s_lshr_b32": lambda: (a32 >> (b32 & 31), nz),
        "s_ashr_i32": lambda: (ai >> (b32 & 31), nz), "s_lshl_b64": lambda: ((a << (b32 & 63)) & _M64, nz),
        "s_lshr_b64": lambda: (a >> (b32 & 63), nz), "s_ashr_i64": lambda: ((_s64(a) >> (b32 & 63)) & _M64, nz),
        "s_bfm_b32": lambda: (((1 << (a32 & 31)) - 1) << (b32 & 31), keep),
        "s_bfm_b64": lambda: ((((1 << (a32 & 63)) - 1) << (b32 & 63)) & _M64, keep),
        "s_bfe_u32": lambda: (_bfe(a32, b32, 32, False), nz), "s_bfe_i32": lambda: (_bfe(a32, b32, 32, True), nz),
        "s_bfe_u64": lambda: (_bfe(a, b32, 64, False), nz), "s_bfe_i64": lambda: (_bfe(a, b32, 64, True), nz),
        "s_bcnt0_i32_b32": lambda: (32 - bin(a32).count("1"), nz), "s_bcnt1_i32_b64": lambda: (bin(a).count("1"), nz),
        "s_ff0_i32_b32": lambda: (_ffs(~a32 & _M32), keep), "s_ff1_i32_b64": lambda: (_ffs(a), keep),
        "s_flbit_i32_b32": lambda: (_lead(a32, 32), keep),
        "s_flbit_i32": lambda: (_lead(~a32 & _M32 if ai < 0 else a32, 32), keep),
        "s_flbit_i32_i64": lambda: (_lead(~a & _M64 if a >> 63 else a, 64), keep),
        "s_brev_b32": lambda: (int(f"{a32:032b}"[::-1], 2), keep), "s_brev_b64": lambda: (int(f"{a:064b}"[::-1], 2), keep),
        "s_bitset0_b32": lambda: (b32 & ~(1 << (a32 & 31)), keep), "s_bitset1_b32": lambda: (b32 | (1 << (a32 & 31)), keep),
        "s_wqm_b64": lambda: (_spread(a, lambda q: 0xf << (4 * q)), nz),
        "s_quadmask_b64": lambda: (_spread(a, lambda q: 1 << q), nz),
        "s_bitreplicate_b64_b32": lambda: (sum(3 << (2 * i) for i in range(32) if (a32 >> i) & 1), keep),
        "s_min_i32": lambda: (a32 if ai < bi else b32, int(ai < bi)), "s_min_u32": lambda: (min(a32, b32), int(a32 < b32)),
        "s_max_i32": lambda: (a32 if ai > bi else b32, int(ai > bi)), "s_max_u32": lambda: (max(a32, b32), int(a32 > b32)),
        "s_cselect_b32": lambda: (a32 if scc else b32, keep), "s_cselect_b64": lambda: ((a if scc else b), keep),
        "s_cmov_b32": lambda: (a32 if scc else b32, keep),
        "s_sext_i32_i8": lambda: (_s32((a32 << 24) & _M32) >> 24, keep), "s_sext_i32_i16": lambda: (_s32((a32 << 16) & _M32) >> 16, keep),
        "s_abs_i32": lambda: (abs(ai), nz),
        "s_pack_ll_b32_b16": lambda: ((a32 & 0xffff) | (b32 << 16), keep),
        "s_pack_lh_b32_b16": lambda: ((a32 & 0xffff) | (b32 & 0xffff0000), keep),
        "s_pack_hh_b32_b16": lambda: ((a32 >> 16) | (b32 & 0xffff0000), keep),
        "s_cmp_eq_i32": lambda: (0, ai == bi), "s_cmp_lg_u32": lambda: (0, a32 != b32), "s_cmp_gt_i32": lambda: (0, ai > bi),
        "s_cmp_ge_u32": lambda: (0, a32 >= b32), "s_cmp_lt_u32": lambda: (0, a32 < b32), "s_cmp_lt_i32": lambda: (0, ai < bi),
        "s_cmp_le_i32": lambda: (0, ai <= bi), "s_cmp_eq_u64": lambda: (0, a == b),
        "s_bitcmp0_b32": lambda: (0, not (a32 >> (b32 & 31)) & 1), "s_bitcmp1_b32": lambda: (0, (a32 >> (b32 & 31)) & 1),
    }
    if op in table:
        r, rule = table[op]()
    else:  # the logic ops, in both widths
        stem = op.rpartition("_")[0]
        r, rule = (table[stem](a, b) if op in _SCALAR_WIDE else table[stem](a32, b32)), nz
    wide = op in _SCALAR_WIDE
    r &= _M64 if wide else _M32
    return r, (scc & 1 if rule == keep else int(r != 0) if rule == nz else int(bool(rule)))


class FakeScalarLib(_SimdFake):
    """``libmi355x_scalar.so`` for a node of ``n`` GPUs of ``xcds`` x 32 CUs: every part clean on every SIMD, and
    ``scalar_apply`` answered by :func:`scalar_model`.

    bad:      ``{(device, part, index): wrong words}`` with part "salu" (index: op), "sgpr" (index 0) or "smem"
              (index: kind), all on SIMD map row ``bad_row`` (xcd5/se1/cu7/simd2); the first of them is chain 1 /
              register s41 under the inverse pattern / table word 0x69, read as ``want ^ 0x100``
    physical: the node's ordinal of the one GPU a narrowed process sees as device 0 (``HIP_VISIBLE_DEVICES``)
    Calls are logged as ``salu{device}``, ``sgpr{device}``, ``smem{device}`` in ``calls``: empty = never called."""

    OPS = 83
    KINDS = 7
    SGPR_LO, SGPR_HI, SGPR_REGS = 20, 95, 75
    WANT = 0x5CA1A29E

    def __init__(self, n: int = 8, bad: Optional[Dict[Tuple[int, str, int], int]] = None,
                 bad_row: int = _SimdFake.BAD_ROW, xcds: int = 8, ms: float = 0.05,
                 physical: Optional[int] = None):
        super().__init__(n, bad, bad_row, xcds, ms, physical)

    def scalar_last_error(self) -> bytes:
        return self.err

    def scalar_device_count(self) -> int:
        return self._count()

    def scalar_slots(self) -> int:
        return self.SLOTS

    def scalar_sgpr_lo(self) -> int:
        return self.SGPR_LO

    def scalar_sgpr_hi(self) -> int:
        return self.SGPR_HI

    def scalar_sgpr_regs(self) -> int:
        return self.SGPR_REGS

    def scalar_salu(self, device, blocks, iters, reps, ops, nops, seed, inject_op, inject_block, inject_skip_iter,
                    errors, first_where, got, want, ms, simd_map, blocks_run):
        device = self._device(device, "salu")
        if device is None:
            return -1
        listed = [ops[i] for i in range(max(0, nops))]
        if not 0 <= device < self.n or blocks < 0 or not 1 <= iters <= 1 << 20 or reps < 1 or not listed \
                or any(not 0 <= k < self.OPS for k in listed):
            self.err = (b"scalar salu: need a valid device, blocks >= 0 (0: 4 per CU), iters 1..2^20, reps >= 1 and a "
                        b"list of known ops")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, (reps + 1) * len(listed), 1000 * iters)
        for k in range(self.OPS):
            on = k in listed
            wrong = self.bad.get((device, "salu", k), 0) if on else 0
            if on and k == inject_op:
                wrong += 1
            errors[k] = wrong
            first_where[k] = ((self.bad_row << 32) | 1) if wrong else (1 << 64) - 1
            want[k] = self.WANT if wrong else 0
            got[k] = self.WANT ^ 0x100 if wrong else 0
            ms[k] = self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def scalar_sgpr(self, device, blocks, reps, hold, seed, inject_block, inject_reg, errors, first_where, got, want,
                    ms, simd_map, blocks_run):
        device = self._device(device, "sgpr")
        if device is None:
            return -1
        if not 0 <= device < self.n or blocks < 0 or reps < 1 or not 0 <= hold <= 65536 or not -1 <= inject_reg <= 1:
            self.err = (b"scalar sgpr: need a valid device, blocks >= 0 (0: 7 per CU), reps >= 1, hold 0..65536 and "
                        b"inject_reg -1, 0 (lowest) or 1 (highest)")
            return -2
        grid = blocks or self.xcds * 32 * 7
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, reps + 1, 4000 * (hold + 1))
        wrong = self.bad.get((device, "sgpr", 0), 0) + (inject_reg >= 0)
        reg = (self.SGPR_LO, self.SGPR_HI)[inject_reg] if inject_reg >= 0 else 41
        _put(errors, ctypes.c_ulonglong, wrong)
        _put(first_where, ctypes.c_ulonglong, ((self.bad_row << 32) | ((0 if inject_reg >= 0 else 1) << 8) | reg)
             if wrong else (1 << 64) - 1)
        _put(want, ctypes.c_ulonglong, self.WANT if wrong else 0)
        _put(got, ctypes.c_ulonglong, self.WANT ^ (0x10 if inject_reg >= 0 else 0x100) if wrong else 0)
        _put(ms, ctypes.c_double, self.ms)
        if wrong:
            self._blame(simd_map, wrong)
        return 0

    def scalar_smem(self, device, blocks, reps, small_bytes, large_bytes, passes, loads, kind_mask, seed, inject_word,
                    errors, first_where, got, want, ms_hit, ms_miss, simd_map, blocks_run):
        device = self._device(device, "smem")
        if device is None:
            return -1
        sized = all(64 <= b <= 1 << 26 and b & (b - 1) == 0 for b in (small_bytes, large_bytes))
        if not 0 <= device < self.n or blocks < 0 or reps < 1 or not sized or not 1 <= passes <= 4096 \
                or not 1 <= loads <= 1 << 20 or not kind_mask or kind_mask >> self.KINDS or inject_word >= small_bytes // 4:
            self.err = (b"scalar smem: need a valid device, blocks >= 0 (0: 4 per CU), reps >= 1, table sizes that are "
                        b"powers of two from 64 B to 64 MiB, passes 1..4096, loads 1..2^20, a mask of known kinds and "
                        b"inject_word inside the small table")
            return -2
        grid = blocks or self.xcds * 32 * 4
        _put(blocks_run, ctypes.c_int, grid)
        self._fill_map(simd_map, grid, 2 * (reps + 1) * bin(kind_mask).count("1"), 200 * (passes + loads))
        for k in range(self.KINDS):
            on = bool((kind_mask >> k) & 1)
            wrong = self.bad.get((device, "smem", k), 0) if on else 0
            if on and inject_word >= 0:
                wrong += 4 * grid * passes  # every wave reads the word on every pass
            errors[k] = wrong
            first_where[k] = ((self.bad_row << 32) | (inject_word if inject_word >= 0 else 0x69)) if wrong else (1 << 64) - 1
            want[k] = self.WANT if wrong else 0
            got[k] = self.WANT ^ (0x10 if inject_word >= 0 else 0x100) if wrong else 0
            ms_hit[k] = self.ms if on else 0.0
            ms_miss[k] = 2 * self.ms if on else 0.0
            if wrong:
                self._blame(simd_map, wrong)
        return 0

    def scalar_apply(self, device, op, n, a, b, scc_in, result, scc_out):
        from ..ops.scalar import OPS
        if not 0 <= device < self.scalar_device_count() or not 0 <= op < self.OPS or not 1 <= n <= 1 << 20 \
                or any(scc_in[i] > 1 for i in range(n)):
            self.err = b"scalar apply: need a valid device, an op of the table, 1..2^20 rows and scc_in 0 or 1"
            return -2
        for i in range(n):
            result[i], scc_out[i] = scalar_model(OPS[op], int(a[i]), int(b[i]), int(scc_in[i]))
        return 0


class FakeFabricLib:
    """``libmi355x_fabric.so`` (in-process RCCL communicator over the node's GPUs)."""

    def __init__(self, busbw: float = 320.0, errors: int = 0, fail_open: bool = False, version: int = 22707,
                 hang_op: Optional[int] = None, async_error_op: Optional[int] = None, ignore_deadline: bool = False):
        self.busbw, self.errors, self.fail_open, self.version = busbw, errors, fail_open, version
        # ignore_deadline: the hang_op collective never returns, deadline or not (a wait stuck in the driver)
        self.ignore_deadline = ignore_deadline
        # hang_op: that collective never completes -- the call waits out its deadline (or forever without
        # one, until `release` is set) and then "aborts" the communicators like fabric.hip's abort_all
        self.hang_op = hang_op
        # async_error_op: a communicator reports an async error during that collective (a link dropping
        # traffic): fabric.hip's wait_comms / sync_all abort every communicator and return ABORTED
        self.async_error_op = async_error_op
        self.release = threading.Event()
        self.opened: List[List[int]] = []
        self.timeouts_ms: List[float] = []
        self.aborts = 0
        self.closed = 0
        self.err = b"ncclCommInitAll: unhandled system error"

    def fabric_open(self, arr, n, timeout_ms=0.0):
        if self.fail_open:
            return None
        self.opened.append([arr[i] for i in range(n)])
        return 1

    def fabric_run(self, ctx, op, nbytes, iters, warmup, out, timeout_ms=0.0):
        self.timeouts_ms.append(timeout_ms)
        if op == self.hang_op:
            self.release.wait(timeout_ms / 1e3 if timeout_ms > 0 and not self.ignore_deadline else None)
            if not self.release.is_set():
                self.aborts += 1  # ncclCommAbort on every communicator
                self.err = (f"timed collectives: not complete within {timeout_ms:.0f} ms: communicators aborted "
                            "(ncclCommAbort)").encode()
                return -4
        if op == self.async_error_op:
            self.aborts += 1
            self.err = b"collective wait: remote process exited or there was a network error (communicators aborted)"
            return -4
        out[0], out[1], out[2], out[3] = 1.0, self.busbw * 0.57, self.busbw, float(self.errors if op == 3 else 0)
        return 0

    def fabric_aborted(self, ctx):
        return 1 if self.aborts else 0

    def fabric_close(self, ctx):
        self.closed += 1

    def fabric_last_error(self):
        return self.err

    def fabric_rccl_version(self):
        return self.version


class NarrowedDiagLib:
    """A :class:`FakeDiagLib` as a process sees it with ``HIP_VISIBLE_DEVICES=k``: one device, ordinal 0 = GPU k
    (what a per-device diagnostic child of the agent sees, agent/isolation.narrow_to)."""

    # the calls whose first argument is a device ordinal (diag_p2p_* take ``src`` and the node's own ordinals)
    _PER_DEVICE = frozenset(name for name, fn in vars(FakeDiagLib).items() if name.startswith("diag_")
                            and list(inspect.signature(fn).parameters)[1:2] == ["device"])

    def __init__(self, lib: FakeDiagLib, physical: int):
        self.lib, self.physical = lib, physical

    def diag_device_count(self) -> int:
        return 1

    def __getattr__(self, name: str):
        fn = getattr(self.lib, name)
        if name not in self._PER_DEVICE:
            return fn

        def on_physical(device, *a):
            if device != 0:
                self.lib.err = b"hipSetDevice: invalid device ordinal"
                return -1
            return fn(self.physical, *a)
        return on_physical


def install(n: int = 1, fabric: Optional[Dict] = None, xgmi: Optional[Dict] = None, atomics: Optional[Dict] = None,
            lanes: Optional[Dict] = None, scalar: Optional[Dict] = None, matrix: Optional[Dict] = None,
            vmem: Optional[Dict] = None, cvt: Optional[Dict] = None, hbmscan: Optional[Dict] = None, ifetch: Optional[Dict] = None,
            handoff: Optional[Dict] = None, scratch: Optional[Dict] = None, **diag_kw) -> None:
    """Make this process's ``ops.diag``, ``ops.fabric`` and ``ops.xgmi`` use the fakes ``FakeDiagLib(n, **diag_kw)``,
    ``FakeFabricLib(**fabric)`` and ``FakeXgmiLib(n, **xgmi)``, and the module ``ops.X`` of every opt-in diagnostic X
    of ``ops/optin.OPT_IN`` its ``FakeXLib(n, **X)``.  The node agent's diagnostic children run it first when the agent
    is given ``diag_setup=("k8s_gpu_node_checker_amd.testing.fake_native", "install", {...})`` (agent/isolation.py),
    so the child code path runs unchanged on CPU with scripted GPUs; a child narrowed to one GPU
    (``HIP_VISIBLE_DEVICES``) sees only that one, as under HIP."""
    import importlib
    import os
    from ..ops import diag
    from ..ops import fabric as fabric_mod
    from ..ops.optin import OPT_IN
    lib: object = FakeDiagLib(n=n, **diag_kw)
    vis = os.environ.get("HIP_VISIBLE_DEVICES", "").strip()
    if vis.isdigit() and int(vis) < n:
        lib = NarrowedDiagLib(lib, int(vis))  # type: ignore[arg-type]
    diag.lib = lambda: lib
    fabric_mod._lib = FakeFabricLib(**(fabric or {}))
    from ..ops import xgmi as xgmi_mod
    xlib = FakeXgmiLib(n=n, **(xgmi or {}))
    xgmi_mod.lib = lambda: xlib
    physical = int(vis) if vis.isdigit() and int(vis) < n else None
    given = {"atomics": atomics, "lanes": lanes, "scalar": scalar, "matrix": matrix, "vmem": vmem, "cvt": cvt,
             "hbmscan": hbmscan, "ifetch": ifetch, "handoff": handoff, "scratch": scratch}
    for name in OPT_IN:
        fake = globals()[f"Fake{name.capitalize()}Lib"](n=n, physical=physical, **(given[name] or {}))
        importlib.import_module(f"..ops.{name}", __package__).lib = lambda fake=fake: fake
