#!/usr/bin/env python3
"""Time the blind signal-quality kernels (csrc/blind.hip) on rows of the size benchmark config 3 leaves resident - 2 modes of 2^22 recovered
64-QAM symbols (here: the unit-power alphabet plus white noise at 22 dB) - in both precisions:

    moments      blind_stats_dev: the sums, their combination and the estimator (three launches); median of warm runs between HIP events
    trace        the same per block of 4096 symbols
    scale        norm_to_s0_dev out of place, the stats at hand (one launch)
    evm M        blind_evm_dev's two launches for M = 4 .. 1024 on the same rows (the rows are 64-QAM: only the work per sample matters), the
                 sums left on the device
    qpsk         qpsk_blind_snr_dev (two launches)
    metrics      pipeline._blind_metrics, what ResidentReceiver.blind_metrics runs after the pending post-processing, with block = 4096: a host
                 clock around the call, which ends with its few scalars and the traces on the host

against a device copy of the bytes each has to move (qh_memcpy_d2d, timed in the same run: the traffic floor) and against the host path on the
same rows: the rows brought to the host (DeviceArray.to_host into pinned memory) and cal_snr_qam + cal_s0 with method="pyt" (numpy; the blind EVM
of 2^23 samples against 64 points is left out of the host figure: it alone takes seconds).

    python3 scripts/bench_blind.py [--reps 20] [--out-dir profiles]

Writes <out-dir>/blind_bench.json and <out-dir>/blind_timings.md and prints the JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)

    from qampy_amd import _lib, pipeline, theory
    from qampy_amd._lib import DeviceArray
    from qampy_amd.core import hip_dsp, signal_quality

    def median_ms(fn):
        fn()
        _lib.sync()
        ts = []
        for _ in range(a.reps):
            s, e = _lib.Event(), _lib.Event()
            s.record()
            fn()
            e.record()
            _lib.sync()
            ts.append(e.elapsed_ms(s))
        return float(np.median(ts))

    def host_ms(fn, n):
        ts = []
        for _ in range(n + 1):
            _lib.sync()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:]))

    _lib.init(0)
    M, nm, N, snr_db, block = 64, 2, 2 ** 22, 22., 4096
    orders = (4, 16, 64, 256, 1024)
    rng = np.random.default_rng(3)
    al = theory.cal_symbols_qam(M).ravel() / np.sqrt(theory.cal_scaling_factor_qam(M))
    rows = al[rng.integers(0, M, (nm, N))] + (rng.standard_normal((nm, N)) + 1j * rng.standard_normal((nm, N))) * np.sqrt(0.5 * 10 ** (-snr_db / 10))
    res = {"device": _lib.device_name(), "reps": a.reps, "M": M, "nmodes": nm, "N": N, "snr_db": snr_db, "block": block}
    for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
        cb = np.dtype(dtype).itemsize
        E = DeviceArray.from_host(rows.astype(dtype))
        out = DeviceArray(E.shape, dtype)
        nbytes = nm * N * cb
        mom, stats, evm_sum, qp = (DeviceArray((nm, k), np.float64) for k in (4, 6, 1, 3))
        tmom, tstats = DeviceArray((nm, N // block, 4), np.float64), DeviceArray((nm, N // block, 6), np.float64)
        fill_src, fill_dst = DeviceArray((nbytes,), np.uint8), DeviceArray((nbytes,), np.uint8)

        def copy_ms(moved):
            return median_ms(lambda: _lib.call("qh_memcpy_d2d", fill_dst.ptr, fill_src.ptr, moved // 2))          # moved: half read, half written

        def evm_launches(order):
            _lib.call("qh_blind_evm_%s_dev" % ("c64" if cb == 8 else "c128"), E.ptr, nm, N, stats.ptr, hip_dsp.blind._blind_alphabet_dev(order, dtype).ptr, order,
                      None, None, evm_sum.ptr)

        hip_dsp.blind_stats_dev(E, M, stats=stats, mom=mom)
        stages = [("moments", lambda: hip_dsp.blind_stats_dev(E, M, stats=stats, mom=mom), nbytes),
                  ("trace", lambda: hip_dsp.blind_stats_dev(E, M, block=block, stats=tstats, mom=tmom), nbytes),
                  ("scale", lambda: hip_dsp.norm_to_s0_dev(E, M, out, stats=stats), 2 * nbytes),
                  ("qpsk", lambda: hip_dsp.qpsk_blind_snr_dev(E, out=qp), nbytes)]
        stages += [("evm %d" % o, (lambda o=o: evm_launches(o)), nbytes) for o in orders]
        r = {}
        for st, fn, moved in stages:
            ms, floor = median_ms(fn), copy_ms(moved)
            r[st] = {"ms": ms, "bytes_moved": moved, "copy_ms": floor, "over_copy": ms / floor, "GBps": moved / ms / 1e6}
        for o in orders:                                                   # distance evaluations (5 vector operations each) per second
            r["evm %d" % o]["Gdist_per_s"] = nm * N * o / r["evm %d" % o]["ms"] / 1e6
        ws = {}
        r["metrics_ms"] = host_ms(lambda: pipeline._blind_metrics(E, M, block, ws), a.reps)
        r["metrics_no_trace_ms"] = host_ms(lambda: pipeline._blind_metrics(E, M, None, ws), a.reps)

        def host_path():
            h = E.to_host(pinned=True)
            signal_quality.cal_snr_qam(h, M)
            signal_quality.cal_s0(h, M)
        r["fetch_ms"] = host_ms(lambda: E.to_host(pinned=True), max(3, a.reps // 4))
        r["host_path_ms"] = host_ms(host_path, max(3, a.reps // 4))
        res[name] = r
    with open(os.path.join(a.out_dir, "blind_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Blind signal quality: timings", "",
             "%s, %d rows of 2^22 64-QAM symbols at %g dB, median of %d warm runs between HIP events (scripts/bench_blind.py)." % (res["device"], nm, snr_db, a.reps),
             "The copy is `qh_memcpy_d2d` moving as many bytes (read plus written) as the stage has to, timed in the same run: the traffic floor.",
             "`evm M`: the distance search against M points on the same rows; Gdist/s counts (sample, point) pairs, 5 vector operations each.", "",
             "| precision | stage | ms | bytes moved | copy ms | multiple of the copy | GB/s | Gdist/s |", "|---|---|---|---|---|---|---|---|"]
    for name in ("complex64", "complex128"):
        for st in ["moments", "trace", "scale", "qpsk"] + ["evm %d" % o for o in orders]:
            r = res[name][st]
            lines.append("| %s | %s | %.4f | %d | %.4f | %.2f | %.0f | %s |" % (name, st, r["ms"], r["bytes_moved"], r["copy_ms"], r["over_copy"], r["GBps"],
                                                                             "%.0f" % r["Gdist_per_s"] if "Gdist_per_s" in r else ""))
    lines.append("")
    for name in ("complex64", "complex128"):
        r = res[name]
        lines.append("%s, a host clock around the call: blind_metrics %.3f ms with the traces of %d-symbol blocks, %.3f ms without (snr, s0 and the blind EVM at "
                     "M = 64, scalars back); the host path %.2f ms, of which %.2f ms bring the rows to pinned host memory and the rest is numpy's cal_snr_qam "
                     "+ cal_s0 (no EVM)." % (name, r["metrics_ms"], block, r["metrics_no_trace_ms"], r["host_path_ms"], r["fetch_ms"]))
    with open(os.path.join(a.out_dir, "blind_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
