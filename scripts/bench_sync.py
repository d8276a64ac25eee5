#!/usr/bin/env python3
"""Time the alignment of an unsynchronised capture at the benchmark's shape (2 rows of 2^22 symbols, complex64, 64-QAM): the transmitted
pattern rolled by tens of thousands of symbols, turned a quarter turn and its modes swapped, so that only a full correlation finds it.

  device   ``cal_metrics_dev(sync="full")`` on rows resident in HBM: wall-clock per call (it ends with the read-back of its scalars), median
           and spread of warm runs; and its parts between HIP events: the full correlation of both rows with one mode, the peak search, the
           gather of one label row.
  host     what the same result took before: the rows copied back and ``SignalQAM.cal_ser`` (one alignment; every further metric method
           aligns again) on the host's threads.

The symbol-error counts of the two are compared.  Prints one JSON line.

    python3 scripts/bench_sync.py [--log2-len 22] [--reps 7] [--host-reps 3] [--shift 70001]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qampy_amd import _lib, theory                                     # noqa: E402
from qampy_amd._lib import DeviceArray                                 # noqa: E402
from qampy_amd.core import ber_functions, hip_dsp                      # noqa: E402
from qampy_amd.signals import SignalQAM                                # noqa: E402


def spread(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "runs": int(ts.size)}


def wall_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        _lib.sync()
        t0 = time.perf_counter()
        fn()
        _lib.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return spread(ts)


def event_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    _lib.sync()
    ts = []
    for _ in range(reps):
        a, b = _lib.Event(), _lib.Event()
        a.record()
        fn()
        b.record()
        _lib.sync()
        ts.append(b.elapsed_ms(a))
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-len", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shift", type=int, default=70001)
    ap.add_argument("--M", type=int, default=64)
    a = ap.parse_args()
    N, M, ct = 2 ** a.log2_len, a.M, np.complex64
    _lib.init(0)
    rng = np.random.default_rng(1)
    coded = np.asarray(theory.coded_symbols_qam(M))
    labels = rng.integers(0, M, (2, N)).astype(np.int32)
    rows = coded[labels]
    rows = (rows + 0.03 * (rng.standard_normal(rows.shape) + 1j * rng.standard_normal(rows.shape))).astype(ct)
    # the pattern the metrics are handed: the other mode first, turned a quarter turn, rolled
    pattern_labels = np.ascontiguousarray(np.roll(labels[::-1], a.shift, axis=-1))
    turned = np.array([int(np.argmin(np.abs(coded - c * 1j))) for c in coded], dtype=np.int32)          # label of 1j * point
    pattern_labels = turned[pattern_labels]
    pattern = coded[pattern_labels].astype(ct)
    d_rows, d_idx, d_al = DeviceArray.from_host(rows), DeviceArray.from_host(pattern_labels), DeviceArray.from_host(coded.astype(ct))
    res = {"device": _lib.device_name(), "shape": [2, N], "dtype": "complex64", "M": M, "shift": a.shift}

    got = ber_functions.cal_metrics_dev(d_rows, d_idx, d_al, sync="full")
    res["device_alignment"] = [{k: m[k] for k in ("tx_mode", "rotation", "lag", "errors", "compared")} for m in got]
    ws = {}                                                             # the buffers a ResidentReceiver keeps between calls
    res["metrics_full_sync"] = wall_ms(lambda: ber_functions.cal_metrics_dev(d_rows, d_idx, d_al, sync="full", sync_ws=ws), a.reps)
    res["ser_full_sync"] = wall_ms(lambda: ber_functions.cal_ser_dev(d_rows, d_idx, d_al, sync="full", sync_ws=ws), a.reps)
    res["metrics_full_sync_fresh_buffers"] = wall_ms(lambda: ber_functions.cal_metrics_dev(d_rows, d_idx, d_al, sync="full"), a.reps)
    del ws
    window = ber_functions.cal_metrics_dev(d_rows, d_idx, d_al)
    res["window_matches"] = [[m["errors"], m["compared"]] for m in window]

    n = 2 * N - 1
    sym = hip_dsp.labels_to_symbols_dev(d_idx, d_al, DeviceArray((2, N), ct))
    cc, pk, lab = DeviceArray((2, n), ct), DeviceArray((2, 6), np.float64), DeviceArray((N,), np.int32)
    res["xcorr_two_rows"] = event_ms(lambda: hip_dsp.xcorr_dev(d_rows, sym.row(0), cc), a.reps)
    res["peak_two_rows"] = event_ms(lambda: hip_dsp.xcorr_peak_dev(cc, n, pk), a.reps)
    res["gather_labels"] = event_ms(lambda: hip_dsp.cyclic_gather_dev(d_idx.row(0), a.shift, 0, lab), a.reps)
    res["labels_to_symbols"] = event_ms(lambda: hip_dsp.labels_to_symbols_dev(d_idx, d_al, sym), a.reps)

    def host():
        back = d_rows.to_host()
        return SignalQAM(back, M, symbols=pattern, coded_symbols=coded.astype(ct)).cal_ser(verbose=True)
    ts = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ser, errs, _ = host()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["host_cal_ser"] = spread(ts)
    res["host_threads"] = len(os.sched_getaffinity(0))
    host_errors = [int(np.count_nonzero(e)) for e in errs]
    res["host_errors"] = host_errors
    res["errors_agree"] = host_errors == [m["errors"] for m in got]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
