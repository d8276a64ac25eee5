#!/usr/bin/env python3
"""Time the hybrid-QAM kernels (csrc/hybrid.hip) on 2 rows of 2^20 symbols of (16, 4) hybrid QAM at fr = 0.25 (frames of 3 + 1) and of (64, 16) at
fr = 0.3 (frames of 7 + 3), in both precisions, median of warm runs between HIP events:

    assemble     tdh_assemble_dev with the labels (one launch)
    class sums   tdh_class_sums_dev (two launches)
    align        tdh_align_dev (one small launch)
    split        tdh_split_dev with the device shift (one launch)
    metrics      tdh_metrics_dev (two launches), the sums left on the device
    point        one SNR point of a resident sweep: impair_pointwise_dev -> class sums -> align -> metrics, and the eight sums per row read
                 back: a host clock around the whole

against a device copy of the bytes each stage has to move (qh_memcpy_d2d, timed in the same run: the traffic floor).

    python3 scripts/bench_hybrid.py [--reps 20] [--out-dir profiles]

Writes <out-dir>/hybrid_bench.json and <out-dir>/hybrid_timings.md and prints the JSON line.
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

    from qampy_amd import _lib, synth
    from qampy_amd._lib import DeviceArray
    from qampy_amd.core import hip_dsp

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
    nm, N, snr_db = 2, 2 ** 20, 14.
    formats = (((16, 4), 0.25), ((64, 16), 0.3))
    res = {"device": _lib.device_name(), "reps": a.reps, "nmodes": nm, "N": N, "snr_db": snr_db, "formats": [list(f[0]) + [f[1]] for f in formats]}
    stages = ("assemble", "class sums", "align", "split", "metrics")
    for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
        cb = np.dtype(dtype).itemsize
        for M, fr in formats:
            d = synth.make_tdh_symbols_dev(M, N, fr, nmodes=nm, dtype=dtype)
            E, fM, fM1, pr = d["symbols"], d["f_M"], d["f_M1"], d["powratio"]
            L = E.shape[1]
            rx, out, idx = DeviceArray(E.shape, dtype), DeviceArray(E.shape, dtype), DeviceArray(E.shape, np.int32)
            p1, p2 = DeviceArray(d["part1"].shape, dtype), DeviceArray(d["part2"].shape, dtype)
            csum, shift, sums = DeviceArray((nm, fM), np.float64), DeviceArray((nm,), np.int32), DeviceArray((nm, 8), np.float64)
            hip_dsp.impair_pointwise_dev(E, rx, snr=(snr_db, 1), seed=1)
            hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(rx, fM, csum), fM1, M, shift)
            field, labels = nm * L * cb, nm * L * 4
            fill_src, fill_dst = DeviceArray((2 * field,), np.uint8), DeviceArray((2 * field,), np.uint8)

            def copy_ms(moved):
                return median_ms(lambda: _lib.call("qh_memcpy_d2d", fill_dst.ptr, fill_src.ptr, moved // 2))          # moved: half read, half written

            runs = {"assemble": (lambda: hip_dsp.tdh_assemble_dev(d["part1"], d["part2"], fM, fM1, pr, out, d["idx_tx1"], d["idx_tx2"], idx), 2 * (field + labels)),
                    "class sums": (lambda: hip_dsp.tdh_class_sums_dev(rx, fM, csum), field),
                    "align": (lambda: hip_dsp.tdh_align_dev(csum, fM1, M, shift), 0),
                    "split": (lambda: hip_dsp.tdh_split_dev(rx, fM, fM1, pr, p1, p2, shift), 2 * field),
                    "metrics": (lambda: hip_dsp.tdh_metrics_dev(rx, d["idx_tx"], fM, fM1, pr, d["alphabet1"], d["alphabet2"], shift, sums), field + labels)}
            r = {}
            for st in stages:
                fn, moved = runs[st]
                ms = median_ms(fn)
                r[st] = {"ms": ms, "bytes_moved": moved}
                if moved:
                    floor = copy_ms(moved)
                    r[st].update(copy_ms=floor, over_copy=ms / floor, GBps=moved / ms / 1e6)
            # (sample, point) pairs per second of the decision search, 7 vector operations each
            r["metrics"]["Gdist_per_s"] = nm * (L // fM) * (fM1 * M[0] + (fM - fM1) * M[1]) / r["metrics"]["ms"] / 1e6

            def point():
                hip_dsp.impair_pointwise_dev(E, rx, snr=(snr_db, 1), seed=1)
                hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(rx, fM, csum), fM1, M, shift)
                return hip_dsp.tdh_rates(hip_dsp.tdh_metrics_dev(rx, d["idx_tx"], fM, fM1, pr, d["alphabet1"], d["alphabet2"], shift, sums).to_host(), M)
            r["point_ms"] = host_ms(point, a.reps)
            r["point_ber"] = [float(v) for v in point()["ber"][1]]
            res.setdefault(name, {})["%d-%d" % M] = r
    with open(os.path.join(a.out_dir, "hybrid_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Time-domain hybrid QAM: timings", "",
             "%s, %d rows of 2^20 symbols at %g dB, median of %d warm runs between HIP events (scripts/bench_hybrid.py)." % (res["device"], nm, snr_db, a.reps),
             "The copy is `qh_memcpy_d2d` moving as many bytes (read plus written) as the stage has to, timed in the same run: the traffic floor.",
             "The alignment reads f_M sums per row: a launch's latency, nothing to copy.  Gdist/s counts the (sample, point) pairs of the decision search,",
             "7 vector operations each.", "",
             "| precision | format | stage | ms | bytes moved | copy ms | multiple of the copy | GB/s | Gdist/s |", "|---|---|---|---|---|---|---|---|---|"]
    for name in ("complex64", "complex128"):
        for key, r in res[name].items():
            for st in stages:
                s = r[st]
                lines.append("| %s | %s | %s | %.4f | %d | %s | %s | %s | %s |" % (
                    name, key, st, s["ms"], s["bytes_moved"], "%.4f" % s["copy_ms"] if "copy_ms" in s else "", "%.2f" % s["over_copy"] if "copy_ms" in s else "",
                    "%.0f" % s["GBps"] if "GBps" in s else "", "%.0f" % s["Gdist_per_s"] if "Gdist_per_s" in s else ""))
    lines.append("")
    for name in ("complex64", "complex128"):
        for key, r in res[name].items():
            lines.append("%s, %s: one SNR point of a resident sweep (impairment, class sums, alignment, metrics, %d sums back), a host clock around the whole: "
                         "%.3f ms; combined BER per row %s." % (name, key, 8 * nm, r["point_ms"], ", ".join("%.4g" % v for v in r["point_ber"])))
    with open(os.path.join(a.out_dir, "hybrid_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
