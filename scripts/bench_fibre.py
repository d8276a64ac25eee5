#!/usr/bin/env python3
"""Time the nonlinear fibre (csrc/fibre.hip) on 2 rows of 2^20 and of 2^23 samples in both precisions, median of warm runs between HIP events:

    nonlinear    one launch of the point-wise step (fibre_nl_dev), without and with the amplifier's noise
    filter       one spectral filter with a complex table (spectral_filter_dev, kind 6): a transform pair
    table        one dispersion table (the difference of two calls that differ by one table, see below)
    step         one whole step of a propagation, filter plus nonlinear launch: (a span of 24 equal steps - a span of 8) / 16
    span         ssfm_dev over one span of 8 equal steps as a user calls it: 9 filters, 8 nonlinear launches, 2 tables, 2 power launches

A single launch is timed as `inner` launches back to back between one pair of events, divided by `inner`: at these sizes a launch lasts
microseconds and a lone one would be timed with its own start-up.  Beside each, a device copy of the bytes the stage has to move
(qh_memcpy_d2d, timed the same way in the same run: the traffic floor).

    python3 scripts/bench_fibre.py [--reps 15] [--inner 10] [--out-dir profiles]

Writes <out-dir>/fibre_bench.json and <out-dir>/fibre_timings.md and prints the JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)

    from qampy_amd import _lib
    from qampy_amd._lib import DeviceArray
    from qampy_amd.core import hip_dsp

    def median_ms(fn, inner=1):
        fn()
        _lib.sync()
        ts = []
        for _ in range(a.reps):
            s, e = _lib.Event(), _lib.Event()
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            _lib.sync()
            ts.append(e.elapsed_ms(s) / inner)
        return float(np.median(ts))

    _lib.init(0)
    nm, fs, D, span = 2, 64e9, 17e-6, 80e3
    res = {"device": _lib.device_name(), "reps": a.reps, "inner": a.inner, "nmodes": nm, "fs": fs, "D": D, "span": span, "sizes": {}}
    rng = np.random.default_rng(1)
    for lg in (20, 23):
        L = 2 ** lg
        for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
            rt = np.float32 if dtype == np.complex64 else np.float64
            x = np.empty((nm, L), dtype)
            x.real = rng.standard_normal((nm, L), dtype=rt) * np.sqrt(0.5)
            x.imag = rng.standard_normal((nm, L), dtype=rt) * np.sqrt(0.5)
            E, out = DeviceArray.from_host(x), DeviceArray((nm, L), dtype)
            ps = DeviceArray.from_host(np.array([1e-3], dtype=np.float64))
            H = DeviceArray.from_host(np.exp(2j * np.pi * rng.random(L)).astype(dtype))
            field = nm * L * np.dtype(dtype).itemsize
            src, dst = DeviceArray((field,), np.uint8), DeviceArray((field,), np.uint8)

            def copy_ms(moved):
                """moved: half read, half written; as copies of one field at most, like the passes of the stage"""
                one_way = moved // 2
                chunks = [field] * (one_way // field) + ([one_way % field] if one_way % field else [])

                def fn():
                    for c in chunks:
                        _lib.call("qh_memcpy_d2d", dst.ptr, src.ptr, c)
                return median_ms(fn, a.inner if len(chunks) == 1 else 1)

            link = dict(gamma=1.3e-3, alpha_db_km=0.2, power_dbm=3.0)
            r = {}
            r["nonlinear"] = {"ms": median_ms(lambda: hip_dsp.fibre_nl_dev(E, out, 0.9, 2.6e-3, ps), a.inner), "bytes_moved": 2 * field}
            r["nonlinear, in place"] = {"ms": median_ms(lambda: hip_dsp.fibre_nl_dev(out, out, 1.0, 2.6e-3, ps), a.inner), "bytes_moved": 2 * field}
            r["nonlinear with noise"] = {"ms": median_ms(lambda: hip_dsp.fibre_nl_dev(E, out, 0.9, 2.6e-3, ps, sigma_w=1e-5, seed=3), a.inner), "bytes_moved": 2 * field}
            # a pair of four-step transforms: each reads the field and writes its work buffer, reads that and writes the field - 8 passes, as
            # DESIGN.md 3.14 counts them (the table is an eighth of a pass)
            r["filter"] = {"ms": median_ms(lambda: hip_dsp.spectral_filter_dev(E, out, H), a.inner), "bytes_moved": 8 * field}
            t8 = median_ms(lambda: hip_dsp.ssfm_dev(E, out, fs, D, span, steps=8, **link))
            t24 = median_ms(lambda: hip_dsp.ssfm_dev(E, out, fs, D, span, steps=24, **link))
            t3 = median_ms(lambda: hip_dsp.ssfm_dev(E, out, fs, D, span, steps=[20e3, 20e3, 40e3], **link))        # 10, 20, 30, 20 km: three tables
            t3e = median_ms(lambda: hip_dsp.ssfm_dev(E, out, fs, D, span, steps=[20e3, 40e3, 20e3], **link))       # 10, 30, 30, 10 km: two tables
            r["table"] = {"ms": t3 - t3e, "bytes_moved": field // nm}
            r["step"] = {"ms": (t24 - t8) / 16, "bytes_moved": 10 * field}
            r["span of 8 steps"] = {"ms": t8, "bytes_moved": (9 * 8 + 8 * 2) * field}
            for k, v in r.items():
                v["copy_ms"] = copy_ms(v["bytes_moved"])
                v["over_copy"] = v["ms"] / v["copy_ms"]
                v["GBps"] = v["bytes_moved"] / v["ms"] / 1e6
            r["samples_per_s_step"] = nm * L / (r["step"]["ms"] * 1e-3)
            res["sizes"].setdefault("2x2^%d" % lg, {})[name] = r
    with open(os.path.join(a.out_dir, "fibre_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Nonlinear fibre: timings", "",
             "%s, %d rows, median of %d warm runs between HIP events; a single launch is timed as %d launches back to back, divided by %d"
             % (res["device"], nm, a.reps, a.inner, a.inner),
             "(scripts/bench_fibre.py).  The copy is `qh_memcpy_d2d` moving as many bytes (read plus written) as the stage has to, timed the same way in the",
             "same run: the traffic floor.  Bytes counted: the nonlinear launch reads and writes the field once (2 passes); a filter is a pair of",
             "four-step transforms, each reading the field, writing and reading its work buffer and writing the field (8 passes, as DESIGN.md 3.14",
             "counts them); a step is one of each; a table is L values written.  `step` is (a span of 24 equal steps - a span of 8) / 16,",
             "`table` the difference of two three-step spans that form three and two tables.", "",
             "| size | precision | stage | ms | bytes moved | copy ms | multiple of the copy | GB/s |", "|---|---|---|---|---|---|---|---|"]
    for size, per in res["sizes"].items():
        for name, r in per.items():
            for st, s in r.items():
                if isinstance(s, dict):
                    lines.append("| %s | %s | %s | %.4f | %d | %.4f | %.2f | %.0f |" % (size, name, st, s["ms"], s["bytes_moved"], s["copy_ms"], s["over_copy"], s["GBps"]))
    lines.append("")
    for size, per in res["sizes"].items():
        for name, r in per.items():
            lines.append("%s, %s: a whole step propagates %.3g samples per second." % (size, name, r["samples_per_s_step"]))
    with open(os.path.join(a.out_dir, "fibre_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
