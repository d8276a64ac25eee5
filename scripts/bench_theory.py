#!/usr/bin/env python3
"""Time the theory kernels: a 31-point Monte-Carlo GMI + MI curve (0 .. 30 dB, ns = 1000 draws per point) for M = 16, 64, 256 and 1024 in both
precisions - the noise launch and the three launches of hip_dsp.awgn_mc_dev on resident buffers, median of warm runs between HIP events - and the
shaped source at 2 modes of 2^22 symbols.

Beside each curve: the exponential count 31 M^2 ns, the rate achieved and its fraction of the chip's transcendental issue rate (one v_exp_f32 of a
64-lane wave issues in 8 cycles per SIMD: 8 lanes per cycle, 4 SIMDs, 256 CUs, 2.4 GHz = 1.97e13 per second; complex128 has no such instruction,
its exp2 is a polynomial in double, so the fraction is given for orientation only), and the same curve by the vectorised float64 numpy of
tests/theory_ref.py on the host: one SNR point is timed at a draw count that keeps M^2 ns near 2^22 and scaled to 31 points of 1000 draws (the
cost is linear in both; the pure-Python reference is far slower still).  The shaped source is held against a device copy of the bytes it writes.

    python3 scripts/bench_theory.py [--reps 10] [--out-dir profiles]

Writes <out-dir>/theory_bench.json and <out-dir>/theory_timings.md and prints the JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EXP_PEAK = 8 * 4 * 256 * 2.4e9          # v_exp_f32 lanes per second of the whole chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--ns", type=int, default=1000)
    ap.add_argument("--nsym", type=int, default=2 ** 22)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)

    import theory_ref
    from qampy_amd import _lib, theory
    from qampy_amd._lib import DeviceArray
    from qampy_amd.core import hip_dsp

    def median_ms(fn, reps):
        fn()
        _lib.sync()
        ts = []
        for _ in range(reps):
            s, e = _lib.Event(), _lib.Event()
            s.record()
            fn()
            e.record()
            _lib.sync()
            ts.append(e.elapsed_ms(s))
        return float(np.median(ts))

    _lib.init(0)
    snr_db = np.arange(31.0)
    lin = 10 ** (snr_db / 10)
    device = _lib.device_name().strip()
    if not device or device.startswith("("):                 # the runtime reported no marketing name: only the architecture string, or nothing
        device = ("AMD Instinct accelerator " + device).strip()
    res = {"device": device, "reps": a.reps, "ns": a.ns, "points": snr_db.size, "exp_peak_per_s": EXP_PEAK, "curves": {}, "host": {}}
    for M in (16, 64, 256, 1024):
        nb = int(np.log2(M))
        count = snr_db.size * M * M * a.ns
        # the host's restatement: one point, few draws, scaled
        ns_host = max(1, 2 ** 22 // (M * M))
        al = theory.coded_symbols_qam(M)
        z = (np.random.default_rng(M).standard_normal(ns_host) + 1j * np.random.default_rng(M + 1).standard_normal(ns_host)) * np.sqrt(0.5 / lin[15])
        t0 = time.perf_counter()
        theory_ref.gmi_mc(al, lin[15], z)
        host_s = (time.perf_counter() - t0) * snr_db.size * a.ns / ns_host
        res["host"][str(M)] = {"ns_timed": ns_host, "curve_s_scaled": host_s}
        for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
            A, S = DeviceArray.from_host(np.ascontiguousarray(al.astype(dtype))), DeviceArray.from_host(lin)
            Z, out = DeviceArray((snr_db.size, a.ns), dtype), DeviceArray((snr_db.size, 2 + nb), np.float64)

            def curve():
                hip_dsp.awgn_mc_noise_dev(Z, S, 1)
                hip_dsp.awgn_mc_dev(A, S, Z, out)
            reps = a.reps if count < 1e10 else max(3, a.reps // 3)
            ms = median_ms(curve, reps)
            noise_ms = median_ms(lambda: hip_dsp.awgn_mc_noise_dev(Z, S, 1), a.reps)
            o = out.to_host()
            res["curves"]["%d_%s" % (M, name)] = {"M": M, "precision": name, "ms": ms, "noise_ms": noise_ms, "exponentials": count, "exp_per_s": count / ms * 1e3,
                                                  "fraction_of_exp_peak": count / ms * 1e3 / EXP_PEAK, "host_curve_s": host_s, "speedup_over_host": host_s / ms * 1e3,
                                                  "gmi_0dB": o[0, 0], "gmi_30dB": o[-1, 0], "mi_30dB": o[-1, 1]}
    res["shaped"] = {}
    nm, N = 2, a.nsym
    for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
        cb = np.dtype(dtype).itemsize
        lev, px = theory.cal_ps_probablts(theory.coded_symbols_qam(64), 2.0)
        table = DeviceArray.from_host(np.ascontiguousarray(theory.gray_code_qam(64).reshape(8, 8).astype(np.int32)))
        sy, idx = DeviceArray((nm, N), dtype), DeviceArray((nm, N), np.int32)
        fill_src, fill_dst = DeviceArray((nm * N * (cb + 4),), np.uint8), DeviceArray((nm * N * (cb + 4),), np.uint8)
        for what, fn, written in (("symbols", lambda: hip_dsp.ps_symbols_dev(sy, lev, px, 5), nm * N * cb),
                                  ("symbols_and_labels", lambda: hip_dsp.ps_symbols_dev(sy, lev, px, 5, labels=idx, label_table=table), nm * N * (cb + 4))):
            ms = median_ms(fn, a.reps)
            copy = median_ms(lambda: _lib.call("qh_memcpy_d2d", fill_dst.ptr, fill_src.ptr, written), a.reps)      # writes as many bytes (and reads them)
            res["shaped"]["%s_%s" % (what, name)] = {"ms": ms, "bytes_written": written, "write_GBps": written / ms / 1e6, "copy_ms": copy, "over_copy": ms / copy}
    with open(os.path.join(a.out_dir, "theory_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Theory curves: timings", "",
             "%s, a %d-point GMI + MI curve (0 .. 30 dB) at ns = %d draws per point: the noise launch and the three launches of `awgn_mc_dev` on resident "
             "buffers, median of warm runs between HIP events (scripts/bench_theory.py).  Exponentials: 31 M^2 ns.  Peak: %.3g v_exp_f32 lanes per second "
             "(8 per cycle and SIMD, 4 SIMDs, 256 CUs, 2.4 GHz); complex128 evaluates exp2 as a double polynomial, its fraction is for orientation.  "
             "Host: tests/theory_ref.py's vectorised float64 numpy, one point timed at M^2 ns near 2^22 and scaled to the curve." % (res["device"], snr_db.size, a.ns, EXP_PEAK), "",
             "| M | precision | curve ms | of which noise ms | exponentials | exp / s | fraction of the exp issue rate | host curve s (scaled) | speed-up |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in res["curves"].values():
        lines.append("| %d | %s | %.3f | %.4f | %.3g | %.3g | %.3f | %.1f | %.0f |" % (r["M"], r["precision"], r["ms"], r["noise_ms"], r["exponentials"], r["exp_per_s"],
                                                                                    r["fraction_of_exp_peak"], r["host_curve_s"], r["speedup_over_host"]))
    lines += ["", "Shaped source, %d modes of %d symbols of shaped 64-QAM; the copy is `qh_memcpy_d2d` of as many bytes as the source writes." % (nm, N), "",
              "| output | ms | bytes written | write GB/s | copy ms | multiple of the copy |", "|---|---|---|---|---|---|"]
    for k, r in res["shaped"].items():
        lines.append("| %s | %.4f | %d | %.0f | %.4f | %.2f |" % (k, r["ms"], r["bytes_written"], r["write_GBps"], r["copy_ms"], r["over_copy"]))
    with open(os.path.join(a.out_dir, "theory_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
