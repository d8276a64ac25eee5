#!/usr/bin/env python3
"""Time the polyphase resampler at a C3-size raw capture: 2 modes, 80 -> 56 GS/s (up / down = 7 / 10), ceil(2^23 10 / 7) input samples,
complex64, root-raised-cosine taps 401 and 4001; HIP events around the kernel, median of --reps runs after a warm-up.  Beside each time its two
floors: bytes read and written at --hbm TB/s, and J FMAs per real output component (2 J flop; J = ceil(taps / up)) at --tflops fp32 vector TFLOP/s.
--renorm times the three launches of a renormalised load as well; --scipy times scipy.signal.resample_poly on the host for the same rows
(one thread per row, no GPU).  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qampy_amd.core import resample as rs                                   # noqa: E402


def median_ms(fn, reps):
    from qampy_amd import _lib
    from qampy_amd._lib import Event
    for _ in range(3):
        fn()
    _lib.sync()
    t = []
    for _ in range(reps):
        a, b = Event(), Event()
        a.record()
        fn()
        b.record()
        _lib.sync()
        t.append(b.elapsed_ms(a))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2len", type=int, default=23)
    ap.add_argument("--hbm", type=float, default=8.0, help="HBM bandwidth of the floor, TB/s")
    ap.add_argument("--tflops", type=float, default=157.3, help="fp32 vector rate of the floor, TFLOP/s")
    ap.add_argument("--renorm", action="store_true")
    ap.add_argument("--scipy", action="store_true")
    a = ap.parse_args()
    up, down, L = 7, 10, 2 ** a.log2len
    Lin = -(-L * down // up)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((2, Lin)) + 1j * rng.standard_normal((2, Lin))).astype(np.complex64)
    if a.scipy:
        from concurrent.futures import ThreadPoolExecutor
        from scipy import signal as scisig
        for taps in (401, 4001):
            h = rs.rrcos_taps(taps, up * 80e9, 1 / 28e9, 0.1)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                with ThreadPoolExecutor(2) as ex:
                    list(ex.map(lambda r: scisig.resample_poly(r, up, down, window=h), x))
                t.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps(dict(taps=taps, scipy_resample_poly_ms=round(min(t), 1), rows=2, Lin=Lin)), flush=True)
        return
    from qampy_amd import _lib
    from qampy_amd._lib import DeviceArray
    _lib.init(0)
    E, out = DeviceArray.from_host(x), DeviceArray((2, L), np.complex64)
    for taps in (401, 4001):
        h = rs.rrcos_taps(taps, up * 80e9, 1 / 28e9, 0.1)
        J = -(-taps // up)
        med, lo, hi = median_ms(lambda: rs.resample_dev(E, out, h, up, down, 1.0), a.reps)
        rec = dict(taps=taps, J=J, Lin=Lin, Lout=L, kernel_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                   floor_hbm_ms=round(2 * (Lin + L) * 8 / (a.hbm * 1e12) * 1e3, 4),
                   floor_fma_ms=round(2 * L * 2 * J * 2 / (a.tflops * 1e12) * 1e3, 4))      # rows x outputs x (re, im) x J FMAs x 2 flop
        if a.renorm:
            mom = DeviceArray((2, 3), np.float64)

            def full():
                rs.resample_dev(E, out, h, up, down, 1.0)
                rs.center_scale_dev(out, rs.row_moments_dev(out, mom), power=1.0)
            rec["with_renorm_ms"] = round(median_ms(full, a.reps)[0], 4)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
