#!/usr/bin/env python3
"""Time the transmitter response on a resident C3-shape field (2 x 2^23 samples) in both precisions: row extrema, the DAC's point-wise pass,
the sections filter (the default Bessel of order 2, a Butterworth of order 6), amplifier and modulator, and the whole of
sim_tx_response_dev, each as the median of warm runs between HIP events.  Each time is set against (a) the bytes the pass must move divided
by the bandwidth a plain device-to-device copy of the same field reaches in the same run, and - the filter - (b) scipy.signal.sosfilt on the
host for the same rows.  Prints one JSON line.

    python3 scripts/bench_txresp.py [--reps 20] [--log2-len 23] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qampy_amd import _lib                                             # noqa: E402
from qampy_amd._lib import DeviceArray                                 # noqa: E402
from qampy_amd.core import hip_dsp                                     # noqa: E402


def median_ms(fn, reps):
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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2-len", type=int, default=23)
    ap.add_argument("--no-host", action="store_true", help="skip scipy's sosfilt on the host")
    a = ap.parse_args()
    nm, L = 2, 2 ** a.log2_len
    fs = 40e9
    rng = np.random.default_rng(1)
    x128 = (rng.choice([-3, -1, 1, 3], (nm, L)) + 1j * rng.choice([-3, -1, 1, 3], (nm, L))) / np.sqrt(10)
    _lib.init(0)
    res = {"device": _lib.device_name(), "shape": [nm, L], "reps": a.reps, "sos_chunk": hip_dsp.SOS_CHUNK, "sos_tile": hip_dsp.SOS_TILE}
    sos2, sos6 = hip_dsp.design_lowpass_sos(fs, 18e9), hip_dsp.design_lowpass_sos(fs, 100e6, "butter", 6)
    for dtype, tag in ((np.complex64, "c64"), (np.complex128, "c128")):
        x = x128.astype(dtype)
        E, out = DeviceArray.from_host(x), DeviceArray(x.shape, dtype)
        ext = hip_dsp.row_extrema_dev(E)
        r = {"field_MiB": x.nbytes / 2 ** 20}
        copy = median_ms(lambda: out.copy_from(E), a.reps)
        r["copy_ms"] = copy                                                  # one read and one write of the field
        # (name, call, reads + writes of the field the pass must make)
        stages = [("extrema", lambda: hip_dsp.row_extrema_dev(E, ext), 1),
                  ("dac_pointwise", lambda: hip_dsp.dac_pointwise_dev(E, out, clip_rat=0.8, quant_bits=6, enob=5, seed=1, ext=ext), 2),
                  ("sosfilt_bessel2", lambda: hip_dsp.sosfilt_dev(E, out, sos2), 3),
                  ("sosfilt_butter6", lambda: hip_dsp.sosfilt_dev(E, out, sos6), 3),
                  ("modulator_amp", lambda: hip_dsp.modulator_response_dev(E, out, tgt_v=0.7, ext=ext), 2),
                  ("sim_tx_response", lambda: hip_dsp.sim_tx_response_dev(E, out, fs, enob=5, clip_rat=0.8, quant_bits=6, tgt_v=0.7, seed=1), 1 + 2 + 3 + 1 + 2)]
        for name, fn, passes in stages:
            ms = median_ms(fn, a.reps)
            r[name + "_ms"] = ms
            r[name + "_over_traffic_floor"] = ms / (copy * passes / 2)
        if not a.no_host:
            for name, sos in (("sosfilt_bessel2", sos2), ("sosfilt_butter6", sos6)):
                import scipy.signal as scisig
                t = time.perf_counter()
                scisig.sosfilt(sos, x, axis=-1)
                host = (time.perf_counter() - t) * 1e3
                r[name + "_host_ms"] = host
                r[name + "_host_over_device"] = host / r[name + "_ms"]
        res[tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
