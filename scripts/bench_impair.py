#!/usr/bin/env python3
"""Time the channel impairments on a resident C3-shape capture (complex64, 2 x 2^23 samples): simulate_transmission_dev with every stage
on (phase noise, carrier offset, SNR, modal delay, PMD), and the fused point-wise pass, the roll and the PMD filter on their own, each as the
median of warm runs between HIP events.  One read of the capture is 128 MiB.  Prints one JSON line.

    python3 scripts/bench_impair.py [--reps 20] [--log2-len 23]
"""
import argparse
import json
import os
import sys

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
    a = ap.parse_args()
    nm, L = 2, 2 ** a.log2_len
    fb, fs = 20e9, 40e9
    rng = np.random.default_rng(1)
    x = ((rng.choice([-3, -1, 1, 3], (nm, L)) + 1j * rng.choice([-3, -1, 1, 3], (nm, L))) / np.sqrt(10)).astype(np.complex64)
    _lib.init(0)
    E, out, tmp = DeviceArray.from_host(x), DeviceArray(x.shape, np.complex64), DeviceArray(x.shape, np.complex64)
    kw = dict(snr=18.0, freq_off=100e6, lwdth=100e3)
    res = {"device": _lib.device_name(), "shape": [nm, L], "capture_MiB": x.nbytes / 2 ** 20, "reps": a.reps}
    res["simulate_all_ms"] = median_ms(lambda: hip_dsp.simulate_transmission_dev(E, out, fb, fs, dgd=30e-12, theta=np.pi / 5.6, modal_delay=[3, -5],
                                                                               seed=1, tmp=tmp, **kw), a.reps)
    res["pointwise_all_ms"] = median_ms(lambda: hip_dsp.impair_pointwise_dev(E, out, snr=(18.0, 2), phase=(100e3, fs), freq=(100e6, fs), seed=1), a.reps)
    res["pointwise_noise_only_ms"] = median_ms(lambda: hip_dsp.impair_pointwise_dev(E, out, sigma=0.1, seed=1), a.reps)
    res["pointwise_freq_only_ms"] = median_ms(lambda: hip_dsp.impair_pointwise_dev(E, out, freq=(100e6, fs)), a.reps)
    res["modal_delay_ms"] = median_ms(lambda: hip_dsp.modal_delay_dev(E, out, [3, -5]), a.reps)
    res["pmd_ms"] = median_ms(lambda: hip_dsp.apply_pmd_dev(E, out, np.pi / 5.6, 30e-12, fs), a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
