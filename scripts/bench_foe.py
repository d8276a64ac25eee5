#!/usr/bin/env python3
"""Time the blind frequency-offset estimate on a resident C3-shape capture (complex64, 2 x 2^23 samples): one block of N = 2^16 (the
reference's estimator) and blocks="all" (128 blocks), then the removal, each as the median of warm runs between HIP events - beside the same
computation composed from torch.fft on the same device (--torch: a process of its own, as in scripts/bench_cd.py).  One read of the capture
is 128 MiB.  Prints one JSON line.

    python3 scripts/bench_foe.py [--reps 20] [--fft-size 65536] [--torch]
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


def torch_ms(x, N, B, reps):
    import torch
    t = torch.from_numpy(x).cuda()

    def fn():
        blk = t[:, :B * N].reshape(t.shape[0], B, N)
        P = (torch.fft.fft(blk ** 4, dim=2).abs() ** 2).sum(dim=1)
        return torch.argmax(P, dim=1)
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), r.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fft-size", type=int, default=2 ** 16)
    ap.add_argument("--log2-len", type=int, default=23)
    ap.add_argument("--torch", action="store_true", help="time the torch.fft comparison instead (a process of its own)")
    a = ap.parse_args()
    nm, L, N = 2, 2 ** a.log2_len, a.fft_size
    rng = np.random.default_rng(1)
    s = (rng.choice([-3, -1, 1, 3], (nm, L)) + 1j * rng.choice([-3, -1, 1, 3], (nm, L))) / np.sqrt(10)
    s += 0.05 * (rng.standard_normal((nm, L)) + 1j * rng.standard_normal((nm, L)))
    x = (s * np.exp(2j * np.pi * (1234 / (4.0 * N)) * np.arange(L))).astype(np.complex64)
    if a.torch:
        res = {"shape": [nm, L], "fft_size": N, "reps": a.reps}
        for name, B in (("one_block", 1), ("all_blocks", L // N)):
            ms, bins = torch_ms(x, N, B, a.reps)
            res[name + "_torch_ms"], res[name + "_torch_bin"] = ms, [int(v) for v in bins]
        print(json.dumps(res))
        return
    _lib.init(0)
    E, out = DeviceArray.from_host(x), DeviceArray(x.shape, np.complex64)
    fo, st = DeviceArray((nm,), np.float64), DeviceArray((nm, 3), np.float64)
    res = {"device": _lib.device_name(), "shape": [nm, L], "fft_size": N, "capture_MiB": x.nbytes / 2 ** 20, "reps": a.reps}
    for name, B in (("one_block", 1), ("all_blocks", L // N)):
        res[name + "_ms"] = median_ms(lambda: hip_dsp.find_freq_offset_dev(E, 2, N, B, True, fo, stats=st), a.reps)
        res[name + "_bin"] = [int(v) for v in st.to_host()[:, 0]]
    res["removal_ms"] = median_ms(lambda: hip_dsp.comp_freq_offset_dev(E, fo, 2, out), a.reps)
    res["estimate_and_remove_ms"] = median_ms(lambda: (hip_dsp.find_freq_offset_dev(E, 2, N, L // N, True, fo, stats=st),
                                                        hip_dsp.comp_freq_offset_dev(E, fo, 2, out)), a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
