#!/usr/bin/env python3
"""Time cd_filter_dev (csrc/cd.hip) at C3 shape - 2 x 2^23 samples - for each block size, complex64 and complex128, against the same
batched block filter in torch.fft (rocFFT) for comparison.  Warm runs timed with HIP events, median of --reps.  Effective bandwidth counts
the input read once and the output written once.  One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qampy_amd import _lib                                       # noqa: E402
from qampy_amd._lib import DeviceArray, Event                    # noqa: E402
from qampy_amd.core import filter as cdf                         # noqa: E402

FS, D, WL = 40e9, 17e-6, 1550e-9
KM = {1024: 100, 2048: 500, 4096: 1000, 8192: 2000}


def time_lib(N, dtype, L, reps):
    x = (np.random.default_rng(1).standard_normal((2, L)) + 1j * np.random.default_rng(2).standard_normal((2, L))).astype(dtype)
    E, out = DeviceArray.from_host(x), DeviceArray((2, L), dtype)
    for _ in range(3):
        cdf.cd_filter_dev(E, out, FS, D, KM[N] * 1e3, WL, N=N)
    _lib.sync()
    t = []
    for _ in range(reps):
        a, b = Event(), Event()
        a.record()
        cdf.cd_filter_dev(E, out, FS, D, KM[N] * 1e3, WL, N=N)
        b.record()
        _lib.sync()
        t.append(b.elapsed_ms(a))
    return float(np.median(t))


def time_torch(N, dtype, L, reps):
    import torch
    ct = torch.complex64 if dtype == np.complex64 else torch.complex128
    dev = torch.device("cuda:0")
    x = torch.randn(2, L, dtype=ct, device=dev)
    n, q = N // 2, N // 4
    nblk = (L + n - 1) // n
    idx = ((torch.arange(nblk, device=dev)[:, None] * n - q + torch.arange(N, device=dev)[None, :]) % L)
    w = 2 * np.pi * np.fft.fftfreq(N)
    c2 = cdf.cd_coeffs_exact(FS, D, KM[N] * 1e3, WL)[0]
    H = torch.from_numpy(np.exp(1j * np.remainder(c2 * w * w, 2 * np.pi))).to(dev, ct)

    def run():
        blocks = x[:, idx]
        y = torch.fft.ifft(torch.fft.fft(blocks, dim=-1) * H, dim=-1)[:, :, q:q + n]
        return y.reshape(2, -1)[:, :L]

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2len", type=int, default=23)
    ap.add_argument("--torch", action="store_true", help="time the torch.fft comparison instead (a process of its own)")
    a = ap.parse_args()
    L = 2 ** a.log2len
    cases = [(N, np.complex64) for N in (1024, 2048, 4096, 8192)] + [(4096, np.complex128)]
    if not a.torch:
        _lib.init(0)
    for N, dt in cases:
        rec = dict(N=N, dtype=np.dtype(dt).name, km=KM[N], samples=2 * L)
        ms = time_torch(N, dt, L, a.reps) if a.torch else time_lib(N, dt, L, a.reps)
        rec["torch_fft_ms" if a.torch else "kernel_ms"] = round(ms, 4)
        rec["GBps"] = round(2 * 2 * L * np.dtype(dt).itemsize / ms / 1e6, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
