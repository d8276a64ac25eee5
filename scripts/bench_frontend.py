#!/usr/bin/env python3
"""Time the whole-row transforms and the analog front end on a resident C3-size complex64 capture (2 x 2^23 samples) and on a Bluestein
length near it (2 x 8 000 000): fft_dev alone, the forward / multiply / inverse round (pre_filter_dev and skew_dev), the IQ passes, and
ResidentReceiver.frontend with everything on, each as the median of warm runs between HIP events.  Each time is set against the bytes its
passes move over HBM divided by the bandwidth a plain device-to-device copy of the same field reaches in the same run.  If torch imports,
torch.fft.fft on the same shapes is reported as an outside yardstick (measurement only).  Prints one JSON line.

    python3 scripts/bench_frontend.py [--reps 20] [--log2-len 23] [--blue-len 8000000] [--no-torch]
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


def transform_passes(L):
    """reads + writes of one transform of rows of L samples, in units of the (nmodes, L) field: a size-M transform reads its input and writes
    its output once (one workgroup per row) or twice each (four-step, through T); Bluestein makes two of them, padded to M"""
    M, N1, _, blue = hip_dsp.fft_plan(L)
    inner = 2 if N1 > 1 else 0                        # T written and read
    if not blue:
        return 2 + inner
    r = M / L
    return (1 + r + inner * r) + (r + 1 + inner * r)    # x -> W, W -> out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2-len", type=int, default=23)
    ap.add_argument("--blue-len", type=int, default=8000000)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    nm = 2
    sr = 50e9
    _lib.init(0)
    res = {"device": _lib.device_name(), "reps": a.reps, "dtype": "complex64"}
    rng = np.random.default_rng(1)
    for tag, L in (("pow2", 2 ** a.log2_len), ("bluestein", a.blue_len)):
        x = np.empty((nm, L), np.complex64)
        x.real = rng.standard_normal((nm, L), dtype=np.float32)
        x.imag = rng.standard_normal((nm, L), dtype=np.float32)
        E, out = DeviceArray.from_host(x), DeviceArray(x.shape, x.dtype)
        mom, coef = DeviceArray((nm, 10), np.float64), DeviceArray((nm, 6), np.float64)
        r = {"shape": [nm, L], "plan": list(hip_dsp.fft_plan(L)), "field_MiB": x.nbytes / 2 ** 20}
        copy = median_ms(lambda: out.copy_from(E), a.reps)
        r["copy_ms"] = copy                                                  # one read and one write of the field
        r["copy_GBps"] = 2 * x.nbytes / copy / 1e6
        tp = transform_passes(L)
        stages = [("fft", lambda: hip_dsp.fft_dev(E, out), tp),
                  ("ifft", lambda: hip_dsp.ifft_dev(E, out), tp),
                  ("pre_filter", lambda: hip_dsp.pre_filter_dev(E, out, 10), 2 * tp),
                  ("skew", lambda: hip_dsp.skew_dev(E, out, 0.0, 0.4 * sr / 2, sr), 2 * tp + 1),
                  ("iq_moments", lambda: hip_dsp.iq_moments_dev(E, 2, mom), 1),
                  ("orthonormalize", lambda: hip_dsp.orthonormalize_dev(E, out, 2, mom, coef), 3)]
        for name, fn, passes in stages:
            ms = median_ms(fn, a.reps)
            r[name + "_ms"] = ms
            r[name + "_passes"] = passes
            r[name + "_traffic_floor_ms"] = copy * passes / 2
            r[name + "_over_traffic_floor"] = ms / (copy * passes / 2)
        del E, out
        if tag == "pow2":
            from qampy_amd.pipeline import ResidentReceiver
            rx = ResidentReceiver(nm, L, 2, 16, 21, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(1, 1), Mtestangles=32, Nbps=20)
            rx.load(x)
            fn = lambda: rx.frontend(orthonormalize=True, skew=(0.0, 0.4 * sr / 2), sampling_rate=sr, pre_filter_bw=10)      # noqa: E731
            passes = 4 * tp + 1 + 3
            ms = median_ms(fn, a.reps)
            r["resident_frontend_ms"], r["resident_frontend_passes"] = ms, passes
            r["resident_frontend_over_traffic_floor"] = ms / (copy * passes / 2)
            del rx
        if not a.no_torch:
            try:
                import torch
                t = torch.from_numpy(x).cuda()
                torch.fft.fft(t, dim=1)
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.reps):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    torch.fft.fft(t, dim=1)
                    e.record()
                    torch.cuda.synchronize()
                    ts.append(s.elapsed_time(e))
                r["torch_fft_ms"] = float(np.median(ts))
                del t
                torch.cuda.empty_cache()
            except Exception as exc:                                         # no torch, or no GPU build of it: the yardstick is optional
                r["torch_fft_ms"] = None
                r["torch_error"] = repr(exc)[:200]
        res[tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
