#!/usr/bin/env python3
"""Time the pilot-frame kernels (csrc/pilot.hip) at the shape of benchmark config 5 - frames of 2^16 symbols, a sequence of 1024, one phase
pilot every 32, 3 frames, 2 modes - in both precisions, each figure the median of warm runs between HIP events:

    frame        pilot_frame_dev with the labels (one launch)
    split        pilot_split_dev, payload and pilots of all frames (one launch)
    cpe          pilot_cpe_dev, N = 5, every pilot of every frame (five launches)
    foe          pilot_foe_dev on the sequence (five launches)

against the bytes each has to move over a device copy of as many bytes timed in the same run (qh_memcpy_d2d: the traffic floor), and against
the host path on the same input: pilotbased_receiver.pilot_based_cpe_new with host arrays in and out (angle, unwrap and average in numpy,
interpolation and removal on the device), a host clock around the call, which ends synchronised.

    python3 scripts/bench_pilotframe.py [--reps 20] [--out-dir profiles]

Writes <out-dir>/pilotframe_bench.json and <out-dir>/pilotframe_timings.md and prints the JSON line.
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
    from qampy_amd.core import hip_dsp, pilotbased_receiver

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

    _lib.init(0)
    M, F, S, R, nfr, nm, N = 256, 2 ** 16, 1024, 32, 3, 2, 5
    NP, ND = hip_dsp.pilot_counts(F, S, R)
    where = hip_dsp.pilot_positions(F, S, R)[0]
    res = {"device": _lib.device_name(), "reps": a.reps, "M": M, "frame_len": F, "seq_len": S, "ins_rat": R, "nframes": nfr, "nmodes": nm, "N": N, "NP": NP, "ND": ND}
    for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
        cb = np.dtype(dtype).itemsize
        d = synth.make_pilot_frames_dev(M, F, S, R, nframes=nfr, nmodes=nm, dtype=dtype)
        x = DeviceArray(d["frame"].shape, dtype)
        hip_dsp.impair_pointwise_dev(d["frame"], x, snr=(30., 1), phase=(1e-6, 1.0), seed=3)
        L = nfr * F
        Eout, trace = DeviceArray((nm, L), dtype), DeviceArray((nm, L), np.zeros(1, dtype).real.dtype)
        pay, pil = DeviceArray((nm, nfr * ND), dtype), DeviceArray((nm, nfr * NP), dtype)
        fit, fo = DeviceArray((nm, 2), np.float64), DeviceArray((nm,), np.float64)
        seq = DeviceArray((nm, S), dtype)
        hip_dsp.pilot_split_dev(x, S, S, 0, [0], pilots=seq)           # the first S symbols: a frame that is all sequence
        seq_ref = DeviceArray.from_host(np.ascontiguousarray(d["pilots"].to_host()[:, :S]))
        fill_src, fill_dst = DeviceArray((3 * nm * L * cb,), np.uint8), DeviceArray((3 * nm * L * cb,), np.uint8)

        def copy_ms(nbytes):
            return median_ms(lambda: _lib.call("qh_memcpy_d2d", fill_dst.ptr, fill_src.ptr, nbytes // 2))          # nbytes moved: half read, half written

        stages = [("frame", lambda: hip_dsp.pilot_frame_dev(d["pilots"], d["payload"], F, S, R, nfr, d["frame"], labels=d["idx_tx"], idx_frame=d["idx_frame"]),
                   nm * L * (2 * cb + 8)),
                  ("split", lambda: hip_dsp.pilot_split_dev(x, F, S, R, None, payload=pay, pilots=pil), nm * L * 2 * cb),
                  ("cpe", lambda: hip_dsp.pilot_cpe_dev(x, where, F, nfr, d["pilots"], N, Eout, trace), nm * L * (2 * cb + cb // 2)),
                  ("foe", lambda: hip_dsp.pilot_foe_dev(seq, seq_ref, fit, fo, average=True), nm * S * 2 * cb)]
        r = {}
        for st, fn, moved in stages:
            ms, floor = median_ms(fn), copy_ms(moved)
            r[st] = {"ms": ms, "bytes_moved": moved, "copy_ms": floor, "over_copy": ms / floor, "GBps": moved / ms / 1e6}
        hx, hp = x.to_host(), d["pilots"].to_host()
        ts = []
        for _ in range(max(3, a.reps // 4) + 1):
            t0 = time.perf_counter()
            pilotbased_receiver.pilot_based_cpe_new(hx, hp, where, F, seq_len=S, num_average=N, nframes=nfr)
            ts.append((time.perf_counter() - t0) * 1e3)
        r["host_cpe_ms"] = float(np.median(ts[1:]))
        ts = []
        for _ in range(max(3, a.reps // 4) + 1):
            t0 = time.perf_counter()
            pilotbased_receiver.pilot_based_cpe_new(hx, hp, where, F, seq_len=S, num_average=N, nframes=nfr, method="hip")
            ts.append((time.perf_counter() - t0) * 1e3)
        r["host_in_out_device_cpe_ms"] = float(np.median(ts[1:]))
        res[name] = r
    with open(os.path.join(a.out_dir, "pilotframe_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Pilot frames: timings", "",
             "%s, frames of 2^16 symbols (sequence %d, one phase pilot every %d: %d pilots and %d payload symbols a frame), %d frames, %d modes, median of %d warm runs "
             "between HIP events (scripts/bench_pilotframe.py)." % (res["device"], S, R, NP, ND, nfr, nm, a.reps),
             "The copy is `qh_memcpy_d2d` moving as many bytes (read plus written) as the stage has to, timed in the same run: the traffic floor.", "",
             "| precision | stage | ms | bytes moved | copy ms | multiple of the copy | GB/s |", "|---|---|---|---|---|---|---|"]
    for name in ("complex64", "complex128"):
        for st in ("frame", "split", "cpe", "foe"):
            r = res[name][st]
            lines.append("| %s | %s | %.4f | %d | %.4f | %.2f | %.0f |" % (name, st, r["ms"], r["bytes_moved"], r["copy_ms"], r["over_copy"], r["GBps"]))
    lines.append("")
    for name in ("complex64", "complex128"):
        lines.append("%s, host arrays in and out (a host clock around the call): pilot_based_cpe_new %.2f ms on the host path (numpy estimate, device interpolation), "
                     "%.2f ms with method=\"hip\" (one upload, the estimate on the device, two downloads)." % (
                         name, res[name]["host_cpe_ms"], res[name]["host_in_out_device_cpe_ms"]))
    with open(os.path.join(a.out_dir, "pilotframe_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
