#!/usr/bin/env python3
"""Time the pre-compensation kernels (csrc/precomp.hip) at the shape of benchmark config 3 - 2 modes of 2^22 symbols, 64-QAM - for patterns of
3 and of 5 symbols (tables of 512 entries, kept in LDS, and of 32768, in global memory), in both precisions, each figure the median of warm runs
between HIP events:

    index        pattern_index_dev, both index rows (one launch)
    table        lut_accumulate_dev from the index rows (three memsets, four launches)
    cal_lut      cal_lut_dev: the two above
    apply        lut_apply_dev from the index rows (one launch)
    predistort   lut_predistort_dev: indices on the fly, no index rows (one launch)
    arcsin       comp_mod_sin_dev with the clamp (one launch)
    dac_table    comp_dac_resp_dev for 2^23 bins (three launches)
    dac_filter   spectral_filter_dev with that table on 2 x 2^23 samples (the transforms of csrc/fft.hip)

against a device copy of the bytes each has to move at the least (qh_memcpy_d2d of as many bytes, timed in the same run: the traffic floor).

    python3 scripts/bench_precomp.py [--reps 20] [--out-dir profiles]

Writes <out-dir>/precomp_bench.json and <out-dir>/precomp_timings.md and prints the JSON line.
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--nsym", type=int, default=2 ** 22)
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

    _lib.init(0)
    M, nm, L = 64, 2, a.nsym
    res = {"device": _lib.device_name(), "reps": a.reps, "M": M, "nmodes": nm, "nsym": L}
    for name, dtype in (("complex64", np.complex64), ("complex128", np.complex128)):
        cb = np.dtype(dtype).itemsize
        src = synth.make_symbols_dev(M, L, nmodes=nm, dtype=dtype)
        tx, lv = src["symbols"], hip_dsp.pattern_levels(src["alphabet_host"])
        rx, out = DeviceArray(tx.shape, dtype), DeviceArray(tx.shape, dtype)
        hip_dsp.impair_pointwise_dev(tx, rx, snr=(25., 1), seed=3)
        iI, iQ = DeviceArray(tx.shape, np.int32), DeviceArray(tx.shape, np.int32)
        wide, wide_out = DeviceArray((nm, 2 * L), dtype), DeviceArray((nm, 2 * L), dtype)
        wide.zero()
        table = DeviceArray((2 * L,), dtype)
        fill_src, fill_dst = DeviceArray((2 * nm * L * cb,), np.uint8), DeviceArray((2 * nm * L * cb,), np.uint8)

        def copy_ms(nbytes):
            return median_ms(lambda: _lib.call("qh_memcpy_d2d", fill_dst.ptr, fill_src.ptr, nbytes // 2))          # nbytes moved: half read, half written

        r = {}
        for mem_len in (3, 5):
            N = lv.N(mem_len)
            ea, nI, nQ = DeviceArray((nm, N), np.complex128), DeviceArray((nm, N), np.int32), DeviceArray((nm, N), np.int32)
            stages = [("index", lambda: hip_dsp.pattern_index_dev(tx, lv, mem_len, iI, iQ), nm * L * (cb + 8)),
                      ("table", lambda: hip_dsp.lut_accumulate_dev(tx, rx, iI, iQ, N, ea=ea, nI=nI, nQ=nQ), nm * L * (2 * cb + 8)),
                      ("cal_lut", lambda: hip_dsp.cal_lut_dev(tx, rx, lv, mem_len, ea=ea, idx_I=iI, idx_Q=iQ, nI=nI, nQ=nQ), nm * L * (2 * cb + 8)),
                      ("apply", lambda: hip_dsp.lut_apply_dev(tx, ea, iI, iQ, out), nm * L * (2 * cb + 8)),
                      ("predistort", lambda: hip_dsp.lut_predistort_dev(tx, lv, mem_len, ea, out), nm * L * 2 * cb)]
            for st, fn, moved in stages:
                ms, floor = median_ms(fn), copy_ms(moved)
                r["%s_m%d" % (st, mem_len)] = {"ms": ms, "bytes_moved": moved, "copy_ms": floor, "over_copy": ms / floor, "GBps": moved / ms / 1e6, "N": N}
        stages = [("arcsin", lambda: hip_dsp.comp_mod_sin_dev(tx, out, vpi=1.14, clip=0.95), nm * L * 2 * cb),
                  ("dac_table", lambda: hip_dsp.comp_dac_resp_dev(20e9, 2 * L, 0.1, dtype=dtype, out=table), 2 * 2 * L * cb),
                  ("dac_filter", lambda: hip_dsp.spectral_filter_dev(wide, wide_out, table), nm * 2 * L * 2 * cb)]
        for st, fn, moved in stages:
            ms, floor = median_ms(fn), copy_ms(moved)
            r[st] = {"ms": ms, "bytes_moved": moved, "copy_ms": floor, "over_copy": ms / floor, "GBps": moved / ms / 1e6}
        res[name] = r
    with open(os.path.join(a.out_dir, "precomp_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Digital pre-compensation: timings", "",
             "%s, %d modes of %d symbols of %d-QAM, patterns of 3 and 5 symbols (tables of 512 and 32768 entries), median of %d warm runs between HIP events "
             "(scripts/bench_precomp.py).  dac_table: 2^23 bins; dac_filter: 2 x 2^23 samples." % (res["device"], nm, L, M, a.reps),
             "The copy is `qh_memcpy_d2d` moving as many bytes (read plus written) as the stage has to at the least, timed in the same run: the traffic floor.  "
             "(dac_table only writes: its copy moves the table's bytes once in and once out.)", "",
             "| precision | stage | ms | bytes moved | copy ms | multiple of the copy | GB/s |", "|---|---|---|---|---|---|---|"]
    for name in ("complex64", "complex128"):
        for st, r in res[name].items():
            lines.append("| %s | %s | %.4f | %d | %.4f | %.2f | %.0f |" % (name, st, r["ms"], r["bytes_moved"], r["copy_ms"], r["over_copy"], r["GBps"]))
    with open(os.path.join(a.out_dir, "precomp_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
