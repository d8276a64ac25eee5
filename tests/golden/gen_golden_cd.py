#!/usr/bin/env python3
"""
Generate tests/golden/cd.npz - the reference's chromatic-dispersion outputs - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_cd.py

Inputs: band-limited unit-power complex rows (tests/cd_ref.py bandlimited, |f| < 0.275 fs, a stand-in for 2-sample/symbol
QAM) of lengths 4096, 16384, 10007 and 12000, rounded to multiples of 2^-10 and stored as int16 (re, im) pairs, so that
complex64 and complex128 hold the same values.  fs = 40 GS/s, D = 17 ps/nm/km, wl = 1550 nm.

Keys: ``x<len>`` input; ``cdcomp_<len>_<km>_<dtype>`` CDcomp(x, fs, 0, km * 1e3, D, wl)[0]; ``adddisp_<len>_<km>_<dtype>``
add_dispersion(x, fs, D, km * 1e3, wl).  ``<km>`` is ``m1000`` for -1000 km.  Outputs are stored in their own dtype; the
combinations are chosen to stay under 1 MiB.  ``blk_in`` (add_dispersion of x4096 over 1000 km, rounded like the inputs) and
``blk_ref`` = CDcomp(blk_in, fs, 1024, -1000e3, D, wl)[0] keep the reference's N > 0 result, whose block spectra meet H in
the wrong order.
"""
import os

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import impairments as ref_imp                               # noqa: E402
from qampy.core.equalisation import equalisation as ref_eq                  # noqa: E402

import sys                                                                  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cd_ref                                                               # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FS, D, WL, SCALE = 40e9, 17e-6, 1550e-9, 1024
CT = {"c64": np.complex64, "c128": np.complex128}
KM = {100: "100", 1000: "1000", -1000: "m1000"}
CDCOMP = [(4096, 100, "c64"), (4096, 1000, "c128"), (4096, -1000, "c128"), (16384, 100, "c64"), (10007, 1000, "c128"),
          (12000, -1000, "c64"), (4096, 1000, "c64")]
ADDDISP = [(4096, 1000, "c128"), (10007, 100, "c64"), (16384, -1000, "c64")]


def quantise(x):
    q = np.round(np.stack([x.real, x.imag], -1) * SCALE)
    assert np.abs(q).max() < 32767
    return q.astype(np.int16)


def dequantise(q):
    return (q[..., 0] + 1j * q[..., 1]) / SCALE


def main():
    data = {"fs": np.float64(FS), "D": np.float64(D), "wl": np.float64(WL), "scale": np.float64(SCALE)}
    xs = {}
    for j, n in enumerate((4096, 16384, 10007, 12000)):
        data["x%d" % n] = quantise(cd_ref.bandlimited(1, n, 100 + j)[0])
        xs[n] = dequantise(data["x%d" % n])
    for n, km, dt in CDCOMP:
        data["cdcomp_%d_%s_%s" % (n, KM[km], dt)] = ref_eq.CDcomp(xs[n].astype(CT[dt]), FS, 0, km * 1e3, D, WL)[0].astype(CT[dt])
    for n, km, dt in ADDDISP:
        data["adddisp_%d_%s_%s" % (n, KM[km], dt)] = ref_imp.add_dispersion(xs[n].astype(CT[dt]), FS, D, km * 1e3, WL).astype(CT[dt])
    data["blk_in"] = quantise(ref_imp.add_dispersion(xs[4096], FS, D, 1000e3, WL))
    data["blk_ref"] = ref_eq.CDcomp(dequantise(data["blk_in"]), FS, 1024, -1000e3, D, WL)[0]
    path = os.path.join(OUT, "cd.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
