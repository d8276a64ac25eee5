#!/usr/bin/env python3
"""
Generate tests/golden/frontend.npz - the reference's analog front end (pre_filter, comp_rf_delay, orthonormalize_signal,
comp_IQ_inbalance) - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_frontend.py

Keys (``<case>``: the names in the tables below, which tests/test_frontend_ref.py and tests/test_gpu_frontend.py read back from ``cases``):
    cases                  JSON text: {"pre": [[case, bws]], "delay": [[case, delays, sampling_rate]], "orth": [[case, os]], "iq": [case]}
    pre_x_<case>           input of pre_filter, its shape and dtype as given to the reference
    pre_y_<case>_<i>       pre_filter(x, bws[i])
    delay_x_<case>         input of comp_rf_delay (real or complex)
    delay_y_<case>_<i>     comp_rf_delay(x, delays[i], sampling_rate)                            float64
    orth_x_<case>          input of orthonormalize_signal (DC offset and quadrature error put on)
    orth_y_<case>          orthonormalize_signal(x, os)                                          always 2-d
    iq_x_<case>            input of comp_IQ_inbalance
    iq_y_<case>            comp_IQ_inbalance(x)
    iq_c_<case>            x after the call: the reference centres its argument in place
"""
import json
import os

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import analog_frontend as ref_af                              # noqa: E402
from qampy.core import filter as ref_filter                                   # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
BWS = [8, 16, 0.01]
SR = 50e9
DELAYS = [0.3 * SR / 2, 5.25 * SR / 2]                  # a fraction of a sample and several samples on the reference's grid, whose spacing is SR / 2

#            case   L     rows (0: 1-d)  dtype
PRE = [("e1_c64", 1000, 0, "complex64"), ("e2_c128", 600, 2, "complex128"), ("o1_c128", 1001, 0, "complex128"), ("o2_c64", 601, 2, "complex64"),
       ("p2_c64", 512, 2, "complex64"), ("p1_c128", 1024, 0, "complex128")]
DELAY = [("e1", 1000, 0, False), ("o2", 601, 2, False), ("p2", 512, 2, False), ("o1c", 1001, 0, True), ("e2c", 600, 2, True)]
ORTH = [("os1_e_c128", 1000, 2, "complex128", 1), ("os2_o_c128", 1001, 2, "complex128", 2), ("os2_o_c64", 1001, 2, "complex64", 2),
        ("os3_1d_c128", 1000, 0, "complex128", 3), ("os1_1d_c64", 1024, 0, "complex64", 1)]
IQ = [("1d_c128", 1500, 0, "complex128"), ("2d_c128", 1500, 2, "complex128"), ("2d_c64", 1001, 2, "complex64"), ("1d_c64", 1024, 0, "complex64")]


def field(rng, L, rows, dtype):
    x = (rng.standard_normal((max(rows, 1), L)) + 1j * rng.standard_normal((max(rows, 1), L))).astype(dtype)
    return x[0] if rows == 0 else x


def hybrid(rng, L, rows, dtype, angles_deg, dc):
    """16-QAM symbols through an imperfect hybrid: Q leans on I by the quadrature error, has its own gain, and both rails carry an offset"""
    r = max(rows, 1)
    lv = np.array([-3, -1, 1, 3]) / np.sqrt(10)
    I, Q = rng.choice(lv, (r, L)), rng.choice(lv, (r, L))
    I = I + 0.05 * rng.standard_normal((r, L))
    Q = Q + 0.05 * rng.standard_normal((r, L))
    x = np.empty((r, L), np.complex128)
    for m in range(r):
        ph = np.deg2rad(angles_deg[m % len(angles_deg)])
        x[m] = I[m] + 1j * (1.15 * (Q[m] * np.cos(ph) + I[m] * np.sin(ph))) + dc[m % len(dc)]
    x = x.astype(dtype)
    return x[0] if rows == 0 else x


def main():
    rng = np.random.default_rng(20261019)
    data = {}
    cases = {"pre": [], "delay": [], "orth": [], "iq": []}
    for c, L, rows, dt in PRE:
        x = field(rng, L, rows, dt)
        data["pre_x_" + c] = x
        for i, bw in enumerate(BWS):
            y = ref_filter.pre_filter(x, bw)
            assert y.dtype == x.dtype and y.shape == x.shape
            assert (bw == 0.01) == (not np.any(y))
            data["pre_y_%s_%d" % (c, i)] = y
        cases["pre"].append([c, BWS])
    for c, L, rows, cplx in DELAY:
        x = field(rng, L, rows, "complex128")
        x = x if cplx else np.ascontiguousarray(x.real)
        data["delay_x_" + c] = x
        for i, d in enumerate(DELAYS):
            y = ref_af.comp_rf_delay(x, d, SR)
            assert y.dtype == np.float64 and y.shape == x.shape
            data["delay_y_%s_%d" % (c, i)] = y
        cases["delay"].append([c, DELAYS, SR])
    for c, L, rows, dt, os_ in ORTH:
        x = hybrid(rng, L, rows, dt, (12.0, -18.0), (0.2 - 0.1j, -0.15 + 0.25j))
        data["orth_x_" + c] = x
        y = ref_af.orthonormalize_signal(x, os_)
        assert y.ndim == 2 and y.dtype == x.dtype
        data["orth_y_" + c] = y
        cases["orth"].append([c, os_])
    for c, L, rows, dt in IQ:
        x = hybrid(rng, L, rows, dt, (15.0,), (0.1 + 0.05j,))
        data["iq_x_" + c] = x.copy()
        # the reference is well-conditioned here: cos of the estimated angle stays far from 0
        z = x - x.mean()
        mon = np.sum(z.real * z.imag) / np.sum(z.real ** 2)
        assert abs(mon) < 0.5, mon
        y = ref_af.comp_IQ_inbalance(x)
        assert y.dtype == x.dtype and y.shape == x.shape
        data["iq_y_" + c], data["iq_c_" + c] = y, x
        cases["iq"].append(c)
    data["cases"] = np.array(json.dumps(cases))
    path = os.path.join(OUT, "frontend.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
