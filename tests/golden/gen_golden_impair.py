#!/usr/bin/env python3
"""
Generate tests/golden/impair.npz - the reference's deterministic channel impairments - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_impair.py

Inputs: two-mode 16-QAM fields of tests/impair_ref.py qam_field (2 samples per symbol, roll-off 0.1, multiples of 2^-12), stored as int16
(re, im) pairs; the sampling rate is 40 GS/s throughout.  Outputs are the reference's results on the complex128 field.

Keys:
    x_4096, x_12388, x_2048      inputs (2, L, 2) int16; value = x / scale
    theta, fs                    pi / 5.6, 40e9
    pmd_4096_30                  apply_PMD_to_field(x_4096, theta, 30 ps, fs)
    pmd_12388_30                 the same of x_12388
    pmd_12388_200                the same at 200 ps, columns cols_200 only (the row ends and the block boundaries; the file stays small)
    rot                          rotate_field(x_4096[:, :512], theta)
    fo_pos, fo_neg               add_carrier_offset(x_4096[:, :512], fo, fs) for fo = fo_values[0] (positive), fo_values[1] (negative)
    delay                        add_modal_delay(x_4096[:, :512], [3, -5])
    sim                          simulate_transmission(x_2048, fb, fs, freq_off=sim_fo, modal_delay=[3, -5], dgd=30 ps, theta=theta)
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import impairments as ref                                     # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import impair_ref                                                             # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SCALE = 4096
FS, THETA = 40e9, np.pi / 5.6


def main():
    data = {"scale": np.float64(SCALE), "fs": np.float64(FS), "theta": np.float64(THETA)}
    x = {}
    for i, L in enumerate((4096, 12388, 2048)):
        x[L] = impair_ref.qam_field(16, 2, L // 2, 2, 0.1, 40 + i)
        q = np.round(np.stack([x[L].real, x[L].imag], -1) * SCALE)
        assert np.abs(q).max() < 32767 and np.array_equal(q / SCALE, np.stack([x[L].real, x[L].imag], -1))
        data["x_%d" % L] = q.astype(np.int16)
    data["pmd_4096_30"] = ref.apply_PMD_to_field(x[4096], THETA, 30e-12, FS)
    data["pmd_12388_30"] = ref.apply_PMD_to_field(x[12388], THETA, 30e-12, FS)
    cols = np.concatenate([np.arange(0, 1024), np.arange(4096 - 512, 4096 + 512), np.arange(8192 - 512, 8192 + 512), np.arange(12388 - 1024, 12388)])
    data["cols_200"] = cols
    data["pmd_12388_200"] = ref.apply_PMD_to_field(x[12388], THETA, 200e-12, FS)[:, cols]
    s = np.ascontiguousarray(x[4096][:, :512])
    data["rot"] = ref.rotate_field(s, THETA)
    fo = np.array([37.3e6, -1.234e9])
    data["fo_values"] = fo
    data["fo_pos"] = ref.add_carrier_offset(s, fo[0], FS)
    data["fo_neg"] = ref.add_carrier_offset(s, fo[1], FS)
    data["delay"] = ref.add_modal_delay(s, [3, -5])
    data["sim_fo"] = np.float64(211e6)
    data["sim"] = ref.simulate_transmission(x[2048], FS / 2, FS, freq_off=211e6, modal_delay=[3, -5], dgd=30e-12, theta=THETA)
    for k, v in data.items():
        assert np.all(np.isfinite(v)), k
    path = os.path.join(OUT, "impair.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
