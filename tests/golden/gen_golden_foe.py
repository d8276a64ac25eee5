#!/usr/bin/env python3
"""
Generate tests/golden/foe.npz - the reference's frequency-offset estimates and removals - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_foe.py

Inputs: rows of tests/foe_ref.py qam_tone (M-QAM at 25 dB, rotated; multiples of 2^-12), stored as int16 (re, im) pairs.  Cases
``<M>_<os>_<N>_<L>`` for M in {4, 16, 64}, os in {1, 2}, N in {256, 4096} and L below, at and above N; two modes with different offsets at
N = 256, the first of them alone at N = 4096 (the file stays small).

Keys:
    x_<case>      input (nmodes, L, 2) int16; value = x / scale
    f_<case>      the rotation applied to each row, in cycles per sample
    fo_<case>     find_freq_offset(x, os, average_over_modes=False, fft_size=N)   (nmodes, 1) float64
    foavg_<case>  the same with average_over_modes=True
    comp_<case>   comp_freq_offset(x, fo_<case>, os), N = 256 only                 (2, L) complex128
    odd_16_1_3000_2500   fo for fft_size=3000 (rounded up to 4096 by the reference) of the x of case 16_1_4096_2500
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import phaserecovery as ref_pr                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import foe_ref                                                                # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SCALE = 4096


def main():
    data = {"scale": np.float64(SCALE)}
    seed = 0
    for M in (4, 16, 64):
        for osf in (1, 2):
            for N, Ls in ((256, (200, 256, 293)), (4096, (2500, 4096, 4133))):
                for L in Ls:
                    seed += 1
                    # 4 f N is the tone's bin: a whole bin in the lower half for row 0, one in the upper half (a negative offset) for row 1
                    f = np.array([(5 + seed) / (4.0 * N), -(9 + 2 * seed) / (4.0 * N)])
                    f = f[:2 if N == 256 else 1]
                    x = foe_ref.qam_tone(M, f.size, L, f, 100 + seed, os=osf)
                    q = np.round(np.stack([x.real, x.imag], -1) * SCALE)
                    assert np.abs(q).max() < 32767 and np.array_equal(q / SCALE, np.stack([x.real, x.imag], -1))
                    c = "%d_%d_%d_%d" % (M, osf, N, L)
                    data["x_" + c] = q.astype(np.int16)
                    data["f_" + c] = f
                    fo = ref_pr.find_freq_offset(x, osf, average_over_modes=False, fft_size=N)
                    data["fo_" + c] = fo
                    data["foavg_" + c] = ref_pr.find_freq_offset(x, osf, average_over_modes=True, fft_size=N)
                    if N == 256:
                        data["comp_" + c] = ref_pr.comp_freq_offset(x, fo, osf)
                    if c == "16_1_4096_2500":
                        data["odd_16_1_3000_2500"] = ref_pr.find_freq_offset(x, osf, average_over_modes=False, fft_size=3000)
    path = os.path.join(OUT, "foe.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
