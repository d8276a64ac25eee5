#!/usr/bin/env python3
"""
Generate tests/golden/cpr.npz - the reference's Viterbi-Viterbi and QPSK-partition carrier recovery - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_cpr.py

Inputs: rows of tests/cpr_ref.py psk_rows / qam16_rows (multiples of 2^-12), stored as int16 (re, im) pairs.

Keys (``<case>``: the names in cpr_ref.GOLDEN_VV / GOLDEN_P16):
    x_<case>        input (nmodes, L, 2) int16; value = x / scale
    vv_E_<case>     viterbiviterbi(x, N, M)[0], the 2-d call                                   (nmodes, L) complex128
    vv_ph_<case>    the trace of every row: viterbiviterbi(x[r], N, M)[1] for each r           (nmodes, L - N + 1) float64
    vv_phlast_<case> viterbiviterbi(x, N, M)[1], what the 2-d call returns (the last row's)    (L - N + 1,) float64
    p16_E_<case>    phase_partition_16qam(x, Nblock)[0]: the reference's field, which rotates every row by the raw fourth-power
                    angle of the LAST row - kept so that the departure of this repository's field is on record   (nmodes, L) complex128
    p16_ph_<case>   phase_partition_16qam(x, Nblock)[1]                                        (nmodes, L) float64
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import phaserecovery as ref_pr                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cpr_ref                                                                # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SCALE = 4096

VV_CASES, P16_CASES = cpr_ref.GOLDEN_VV, cpr_ref.GOLDEN_P16


def pack(x):
    q = np.round(np.stack([x.real, x.imag], -1) * SCALE)
    assert np.abs(q).max() < 32767 and np.array_equal(q / SCALE, np.stack([x.real, x.imag], -1))
    return q.astype(np.int16)


def main():
    data = {"scale": np.float64(SCALE)}
    for c, M, N, nm, L, seed in VV_CASES:
        x = cpr_ref.psk_rows(M, nm, L, seed, cpr_ref.VV_SNR[M])
        data["x_vv_" + c] = pack(x)
        E, last = ref_pr.viterbiviterbi(x, N, M)
        data["vv_E_" + c], data["vv_phlast_" + c] = E, last
        data["vv_ph_" + c] = np.stack([ref_pr.viterbiviterbi(x[r], N, M)[1] for r in range(nm)])
    for c, Nb, nm, L, seed in P16_CASES:
        x = cpr_ref.qam16_rows(nm, L, seed)
        data["x_p16_" + c] = pack(x)
        E, ph = ref_pr.phase_partition_16qam(x, Nb)
        data["p16_E_" + c], data["p16_ph_" + c] = E, ph
    path = os.path.join(OUT, "cpr.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
