#!/usr/bin/env python3
"""
Generate tests/golden/resample.npz - the reference's resampling and pulse-shaping outputs - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_resample.py

Inputs: unit-power complex noise rows (tests/resample_ref.py unit_noise), rounded to multiples of 2^-10 and stored as int16 (re, im)
pairs, so that complex64 and complex128 hold the same values.  Ts = 1 / 28e9; the input rate is 80e9 and the output rate 80e9 up / down.
Outputs are complex128.

Keys (``<c>`` = ``<up>_<down>_<n>_<taps>``):
    x_<n>                input row of length n
    rrc_<c>_fft          rrcos_resample(x, fold, fnew, Ts, beta=0.1, taps, fftconv=True)
    rrc_<c>_poly         the same with fftconv=False
    taps_<c>             the taps the reference hands to resample_poly for that case (rrcos_time, divided by their maximum)
    rrcb1_7_10_1000_401  beta = 1, fftconv=True;  tapsb1_7_10_1000_401 its taps
    poly_<up>_<down>_<n> resample_poly(x, fold, fnew): scipy's default window
    win_<up>_<down>      that default window (scipy.signal.firwin, before resample_poly scales it by up)
    renorm_7_10_1000_401 rrcos_resample(..., beta=0.1, taps=401, renormalise=True)
    shape_in, shape_out  rrcos_pulseshaping of a (2, 512) array at fs = 56e9, T = 1 / 28e9, beta = 0.1, taps = 101
    sig_in, sig_sym, sig_out   a 2-mode SignalQAMGrayCoded(16, 2048, fb=28e9) (its samples rounded like the inputs), its symbols, and
                         sig.resample(2 * fb, beta=0.1, renormalise=True)
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from scipy import signal as scisig                                          # noqa: E402
from qampy import signals as ref_signals                                    # noqa: E402
from qampy.core import resample as ref_rs                                   # noqa: E402
from qampy.core import filter as ref_filter                                 # noqa: E402
from qampy.core.special_fcts import rrcos_time as ref_rrcos_time            # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import resample_ref                                                         # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FOLD, TS, BETA, SCALE = 80e9, 1 / 28e9, 0.1, 1024
CASES = [(7, 10, 1000, 401), (7, 10, 1000, 400), (7, 10, 1003, 4001), (2, 1, 1000, 401), (28, 25, 997, 255), (1, 1, 512, 101)]


def quantise(x):
    q = np.round(np.stack([x.real, x.imag], -1) * SCALE)
    assert np.abs(q).max() < 32767
    return q.astype(np.int16)


def dequantise(q):
    return (q[..., 0] + 1j * q[..., 1]) / SCALE


def ref_taps(taps, fup, beta):
    t = np.linspace(0, taps, taps, endpoint=False)
    t -= t[(t.size - 1) // 2]
    t /= fup
    h = ref_rrcos_time(t, beta, TS)
    return h / h.max()


def main():
    np.random.seed(5)
    data = {"fold": np.float64(FOLD), "Ts": np.float64(TS), "beta": np.float64(BETA), "scale": np.float64(SCALE)}
    xs = {}
    for j, n in enumerate(sorted({c[2] for c in CASES})):
        data["x_%d" % n] = quantise(resample_ref.unit_noise(1, n, 200 + j)[0])
        xs[n] = dequantise(data["x_%d" % n])
    for up, down, n, taps in CASES:
        fnew = FOLD * up / down
        assert ref_rs._resamplingfactors(FOLD, fnew) == (up, down)
        c = "%d_%d_%d_%d" % (up, down, n, taps)
        data["rrc_%s_fft" % c] = ref_rs.rrcos_resample(xs[n], FOLD, fnew, Ts=TS, beta=BETA, taps=taps, fftconv=True)
        data["rrc_%s_poly" % c] = ref_rs.rrcos_resample(xs[n], FOLD, fnew, Ts=TS, beta=BETA, taps=taps, fftconv=False)
        data["taps_%s" % c] = ref_taps(taps, up * FOLD, BETA)
    data["rrcb1_7_10_1000_401"] = ref_rs.rrcos_resample(xs[1000], FOLD, FOLD * 0.7, Ts=TS, beta=1, taps=401, fftconv=True)
    data["tapsb1_7_10_1000_401"] = ref_taps(401, 7 * FOLD, 1)
    for up, down in ((7, 10), (2, 1)):
        data["poly_%d_%d_1000" % (up, down)] = ref_rs.resample_poly(xs[1000], FOLD, FOLD * up / down)
        mx = max(up, down)
        data["win_%d_%d" % (up, down)] = scisig.firwin(20 * mx + 1, 1 / mx, window=("kaiser", 5.0))
    data["renorm_7_10_1000_401"] = ref_rs.rrcos_resample(xs[1000], FOLD, FOLD * 0.7, Ts=TS, beta=BETA, taps=401, renormalise=True)
    data["shape_in"] = quantise(resample_ref.unit_noise(2, 512, 300))
    data["shape_out"] = ref_filter.rrcos_pulseshaping(dequantise(data["shape_in"]), 56e9, TS, BETA, taps=101)
    sig = ref_signals.SignalQAMGrayCoded(16, 2048, fb=28e9, nmodes=2)
    data["sig_in"] = quantise(np.asarray(sig))
    data["sig_sym"] = np.asarray(sig.symbols)
    sigq = sig.recreate_from_np_array(dequantise(data["sig_in"]))
    out = sigq.resample(2 * sig.fb, beta=BETA, renormalise=True)
    assert out.fs == 2 * sig.fb and type(out) is type(sig)
    data["sig_out"] = np.asarray(out)
    path = os.path.join(OUT, "resample.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
