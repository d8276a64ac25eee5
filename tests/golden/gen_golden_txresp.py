#!/usr/bin/env python3
"""
Generate tests/golden/txresp.npz - the reference's transmitter response (DAC, low-pass, amplifier, modulator) - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_txresp.py

Inputs: the two-mode 16-QAM fields of tests/impair_ref.py qam_field (2 samples per symbol, roll-off 0.1, multiples of 2^-12) of lengths
2048 and 12388, stored as int16 (re, im) pairs; the sampling rate is 40 GS/s throughout.  Everything that goes through the quantiser
starts from txresp_ref.exact_quant_field(x): row maxima of exactly 2, so the scaling is exact and the thresholds are dyadic.  This script
asserts that the float32 and float64 restatements (tests/txresp_ref.py) decide every sample of every quantiser fixture identically, that
each has at least one sample exactly on a threshold, and that the float64 restatement decides as the reference does.  Outputs are the
reference's results on the complex128 field; for the length 12388 only the columns ``cols`` are kept (row start, the chunk and tile
boundaries of the filter, row end).

Keys:
    x_2048, x_12388              inputs (2, L, 2) int16; value = x / scale
    cols                         the columns kept of every output of length 12388
    q{b}_{L}                     quantize_signal_New(xq_L, nbits=b), b = 1, 4, 8
    cq{b}_{L}                    sim_DAC_response(xq_L, fs, enob=0, clip_rat=0.8, quant_bits=b)
    clip_{L}                     sim_DAC_response(xq_L, fs, enob=0, clip_rat=0.8)
    filt_{L}                     filter_signal(x_L, fs, 18e9)  (the default DAC filter: Bessel of order 2)
    filt_bessel4, filt_butter6, filt_bessel3, filt_butter8
                                 filter_signal(x_2048, fs, cutoff, ftype, order) for (50 MHz, bessel, 4), (100 MHz, butter, 6), (2 GHz, bessel, 3),
                                 (1 GHz, butter, 8); the first 1024 columns
    mod_ideal, mod_real, mod_amp modulator_response(s) with the defaults; with mod_prms; ideal_amplifier_response(s, 0.7) then the defaults;
                                 s = x_2048[:, :512]
    chain_a_{L}                  sim_tx_response(xq_L, fs, enob=0, tgt_v=0.7, clip_rat=0.8, quant_bits=5) (DAC filter at 18 GHz)
    chain_b_{L}                  sim_tx_response(xq_L, fs, enob=0, tgt_v=0.5, quant_bits=4, dac_params={}, **mod_prms)
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy.core import impairments as ref                                     # noqa: E402
from qampy.core import filter as ref_filter                                   # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import impair_ref                                                             # noqa: E402
import txresp_ref                                                             # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SCALE = 4096
FS = 40e9
MOD = dict(dcbias=1.02 + 0.97j, gfactr=0.95 + 0.9j, cfactr=0.05 - 0.03j, dcbias_out=0.45, gfactr_out=0.9)
COLS = np.concatenate([np.arange(0, 512), np.arange(8192 - 256, 8192 + 256), np.arange(12388 - 512, 12388)])


class Arr(np.ndarray):
    """The least of a signal object that quantize_signal_New asks for."""
    def recreate_from_np_array(self, arr):
        return np.asarray(arr).view(Arr)


def check(cond, what):
    if not cond:
        raise SystemExit("gen_golden_txresp: " + what)


def check_quantiser(xin, nbits, got, what):
    """float32 and float64 decide alike, a sample lies on a threshold, and the float64 restatement is the reference's result"""
    o64, r64, i64, u64 = txresp_ref.quantise(xin, nbits, np.float64)
    o32, r32, i32, _ = txresp_ref.quantise(xin, nbits, np.float32)
    check(np.array_equal(r64, r32) and np.array_equal(i64, i32), "%s: float32 and float64 decide differently" % what)
    check(txresp_ref.on_threshold(u64, nbits) >= 1, "%s: no sample on a threshold" % what)
    check(np.abs(o64 - got).max() <= 1e-15 * np.abs(got).max(), "%s: the restatement is not the reference's result" % what)


def main():
    data = {"scale": np.float64(SCALE), "fs": np.float64(FS), "cols": COLS}
    data.update({"mod_" + k: np.complex128(v) if np.iscomplexobj(v) else np.float64(v) for k, v in MOD.items()})
    x = {}
    for i, L in enumerate((2048, 12388)):
        x[L] = impair_ref.qam_field(16, 2, L // 2, 2, 0.1, 50 + i)
        q = np.round(np.stack([x[L].real, x[L].imag], -1) * SCALE)
        check(np.abs(q).max() < 32767 and np.array_equal(q / SCALE, np.stack([x[L].real, x[L].imag], -1)), "the input is not on the grid")
        data["x_%d" % L] = q.astype(np.int16)

    def keep(a, L):
        a = np.asarray(a, np.complex128)
        return a if L == 2048 else a[:, COLS]

    for L in (2048, 12388):
        xq = txresp_ref.exact_quant_field(x[L])
        check(np.array_equal(txresp_ref.row_max(xq), [2.0, 2.0]), "row maxima of the quantiser's input")
        c64, c32 = txresp_ref.clip(xq, 0.8, np.float64), txresp_ref.clip(xq, 0.8, np.float32)
        check(np.array_equal(c64, c32.astype(np.complex128)), "clip_rat 0.8: float32 and float64 clip differently")
        got = ref.sim_DAC_response(xq.view(Arr), FS, enob=0, clip_rat=0.8)
        check(np.abs(c64 - got).max() <= 1e-15, "clip: the restatement is not the reference's result")
        data["clip_%d" % L] = keep(got, L)
        for b in (1, 3, 4, 5, 6, 8):
            got = ref.quantize_signal_New(xq.view(Arr), nbits=b)
            check_quantiser(xq, b, got, "q%d_%d" % (b, L))
            gotc = ref.sim_DAC_response(xq.view(Arr), FS, enob=0, clip_rat=0.8, quant_bits=b)
            check_quantiser(c64, b, gotc, "cq%d_%d" % (b, L))
            if b in (1, 4, 8):
                data["q%d_%d" % (b, L)] = keep(got, L)
                data["cq%d_%d" % (b, L)] = keep(gotc, L)
        data["filt_%d" % L] = keep(ref_filter.filter_signal(x[L], FS, 18e9), L)
        data["chain_a_%d" % L] = keep(ref.sim_tx_response(xq.view(Arr), FS, enob=0, tgt_v=0.7, clip_rat=0.8, quant_bits=5), L)
        data["chain_b_%d" % L] = keep(ref.sim_tx_response(xq.view(Arr), FS, enob=0, tgt_v=0.5, quant_bits=4, dac_params={}, **MOD), L)
    for name, cutoff, ftype, order in (("bessel4", 50e6, "bessel", 4), ("butter6", 100e6, "butter", 6), ("bessel3", 2e9, "bessel", 3), ("butter8", 1e9, "butter", 8)):
        data["filt_" + name] = np.asarray(ref_filter.filter_signal(x[2048], FS, cutoff, ftype=ftype, order=order))[:, :1024]
    s = np.ascontiguousarray(x[2048][:, :512])
    data["mod_ideal"] = ref.modulator_response(s)
    data["mod_real"] = ref.modulator_response(s, **MOD)
    data["mod_amp"] = ref.modulator_response(ref.ideal_amplifier_response(s, 0.7))
    for k, v in data.items():
        check(np.all(np.isfinite(v)), "%s is not finite" % k)
    path = os.path.join(OUT, "txresp.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    check(os.path.getsize(path) < 1000000, "the file must stay under 1 MB")


if __name__ == "__main__":
    main()
