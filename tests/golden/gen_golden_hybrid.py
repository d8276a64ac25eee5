#!/usr/bin/env python3
"""
Generate tests/golden/hybrid.npz - the reference's PSK signals, a resampled QAM row and time-domain hybrid QAM signals - by IMPORTING THE
REFERENCE.

Run from the repo root with the reference's source tree on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python3 -O tests/golden/gen_golden_hybrid.py

Only data is written.  ``dt`` is c64 or c128 throughout; symbol arrays are stored as uint8 labels into the alphabets stored beside them, and
every label array is checked to give back the reference's values bit for bit before it is written.

PSK, ``SignalPSKGrayCoded(M, 96, nmodes=2, seed=PSK_SEED, dtype=...)`` for M = 2, 4, 8, 16, prefix ``psk<M>_<dt>_``:
    coded      ``coded_symbols``
    bits       ``sig.bits`` (2, 96 log2 M) bool (the same for both dtypes, stored once as ``psk<M>_bits``)
    labels     the signal as labels into ``coded`` (stored once as ``psk<M>_labels``)

Hybrid signals, ``TDHQAMSymbols(M, N, fr=fr, nmodes=nm, seed=TDH_SEED + k, dtype=...)`` for the rows ``k`` of ``tdh_cases`` = (M1, M2, N) with
``tdh_fr[k]``, at nm = 1 and 2, prefix ``t<k>_n<nm>_``:
    <dt>_coded1, <dt>_coded2    the parts' ``coded_symbols``
    <dt>_scaled2                what ``symbols_M2`` holds for every label: ``coded2`` after the reference's in-place division
    <dt>_powratio               ``sig.powratio``
    geometry                    (f_M, f_M1, f_M2)
    part1, part2                ``symbols_M1`` as labels into coded1, ``symbols_M2`` as labels into scaled2 (the same for both dtypes)
    frame                       the signal as labels into ``concatenate([coded1, scaled2])``
``tfs_``: ``from_symbol_arrays`` of two parts that fit exactly (16-QAM, 70 symbols, seed 11; 4-QAM, 30 symbols, seed 12; fr = 0.3; 2 modes);
``tpsk_``: ``TDHQAMSymbols((16, 4), 40, fr=0.25, M2class=SignalPSKGrayCoded, nmodes=1, seed=5)``.  Same keys.

Resampling, ``ResampledQAM(16, 128, fb=1, fs=2, resamplekwargs=dict(beta=0.1, taps=RS_TAPS), nmodes=2, seed=RS_SEED, dtype=...)``:
    rs_labels, rs_<dt>_coded    the symbols (``sig.symbols``) as labels, and the alphabet
    rs_<dt>_out                 the signal (2, 256)
    rs_params                   (fb, fs, beta, taps)
"""
import os
import warnings

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import signals as ref_signals                                     # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
DT = {"c64": np.complex64, "c128": np.complex128}
PSK_SEED, TDH_SEED, RS_SEED, RS_TAPS = 21, 100, 3, 129
TDH_CASES = ((16, 4, 4130), (64, 16, 4098), (4, 16, 4132), (16, 4, 40))
TDH_FR = (0.3, 0.5, 0.75, 0.25)


def labels_of(x, coded):
    x = np.asarray(x)
    idx = np.argmin(np.abs(x[..., None] - coded), axis=-1)
    if not np.array_equal(coded[idx], x):                                    # (no assert: this script runs under -O)
        raise RuntimeError("the labels do not give the values back")
    return idx.astype(np.uint8)


def once(arr, key, value):
    """Store ``value`` under ``key``, or check that what both dtypes give is the same."""
    if key in arr and not np.array_equal(arr[key], value):
        raise RuntimeError("%s differs between the dtypes" % key)
    arr[key] = value


def tdh_keys(arr, prefix, sig, dt):
    s1, s2 = sig.symbols_M1, sig.symbols_M2
    coded1, coded2 = np.asarray(s1.coded_symbols), np.asarray(s2.coded_symbols)
    scaled2 = coded2.copy()
    scaled2 /= np.sqrt(sig.powratio)
    arr[prefix + dt + "_coded1"], arr[prefix + dt + "_coded2"], arr[prefix + dt + "_scaled2"] = coded1, coded2, scaled2
    arr[prefix + dt + "_powratio"] = np.float64(sig.powratio)
    once(arr, prefix + "geometry", np.array([sig.f_M, sig.f_M1, sig.f_M2], dtype=np.int64))
    once(arr, prefix + "part1", labels_of(s1, coded1))
    once(arr, prefix + "part2", labels_of(s2, scaled2))
    # (an inner point of coded1 can equal a point of scaled2: every position is looked up in the alphabet of its own format)
    n = np.arange(sig.shape[1])
    first = n % sig.f_M < sig.f_M1
    frame = np.empty(sig.shape, dtype=np.uint8)
    frame[:, first] = labels_of(np.asarray(sig)[:, first], coded1)
    frame[:, ~first] = labels_of(np.asarray(sig)[:, ~first], scaled2) + coded1.size
    once(arr, prefix + "frame", frame)


def main():
    warnings.simplefilter("ignore")
    arr = {"tdh_cases": np.array(TDH_CASES, dtype=np.int64), "tdh_fr": np.array(TDH_FR), "tdh_seed": np.int64(TDH_SEED), "psk_seed": np.int64(PSK_SEED),
           "rs_params": np.array([1.0, 2.0, 0.1, RS_TAPS]), "rs_seed": np.int64(RS_SEED)}
    for dt, dtype in DT.items():
        for M in (2, 4, 8, 16):
            sig = ref_signals.SignalPSKGrayCoded(M, 96, nmodes=2, seed=PSK_SEED, dtype=dtype)
            coded = np.asarray(sig.coded_symbols)
            arr["psk%d_%s_coded" % (M, dt)] = coded
            once(arr, "psk%d_bits" % M, np.asarray(sig.bits).astype(bool))
            once(arr, "psk%d_labels" % M, labels_of(sig, coded))
        for k, ((M1, M2, N), fr) in enumerate(zip(TDH_CASES, TDH_FR)):
            for nm in (1, 2):
                sig = ref_signals.TDHQAMSymbols((M1, M2), N, fr=fr, nmodes=nm, seed=TDH_SEED + k, dtype=dtype)
                if sig.shape != (nm, N):
                    raise RuntimeError("case %d was truncated" % k)
                tdh_keys(arr, "t%d_n%d_" % (k, nm), sig, dt)
        s1 = ref_signals.SignalQAMGrayCoded(16, 70, nmodes=2, seed=11, dtype=dtype)
        s2 = ref_signals.SignalQAMGrayCoded(4, 30, nmodes=2, seed=12, dtype=dtype)
        tdh_keys(arr, "tfs_", ref_signals.TDHQAMSymbols.from_symbol_arrays(s1, s2, 0.3), dt)
        tdh_keys(arr, "tpsk_", ref_signals.TDHQAMSymbols((16, 4), 40, fr=0.25, M2class=ref_signals.SignalPSKGrayCoded, nmodes=1, seed=5, dtype=dtype), dt)
        rs = ref_signals.ResampledQAM(16, 128, fb=1, fs=2, resamplekwargs=dict(beta=0.1, taps=RS_TAPS), nmodes=2, seed=RS_SEED, dtype=dtype)
        coded = np.asarray(rs.coded_symbols)
        arr["rs_%s_coded" % dt], arr["rs_%s_out" % dt] = coded, np.asarray(rs)
        once(arr, "rs_labels", labels_of(rs.symbols, coded))
        if rs.shape != (2, 256) or rs.fs != 2 or rs.fb != 1:
            raise RuntimeError("unexpected resampled signal")
    path = os.path.join(OUT, "hybrid.npz")
    np.savez_compressed(path, **arr)
    print("wrote %s (%d bytes, %d keys)" % (path, os.path.getsize(path), len(arr)))


if __name__ == "__main__":
    main()
