#!/usr/bin/env python3
"""
Generate tests/golden/metrics.npz - the reference's signal-quality metrics - by IMPORTING THE REFERENCE (this container only).

Run from the repo root like gen_golden.py, with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_metrics.py

Transmitted symbols come from qampy_amd.synth (the build's own generator), noise from a seeded numpy generator; the
reference signal is SignalQAMGrayCoded.from_symbol_array of those symbols.  The received samples are rounded to multiples of
1 / rx_scale (2^-10), so that complex64 and complex128 hold the same values, and stored compactly as int16 (re, im) * rx_scale:
``*_rxq`` as they are, ``M<M>_s<j>_rxd`` as the difference from the rounded transmitted point (``tests/test_gpu_metrics.py``
puts them back together); transmitted symbols are stored as their labels (uint8).  Only data is written: these inputs and the
reference's outputs (LLRs of the complex64 runs as float32, which holds them to far below the test tolerance).

Per M in {4, 16, 32, 64, 128, 256}, two SNRs, complex64 and complex128 (key prefix ``M<M>_s<j>_<dtype>_``):
est_snr(verbose=True), cal_evm (known and blind), cal_ber, cal_ser, cal_gmi (exact and max-log LLRs), cal_mi (fast; the
slow Monte-Carlo form on the first ``mi_slow_n`` symbols, first SNR only), and the LLR matrices of both demappers on the
first ``nllr`` (128) symbols of mode 0.  Further: ``sync_*`` (a capture with a quarter turn, a cyclic shift and swapped modes,
synced=False) and ``hisnr_*`` (64-QAM at 25 dB: exact LLRs beyond fp32's exp range, finite in the reference).
"""
import os
import time

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import signals as ref_signals                                    # noqa: E402
from qampy.core import pythran_dsp as ref_dsp                               # noqa: E402
from qampy.core import signal_quality as ref_sq                             # noqa: E402

from qampy_amd import synth                                                 # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CT = {"c64": np.complex64, "c128": np.complex128}
NSYM, NLLR, SCALE = 2 ** 12, 128, 1024
SNRS = {4: (8., 14.), 16: (14., 20.), 32: (17., 23.), 64: (19., 25.), 128: (22., 28.), 256: (25., 31.)}


def received(M, snr_db, seed):
    """(tx symbols (2, NSYM) complex128 from synth, rx = tx + complex AWGN at snr_db (per-symbol SNR, unit power))."""
    tx = np.asarray(synth.make_capture(M, NSYM, nmodes=2, os=1, seed=seed, dtype=np.complex128).symbols)
    rng = np.random.default_rng(seed + 1)
    sigma = 10 ** (-snr_db / 20)
    rx = tx + sigma * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape)) / np.sqrt(2)
    return tx, np.round(rx * SCALE) / SCALE


def quantised(rx):
    """int16 (..., 2) holding re, im * SCALE exactly."""
    q = np.stack([rx.real, rx.imag], axis=-1) * SCALE
    assert np.all(np.abs(q) < 2 ** 15) and np.array_equal(q, np.round(q))
    return q.astype(np.int16)


def labels(sig, symbols):
    """Index of the coded point every symbol equals exactly (all of them must be points)."""
    coded = np.asarray(sig.coded_symbols)
    lab = np.argmax(np.asarray(symbols)[..., None] == coded, axis=-1)
    assert np.array_equal(coded[lab], symbols)
    return lab.astype(np.uint8)


def ref_signal(tx, rx, M, ct):
    sig = ref_signals.SignalQAMGrayCoded.from_symbol_array(tx.astype(ct), M=M, dtype=ct)
    return sig, sig.recreate_from_np_array(rx.astype(ct))


def metrics(arr, pre, sig, rx, M, slow_n=0):
    snr, s0, n0 = rx.est_snr(verbose=True)
    arr[pre + "snr"], arr[pre + "s0"], arr[pre + "n0"] = snr, s0, n0
    arr[pre + "evm"] = rx.cal_evm()
    arr[pre + "evm_blind"] = rx.cal_evm(blind=True)
    arr[pre + "ber"] = rx.cal_ber()
    arr[pre + "ser"] = rx.cal_ser()
    arr[pre + "gmi"], arr[pre + "gmi_per_bit"] = rx.cal_gmi()
    arr[pre + "gmi_minmax"], arr[pre + "gmi_per_bit_minmax"] = rx.cal_gmi(llr_minmax=True)
    arr[pre + "mi"] = rx.cal_mi()
    if slow_n:
        tx = np.asarray(sig.symbols)
        arr[pre + "mi_slow"] = np.array([ref_sq.cal_mi(np.asarray(rx)[m, :slow_n], tx[m, :slow_n], sig.coded_symbols, 1 / snr[m], fast=False)
                                         for m in range(2)])
    return snr


def main():
    t0 = time.time()
    arr = {"Ms": np.array(sorted(SNRS)), "nsym": np.int64(NSYM), "nllr": np.int64(NLLR), "rx_scale": np.float64(SCALE)}
    for M, snrs in sorted(SNRS.items()):
        nb = int(np.log2(M))
        slow_n = max(8, 2 ** 16 // (M * M))
        arr["M%d_snr_db" % M] = np.array(snrs)
        arr["M%d_mi_slow_n" % M] = np.int64(slow_n)
        for j, snr_db in enumerate(snrs):
            tx, rx = received(M, snr_db, seed=100 * M + j)
            for dn, ct in CT.items():
                sig, rsig = ref_signal(tx, rx, M, ct)
                if j == 0:
                    coded_bits = sig.demodulate(sig.coded_symbols)
                    arr["M%d_%s_coded" % (M, dn)] = sig.coded_symbols
                    arr["M%d_%s_coded_bits" % (M, dn)] = coded_bits
                    arr["M%d_%s_bitmap" % (M, dn)] = ref_sq.generate_bitmapping_mtx(sig.coded_symbols, coded_bits, M, dtype=ct)
                    arr["M%d_%s_bitmap_sig" % (M, dn)] = sig._bitmap_mtx
                lab = labels(sig, sig.symbols)
                if dn == "c64":
                    arr["M%d_s%d_tx_label" % (M, j)] = lab
                assert np.array_equal(arr["M%d_s%d_tx_label" % (M, j)], lab)
                pre = "M%d_s%d_%s_" % (M, j, dn)
                if dn == "c128":
                    base = np.round(np.asarray(sig.coded_symbols)[lab] * SCALE)
                    arr["M%d_s%d_rxd" % (M, j)] = (quantised(rx) - np.stack([base.real, base.imag], axis=-1)).astype(np.int16)
                snr = metrics(arr, pre, sig, rsig, M, slow_n if j == 0 else 0)
                r0 = np.ascontiguousarray(np.asarray(rsig)[0, :NLLR])
                ft = np.float32 if dn == "c64" else np.float64
                arr[pre + "llr"] = ref_dsp.soft_l_value_demapper(r0, nb, snr[0], sig._bitmap_mtx).astype(ft)
                arr[pre + "llr_minmax"] = ref_dsp.soft_l_value_demapper_minmax(r0, nb, snr[0], sig._bitmap_mtx).astype(ft)
        print("M=%d done (%.1f s)" % (M, time.time() - t0), flush=True)

    # synced=False: quarter turn, cyclic shift, swapped modes
    M, snr_db = 16, 16.
    tx, rx = received(M, snr_db, seed=4242)
    rx_imp = np.roll(rx[::-1] * 1j, 37, axis=-1)
    arr["sync_M"], arr["sync_rxq"] = np.int64(M), quantised(rx_imp)
    for dn, ct in CT.items():
        sig, rsig = ref_signal(tx, rx_imp, M, ct)
        arr["sync_%s_tx_label" % dn] = labels(sig, sig.symbols)
        t_al, r_al = sig._sync_and_adjust(sig.symbols, np.asarray(rsig))
        assert t_al.dtype == r_al.dtype == ct
        arr["sync_%s_tx_aligned_label" % dn], arr["sync_%s_rx_alignedq" % dn] = labels(sig, t_al), quantised(r_al)
        metrics(arr, "sync_%s_" % dn, sig, rsig, M)

    # high SNR: 64-QAM at 25 dB, exact LLRs of the MSBs beyond fp32's exp range
    M, snr_db = 64, 25.
    tx, rx = received(M, snr_db, seed=777)
    arr["hisnr_M"], arr["hisnr_snr_db"], arr["hisnr_rxq"] = np.int64(M), np.float64(snr_db), quantised(rx[0, :NLLR])
    for dn, ct in CT.items():
        sig, rsig = ref_signal(tx, rx, M, ct)
        r0 = np.ascontiguousarray(np.asarray(rsig)[0, :NLLR])
        snr = 10 ** (snr_db / 10)
        ft = np.float32 if dn == "c64" else np.float64
        arr["hisnr_%s_llr" % dn] = ref_dsp.soft_l_value_demapper(r0, 6, snr, sig._bitmap_mtx).astype(ft)
        arr["hisnr_%s_llr_minmax" % dn] = ref_dsp.soft_l_value_demapper_minmax(r0, 6, snr, sig._bitmap_mtx).astype(ft)
    path = os.path.join(OUT, "metrics.npz")
    np.savez_compressed(path, **arr)
    print("wrote metrics.npz (%d arrays, %.1f KiB) in %.1f s" % (len(arr), os.path.getsize(path) / 1024, time.time() - t0))


if __name__ == "__main__":
    main()
