#!/usr/bin/env python3
"""
Generate tests/golden/theory.npz - the reference's theory curves - by IMPORTING THE REFERENCE (where its source tree is at hand only).

Run from the repo root like gen_golden_metrics.py, with the reference's source tree on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python3 -O tests/golden/gen_golden_theory.py

Only data is written:
- the closed-form curves on fixed grids: ``ser_qam_<M>``, ``ber_qam_<M>`` (linear SNR grid ``snr_lin``), ``ber_evm_<M>`` (grid ``evm_db``) for
  M = 4, 16, 64, 256, ``ser_psk_<M>`` for M = 4, 8, ``ser_4pam``, ``q_function`` on ``q_x``, ``db2lin`` / ``lin2db`` of the grids;
- ``psk_<M>`` = cal_symbols_psk(M), M = 2, 4, 8, 16;
- ``ps_<M>_<j>_levels`` / ``_px`` = cal_ps_probablts(unit-power M-QAM, nu[j]), M = 16, 64, ``ps_nu`` the two shaping factors;
- per Monte-Carlo case c = (M, ns, snr dB) of ``mc_cases``: ``mc<c>_z``, the draws np.random.seed(c) makes cal_gmi_mc take (re-drawn by the same two
  randn(ns) calls), ``mc<c>_gmi`` = cal_gmi_mc(coded symbols, snr, ns, bit map) under that seed and ``mc<c>_mi`` = cal_mi_mc(z, coded symbols,
  1 / snr); ``coded_<M>`` and ``bitmap_<M>`` are SignalQAMGrayCoded's coded symbols and bit map.
"""
import os
import time

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import helpers as ref_helpers, theory as ref_theory                 # noqa: E402
from qampy.core import pythran_dsp as ref_dsp                                  # noqa: E402
from qampy.core.special_fcts import q_function as ref_q                        # noqa: E402
from qampy.signals import SignalQAMGrayCoded                                   # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MC_CASES = [(4, 64, 6.), (16, 64, 12.), (64, 16, 15.), (256, 4, 22.)]
PS_NU = (0.5, 2.0)


def main():
    t0 = time.time()
    snr_db = np.arange(0., 30.5, 1.5)
    evm_db = np.arange(-30., -4.5, 1.5)
    arr = {"snr_db": snr_db, "snr_lin": ref_helpers.dB2lin(snr_db), "evm_db": evm_db, "q_x": np.linspace(-3, 8, 45)}
    arr["db2lin"], arr["lin2db"] = ref_helpers.dB2lin(evm_db), ref_helpers.lin2dB(arr["snr_lin"])
    arr["q_function"] = ref_q(arr["q_x"])
    for M in (4, 16, 64, 256):
        arr["ser_qam_%d" % M] = ref_theory.ser_vs_es_over_n0_qam(arr["snr_lin"], M)
        arr["ber_qam_%d" % M] = ref_theory.ber_vs_es_over_n0_qam(arr["snr_lin"], M)
        arr["ber_evm_%d" % M] = ref_theory.ber_vs_evm_qam(evm_db, M)
    for M in (4, 8):
        arr["ser_psk_%d" % M] = ref_theory.ser_vs_es_over_n0_psk(arr["snr_lin"], M)
    arr["ser_4pam"] = ref_theory.ser_vs_es_over_n0_4pam(arr["snr_lin"])
    for M in (2, 4, 8, 16):
        arr["psk_%d" % M] = ref_theory.cal_symbols_psk(M)
    arr["ps_nu"] = np.array(PS_NU)
    for M in (16, 64):
        syms = ref_theory.cal_symbols_qam(M) / np.sqrt(ref_theory.cal_scaling_factor_qam(M))
        for j, nu in enumerate(PS_NU):
            arr["ps_%d_%d_levels" % (M, j)], arr["ps_%d_%d_px" % (M, j)] = ref_theory.cal_ps_probablts(syms, nu)
    arr["mc_cases"] = np.array(MC_CASES)
    for c, (M, ns, db) in enumerate(MC_CASES):
        sig = SignalQAMGrayCoded(M, 1000, nmodes=1)
        syms, btx = np.asarray(sig.coded_symbols), np.asarray(sig._bitmap_mtx)
        arr["coded_%d" % M], arr["bitmap_%d" % M] = syms, btx
        snr = 10 ** (db / 10)
        np.random.seed(c)
        z = np.sqrt(1 / snr) * (np.random.randn(ns) + 1j * np.random.randn(ns)) / np.sqrt(2)
        np.random.seed(c)
        arr["mc%d_z" % c], arr["mc%d_gmi" % c] = z, np.float64(ref_dsp.cal_gmi_mc(syms, snr, ns, btx))
        arr["mc%d_mi" % c] = np.float64(ref_dsp.cal_mi_mc(z, syms, 1 / snr))
        print("case %d (M=%d) done (%.1f s)" % (c, M, time.time() - t0), flush=True)
    path = os.path.join(OUT, "theory.npz")
    np.savez_compressed(path, **arr)
    print("wrote theory.npz (%d arrays, %.1f KiB) in %.1f s" % (len(arr), os.path.getsize(path) / 1024, time.time() - t0))


if __name__ == "__main__":
    main()
