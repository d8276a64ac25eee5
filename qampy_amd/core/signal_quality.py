"""
Signal-quality helpers of ``qampy.core.signal_quality`` (qampy/core/signal_quality.py:298-335) on top of the metric kernels
of :mod:`qampy_amd.core.hip_dsp` (the soft demapper, ``estimate_snr`` and the MI estimators live there, under the names the
reference imports from its compiled module).
"""
import numpy as np

from .hip_dsp import soft_l_value_demapper, soft_l_value_demapper_minmax, estimate_snr, cal_mi_mc, cal_mi_mc_fast  # noqa: F401


def generate_bitmapping_mtx(coded_symbs, coded_bits, M, dtype=np.complex128):
    """``(nbits, M/2, 2)``: ``[k, :, 0]`` the points whose bit ``k`` is 0, ``[k, :, 1]`` those whose bit ``k`` is 1, each in
    alphabet order.  ``coded_bits``: the ``M * nbits`` bits of ``coded_symbs`` (booleans, MSB first per symbol)."""
    nbits = int(np.log2(M))
    bits = np.reshape(np.asarray(coded_bits), (M, nbits)).astype(bool)
    points = np.asarray(coded_symbs)
    out = np.zeros((nbits, M // 2, 2), dtype=dtype)
    for k in range(nbits):
        out[k, :, 0] = points[~bits[:, k]]
        out[k, :, 1] = points[bits[:, k]]
    return out


def cal_mi(signal, symbols_tx, alphabet, N0, fast=True):
    """Mutual information of one received row against its transmitted symbols at noise power ``N0`` (linear).  ``fast``:
    from the received / transmitted pairs; else from the noise ``signal - symbols_tx`` averaged over every point."""
    if fast:
        return cal_mi_mc_fast(signal, symbols_tx, alphabet, N0)
    return cal_mi_mc(np.asarray(signal) - np.asarray(symbols_tx), alphabet, N0)
