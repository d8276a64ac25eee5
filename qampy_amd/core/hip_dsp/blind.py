"""
Blind signal quality: qampy/core/signal_quality.py:122-271 (norm_to_s0, cal_evm, cal_snr_qam, cal_s0, cal_snr_blind_qpsk) on
DeviceArrays; kernels in qampy_amd/csrc/blind.hip.  Nothing here needs the transmitted symbols.
"""
import threading

import numpy as np

from ... import _lib
from ._args import buffer, field, thread_table

BLIND_M_MAX = 1024                 # most alphabet points of the distance search (csrc/blind.hip BL_M_MAX)
BLIND_SLICE = 1024                 # fewest samples a workgroup sums before a row or block is cut (BL_MIN)
BLIND_SLICES = 256                 # most workgroups per row or block (BL_NB)
BLIND_STATS = ("r2", "r4", "S1", "S2", "snr", "s0")


def cal_gamma(M):
    """``mean |a|^4`` of the unit-power M-QAM alphabet, the reference's ``_cal_gamma`` (signal_quality.py:227-231) on the host."""
    from ... import theory
    M = int(M)
    if M < 2:
        raise ValueError("cal_gamma: M must be at least 2")
    A = abs(theory.cal_symbols_qam(M)) / np.sqrt(theory.cal_scaling_factor_qam(M))
    uniq, counts = np.unique(A, return_counts=True)
    return float(np.sum(uniq ** 4 * counts / M))


def stats_from_moments(r2, r4, gamma):
    """``(S1, S2, snr, s0)`` of the moment estimator from ``mean |E|^2`` and ``mean |E|^4`` in host arithmetic (signal_quality.py:218-224,
    :251-258); arrays or scalars."""
    with np.errstate(all="ignore"):
        S1 = 1 - 2 * r2 ** 2 / r4 - np.sqrt((2 - gamma) * (2 * r2 ** 4 / r4 ** 2 - r2 ** 2 / r4))
        S2 = gamma * r2 ** 2 / r4 - 1
        return S1, S2, S1 / S2, r2 / (1 + S2 / S1)


_BLIND_IDEAL = {}


def blind_ideal(M):
    """``(Pi, mean |Pi|^2, gamma)`` of M-QAM on the host in double: the ideal alphabet normalised by its own moment estimate of the signal power,
    ``Pi = ideal / sqrt(cal_s0(ideal, M))`` (signal_quality.py:158-159), kept per M."""
    from ... import theory
    M = int(M)
    if M not in _BLIND_IDEAL:
        gamma = cal_gamma(M)
        ideal = np.asarray(theory.cal_symbols_qam(M), dtype=np.complex128).ravel()
        a2 = abs(ideal) ** 2
        s0 = stats_from_moments(np.mean(a2), np.mean(a2 ** 2), gamma)[3]
        Pi = ideal / np.sqrt(s0)
        _BLIND_IDEAL[M] = (Pi, float(np.mean(abs(Pi) ** 2)), gamma)
    return _BLIND_IDEAL[M]


_BLIND_TABLES = threading.local()


def _blind_alphabet_dev(M, dtype):
    """The device copy of :func:`blind_ideal`'s alphabet in ``dtype``, uploaded once per (M, dtype) and host thread."""
    return thread_table(_BLIND_TABLES, (int(M), np.dtype(dtype).str), lambda: _lib.DeviceArray.from_host(np.ascontiguousarray(blind_ideal(M)[0], dtype=dtype)))


def _blind_field(E, what, name="E"):
    """``(c, rows, L)`` of a row or a stack of at most 65535 rows; a host array is refused."""
    if not hasattr(E, "ptr"):
        raise TypeError("%s: %s must be a complex64 or complex128 DeviceArray" % (what, name))
    return field(E, what, name, ndim=(1, 2), max_rows=65535)


def _blind_block(what, block, L):
    """``(block argument of the library, blocks per row)``; ``block`` None or 0: whole rows."""
    if block is None or block == 0:
        return 0, 1
    if int(block) != block or block < 0:
        raise ValueError("%s: block must be a positive whole number of samples" % what)
    if block > L:
        raise ValueError("%s: block = %d is longer than a row of %d samples" % (what, block, L))
    return int(block), L // int(block)


def _blind_M(what, M):
    if int(M) != M or not 2 <= M <= BLIND_M_MAX:
        raise ValueError("%s: M from 2 to %d" % (what, BLIND_M_MAX))
    return int(M)


def _blind_buf(buf, what, name, shape):
    """A float64 result buffer, made when None; any shape of as many elements passes."""
    return buffer(buf, what, name, shape, np.float64, make=True, by_size=True)


def blind_moments_dev(E, block=None, mom=None):
    """``mean |E|^2, mean |E|^4, mean re, mean im`` of every row of the complex DeviceArray ``E`` ((L,) or (nrows, L)) into the float64 DeviceArray
    ``mom (nrows, 4)`` (made when None) - or, with ``block``, of every whole block of ``block`` samples into ``mom (nrows, L // block, 4)``; a
    shorter tail is left out.  Terms and sums in double, in a fixed order: two calls give the same bits.  Nothing is read back."""
    what = "blind_moments_dev"
    c, rows, L = _blind_field(E, what)
    blk, nblocks = _blind_block(what, block, L)
    mom = _blind_buf(mom, what, "mom", (rows, 4) if not blk else (rows, nblocks, 4))
    _lib.call("qh_blind_moments_%s_dev" % c, E.ptr, rows, L, blk, mom.ptr)
    return mom


def blind_stats_dev(E, M, block=None, stats=None, mom=None):
    """The moment estimator of an M-QAM signal (Gao and Tepedelenlioglu; ``cal_snr_qam`` / ``cal_s0``) per row - or per block - of ``E``: the
    float64 DeviceArray ``stats (nrows, 6)`` / ``(nrows, L // block, 6)`` = ``(r2, r4, S1, S2, snr, s0)`` (:data:`BLIND_STATS`), ``snr`` linear.
    ``stats`` and the intermediate ``mom`` are made when None.  NaN / inf where the formula gives them.  Nothing is read back."""
    what = "blind_stats_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    blk, nblocks = _blind_block(what, block, L)
    shape = (rows,) if not blk else (rows, nblocks)
    stats = _blind_buf(stats, what, "stats", shape + (6,))
    mom = blind_moments_dev(E, block, mom)
    _lib.call("qh_blind_finish_dev", mom.ptr, rows * nblocks, blind_ideal(M)[2], stats.ptr)
    return stats


def _blind_row_stats(what, E, M, stats, rows):
    """``stats``, checked to be the (rows, 6) of :func:`blind_stats_dev` on whole rows; formed here when None."""
    return blind_stats_dev(E, M) if stats is None else buffer(stats, what, "stats", (rows, 6), np.float64)


def norm_to_s0_dev(E, M, out, stats=None):
    """``out = E / sqrt(s0)`` per row, ``s0`` the moment estimate of the signal power read from ``stats`` in HBM (``blind_stats_dev(E, M)``, formed
    here when None): the reference's ``norm_to_s0``.  ``out`` has E's shape and dtype and may be ``E``.  Nothing is read back."""
    what = "norm_to_s0_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    if not hasattr(out, "ptr") or tuple(out.shape) != tuple(E.shape) or np.dtype(out.dtype) != np.dtype(E.dtype):
        raise ValueError("%s: out must have E's shape and dtype" % what)
    stats = _blind_row_stats(what, E, M, stats, rows)
    _lib.call("qh_scale_by_stat_%s_dev" % c, E.ptr, rows, L, stats.ptr, out.ptr)
    return out


def blind_evm_dev(E, M, known=None, stats=None, stats_known=None, evm_sum=None):
    """The reference's ``cal_evm(sig, M, known)`` per row of ``E`` as a host array ``(nrows,)``: the RMS distance of ``E / sqrt(s0)`` to the
    nearest point of the equally normalised ideal M-QAM alphabet, relative to that alphabet's RMS - or, with ``known`` (a DeviceArray of E's
    shape and dtype), to ``known / sqrt(s0(known))``, relative to its RMS.  ``stats`` / ``stats_known``: ``blind_stats_dev`` of E / known when at
    hand; ``evm_sum``: a float64 ``(nrows,)`` work buffer.  Reads back ``nrows`` sums (and the stats of ``known``)."""
    what = "blind_evm_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    if known is not None:
        ck, rk, Lk = _blind_field(known, what, "known")
        if (ck, rk, Lk) != (c, rows, L):
            raise ValueError("%s: known must have E's shape and dtype" % what)
    stats = _blind_row_stats(what, E, M, stats, rows)
    evm_sum = _blind_buf(evm_sum, what, "evm_sum", (rows,))
    if known is None:
        pi2 = blind_ideal(M)[1]
        _lib.call("qh_blind_evm_%s_dev" % c, E.ptr, rows, L, stats.ptr, _blind_alphabet_dev(M, E.dtype).ptr, M, None, None, evm_sum.ptr)
    else:
        stats_known = _blind_row_stats(what, known, M, stats_known, rows)
        _lib.call("qh_blind_evm_%s_dev" % c, E.ptr, rows, L, stats.ptr, None, 0, known.ptr, stats_known.ptr, evm_sum.ptr)
        sk = stats_known.to_host().reshape(rows, 6)
        with np.errstate(all="ignore"):
            pi2 = sk[:, 0] / sk[:, 5]                   # mean |known|^2 / s0(known)
    with np.errstate(all="ignore"):
        return np.sqrt(evm_sum.to_host().reshape(rows) / L / pi2)


def qpsk_blind_snr_dev(E, block=None, out=None):
    """The reference's ``cal_snr_blind_qpsk`` per row - or per block - of ``E``: the float64 DeviceArray ``out (nrows, 3)`` / ``(nrows, L // block,
    3)`` = ``(P, var, 10 log10(P / var))`` with ``Eref = (-E**4)**(1/4)`` on the principal branch, ``P = mean |Eref|^2``, ``var = P - |mean
    Eref|^2``.  Nothing is read back."""
    what = "qpsk_blind_snr_dev"
    c, rows, L = _blind_field(E, what)
    blk, nblocks = _blind_block(what, block, L)
    out = _blind_buf(out, what, "out", (rows, 3) if not blk else (rows, nblocks, 3))
    _lib.call("qh_qpsk_blind_%s_dev" % c, E.ptr, rows, L, blk, out.ptr)
    return out
