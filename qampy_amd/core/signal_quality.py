"""
Signal-quality helpers of ``qampy.core.signal_quality`` (qampy/core/signal_quality.py:46-74, :122-335) on top of the metric kernels
of :mod:`qampy_amd.core.hip_dsp` (the soft demapper, ``estimate_snr`` and the MI estimators live there, under the names the
reference imports from its compiled module), and the blind estimators that need no transmitted symbols.
"""
import numpy as np

from .. import _lib
from . import hip_dsp as _dsp
from .hip_dsp import soft_l_value_demapper, soft_l_value_demapper_minmax, estimate_snr, cal_mi_mc, cal_mi_mc_fast  # noqa: F401


# ------------------------------------------------------------------------------------------------ blind estimators
# qampy/core/signal_quality.py:122-271.  ``method="pyt"`` (default): the reference's expressions in numpy on the host; ``method="hip"``: one
# upload, then the kernels of csrc/blind.hip (hip_dsp.blind_*_dev).  A 1-d signal gives a scalar as in the reference; a 2-d (nmodes, L)
# signal one value per row (the reference pools the rows into one SNR and fails on the blind EVM: INTEGRATION.md).
def _method(method):
    if method not in ("pyt", "hip"):
        raise ValueError("method must be 'pyt' (host) or 'hip' (device), not %r" % (method,))
    return method == "hip"


def _blind_rows(E, what):
    """``(is 1-d, rows)`` of a complex signal; complex64 stays, any other complex type runs as complex128."""
    x = np.asarray(E)
    if x.ndim not in (1, 2) or x.size == 0:
        raise ValueError("%s: a non-empty 1-d row or 2-d (nmodes, L) stack of rows" % what)
    if not np.iscomplexobj(x):
        raise TypeError("%s: the signal must be complex" % what)
    if x.dtype != np.complex64:
        x = x.astype(np.complex128, copy=False)
    return x.ndim == 1, np.atleast_2d(x)


def _per_row(one, values):
    values = np.asarray(values, dtype=np.float64)
    return values[0] if one else values


def _cal_gamma(M):
    """Calculate the gamma factor for SNR estimation (signal_quality.py:227-231)."""
    return np.float64(_dsp.cal_gamma(M))


def _host_stats(row, M):
    """``(r2, S1, S2)`` of one row as the reference forms them (signal_quality.py:218-223)."""
    with np.errstate(all="ignore"):
        r2 = np.mean(abs(row) ** 2)
        r4 = np.mean(abs(row) ** 4)
    S1, S2 = _dsp.stats_from_moments(r2, r4, _cal_gamma(M))[:2]
    return r2, S1, S2


def _dev_stats(rows, M):
    """The rows uploaded once and their device stats ``(nrows, 6)`` on the host."""
    _dsp.blind._blind_M("blind signal quality", M)
    dE = _lib.DeviceArray.from_host(np.ascontiguousarray(rows))
    stats = _dsp.blind_stats_dev(dE, M)
    return dE, stats, stats.to_host().reshape(rows.shape[0], 6)


def cal_snr_qam(E, M, method="pyt"):
    """Linear SNR of an M-QAM signal from its second and fourth moments (Gao and Tepedelenlioglu, IEEE Trans. Signal Process. 53, 865 (2005);
    signal_quality.py:196-224)."""
    hip = _method(method)
    one, rows = _blind_rows(E, "cal_snr_qam")
    if hip:
        return _per_row(one, _dev_stats(rows, M)[2][:, 4])
    with np.errstate(all="ignore"):
        return _per_row(one, [S1 / S2 for _, S1, S2 in (_host_stats(r, M) for r in rows)])


def cal_s0(E, M, method="pyt"):
    """Signal power of an M-QAM signal by the same estimator: ``r2 / (1 + S2 / S1)`` (signal_quality.py:234-258)."""
    hip = _method(method)
    one, rows = _blind_rows(E, "cal_s0")
    if hip:
        return _per_row(one, _dev_stats(rows, M)[2][:, 5])
    with np.errstate(all="ignore"):
        return _per_row(one, [r2 / (1 + S2 / S1) for r2, S1, S2 in (_host_stats(r, M) for r in rows)])


def norm_to_s0(sig, M, method="pyt"):
    """The signal divided by the root of its estimated signal power, row by row (signal_quality.py:122-139)."""
    hip = _method(method)
    one, rows = _blind_rows(sig, "norm_to_s0")
    if hip:
        dE, stats, _ = _dev_stats(rows, M)
        out = _dsp.norm_to_s0_dev(dE, M, dE, stats=stats).to_host()
    else:
        with np.errstate(all="ignore"):
            out = np.array([r / np.sqrt(cal_s0(r, M)) for r in rows])
    return out[0] if one else out


def cal_evm(sig, M, known=None, method="pyt"):
    """Linear error vector magnitude of an M-QAM signal normalised to its estimated signal power: against the nearest point of the equally
    normalised ideal alphabet, or against the error-free symbols ``known`` (signal_quality.py:142-193).  Symbol errors are not considered."""
    hip = _method(method)
    one, rows = _blind_rows(sig, "cal_evm")
    if known is not None:
        kone, krows = _blind_rows(known, "cal_evm")
        if krows.shape != rows.shape:
            raise ValueError("cal_evm: known must have the signal's shape")
        krows = krows.astype(rows.dtype, copy=False)
    if hip:
        dE, stats, _ = _dev_stats(rows, M)
        dK = None if known is None else _lib.DeviceArray.from_host(np.ascontiguousarray(krows))
        return _per_row(one, _dsp.blind_evm_dev(dE, M, known=dK, stats=stats))
    out = []
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            Ps = norm_to_s0(r, M)
            if known is None:
                Pi = _dsp.blind_ideal(M)[0]
                evm = np.mean(np.min(abs(Ps[:, np.newaxis].real - Pi.real) ** 2 + abs(Ps[:, np.newaxis].imag - Pi.imag) ** 2, axis=1))
            else:
                Pi = norm_to_s0(krows[i], M)
                evm = np.mean(abs(Pi.real - Ps.real) ** 2 + abs(Pi.imag - Ps.imag) ** 2)
            out.append(np.sqrt(evm / np.mean(abs(Pi) ** 2)))
    return _per_row(one, out)


def cal_snr_blind_qpsk(E, method="pyt"):
    """SNR in dB of a QPSK signal from the spread of its fourth-power-folded constellation, assuming no symbol errors
    (signal_quality.py:261-271)."""
    hip = _method(method)
    one, rows = _blind_rows(E, "cal_snr_blind_qpsk")
    if hip:
        dE = _lib.DeviceArray.from_host(np.ascontiguousarray(rows))
        return _per_row(one, _dsp.qpsk_blind_snr_dev(dE).to_host().reshape(rows.shape[0], 3)[:, 2])
    out = []
    with np.errstate(all="ignore"):
        for r in rows:
            Eref = (-r ** 4) ** (1. / 4)
            P = np.mean(Eref.real ** 2 + Eref.imag ** 2)
            out.append(10 * np.log10(P / np.var(Eref)))
    return _per_row(one, out)


def make_decision(signal, symbols, method="pyt", **kwargs):
    """Every sample of the 1-d ``signal`` quantised onto the nearest of ``symbols`` (signal_quality.py:46-74; the decision runs on the device
    for either ``method`` name of the reference)."""
    from .equalisation import hip_equalisation as _hk
    if method not in ("pyt", "pyx", "hip"):
        raise ValueError("method '%s' unknown" % method)
    signal = np.asarray(signal)
    return _hk.make_decision(np.ascontiguousarray(signal), np.ascontiguousarray(symbols, dtype=signal.dtype))[0]


def cal_ser_qam(data_rx, symbol_tx, M, method="pyt"):
    """Symbol error rate of the 1-d ``data_rx`` decided onto the unit-power M-QAM alphabet against ``symbol_tx`` (signal_quality.py:274-296,
    which hands ``M`` to the decision where the alphabet belongs; this is its evident intent)."""
    from .. import theory
    data_demod = make_decision(data_rx, theory.normalised_symbols_qam(M), method=method)
    return np.count_nonzero(data_demod - symbol_tx) / len(data_rx)


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
