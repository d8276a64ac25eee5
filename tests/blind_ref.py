"""
Float64 numpy restatement of the blind signal-quality estimators (qampy/core/signal_quality.py:122-271), written from their formulas: what the
device values are compared with where tests/golden/blind.npz has no value (odd lengths, edge rows), and - with ``fsum=True``, every mean an
exactly rounded ``math.fsum`` - the second summation order the complex128 tolerance of the fixture is measured with.
"""
import math

import numpy as np


def _mean(x, fsum):
    x = np.asarray(x, dtype=np.float64)
    return math.fsum(x.tolist()) / x.size if fsum else float(np.mean(x))


def moments(row, fsum=False):
    """``(mean |E|^2, mean |E|^4, mean re, mean im)`` of one row, every term formed in double."""
    z = np.asarray(row).astype(np.complex128)
    p = z.real * z.real + z.imag * z.imag
    return np.array([_mean(p, fsum), _mean(p * p, fsum), _mean(z.real, fsum), _mean(z.imag, fsum)])


def block_moments(row, block, fsum=False):
    """The moments of every whole block of ``block`` samples: ``(len(row) // block, 4)``."""
    row = np.asarray(row)
    n = row.size // block
    return np.array([moments(row[b * block:(b + 1) * block], fsum) for b in range(n)]).reshape(n, 4)


def stats(r2, r4, gamma):
    """``(r2, r4, S1, S2, snr, s0)`` of the moment estimator; NaN / inf where the formula gives them."""
    with np.errstate(all="ignore"):
        r2, r4 = np.float64(r2), np.float64(r4)
        k = r2 * r2 / r4
        S1 = 1 - 2 * k - np.sqrt((2 - gamma) * (2 * k * k - k))
        S2 = gamma * k - 1
        return np.array([r2, r4, S1, S2, S1 / S2, r2 / (1 + S2 / S1)])


def row_stats(row, gamma, fsum=False):
    m = moments(row, fsum)
    return stats(m[0], m[1], gamma)


def gamma_of(alphabet):
    """``mean |a|^4`` of the alphabet scaled to unit power."""
    a2 = abs(np.asarray(alphabet, dtype=np.complex128)) ** 2
    a2 = a2 / a2.mean()
    return float(np.mean(a2 * a2))


def norm_to_s0(row, gamma, fsum=False):
    z = np.asarray(row).astype(np.complex128)
    with np.errstate(all="ignore"):
        return z / np.sqrt(row_stats(z, gamma, fsum)[5])


def evm(row, ideal, gamma, known=None, fsum=False, chunk=1 << 12):
    """``cal_evm``: the RMS distance of the normalised row to the nearest point of the normalised ideal alphabet (or to the normalised known
    symbols) over the RMS of that reference."""
    with np.errstate(all="ignore"):
        Ps = norm_to_s0(row, gamma, fsum)
        if known is None:
            Pi = norm_to_s0(ideal, gamma, fsum)
            d = np.concatenate([np.min((Ps[a:a + chunk, None].real - Pi.real) ** 2 + (Ps[a:a + chunk, None].imag - Pi.imag) ** 2, axis=1)
                                for a in range(0, Ps.size, chunk)])
        else:
            Pi = norm_to_s0(known, gamma, fsum)
            d = (Pi.real - Ps.real) ** 2 + (Pi.imag - Ps.imag) ** 2
        return float(np.sqrt(_mean(d, fsum) / _mean(abs(Pi) ** 2, fsum)))


def qpsk_fold(row):
    """``(-E**4)**(1/4)`` on the principal branch, from the angle."""
    z = np.asarray(row).astype(np.complex128)
    return abs(z) * np.exp(0.25j * np.angle(-z ** 4))


def qpsk_snr(row, fsum=False):
    """``(P, var, 10 log10(P / var))`` of ``cal_snr_blind_qpsk``."""
    e = qpsk_fold(row)
    with np.errstate(all="ignore"):
        P = _mean(e.real ** 2 + e.imag ** 2, fsum)
        mr, mi = _mean(e.real, fsum), _mean(e.imag, fsum)
        var = P - (mr * mr + mi * mi)
        return np.array([P, var, 10 * np.log10(np.float64(P) / np.float64(var))])
