"""
Rational resampling and root-raised-cosine shaping on the GPU (the call surface of qampy/core/resample.py).

With ``up, down = Fraction(fnew / fold).limit_denominator()``, real taps ``h[0..T-1]``, ``half = (T - 1) // 2`` and a row ``x[0..n-1]``
that is zero outside, every function here is one polyphase FIR per row (qh_resample_*, csrc/resample.hip):

    n_out = ceil(n up / down),    y[k] = g sum_m h[k down + half - m up] x[m],    k = 0 .. n_out - 1

``g = up`` is ``scipy.signal.resample_poly(x, up, down, window=h)``; ``g = 1`` is zero insertion, ``fftconvolve(.., 'same')`` and
decimation (the reference's default ``fftconv=True``); ``up = down = 1`` with ``g = 1`` is ``rrcos_pulseshaping``.  1-d and 2-d input:
every row is filtered on its own.  complex64 stays complex64, anything else runs as complex128.  Supported: up, down <= 64 and at most
8191 taps; the library rejects anything else.
"""
import fractions

import numpy as np

from .special_fcts import rrcos_time

MAX_FACTOR, MAX_TAPS = 64, 8191


def _resamplingfactors(fold, fnew):
    ratn = fractions.Fraction(fnew / fold).limit_denominator()
    return ratn.numerator, ratn.denominator


def n_out(n, up, down):
    """Output length of a row of n samples: ceil(n up / down)."""
    return -(-int(n) * int(up) // int(down))


def polyphase_table(h, up):
    """The taps in the order the kernel reads them: ``tab[p, j] = h[p + j up]``, zero-padded to ``J = ceil(T / up)`` columns."""
    h = np.asarray(h, dtype=np.float64).ravel()
    J = -(-h.size // up)
    tab = np.zeros(J * up)
    tab[:h.size] = h
    return np.ascontiguousarray(tab.reshape(J, up).T)


def default_window(up, down):
    """scipy.signal.resample_poly's default filter before its scaling by ``up``: 20 max(up, down) + 1 taps of a sinc with cutoff
    1 / max(up, down) of the upsampled Nyquist frequency under a Kaiser window (beta 5.0), scaled to unit gain at DC."""
    mx = max(int(up), int(down))
    half_len = 10 * mx
    m = np.arange(-half_len, half_len + 1, dtype=np.float64)
    h = np.sinc(m / mx) / mx * np.kaiser(2 * half_len + 1, 5.0)
    return h / h.sum()


def rrcos_taps(taps, fs, T, beta):
    """``taps`` samples of the root-raised-cosine response of symbol period T at the rate fs, centred on sample (taps - 1) // 2 and
    divided by their maximum (what rrcos_pulseshaping and rrcos_resample filter with)."""
    taps = int(taps)
    t = (np.arange(taps, dtype=np.float64) - (taps - 1) // 2) / fs
    h = rrcos_time(t, beta, T)
    return h / h.max()


def _suffix(dtype):
    return "64" if np.dtype(dtype) == np.dtype(np.complex64) else "128"


def _rows(shape):
    shape = tuple(shape)
    return (1, int(shape[0])) if len(shape) == 1 else (int(np.prod(shape[:-1])), int(shape[-1]))


def resample_dev(E, out, h, up, down, gain=1.0):
    """``qh_resample_*_dev`` on DeviceArrays: every row of E (nmodes, L) or (L,) through the polyphase FIR of the host taps ``h`` into
    ``out`` (nmodes, Lout), Lout <= ceil(L up / down): the first Lout outputs of each row.  Out of place; enqueued on the current
    library stream.  The phase table is uploaded when (h, up, dtype) differ from the last call's."""
    from .. import _lib
    ct = np.dtype(E.dtype)
    if ct not in (np.dtype(np.complex64), np.dtype(np.complex128)) or np.dtype(out.dtype) != ct:
        raise TypeError("resample works on complex64 or complex128, out of the same dtype as E")
    nmodes, L = _rows(E.shape)
    nm_out, Lout = _rows(out.shape)
    if nm_out != nmodes:
        raise ValueError("out has %d rows, E has %d" % (nm_out, nmodes))
    h = np.ascontiguousarray(h, dtype=np.float64).ravel()
    _lib.call("qh_resample_c%s_dev" % _suffix(ct), E.ptr, nmodes, L, _lib.ptr(h), h.size, int(up), int(down), float(gain), Lout, out.ptr)
    return out


def row_moments_dev(E, mom=None):
    """Mean re, mean im and mean |.|^2 of every row of the DeviceArray E into the DeviceArray ``mom`` (nmodes, 3) float64 (made when
    None); nothing is read back."""
    from .. import _lib
    nmodes, L = _rows(E.shape)
    if mom is None:
        mom = _lib.DeviceArray((nmodes, 3), np.float64)
    _lib.call("qh_row_moments_c%s_dev" % _suffix(E.dtype), E.ptr, nmodes, L, mom.ptr)
    return mom


def center_scale_dev(X, mom, mom_in=None, power=1.0):
    """In place on the device: every row of X minus its mean, scaled to the mean power of the rows ``mom_in`` describes (the moments of
    another array), or to ``power``.  ``mom``: the moments of X (:func:`row_moments_dev`)."""
    from .. import _lib
    nmodes, L = _rows(X.shape)
    _lib.call("qh_center_scale_c%s_dev" % _suffix(X.dtype), X.ptr, nmodes, L, mom.ptr, None if mom_in is None else mom_in.ptr, float(power))
    return X


def _as_rows(signal):
    x = np.asarray(signal)
    X = np.atleast_2d(x)
    if X.ndim != 2:
        raise ValueError("resampling takes 1-d or 2-d input")
    if X.dtype != np.complex64:
        X = X.astype(np.complex128)
    return x.ndim == 1, np.ascontiguousarray(X)


def _filter_rows(X, h, up, down, gain, renormalise):
    """Rows of the host array X through the device: the FIR (h None: a copy), then the reference's renormalisation
    normalise_and_center(out) * sqrt(mean |in|^2) per row."""
    from .. import _lib
    nm, n = X.shape
    if h is not None and not renormalise:
        out = np.empty((nm, n_out(n, up, down)), dtype=X.dtype)
        h = np.ascontiguousarray(h, dtype=np.float64).ravel()
        _lib.call("qh_resample_c%s" % _suffix(X.dtype), _lib.ptr(X), nm, n, _lib.ptr(h), h.size, int(up), int(down), float(gain), out.shape[1],
                  _lib.ptr(out))
        return out
    if h is None and not renormalise:
        return X.copy()
    E = _lib.DeviceArray.from_host(X)
    mom_in = row_moments_dev(E)
    if h is None:
        out, mom = E, mom_in
    else:
        out = resample_dev(E, _lib.DeviceArray((nm, n_out(n, up, down)), X.dtype), h, up, down, gain)
        mom = row_moments_dev(out)
    center_scale_dev(out, mom, mom_in)
    return out.to_host()


def resample_poly(signal, fold, fnew, window=None, renormalise=False):
    """
    Resample every row of ``signal`` from the rate ``fold`` to ``fnew`` as ``scipy.signal.resample_poly(x, up, down, window=window)``
    does: output length ceil(n up / down).  ``window``: the FIR taps at the rate ``up fold`` (``None``: :func:`default_window`).
    ``renormalise``: centre every output row and give it the mean power of its input row.  Like SciPy, a ratio of 1 returns a copy and
    filters nothing.
    """
    one, X = _as_rows(signal)
    up, down = _resamplingfactors(fold, fnew)
    if up == 1 and down == 1:
        h = None
    else:
        h = default_window(up, down) if window is None else np.asarray(window, dtype=np.float64)
    out = _filter_rows(X, h, up, down, up, renormalise)
    return out[0] if one else out


def rrcos_resample(signal, fold, fnew, Ts=None, beta=None, taps=4001, renormalise=False, fftconv=True):
    """
    Resample with a root-raised-cosine filter: pulse shaping and rate change in one polyphase FIR.

    ``Ts``: symbol period of the filter (default 1 / fold); ``beta``: roll-off in (0, 1] - ``None`` is ``resample_poly(signal, fold, fnew)``
    with its default filter and, as in the reference, without renormalisation; ``taps``: length of the filter at the rate ``up fold``.
    ``fftconv`` selects which of the reference's two paths is reproduced: True (default) zero insertion, 'same' convolution with the
    taps and decimation (unit gain on the taps); False ``scipy.signal.resample_poly`` with the taps as window (gain ``up``, and a copy
    for a ratio of 1).  Both run the same kernel.  ``taps=None``, the reference's whole-row spectral filter, is not implemented.
    """
    if beta is None:
        return resample_poly(signal, fold, fnew)
    if not 0 < beta <= 1:
        raise ValueError("beta needs to be in interval (0,1]")
    if taps is None:
        raise NotImplementedError("taps=None (the whole-row spectral root-raised-cosine filter) is not implemented: give a tap count")
    if Ts is None:
        Ts = 1 / fold
    one, X = _as_rows(signal)
    up, down = _resamplingfactors(fold, fnew)
    if not fftconv and up == 1 and down == 1:
        out = _filter_rows(X, None, 1, 1, 1, renormalise)
    else:
        out = _filter_rows(X, rrcos_taps(taps, up * fold, Ts, beta), up, down, 1 if fftconv else up, renormalise)
    return out[0] if one else out
