"""
Whole-row transforms and the analog front end: csrc/fft.hip and csrc/iq.hip on DeviceArrays, for qampy/core/analog_frontend.py and
pre_filter / pre_filter_wdm of qampy/core/filter.py.
"""
import numpy as np

from ... import _lib
from ._args import buffer, resident, same_as

FFT_POW2_MIN, FFT_POW2_MAX, FFT_ANY_MAX = 2 ** 8, 2 ** 24, 2 ** 23       # limits of csrc/fft.hip
IQ_TILE = 4096                                                           # samples per workgroup of the moments pass (csrc/iq.hip)
FH_BRICK, FH_BAND, FH_TWORAIL, FH_RAMP, FH_REAL, FH_COMPLEX = 1, 2, 3, 4, 5, 6
IQ_ORTHONORMALIZE, IQ_IMBALANCE, IQ_CENTRE = 0, 1, 2


def fft_length_ok(L):
    """Whether csrc/fft.hip transforms rows of ``L`` samples: a power of two from 2**8 to 2**24, or any other length from 2 to 2**23."""
    L = int(L)
    if L < 2:
        return False
    if L & (L - 1) == 0 and L >= FFT_POW2_MIN:
        return L <= FFT_POW2_MAX
    return L <= FFT_ANY_MAX


def fft_plan(L):
    """``(M, N1, N2, bluestein)`` of a row length: the power-of-two transform size, its four-step split (``N1 = 1``: one workgroup per row)
    and whether the row goes through Bluestein's chirp transform."""
    L = int(L)
    if not fft_length_ok(L):
        raise ValueError("a row of %d samples: the whole-row transform takes a power of two from 2**8 to 2**24, or any other length from 2 to 2**23" % L)
    blue = not (L & (L - 1) == 0 and L >= FFT_POW2_MIN)
    lg = 8
    while (1 << lg) < (2 * L - 1 if blue else L):
        lg += 1
    lg1 = lg // 2 if lg > 13 else 0
    return 1 << lg, 1 << lg1, 1 << (lg - lg1), blue


def _fft_field(E, out, what):
    c = resident(E, what)
    same_as(E, out, what)
    fft_plan(E.shape[1])
    return c


def fft_dev(E, out):
    """``np.fft.fft`` along the last axis of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (same shape and dtype; it may be ``E``),
    csrc/fft.hip.  ``L``: a power of two from 2**8 to 2**24 or any other length from 2 to 2**23; ValueError otherwise, before a launch.
    Nothing is read back; enqueued on the current library stream; a repeated call is bit-identical."""
    c = _fft_field(E, out, "fft_dev")
    _lib.call("qh_fft_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], 0, out.ptr)
    return out


def ifft_dev(E, out):
    """``np.fft.ifft`` along the last axis: see :func:`fft_dev`."""
    c = _fft_field(E, out, "ifft_dev")
    _lib.call("qh_fft_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], 1, out.ptr)
    return out


def _spectral(E, out, what, kind, p0=0.0, p1=0.0, p2=0.0, i0=0, i1=0, H=None):
    c = _fft_field(E, out, what)
    p = [float(v) for v in (p0, p1, p2)]
    if not all(np.isfinite(p)):
        raise ValueError("%s: parameters must be finite" % what)
    _lib.call("qh_spectral_filter_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], kind, p[0], p[1], p[2], int(i0), int(i1), None if H is None else H.ptr, out.ptr)
    return out


def spectral_filter_dev(E, out, H):
    """``ifft(H * fft(E))`` of every row of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (it may be ``E``).  ``H``: an (L,)
    DeviceArray in ``fftfreq`` order, real in the field's real type or complex in the field's dtype."""
    suf, rt, ct = _lib.suffix(E.dtype)
    resident(E, "spectral_filter_dev")
    if tuple(H.shape) != (E.shape[1],):
        raise ValueError("H must hold one value per bin: (%d,)" % E.shape[1])
    if np.dtype(H.dtype) == np.dtype(rt):
        kind = FH_REAL
    elif np.dtype(H.dtype) == np.dtype(ct):
        kind = FH_COMPLEX
    else:
        raise TypeError("H must be %s or %s for a %s field" % (np.dtype(rt).name, np.dtype(ct).name, np.dtype(ct).name))
    return _spectral(E, out, "spectral_filter_dev", kind, H=H)


def pre_filter_bins(L, bw):
    """``(lo, hi)``: the reference's ``h[:, int(L / (bw / 2)):-int(L / (bw / 2))] = 1`` keeps the positions ``lo <= j < hi`` after
    ``fftshift`` (qampy/core/filter.py:44, as written: ``bw`` is no fraction, and an empty slice - ``bw=0.01``, or a count of 0 - keeps
    nothing)."""
    if not (np.isfinite(bw) and bw != 0):
        raise ValueError("bw must be finite and not zero")
    c = L / (bw / 2)
    if not abs(c) < 2.0 ** 62:
        return 0, 0
    c = int(c)
    lo, hi, _ = slice(c, -c).indices(int(L))
    return (lo, hi) if hi > lo else (0, 0)


def pre_filter_dev(E, out, bw):
    """The brick-wall ``pre_filter(signal, bw)`` of qampy/core/filter.py:28-49 on every row of the (nmodes, L) complex DeviceArray ``E``, into
    ``out`` (it may be ``E``): see :func:`pre_filter_bins` for the bins that survive."""
    resident(E, "pre_filter_dev")
    fft_plan(E.shape[1])
    lo, hi = pre_filter_bins(E.shape[1], float(bw))
    return _spectral(E, out, "pre_filter_dev", FH_BRICK, i0=lo, i1=hi)


def pre_filter_wdm_dev(E, out, bw, os, center_freq=0):
    """Band selection on every row: keep the bins where ``abs(fftfreq(L, 1 / os) - center_freq) < bw / 2`` (``pre_filter_wdm`` of
    qampy/core/filter.py:51-84, restated for rows along the last axis)."""
    resident(E, "pre_filter_wdm_dev")
    fft_plan(E.shape[1])
    if not (np.isfinite(os) and os > 0):
        raise ValueError("os must be positive")
    L = E.shape[1]
    val = 1.0 / (L * (1 / os))                                           # numpy's fftfreq: k * (1 / (n d))
    return _spectral(E, out, "pre_filter_wdm_dev", FH_BAND, p0=val, p1=center_freq, p2=bw / 2)


def _skew_step(L, sampling_rate):
    if not (np.isfinite(sampling_rate) and sampling_rate > 0):
        raise ValueError("sampling_rate must be positive")
    return 1.0 / (L * (sampling_rate / 2))                               # fftfreq(L, sampling_rate / 2), the reference's grid as written


def skew_dev(E, out, delay_i, delay_q, sampling_rate):
    """Delay the rails of every row of the (nmodes, L) complex DeviceArray ``E`` separately: ``out = comp_rf_delay(E.real, delay_i,
    sampling_rate) + 1j * comp_rf_delay(E.imag, delay_q, sampling_rate)`` (qampy/core/analog_frontend.py:54-88, its frequency grid
    ``fftfreq(L, sampling_rate / 2)`` as written), one forward and one inverse transform for both rails.  ``out`` may be ``E``."""
    resident(E, "skew_dev")
    fft_plan(E.shape[1])
    return _spectral(E, out, "skew_dev", FH_TWORAIL, p0=_skew_step(E.shape[1], sampling_rate), p1=delay_i, p2=delay_q)


def delay_dev(E, out, delay, sampling_rate):
    """``ifft(exp(-2j pi delay f) * fft(E))`` with ``f = fftfreq(L, sampling_rate / 2)``: the complex output of ``comp_rf_delay`` before its
    real part is taken."""
    resident(E, "delay_dev")
    fft_plan(E.shape[1])
    return _spectral(E, out, "delay_dev", FH_RAMP, p0=_skew_step(E.shape[1], sampling_rate), p1=delay)


def _iq_field(E, what, os=1):
    c = resident(E, what)
    if int(os) != os or int(os) < 1:
        raise ValueError("os must be a positive integer")
    if E.shape[1] < 1:
        raise ValueError("%s needs at least one sample" % what)
    return c


def iq_moments_dev(E, os=1, mom=None):
    """Per row of the (nmodes, L) complex DeviceArray ``E``: sum I, sum Q, sum I**2, sum Q**2, sum I Q over all samples and the same five
    over ``E[:, ::os]``, in double, into ``mom`` (nmodes, 10) float64 (allocated if None; returned).  Two launches, bit-reproducible."""
    c = _iq_field(E, "iq_moments_dev", os)
    mom = buffer(mom, "iq_moments_dev", "mom", (E.shape[0], 10), np.float64, make=True)
    _lib.call("qh_iq_moments_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], int(os), mom.ptr)
    return mom


def iq_coeffs_dev(mom, L, os, kind, coef=None):
    """The coefficients ``(a00, a01, a10, a11, b0, b1)`` per row of ``y = A (I, Q)^T + b`` from the moments of :func:`iq_moments_dev`, formed on
    the device: ``kind`` IQ_ORTHONORMALIZE, IQ_IMBALANCE (pooled over the rows) or IQ_CENTRE."""
    if len(mom.shape) != 2 or mom.shape[1] != 10 or np.dtype(mom.dtype) != np.dtype(np.float64):
        raise ValueError("mom must be an (nmodes, 10) float64 DeviceArray")
    if kind not in (IQ_ORTHONORMALIZE, IQ_IMBALANCE, IQ_CENTRE):
        raise ValueError("unknown kind")
    coef = buffer(coef, "iq_coeffs_dev", "coef", (mom.shape[0], 6), np.float64, make=True)
    _lib.call("qh_iq_coeffs_dev", mom.ptr, mom.shape[0], int(L), int(os), kind, coef.ptr)
    return coef


def iq_affine_dev(E, out, coef):
    """``out = A (E.real, E.imag)^T + b`` per row, evaluated in double; ``out`` may be ``E``."""
    c = _iq_field(E, "iq_affine_dev")
    same_as(E, out, "iq_affine_dev")
    buffer(coef, "iq_affine_dev", "coef", (E.shape[0], 6), np.float64)
    _lib.call("qh_iq_affine_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], coef.ptr, out.ptr)
    return out


def orthonormalize_dev(E, out, os=1, mom=None, coef=None):
    """``orthonormalize_signal(E, os)`` (qampy/core/analog_frontend.py:91-132) of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (it may
    be ``E``): one moments pass, the closed-form map, one affine pass; nothing is read back."""
    _iq_field(E, "orthonormalize_dev", os)
    same_as(E, out, "orthonormalize_dev")
    mom = iq_moments_dev(E, os, mom)
    coef = iq_coeffs_dev(mom, E.shape[1], os, IQ_ORTHONORMALIZE, coef)
    return iq_affine_dev(E, out, coef)


def comp_iq_imbalance_dev(E, out, mom=None, coef=None):
    """``comp_IQ_inbalance(E)`` (qampy/core/analog_frontend.py:30-52) into ``out``, which must not be ``E``: mean, sum I Q and sum I**2 pooled
    over the whole array as the reference pools them, and ``E`` itself centred in place as the reference centres its argument."""
    _iq_field(E, "comp_iq_imbalance_dev")
    same_as(E, out, "comp_iq_imbalance_dev")
    if out.ptr == E.ptr:
        raise ValueError("comp_iq_imbalance_dev centres E in place: out must be another buffer")
    mom = iq_moments_dev(E, 1, mom)
    coef = iq_coeffs_dev(mom, E.shape[1], 1, IQ_IMBALANCE, coef)
    iq_affine_dev(E, out, coef)
    iq_affine_dev(E, E, iq_coeffs_dev(mom, E.shape[1], 1, IQ_CENTRE, coef))
    return out
