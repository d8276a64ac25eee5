"""DSP-based compensation of analog impairments ahead of the ADC (qampy/core/analog_frontend.py) on plain ndarrays, through the GPU's
kernels: csrc/iq.hip for the two IQ conditioners, csrc/fft.hip for the delay.  1-d or 2-d input, rows along the last axis; output shapes
and dtypes are the reference's."""
import numpy as np

from . import hip_dsp as _dsp


def _complex_rows(signal, what):
    x = np.asarray(signal)
    if x.ndim not in (1, 2):
        raise ValueError("%s works on 1-d or 2-d arrays" % what)
    if x.dtype not in (np.complex64, np.complex128):
        raise TypeError("%s works on complex64 or complex128 arrays" % what)
    if x.size == 0:
        raise ValueError("%s needs at least one sample" % what)
    return np.ascontiguousarray(np.atleast_2d(x)), x.ndim == 1


def comp_IQ_inbalance(signal):
    """Compensate the imbalance between I and Q of an optical hybrid: I is kept, Q is made orthogonal to it and scaled to its power
    (qampy/core/analog_frontend.py:30-52).  As in the reference, the mean and the sums are pooled over the whole array - across the rows
    of a 2-d input - and ``signal`` itself is centred in place.  Returns an array of ``signal``'s shape and dtype."""
    from .. import _lib
    if not isinstance(signal, np.ndarray):
        raise TypeError("comp_IQ_inbalance centres its argument in place: give an ndarray")
    X, one = _complex_rows(signal, "comp_IQ_inbalance")
    E = _lib.DeviceArray.from_host(X)
    out = _lib.DeviceArray(X.shape, X.dtype)
    _dsp.comp_iq_imbalance_dev(E, out)
    res, centred = out.to_host(), E.to_host()
    signal[...] = centred[0] if one else centred
    return res[0] if one else res


def comp_rf_delay(signal, delay, sampling_rate=50e9):
    """Delay ``signal`` by ``delay`` seconds in the frequency domain and keep the real part (qampy/core/analog_frontend.py:54-88): the phase
    ramp lives on the reference's grid ``fftfreq(L, sampling_rate / 2)``, as written.  The computation is complex128 and the result float64,
    as with ``np.fft``; 1-d input gives 1-d output.

    A real ``signal`` is rail I of the two-rail multiply (:func:`qampy_amd.core.hip_dsp.skew_dev`) with ``delay_q = 0``; a complex one goes
    through the plain ramp (:func:`qampy_amd.core.hip_dsp.delay_dev`), whose real part the reference returns."""
    from .. import _lib
    x = np.asarray(signal)
    if x.ndim not in (1, 2):
        raise ValueError("comp_rf_delay works on 1-d or 2-d arrays")
    if not np.isfinite(delay):
        raise ValueError("delay must be finite")
    X = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex128)
    _dsp.fft_plan(X.shape[1])
    E = _lib.DeviceArray.from_host(X)
    if np.iscomplexobj(x):
        _dsp.delay_dev(E, E, delay, sampling_rate)
    else:
        _dsp.skew_dev(E, E, delay, 0.0, sampling_rate)
    res = np.ascontiguousarray(E.to_host().real)
    return res if x.ndim > 1 else res.flatten()


def orthonormalize_signal(E, os=1):
    """Orthonormalise I and Q of every row by the Gram-Schmidt process (qampy/core/analog_frontend.py:91-132): centre, take the in-phase
    part out of the quadrature, centre on ``E[:, ::os]`` and scale its mean power to 1.  Always 2-d, like the reference: a 1-d input comes
    back as (1, L); the dtype is kept."""
    from .. import _lib
    X, _ = _complex_rows(E, "orthonormalize_signal")
    if int(os) != os or int(os) < 1:
        raise ValueError("os must be a positive integer")
    d = _lib.DeviceArray.from_host(X)
    _dsp.orthonormalize_dev(d, d, os)
    return d.to_host()
