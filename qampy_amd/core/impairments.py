"""Channel impairments on plain ndarrays (qampy/core/impairments.py:63-328 and :673-703 add_dispersion), through the GPU's kernels.

Every function takes complex64 or complex128 input, 1-d or 2-d, and keeps its dtype; anything else is promoted to complex128.  The random
ones take an extra keyword ``seed``: the noise is counter-based (Philox4x32-10), a function of (seed, mode, sample index).  ``seed=None``
draws a fresh seed from ``np.random``, so ``np.random.seed(...)`` at the top of a script makes them reproducible, as it does for the
reference (the values differ from the reference's: another generator)."""
import warnings

import numpy as np

from . import filter as _filter
from . import hip_dsp as _dsp


def _fresh_seed(seed):
    if seed is None:
        return int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
    if int(seed) != seed:
        raise ValueError("seed must be an integer or None")
    return int(seed)


def _rows(sig):
    """(2-d contiguous complex64 / complex128 copy or view, the input was 1-d)"""
    x = np.asarray(sig)
    if x.ndim not in (1, 2):
        raise ValueError("the impairments work on 1-d or 2-d arrays")
    X = np.atleast_2d(x)
    if X.dtype not in (np.complex64, np.complex128):
        X = X.astype(np.complex128)
    return np.ascontiguousarray(X), x.ndim == 1


def _on_device(sig, fn, inplace=True):
    """Upload, ``fn(E, out)``, download."""
    from .. import _lib
    X, one = _rows(sig)
    if X.size == 0:
        return X[0].copy() if one else X.copy()
    E = _lib.DeviceArray.from_host(X)
    out = E if inplace else _lib.DeviceArray(X.shape, X.dtype)
    fn(E, out)
    res = out.to_host()
    return res[0] if one else res


def rotate_field(field, theta):
    """Rotate a dual-polarisation field (2, L) by ``theta``: ``[[cos, -sin], [sin, cos]] @ field``."""
    X, _ = _rows(field)
    if np.asarray(field).ndim != 2 or X.shape[0] != 2:
        raise ValueError("rotate_field needs a field of two modes")
    return _on_device(field, lambda E, out: _dsp.rotate_field_dev(E, out, theta))


def apply_PMD_to_field(field, theta, t_dgd, fs):
    """First-order PMD on a dual-polarisation field (2, L): see :func:`qampy_amd.core.hip_dsp.apply_pmd_dev` - one exact transform per row
    for a row length that is a power of two from 256 to 8192, overlap-save blocks of 8192 samples with their truncation error (2.2e-4 of
    the rms at most for 30 ps at 40 GS/s and 2 samples per symbol) for every other length."""
    X, _ = _rows(field)
    if np.asarray(field).ndim != 2 or X.shape[0] != 2:
        raise ValueError("apply_PMD_to_field needs a field of two modes")
    return _on_device(field, lambda E, out: _dsp.apply_pmd_dev(E, out, theta, t_dgd, fs), inplace=False)


def phase_noise(sz, df, fs, seed=None, dtype=np.float64):
    """Wiener phase noise of variance ``2 pi df / fs`` per sample, of shape ``sz`` (an int, ``(L,)`` or ``(nmodes, L)``), accumulated along the
    last axis.  float64, drawn in double; ``dtype=np.float32`` returns the trace the complex64 pass draws (float draws, double sums)."""
    from .. import _lib
    shape = (int(sz),) if np.ndim(sz) == 0 else tuple(int(s) for s in sz)
    if len(shape) not in (1, 2):
        raise ValueError("phase_noise makes 1-d or 2-d arrays")
    nm, L = (1, shape[0]) if len(shape) == 1 else shape
    seed = _fresh_seed(seed)
    if nm * L == 0:
        return np.zeros(shape, np.float64)
    out = _lib.DeviceArray((nm, L), np.float64)
    _dsp.phase_noise_dev(out, df, fs, seed, draws=np.complex64 if np.dtype(dtype) == np.float32 else np.complex128)
    return out.to_host().reshape(shape)


def apply_phase_noise(signal, df, fs, seed=None):
    """Multiply every mode by ``exp(1j phi)``, ``phi`` an independent Wiener phase of combined linewidth ``df``."""
    seed = _fresh_seed(seed)
    return _on_device(signal, lambda E, out: _dsp.impair_pointwise_dev(E, out, phase=(df, fs), seed=seed))


def add_awgn(sig, strgth, seed=None):
    """Add complex white Gaussian noise of standard deviation ``strgth`` (split over I and Q) to every mode."""
    seed = _fresh_seed(seed)
    return _on_device(sig, lambda E, out: _dsp.impair_pointwise_dev(E, out, sigma=strgth, seed=seed))


def change_snr(sig, snr, fb, fs, seed=None):
    """Set the SNR (dB) of a noiseless signal: noise of ``sqrt(p) 10**(-snr/20) sqrt(fs/fb)`` with ``p`` the mean power over all modes."""
    seed = _fresh_seed(seed)
    return _on_device(sig, lambda E, out: _dsp.impair_pointwise_dev(E, out, snr=(snr, fs / fb), seed=seed))


def add_carrier_offset(sig, fo, fs):
    """``sig[:, n] * exp(2j pi n fo / fs)``.  The phase is formed in double and reduced modulo one turn for both precisions; the
    reference's complex64 path builds ``np.arange`` in float32 and loses the sample index above 2**24, which is not reproduced."""
    return _on_device(sig, lambda E, out: _dsp.impair_pointwise_dev(E, out, freq=(fo, fs)))


def add_modal_delay(sig, delay):
    """Roll mode ``i`` of a 2-d signal by ``delay[i]`` whole samples (``np.roll``)."""
    x = np.asarray(sig)
    if x.ndim != 2:
        raise ValueError("add_modal_delay needs a 2-d signal")
    _dsp._delays(delay, x.shape[0])
    return _on_device(sig, lambda E, out: _dsp.modal_delay_dev(E, out, delay), inplace=False)


def simulate_transmission(sig, fb, fs, snr=None, freq_off=None, lwdth=None, dgd=None, theta=np.pi / 3.731, modal_delay=None, roll_frame_sync=False,
                          seed=None):
    """All impairments at once, in the reference's order: (frame roll,) phase noise, carrier offset, SNR, modal delay, PMD - the first three
    as one fused pass on the device (:func:`qampy_amd.core.hip_dsp.simulate_transmission_dev`)."""
    if roll_frame_sync:
        if not (sig.nframes > 1):
            warnings.warn("Only single frame present, discontinuity introduced")
        sig = np.roll(sig, sig.pilots.shape[1], axis=-1)
    seed = _fresh_seed(seed)
    x = np.asarray(sig)
    if (modal_delay is not None or dgd is not None) and x.ndim != 2:
        raise ValueError("the modal delay and PMD need a 2-d signal")
    if modal_delay is not None:
        _dsp._delays(modal_delay, x.shape[0])
    return _on_device(sig, lambda E, out: _dsp.simulate_transmission_dev(E, out, fb, fs, snr=snr, freq_off=freq_off, lwdth=lwdth, dgd=dgd, theta=theta,
                                                                         modal_delay=modal_delay, seed=seed))


def add_dispersion(sig, fs, D, L, wl0=1550e-9):
    """
    Add the dispersion of ``L`` metres of fibre (``D`` in s/m/m, centre wavelength ``wl0``) to every row of ``sig``: circular filtering
    by exp(-0.5j beta2 L omega^2) on the fftfreq grid of the row length, in the input's dtype (complex64 or complex128).

    A row length that is a power of two up to 8192 is one exact transform per row; longer or other lengths run as overlap-save blocks of
    the default size of :func:`qampy_amd.core.filter.cd_filter_dev`, with its truncation error (about 2e-5 to 5e-5 of the signal rms).
    Every row is filtered on its own: the reference's 2-d input goes through a final ``fftshift`` over all axes, which also rolls the
    rows (two modes come back swapped); that is not reproduced.
    """
    x = np.asarray(sig)
    one = x.ndim == 1
    X = np.atleast_2d(x)
    if X.dtype not in (np.complex64, np.complex128):
        X = X.astype(np.complex128)
    n = X.shape[-1]
    N = n if (n & (n - 1)) == 0 and _filter.CD_NMIN <= n <= _filter.CD_NMAX else _filter.cd_block_size(_filter.cd_spread(fs, D, L, wl0))
    out = _filter.cd_filter_host(X, N, _filter.cd_coeffs_exact(fs, D, L, wl0))
    return out[0] if one else out
