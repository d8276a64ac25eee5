"""Channel and transmitter impairments on plain ndarrays (qampy/core/impairments.py:63-328, :370-671 and :673-703 add_dispersion), through
the GPU's kernels.

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
    _dsp.impair._delays(delay, x.shape[0])
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
        _dsp.impair._delays(modal_delay, x.shape[0])
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


# ------------------------------------------------------------------------------------------------ transmitter response
# qampy/core/impairments.py:370-671 through csrc/txresp.hip.  Real input is promoted to complex128 like everywhere in this module, and the
# result is complex: the reference's real-in, real-out paths (quantize_signal_New, apply_enob_as_awgn, filter_signal) are not reproduced.
def _recreate(sig, arr):
    return sig.recreate_from_np_array(arr) if hasattr(sig, "recreate_from_np_array") else arr


def er_to_g(ext_rat):
    """Gain factor of a Mach-Zehnder modulator of extinction ratio ``ext_rat`` (dB): ``(10**(er/20) - 1) / (10**(er/20) + 1)``."""
    return (10 ** (ext_rat / 20) - 1) / (10 ** (ext_rat / 20) + 1)


def clipper(sig, clipping_level):
    """Clamp re and im to ``+-clipping_level`` (qampy/core/digital_pre_compensation.py:30-38), on the host: ``np.clip`` of both parts."""
    x = np.asarray(sig)
    lv = float(clipping_level)
    if not np.iscomplexobj(x):
        return np.clip(x, -lv, lv)
    return (np.clip(x.real, -lv, lv) + 1j * np.clip(x.imag, -lv, lv)).astype(x.dtype if x.dtype in (np.complex64, np.complex128) else np.complex128)


def quantize_signal_New(sig_in, nbits=6, rescale_in=True, rescale_out=True):
    """Quantise to ``2**nbits`` levels with the thresholds midway between the output levels (``quantize_signal_New`` of the reference with
    its defaults: every row scaled to +-1 by its own maximum, the result scaled back by the maximum over all rows); a value on a threshold
    goes up.  Works on plain ndarrays and on signal objects (the subclass is kept).  Real input is promoted to complex128 and comes back
    complex.  Other values of ``rescale_in`` / ``rescale_out`` are not implemented."""
    if not (rescale_in and rescale_out):
        raise NotImplementedError("quantize_signal_New runs with rescale_in=True and rescale_out=True only")
    _dsp.txresp._dac_stages(1, nbits, 0)
    if np.isclose(float(nbits), 0):
        raise ValueError("nbits must be a whole number from 1 to 16")
    return _recreate(sig_in, _on_device(sig_in, lambda E, out: _dsp.dac_pointwise_dev(E, out, quant_bits=nbits)))


def apply_enob_as_awgn(sig, enob, verbose=False, seed=None):
    """Noise of a converter of ``enob`` effective bits as white Gaussian noise: ``sigma = sqrt(2 (x_max / 2**(enob - 1))**2 / 12)`` with
    ``x_max`` the largest ``|re|`` or ``|im|`` over all modes, read on the device.  ``verbose``: also the SNR in dB that corresponds to the
    ENOB, ``10 log10(mean |sig|**2 / 2 / (delta**2 / 12))``, computed on the host.  Real input is promoted to complex128."""
    seed = _fresh_seed(seed)
    _dsp.txresp._dac_stages(1, 0, enob)
    out = _on_device(sig, lambda E, o: _dsp.dac_pointwise_dev(E, o, enob=enob, seed=seed))
    if not verbose:
        return out
    x = np.asarray(sig)
    x_max = max(np.abs(x.real).max(), np.abs(x.imag).max())
    return out, 10 * np.log10(np.mean(np.abs(x) ** 2) / 2 / ((x_max / 2 ** (float(enob) - 1)) ** 2 / 12))


def apply_DAC_filter(sig, fs, cutoff=18e9, fn=None, ch=1):
    """The DAC's frequency response as a second-order Bessel low-pass at ``cutoff`` (:func:`qampy_amd.core.filter.filter_signal`).  A measured
    response (``fn``) multiplies the spectrum of the whole row: NotImplementedError."""
    if fn is not None:
        raise NotImplementedError("a measured DAC response (fn=...) multiplies the spectrum of the whole row, which is not implemented")
    return _filter.filter_signal(sig, fs, cutoff, ftype="bessel", order=2)


def sim_DAC_response(sig, fs, enob=5, clip_rat=1, quant_bits=0, seed=None, **dac_params):
    """Clip, quantise, add ENOB noise and - if any ``dac_params`` are given - low-pass: ``sim_DAC_response`` of the reference on the device
    (:func:`qampy_amd.core.hip_dsp.sim_dac_response_dev`).  Real input is promoted to complex128."""
    seed = _fresh_seed(seed)
    _dsp.txresp._dac_stages(clip_rat, quant_bits, enob)
    if _dsp.txresp._dac_filter(dac_params) is not None:
        _dsp.design_lowpass_sos(fs, _dsp.txresp._dac_filter(dac_params), "bessel", 2)
    return _on_device(sig, lambda E, out: _dsp.sim_dac_response_dev(E, out, fs, enob=enob, clip_rat=clip_rat, quant_bits=quant_bits, seed=seed, **dac_params))


def ideal_amplifier_response(sig, out_volt):
    """``sig / max * out_volt`` with the largest ``|re|`` or ``|im|`` over all modes, on the host (one pass of numpy; on the device the
    amplifier is part of the modulator's launch)."""
    x = np.asarray(sig)
    return x / max(np.abs(x.real).max(), np.abs(x.imag).max()) * out_volt


def modulator_response(rfsig, dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1):
    """Response of an IQ modulator to the drive voltages ``rfsig`` (I in the real part, Q in the imaginary part, in fractions of Vpi):
    ``modulator_response`` of the reference on the device.  Real input is promoted to complex128."""
    _dsp.txresp._mod_params(dcbias, gfactr, cfactr, dcbias_out, gfactr_out)
    return _on_device(rfsig, lambda E, out: _dsp.modulator_response_dev(E, out, dcbias=dcbias, gfactr=gfactr, cfactr=cfactr, dcbias_out=dcbias_out,
                                                                         gfactr_out=gfactr_out))


def sim_tx_response(sig, fs, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_dsp.txresp._DAC_DEFAULT, seed=None, **mod_prms):
    """A transmitter: DAC (clip, quantise, ENOB noise, Bessel low-pass), ideal amplifier to ``tgt_v`` (fractions of Vpi) and IQ modulator -
    ``sim_tx_response`` of the reference in one visit to the device (:func:`qampy_amd.core.hip_dsp.sim_tx_response_dev`).  Real input is
    promoted to complex128."""
    seed = _fresh_seed(seed)
    _dsp.txresp._dac_stages(clip_rat, quant_bits, enob)
    _dsp.txresp._mod_params(**mod_prms)
    if not np.isfinite(float(tgt_v)):
        raise ValueError("tgt_v must be finite")
    if _dsp.txresp._dac_filter(dac_params) is not None:
        _dsp.design_lowpass_sos(fs, _dsp.txresp._dac_filter(dac_params), "bessel", 2)
    return _on_device(sig, lambda E, out: _dsp.sim_tx_response_dev(E, out, fs, enob=enob, tgt_v=tgt_v, clip_rat=clip_rat, quant_bits=quant_bits,
                                                                   dac_params=dac_params, seed=seed, **mod_prms))
