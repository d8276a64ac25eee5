"""
Channel impairments on a resident field: the channel part of qampy/core/impairments.py (:29-328) on DeviceArrays; kernels in
qampy_amd/csrc/impair.hip.
"""
import numpy as np

from ... import _lib
from ._args import buffer, resident, same_as, seed64, two_modes

IMPAIR_TILE = 1024                 # samples of one mode per workgroup of the point-wise pass (csrc/impair.hip IMP_TILE)
PMD_NMIN, PMD_N = 256, 8192        # whole-row transform sizes; block size of the overlap-save form


def snr_noise_factor(snr_db, os):
    """``sigma / sqrt(p)`` of the reference's ``change_snr`` (qampy/core/impairments.py:230-233): ``10**(-snr/20) sqrt(fs/fb)``."""
    if not os > 0:
        raise ValueError("the oversampling fs / fb must be positive")
    return 10 ** (-float(snr_db) / 20) * np.sqrt(float(os))


def snr_power_factor(snr_db, os):
    """Factor by which ``change_snr`` at ``snr_db`` and ``os = fs / fb`` samples per symbol raises the mean power of a noiseless signal:
    ``1 + os 10**(-snr/10)``."""
    return 1.0 + float(os) * 10 ** (-float(snr_db) / 10)


def impair_pointwise_dev(E, out, *, sigma=None, snr=None, phase=None, freq=None, seed=0, trace=None):
    """
    The fused point-wise impairment pass on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one::

        out[m, n] = E[m, n] exp(j (phi[m, n] + 2 pi n fo / fs)) + sigma w[m, n]

    ``sigma``: noise strength as ``add_awgn`` takes it; or ``snr=(snr_db, os)``: ``sigma = sqrt(p) 10**(-snr_db/20) sqrt(os)`` with
    ``p = mean |E|**2`` over all modes together, reduced on the device (``change_snr``); neither: no noise (``sigma=0`` too: the field comes
    back bit for bit).  ``phase=(df, fs)``: a Wiener phase per mode with increments of variance ``2 pi df / fs`` (``apply_phase_noise``);
    ``trace``, an (nmodes, L) float64 DeviceArray, receives it.  ``freq=(fo, fs)``: carrier offset (``add_carrier_offset``); ``2 pi n fo / fs``
    is formed in double and reduced modulo one turn for both precisions - the reference's complex64 path builds ``np.arange`` in float32 and
    loses the sample index above 2**24, which is not reproduced.

    The noise is counter-based (Philox4x32-10 keyed by ``seed``): a draw depends on (seed, mode, n) only, noise and phase noise of one
    seed are independent, and a repeated call is bit-identical.  At most three launches on the current library stream, nothing read back.
    """
    c = resident(E, "impair_pointwise_dev")
    same_as(E, out, "impair_pointwise_dev")
    if sigma is not None and snr is not None:
        raise ValueError("give sigma or snr, not both")
    mode, noise = 0, 0.0
    if sigma is not None:
        mode, noise = 1, float(sigma)
    elif snr is not None:
        mode, noise = 2, snr_noise_factor(*snr)
    if mode and not (np.isfinite(noise) and noise >= 0):
        raise ValueError("the noise strength must be finite and not negative")
    var = 0.0
    if phase is not None:
        df, fs = phase
        var = 2 * np.pi * float(df) / float(fs)
        if not (np.isfinite(var) and var >= 0):
            raise ValueError("the linewidth must be finite and not negative")
    ft = 0.0
    if freq is not None:
        fo, fs = freq
        ft = float(fo) / float(fs)
        if not np.isfinite(ft):
            raise ValueError("the carrier offset must be finite")
    if trace is not None:
        if phase is None:
            raise ValueError("a trace needs phase=(df, fs)")
        buffer(trace, "impair_pointwise_dev", "trace", E.shape, np.float64)
    _lib.call("qh_impair_pointwise_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], mode, noise, int(phase is not None), var, int(freq is not None), ft,
              seed64(seed), trace.ptr if trace is not None else None, out.ptr)
    return out


def phase_noise_dev(out, df, fs, seed, cumulative=True, draws=np.complex128):
    """The Wiener phase of :func:`impair_pointwise_dev` on its own, into the (nmodes, L) float64 DeviceArray ``out`` (``phase_noise`` of the
    reference); ``cumulative=False`` writes the raw increments instead of their running sum.  ``draws``: the precision of the pass whose
    draws are wanted - complex64 draws in float with the fast intrinsics, complex128 in double; the sums are double in both."""
    if len(out.shape) != 2 or np.dtype(out.dtype) != np.float64:
        raise TypeError("phase_noise_dev writes an (nmodes, L) float64 DeviceArray")
    c = {np.dtype(np.complex64): "c64", np.dtype(np.complex128): "c128"}.get(np.dtype(draws))
    if c is None:
        raise TypeError("draws is complex64 or complex128")
    var = 2 * np.pi * float(df) / float(fs)
    if not (np.isfinite(var) and var >= 0):
        raise ValueError("the linewidth must be finite and not negative")
    _lib.call("qh_phase_noise_%s_dev" % c, out.ptr, out.shape[0], out.shape[1], var, seed64(seed), int(bool(cumulative)))
    return out


def rotate_field_dev(E, out, theta):
    """``[[cos, -sin], [sin, cos]] @ E`` for a (2, L) field (``rotate_field``); ``out`` may be ``E``."""
    c = resident(E, "rotate_field_dev")
    same_as(E, out, "rotate_field_dev")
    two_modes(E, "rotate_field_dev")
    _lib.call("qh_rotate_field_%s_dev" % c, E.ptr, 2, E.shape[1], float(theta), out.ptr)
    return out


def apply_pmd_dev(E, out, theta, t_dgd, fs):
    """
    First-order PMD on a (2, L) field in HBM (``apply_PMD_to_field``): ``R(-theta) diag(H, conj H) R(theta)`` with ``H = exp(-j omega t_dgd / 2)``,
    into ``out`` (not ``E``).  Two launches on the current library stream.

    A row length that is a power of two from 256 to 8192 is one exact circular transform per row - the reference's operation.  Every other
    length runs as overlap-save blocks of 8192 samples (4096 kept, 2048 of halo either side, the field taken modulo L), which is NOT the
    reference's operation: a delay of a fraction of a sample has a 1/n tail that the block cuts off and wraps.  On 16-QAM at 2 samples per
    symbol, roll-off 0.1, 40 GS/s, theta = pi/5.6, against the full-length transform: 30 ps (+-0.6 sample) deviates by 2.2e-4 of the rms at
    most (rms 1.1e-4), a delay of whole samples (200 ps) by 4e-15; at one sample per symbol 30 ps deviates by 1.3e-2.  For an odd row
    length the reference's own frequency grid is off numpy's fftfreq grid by half a bin; the blocks use the fftfreq grid.
    """
    c = resident(E, "apply_pmd_dev")
    same_as(E, out, "apply_pmd_dev")
    two_modes(E, "apply_pmd_dev")
    if out.ptr == E.ptr:
        raise ValueError("apply_pmd_dev is out of place: out must not be E")
    d = float(t_dgd) * float(fs)
    if not (np.isfinite(d) and np.isfinite(float(theta))):
        raise ValueError("theta and the delay must be finite")
    _lib.call("qh_apply_pmd_%s_dev" % c, E.ptr, 2, E.shape[1], float(theta), d, out.ptr)
    return out


def _delays(delay, nmodes):
    d = np.asarray(delay)
    if d.ndim != 1 or d.shape[0] != nmodes:
        raise ValueError("Delay array must have the same length as number of modes of signal")
    if not np.all(np.equal(np.mod(d, 1), 0)):
        raise ValueError("the modal delays are whole numbers of samples")
    return np.ascontiguousarray(d, dtype=np.int64)


def modal_delay_dev(E, out, delay):
    """Row m of ``E`` rolled by ``delay[m]`` samples into ``out`` (``add_modal_delay``: ``np.roll`` per mode); ``out`` is not ``E``."""
    c = resident(E, "modal_delay_dev")
    same_as(E, out, "modal_delay_dev")
    if out.ptr == E.ptr:
        raise ValueError("modal_delay_dev is out of place: out must not be E")
    d = _delays(delay, E.shape[0])
    _lib.call("qh_modal_delay_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], _lib.ptr(d), out.ptr)
    return out


def simulate_transmission_dev(E, out, fb, fs, snr=None, freq_off=None, lwdth=None, dgd=None, theta=np.pi / 3.731, modal_delay=None, seed=0, tmp=None):
    """
    ``simulate_transmission`` of the reference on (nmodes, L) DeviceArrays, in its order: phase noise, carrier offset and SNR - one fused
    pass (:func:`impair_pointwise_dev`) - then the modal delay, then PMD (:func:`apply_pmd_dev`).  ``out`` may be ``E``.  The two
    out-of-place stages alternate between ``out`` and ``tmp``, a DeviceArray like ``E`` (allocated here when one is needed and none is
    given), so that the last one writes ``out``.  Returns ``out``.
    """
    resident(E, "simulate_transmission_dev")
    same_as(E, out, "simulate_transmission_dev")
    nfilt = int(modal_delay is not None) + int(dgd is not None)
    if dgd is not None:
        two_modes(E, "PMD")
    if nfilt and tmp is None:
        tmp = _lib.DeviceArray(E.shape, E.dtype)
    # the out-of-place stages alternate between tmp and out so that the last one writes out
    first = out if nfilt != 1 else tmp
    impair_pointwise_dev(E, first, snr=None if snr is None else (snr, fs / fb), phase=None if lwdth is None else (lwdth, fs),
                         freq=None if freq_off is None else (freq_off, fs), seed=seed)
    cur = first
    if modal_delay is not None:
        nxt = tmp if cur is out else out
        modal_delay_dev(cur, nxt, modal_delay)
        cur = nxt
    if dgd is not None:
        nxt = tmp if cur is out else out
        apply_pmd_dev(cur, nxt, theta, dgd, fs)
        cur = nxt
    assert cur is out
    return out
