"""Small filters used by the pilot receiver (behaviour of qampy/core/filter.py:215-237), root-raised-cosine shaping, the digital low-pass
of ``filter_signal``, the brick-wall pre-filters and chromatic dispersion."""
import numpy as np


def moving_average(sig, N=3):
    """Length ``len - N + 1`` running mean along the last axis, formed from a cumulative sum like the reference."""
    s2 = np.atleast_2d(sig)
    acc = np.cumsum(np.insert(s2, 0, 0, axis=-1), dtype=sig.dtype, axis=-1)
    out = (acc[:, N:] - acc[:, :-N]) / N
    return out.flatten() if sig.ndim == 1 else out


def rrcos_pulseshaping(sig, fs, T, beta, taps=1001):
    """Root-raised-cosine filtering of every row of ``sig`` at the rate ``fs`` (qampy/core/filter.py:177-212): a 'same' convolution
    with ``taps`` samples of the response of symbol period ``T`` and roll-off ``beta``, scaled to a peak of 1, on the GPU
    (qh_resample_* with up = down = 1).  ``taps=None``, the reference's spectral filter, is not implemented."""
    from . import resample as _rs
    if taps is None:
        raise NotImplementedError("taps=None (the whole-row spectral root-raised-cosine filter) is not implemented: give a tap count")
    one, X = _rs._as_rows(sig)
    out = _rs._filter_rows(X, _rs.rrcos_taps(taps, fs, T, beta), 1, 1, 1.0, False)
    return out[0] if one else out


def filter_signal(signal, fs, cutoff, ftype="bessel", order=2, analog=False):
    """Low-pass every row of ``signal`` (1-d or 2-d, the dtype kept; anything but complex64 / complex128 is promoted to complex128) by a
    digital Bessel (``norm='mag'``) or Butterworth filter of ``order`` 1 to 8 with the 3 dB ``cutoff`` (qampy/core/filter.py:86-147): the
    sections of ``scipy.signal.bessel`` / ``butter`` run on the GPU as ``scipy.signal.sosfilt`` does, exact and parallel in time
    (:func:`qampy_amd.core.hip_dsp.sosfilt_dev`).  ``ftype`` 'gauss' and 'exp' and ``analog=True`` need a transform of the whole row of
    arbitrary length, or ``lsim``: NotImplementedError."""
    from . import hip_dsp as _dsp
    from . import impairments as _imp
    if analog:
        raise NotImplementedError("analog=True integrates the analog prototype with lsim, which is not implemented: use the digital filter")
    sos = _dsp.design_lowpass_sos(fs, cutoff, ftype, order)
    return _imp._on_device(signal, lambda E, out: _dsp.sosfilt_dev(E, out, sos))


def _spectral_rows(signal, run, what):
    from .. import _lib
    x = np.asarray(signal)
    if x.ndim not in (1, 2):
        raise ValueError("%s works on 1-d or 2-d arrays" % what)
    X = np.atleast_2d(x)
    if X.dtype not in (np.complex64, np.complex128):
        X = X.astype(np.complex128)
    E = _lib.DeviceArray.from_host(np.ascontiguousarray(X))
    run(E)
    res = E.to_host()
    return res.flatten() if x.ndim < 2 else res


def pre_filter(signal, bw):
    """Brick-wall pre-filter of every row of ``signal`` (qampy/core/filter.py:28-49), on the GPU as one whole-row transform pair
    (:func:`qampy_amd.core.hip_dsp.pre_filter_dev`).  As written in the reference, ``bw`` is not a fraction: after ``fftshift`` the positions
    ``int(L / (bw / 2)) <= j < L - int(L / (bw / 2))`` are kept, so ``bw=0.01`` - and any ``bw`` whose count is 0 - gives all zeros.
    complex64 stays complex64, complex128 stays complex128, anything else is promoted to complex128; 1-d input gives 1-d output."""
    from . import hip_dsp as _dsp
    _dsp.fft_plan(np.asarray(signal).shape[-1])
    _dsp.pre_filter_bins(np.asarray(signal).shape[-1], float(bw))
    return _spectral_rows(signal, lambda E: _dsp.pre_filter_dev(E, E, bw), "pre_filter")


def pre_filter_wdm(signal, bw, os, center_freq=0):
    """Ideal band selection: keep the bins where ``abs(fftfreq(L, 1 / os) - center_freq) < bw / 2``.  The reference function
    (qampy/core/filter.py:51-84) raises NameError - it sizes its window from an undefined ``sig`` - so this restates it with that one name
    read as ``signal``, for rows along the last axis; dtypes and shapes as :func:`pre_filter`."""
    from . import hip_dsp as _dsp
    if not (np.isfinite(os) and os > 0 and np.isfinite(bw) and np.isfinite(center_freq)):
        raise ValueError("os must be positive, bw and center_freq finite")
    _dsp.fft_plan(np.asarray(signal).shape[-1])
    return _spectral_rows(signal, lambda E: _dsp.pre_filter_wdm_dev(E, E, bw, os, center_freq), "pre_filter_wdm")


# ------------------------------------------------------------------------------------------------ chromatic dispersion
# All-pass filtering of every row by H(w) = exp(j (c2 w^2 + c1 w + c0)), w = 2 pi fftfreq(N) in rad / sample, as block FFTs of size N
# on the GPU (qh_cd_filter_*, csrc/cd.hip).  H = exp(-0.5j beta2 L omega^2) is the fibre's response (qampy/core/impairments.py:673-703);
# compensating a dispersion D over L means filtering with -L (the reference's CDcomp convention, equalisation.py:596-669).

C_LIGHT = 2.99792458e8
CD_NMIN, CD_NMAX = 256, 8192          # block sizes of the kernel, both precisions (LDS: N complex values per workgroup)
CD_MODES = {"circular": 0, "linear": 1}


def beta2(D, wl):
    """Group-velocity dispersion (s^2 / m) of a dispersion parameter D (s / m / m) at wavelength wl (m)."""
    return D * wl ** 2 / (2 * np.pi * C_LIGHT)


def cd_spread(fs, D, L, wl=1550e-9):
    """Spread of the dispersion across the sampled band, in samples: 2 pi |beta2 L| fs^2."""
    return 2 * np.pi * abs(beta2(D, wl) * L) * fs ** 2


def cd_coeffs_exact(fs, D, L, wl=1550e-9):
    """(c2, c1, c0) of exp(-0.5j beta2 L omega^2) on the exact fftfreq grid (add_dispersion), omega = w fs."""
    return -0.5 * beta2(D, wl) * L * fs ** 2, 0.0, 0.0


def cd_coeffs_linspace(fs, D, L, wl, Ntot):
    """(c2, c1, c0) of CDcomp's H, which the reference samples on pi fs linspace(-1, 1, Ntot) in fftshift order.  In fftfreq order that
    grid is omega_ref = a omega + delta with a = Ntot / (Ntot - 1) and delta = pi fs / (Ntot - 1) (even Ntot; 0 for odd Ntot, where the
    zero frequency sits in the middle), so the phase -0.5 beta2 L omega_ref^2 is a quadratic in omega."""
    b = beta2(D, wl) * L
    a = Ntot / (Ntot - 1)
    d = np.pi * fs / (Ntot - 1) if Ntot % 2 == 0 else 0.0
    return -0.5 * b * a * a * fs ** 2, -b * a * d * fs, -0.5 * b * d * d


def cd_block_size(spread):
    """Default block size: the smallest power of two >= max(1024, 16 spread), capped at CD_NMAX.  A spread longer than CD_NMAX / 4 (the
    halo of a block) cannot be filtered in blocks: ValueError."""
    if spread > CD_NMAX / 4:
        raise ValueError("dispersion spread of %.0f samples is longer than the largest block's halo (%d samples)" % (spread, CD_NMAX // 4))
    N = 1024
    while N < 16 * spread and N < CD_NMAX:
        N *= 2
    return N


def _check_block(N):
    N = int(N)
    if N < CD_NMIN or N > CD_NMAX or N & (N - 1):
        raise ValueError("block size N=%d: a power of two from %d to %d" % (N, CD_NMIN, CD_NMAX))
    return N


def cd_filter_coeffs_dev(E, out, N, coeffs, mode="circular"):
    """``qh_cd_filter_*_dev`` on DeviceArrays: every row of E (nmodes, L) or (L,) through H(w) = exp(j (c2 w^2 + c1 w + c0)) in blocks of N.
    ``out``: (nmodes, L) for mode "circular", (nmodes, (L // (N/2)) * (N/2)) for "linear"; not E.  Enqueued on the current library stream."""
    from .. import _lib
    N = _check_block(N)
    if mode not in CD_MODES:
        raise ValueError("mode is 'circular' or 'linear'")
    shape = tuple(E.shape)
    nmodes, L = (1, shape[0]) if len(shape) == 1 else (int(np.prod(shape[:-1])), shape[-1])
    Lout = L if mode == "circular" else (L // (N // 2)) * (N // 2)
    if np.dtype(E.dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)) or np.dtype(out.dtype) != np.dtype(E.dtype):
        raise TypeError("cd_filter works on complex64 or complex128, out of the same dtype as E")
    if int(np.prod(out.shape)) != nmodes * Lout:
        raise ValueError("out holds %d samples, the filter writes %d" % (int(np.prod(out.shape)), nmodes * Lout))
    if out.ptr == E.ptr:
        raise ValueError("cd_filter is out of place: out must not be E")
    c2, c1, c0 = (float(c) for c in coeffs)
    suf = "64" if np.dtype(E.dtype) == np.dtype(np.complex64) else "128"
    _lib.call("qh_cd_filter_c%s_dev" % suf, E.ptr, nmodes, L, N, c2, c1, c0, CD_MODES[mode], out.ptr)
    return out


def cd_filter_dev(E, out, fs, D, L, wl0=1550e-9, N=None):
    """
    Chromatic dispersion on the device: every row of the DeviceArray ``E`` - (nmodes, L), or one channel of a ChannelBank - filtered
    circularly by the fibre's response exp(-0.5j beta2 L omega^2) on the exact fftfreq grid, into ``out`` (same shape and dtype, not E).
    ``L`` > 0 adds the dispersion of L metres of fibre; ``-L`` takes it out again.

    The filter runs as overlap-save blocks of ``N`` samples (a power of two, 256 .. 8192) that keep N/2 output samples and a halo of N/4
    on each side.  Default N: the smallest power of two >= max(1024, 16 spread), spread = 2 pi |beta2 L| fs^2 samples, capped at 8192.
    The impulse response outside the halo is cut off: on band-limited 2-sample/symbol QAM at 40 GS/s (D = 17 ps/nm/km) the rms error
    relative to the signal rms is 3e-5 (100 km, N = 1024), 5e-5 (500 km, 2048), 2e-5 (1000 km, 4096) and 1.5e-5 (2000 km, 8192),
    falling about as 1 / N^2.  Past the cap (spread > 512 samples, about 2350 km at 40 GS/s) the block no longer grows with the
    spread, and the error grows with it: 2.6e-5 at 4000 km and 5.6e-5 at 8000 km.  A spread longer than the halo of the largest block (2048 samples, about
    9400 km at 40 GS/s) raises ValueError.  A row whose length equals N is one exact circular transform.
    """
    sp = cd_spread(fs, D, L, wl0)
    N = cd_block_size(sp) if N is None else _check_block(N)
    if sp > N / 4:
        raise ValueError("dispersion spread of %.0f samples is longer than the halo (%d samples) of blocks of %d" % (sp, N // 4, N))
    return cd_filter_coeffs_dev(E, out, N, cd_coeffs_exact(fs, D, L, wl0), "circular")


def cd_filter_host(E, N, coeffs, mode="circular"):
    """Host-array form (``qh_cd_filter_*``): returns the filtered copy of the 2-D complex array E."""
    from .. import _lib
    N = _check_block(N)
    E = np.ascontiguousarray(E)
    if E.dtype not in (np.complex64, np.complex128) or E.ndim != 2:
        raise TypeError("cd_filter works on a 2-d complex64 or complex128 array")
    nmodes, L = E.shape
    Lout = L if mode == "circular" else (L // (N // 2)) * (N // 2)
    out = np.empty((nmodes, Lout), dtype=E.dtype)
    if out.size:
        c2, c1, c0 = (float(c) for c in coeffs)
        _lib.call("qh_cd_filter_c%s" % ("64" if E.dtype == np.complex64 else "128"), _lib.ptr(E), nmodes, L, N, c2, c1, c0, CD_MODES[mode],
                  _lib.ptr(out))
    return out
