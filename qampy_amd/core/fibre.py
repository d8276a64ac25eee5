"""Nonlinear fibre on plain ndarrays through the GPU's kernels: split-step Fourier propagation of the (Manakov) nonlinear Schroedinger equation
over amplified spans (:func:`ssfm`) and digital back-propagation (:func:`dbp`).  The model is stated in
:func:`qampy_amd.core.hip_dsp.ssfm_dev`.

Input is a 1-d or 2-d (one or two rows) complex64 or complex128 array and keeps its dtype; anything else is promoted to complex128.  The
amplifier noise is counter-based like every noise of :mod:`qampy_amd.core.impairments`: a function of (seed, span, mode, sample index);
``seed=None`` draws a fresh seed from ``np.random``."""
import numpy as np

from . import hip_dsp as _dsp
from . import impairments as _imp


def _check(sig, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, wl0):
    """Everything that can be refused without the device, on the host copy's shape."""
    X, _ = _imp._rows(sig)
    if X.shape[0] not in (1, 2):
        raise ValueError("the fibre takes one row, or two (Manakov), not %d" % X.shape[0])
    if X.size:
        _dsp.fft_plan(X.shape[1])
    _dsp.fibre._fibre_steps(steps, span_length)
    _dsp.fibre._fibre_spans(nspans)
    if (power_dbm is None) == (pscale is None):
        raise ValueError("give exactly one of power_dbm (the launch power over all rows) and pscale (watts per unit of |E|**2)")
    if not all(np.isfinite(float(v)) for v in (fs, D, gamma, alpha_db_km, wl0)) or not float(fs) > 0:
        raise ValueError("fs must be positive; D, gamma, alpha_db_km and wl0 finite")


def ssfm(sig, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, nf_db=None,
         wl0=1550e-9, seed=None):
    """``nspans`` spans of ``span_length`` metres of nonlinear fibre: :func:`qampy_amd.core.hip_dsp.ssfm_dev` on a copy of ``sig`` in HBM."""
    _check(sig, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, wl0)
    seed = _imp._fresh_seed(seed)
    return _imp._on_device(sig, lambda E, out: _dsp.ssfm_dev(E, out, fs, D, span_length, nspans=nspans, gamma=gamma, alpha_db_km=alpha_db_km, steps=steps,
                                                           power_dbm=power_dbm, pscale=pscale, amplify=amplify, nf_db=nf_db, wl0=wl0, seed=seed))


def dbp(sig, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, wl0=1550e-9, **kw):
    """Digital back-propagation, the inverse of the noise-free :func:`ssfm` with the same arguments: :func:`qampy_amd.core.hip_dsp.dbp_dev`."""
    if kw.pop("nf_db", None) is not None:
        raise ValueError("back-propagation adds no amplifier noise (nf_db)")
    if kw:
        raise TypeError("dbp: unexpected arguments %s" % sorted(kw))
    _check(sig, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, wl0)
    return _imp._on_device(sig, lambda E, out: _dsp.dbp_dev(E, out, fs, D, span_length, nspans=nspans, gamma=gamma, alpha_db_km=alpha_db_km, steps=steps,
                                                          power_dbm=power_dbm, pscale=pscale, amplify=amplify, wl0=wl0))
