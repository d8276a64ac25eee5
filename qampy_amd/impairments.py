"""Signal-object impairments (qampy/impairments.py): the wrappers of :mod:`qampy_amd.core.impairments` that take a signal object at its own
``fs`` / ``fb`` and return ``sig.recreate_from_np_array(...)``.  The random ones take the extra keyword ``seed`` of the core functions."""
import warnings

import numpy as np

from .core import impairments as _core


def add_dispersion(sig, D, L, wl0=1550e-9):
    """Add the dispersion of ``L`` metres of fibre (``D`` in s/m/m) to a signal object at its own ``fs``: see
    :func:`qampy_amd.core.impairments.add_dispersion`."""
    return sig.recreate_from_np_array(_core.add_dispersion(sig, sig.fs, D, L, wl0=wl0))


def apply_PMD(sig, theta, t_dgd):
    """First-order PMD of differential group delay ``t_dgd`` at the angle ``theta`` to the principal states: see
    :func:`qampy_amd.core.impairments.apply_PMD_to_field`."""
    return sig.recreate_from_np_array(_core.apply_PMD_to_field(sig, theta, t_dgd, sig.fs))


def apply_phase_noise(sig, df, seed=None):
    """Wiener phase noise of combined linewidth ``df`` on every mode."""
    return sig.recreate_from_np_array(_core.apply_phase_noise(sig, df, sig.fs, seed=seed))


def change_snr(sig, snr, seed=None):
    """Set the SNR (dB) of a noiseless signal object."""
    return sig.recreate_from_np_array(_core.change_snr(sig, snr, sig.fb, sig.fs, seed=seed))


def add_carrier_offset(sig, fo):
    """Add a carrier offset of ``fo`` Hz."""
    return sig.recreate_from_np_array(_core.add_carrier_offset(sig, fo, sig.fs))


def simulate_transmission(sig, snr=None, freq_off=None, lwdth=None, dgd=None, theta=np.pi / 3.731, modal_delay=None, dispersion=None,
                          roll_frame_sync=False, seed=None):
    """All impairments at once on a signal object, in the reference's order: (frame roll,) phase noise, carrier offset, SNR - one fused
    pass on the device - modal delay, dispersion, PMD.  ``dispersion`` is the accumulated dispersion in s/m, applied as
    ``add_dispersion(sig, dispersion, 1)`` (the reference's line names an undefined ``D`` there and raises; this is what it intends)."""
    if roll_frame_sync:
        if not (sig.nframes > 1):
            warnings.warn("Only single frame present, discontinuity introduced")
        sig = sig.recreate_from_np_array(np.roll(sig, sig.pilots.shape[1], axis=-1))
    out = sig.recreate_from_np_array(_core.simulate_transmission(sig, sig.fb, sig.fs, snr=snr, freq_off=freq_off, lwdth=lwdth, modal_delay=modal_delay,
                                                                 seed=seed))
    if dispersion is not None:
        out = add_dispersion(out, dispersion, 1)
    if dgd is not None:
        out = apply_PMD(out, theta, dgd)
    return out


def sim_tx_response(sig, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_core._dsp.txresp._DAC_DEFAULT, seed=None, **mod_prms):
    """A transmitter - DAC, ideal amplifier to ``tgt_v``, IQ modulator - on a signal object at its own ``fs``: see
    :func:`qampy_amd.core.impairments.sim_tx_response`."""
    return sig.recreate_from_np_array(_core.sim_tx_response(sig, sig.fs, enob=enob, tgt_v=tgt_v, clip_rat=clip_rat, quant_bits=quant_bits,
                                                            dac_params=dac_params, seed=seed, **mod_prms))


def sim_DAC_response(sig, enob=5, clip_rat=1, quant_bits=0, seed=None, **dac_params):
    """Clip, quantise, ENOB noise and the DAC's low-pass on a signal object at its own ``fs``: see
    :func:`qampy_amd.core.impairments.sim_DAC_response`."""
    return sig.recreate_from_np_array(_core.sim_DAC_response(sig, sig.fs, enob=enob, clip_rat=clip_rat, quant_bits=quant_bits, seed=seed, **dac_params))


def sim_mod_response(sig, dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1):
    """Response of an IQ modulator to a signal object: see :func:`qampy_amd.core.impairments.modulator_response`."""
    return sig.recreate_from_np_array(_core.modulator_response(sig, dcbias=dcbias, gfactr=gfactr, cfactr=cfactr, dcbias_out=dcbias_out,
                                                               gfactr_out=gfactr_out))


def simulate_fibre(sig, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, nf_db=None,
                   wl0=1550e-9, seed=None):
    """``nspans`` amplified spans of nonlinear fibre on a signal object at its own ``fs`` (split-step Fourier, Manakov for two modes): see
    :func:`qampy_amd.core.fibre.ssfm`."""
    from .core import fibre as _fibre
    return sig.recreate_from_np_array(_fibre.ssfm(sig, sig.fs, D, span_length, nspans=nspans, gamma=gamma, alpha_db_km=alpha_db_km, steps=steps,
                                                  power_dbm=power_dbm, pscale=pscale, amplify=amplify, nf_db=nf_db, wl0=wl0, seed=seed))
