"""
Transmitter response on a resident field: the transmitter part of qampy/core/impairments.py (:370-671) and filter_signal
(qampy/core/filter.py:86-147) on DeviceArrays; kernels in qampy_amd/csrc/txresp.hip.
"""
import numpy as np

from ... import _lib
from ._args import buffer, modes_upto, resident, same_as, seed64

SOS_CHUNK, SOS_TILE = 128, 8192     # samples per lane and per workgroup of the sections filter (csrc/txresp.hip SOS_C, SOS_T; qh_sos_geometry)
SOS_MAXSEC = 4
TX_MAXMODES = 1024


def row_extrema_dev(E, ext=None):
    """``(max |re|, max |im|)`` of every row of the (nmodes, L) complex DeviceArray ``E`` into the (nmodes, 2) float64 DeviceArray ``ext``
    (made when None); two launches, nothing read back, bit-reproducible.  The later stages read their scale factors from it on the device."""
    c = resident(E, "row_extrema_dev")
    modes_upto(E, "row_extrema_dev", TX_MAXMODES)
    if E.shape[1] < 1:
        raise ValueError("row_extrema_dev needs at least one sample per row")
    ext = buffer(ext, "row_extrema_dev", "ext", (E.shape[0], 2), np.float64, make=True)
    _lib.call("qh_row_extrema_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr)
    return ext


def _dac_stages(clip_rat, quant_bits, enob):
    """(mask, clip_rat, bits, enob) of the DAC's point-wise stages, checked; a stage is off where the reference's ``np.isclose`` says so."""
    clip_rat, enob = float(clip_rat), float(enob)
    if not (np.isfinite(clip_rat) and clip_rat > 0):
        raise ValueError("clip_rat must be positive")
    if not (np.isfinite(enob) and enob >= 0):
        raise ValueError("enob must not be negative")
    qb = float(quant_bits)
    bits = 0
    if not np.isclose(qb, 0):
        if not (np.isfinite(qb) and qb == int(qb) and 1 <= qb <= 16):
            raise ValueError("quant_bits must be 0 or a whole number from 1 to 16")
        bits = int(qb)
    stages = (0 if np.isclose(clip_rat, 1) else 1) | (2 if bits else 0) | (0 if np.isclose(enob, 0) else 4)
    return stages, clip_rat, bits, enob


def dac_pointwise_dev(E, out, clip_rat=1, quant_bits=0, enob=0, seed=0, ext=None):
    """
    The point-wise part of ``sim_DAC_response`` on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one: clip,
    then quantise, then ENOB noise, each optional, in the reference's order and with its conventions.

    Clip (unless ``np.isclose(clip_rat, 1)``): every row scaled to ``+-1 / clip_rat`` by its own maximum, re and im clamped to ``+-1``.
    Quantise (unless ``np.isclose(quant_bits, 0)``; ``quantize_signal_New``): every row scaled to ``+-1`` by its own maximum, the level index
    the number of thresholds ``-1 + k d`` (``d = 2 / 2**bits``) that are <= the value - a value on a threshold goes up -, the output level
    ``-1 + d / 2 + index d`` times the maximum over all rows of the quantiser's input.  Noise (unless ``np.isclose(enob, 0)``;
    ``apply_enob_as_awgn``): ``sigma = sqrt(2 (x_max / 2**(enob - 1))**2 / 12)`` with ``x_max`` over all rows of the stage's input, added
    exactly as ``impair_pointwise_dev(sigma=sigma, seed=seed)`` adds it.

    ``ext``: the row extrema of ``E`` (:func:`row_extrema_dev`); None: formed here.  One extrema pass serves all three stages - after
    clipping every row's maximum is ``min(1 / clip_rat, 1)``, after quantising ``(1 - d / 2) max_swing``.  Launches: 1, plus 2 for the
    extrema when ``ext`` is None; with nothing to do none (``out is E``) or one copy, and the field comes back bit for bit.
    """
    c = resident(E, "dac_pointwise_dev")
    same_as(E, out, "dac_pointwise_dev")
    modes_upto(E, "dac_pointwise_dev", TX_MAXMODES)
    stages, clip_rat, bits, enob = _dac_stages(clip_rat, quant_bits, enob)
    buffer(ext, "dac_pointwise_dev", "ext", (E.shape[0], 2), np.float64, optional=True)
    _lib.call("qh_dac_pointwise_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr if ext is not None else None, stages, clip_rat, bits, enob,
              seed64(seed), out.ptr)
    return out


def enob_sigma(x_max, enob):
    """The noise strength of ``apply_enob_as_awgn``: ``sqrt(2 (x_max / 2**(enob - 1))**2 / 12)``."""
    return np.sqrt(2 * (float(x_max) / 2 ** (float(enob) - 1)) ** 2 / 12)


def _check_sos(sos):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= SOS_MAXSEC:
        raise ValueError("sos must be (n_sections, 6) with 1 to %d sections" % SOS_MAXSEC)
    if not np.all(np.isfinite(sos)):
        raise ValueError("the section coefficients must be finite")
    if not np.all(sos[:, 3] == 1.0):
        raise ValueError("every section must be normalised to a0 = 1")
    return sos


def sos_transition(sos, C):
    """The (2 nsec, 2 nsec) matrix that maps the state of the cascade ``sos`` - (z0, z1) of section 0, then of section 1, ... as
    ``scipy.signal.sosfilt`` keeps them - over ``C`` samples of zero input: ``M**C`` with ``M`` the map over one sample.  The power is
    formed in ``np.longdouble`` and rounded to float64 once: for a narrow low-pass the entries reach 1e9 and cancel in every product, and a
    power formed in float64 is off by 1e-9 of its largest entry - 3e-12 of the input's rms in the filtered field instead of 5e-14."""
    sos = _check_sos(sos)
    C = int(C)
    if C < 0:
        raise ValueError("C must not be negative")
    n = 2 * sos.shape[0]
    M = np.zeros((n, n), np.longdouble)
    for j in range(n):
        z = np.zeros(n, np.longdouble)
        z[j] = 1
        x = np.longdouble(0)
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos.astype(np.longdouble)):
            y = b0 * x + z[2 * s]
            z[2 * s] = b1 * x - a1 * y + z[2 * s + 1]
            z[2 * s + 1] = b2 * x - a2 * y
            x = y
        M[:, j] = z
    P = np.eye(n, dtype=np.longdouble)
    while C:
        if C & 1:
            P = P @ M
        M = M @ M
        C >>= 1
    return P.astype(np.float64)


_TRANSITIONS = {}


def _chunk_transition(key, nsec):
    """``sos_transition(sos, SOS_CHUNK)`` of the sections whose bytes are ``key``, kept for the next call: a sweep filters with the same
    sections again and again, and the extended-precision power costs more host time than the filter takes on the device."""
    P = _TRANSITIONS.get(key)
    if P is None:
        if len(_TRANSITIONS) >= 64:
            _TRANSITIONS.clear()
        P = _TRANSITIONS[key] = np.ascontiguousarray(sos_transition(np.frombuffer(key, np.float64).reshape(nsec, 6), SOS_CHUNK))
    return P


def sosfilt_dev(E, out, sos):
    """
    ``scipy.signal.sosfilt(sos, E, axis=-1)`` on (nmodes, L) complex DeviceArrays: zero initial state, every row on its own, real
    coefficients (re and im are filtered alike), up to 4 sections; ``out`` may be ``E``.  Coefficients and state are double in both
    precisions; only the samples are complex64 in the complex64 form.

    Exact and parallel in time: a lane filters ``SOS_CHUNK`` consecutive samples from a zero state, the chunks' start states follow from
    ``s[k + 1] = P s[k] + f[k]`` with ``P = sos_transition(sos, SOS_CHUNK)`` by a log-step scan inside a workgroup (``SOS_TILE`` samples) and a
    second one across workgroups, and every lane runs its chunk again from its true start state.  Three launches, one when a row fits a tile.
    """
    c = resident(E, "sosfilt_dev")
    same_as(E, out, "sosfilt_dev")
    sos = _check_sos(sos)
    P = _chunk_transition(sos.tobytes(), sos.shape[0])
    _lib.call("qh_sosfilt_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], _lib.ptr(sos), sos.shape[0], _lib.ptr(P), out.ptr)
    return out


_DESIGNS = {}            # sections by (fs, cutoff, ftype, order): scipy's design takes longer than the filter on the device


def design_lowpass_sos(fs, cutoff, ftype="bessel", order=2):
    """The sections of the reference's digital low-pass (``filter_signal``, qampy/core/filter.py:129-135): ``scipy.signal.bessel(order,
    cutoff, 'low', norm='mag', output='sos', fs=fs)`` or ``scipy.signal.butter(order, cutoff, 'low', output='sos', fs=fs)``, checked."""
    if ftype in ("gauss", "exp"):
        raise NotImplementedError("ftype=%r filters the whole row in the frequency domain, which is not implemented: 'bessel' or 'butter'" % ftype)
    if ftype not in ("bessel", "butter"):
        raise ValueError("ftype is 'bessel' or 'butter'")
    if int(order) != order or not 1 <= int(order) <= 2 * SOS_MAXSEC:
        raise ValueError("order must be a whole number from 1 to %d" % (2 * SOS_MAXSEC))
    fs, cutoff = float(fs), float(cutoff)
    if not (np.isfinite(fs) and np.isfinite(cutoff) and 0 < cutoff < fs / 2):
        raise ValueError("the cutoff must lie between 0 and fs / 2")
    key = (fs, cutoff, ftype, int(order))
    sos = _DESIGNS.get(key)
    if sos is None:
        import scipy.signal as scisig
        if len(_DESIGNS) >= 64:
            _DESIGNS.clear()
        if ftype == "bessel":
            sos = scisig.bessel(int(order), cutoff, "low", norm="mag", output="sos", fs=fs)
        else:
            sos = scisig.butter(int(order), cutoff, "low", output="sos", fs=fs)
        _DESIGNS[key] = sos
    return sos.copy()


def filter_signal_dev(E, out, fs, cutoff, ftype="bessel", order=2):
    """``filter_signal`` of the reference on (nmodes, L) complex DeviceArrays: a digital Bessel (``norm='mag'``) or Butterworth low-pass of
    ``order`` 1 to 8 with the 3 dB ``cutoff``, designed on the host (:func:`design_lowpass_sos`) and run by :func:`sosfilt_dev`; ``out`` may be
    ``E``.  ``ftype`` 'gauss' and 'exp' raise NotImplementedError."""
    resident(E, "filter_signal_dev")
    same_as(E, out, "filter_signal_dev")
    return sosfilt_dev(E, out, design_lowpass_sos(fs, cutoff, ftype, order))


def _iq(v, name):
    """(I, Q) of a modulator parameter: a real value serves both arms (``np.iscomplex`` of the reference: an imaginary part of 0 is real)."""
    v = complex(v)
    if not (np.isfinite(v.real) and np.isfinite(v.imag)):
        raise ValueError("%s must be finite" % name)
    return (v.real, v.imag) if v.imag != 0 else (v.real, v.real)


def _mod_params(dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1):
    d, g, c = _iq(dcbias, "dcbias"), _iq(gfactr, "gfactr"), _iq(cfactr, "cfactr")
    for name, v in (("dcbias_out", dcbias_out), ("gfactr_out", gfactr_out)):
        if np.iscomplexobj(v) or not np.isfinite(float(v)):
            raise ValueError("%s must be real and finite" % name)
    return np.array([d[0], d[1], g[0], g[1], c[0], c[1], float(dcbias_out), float(gfactr_out)], np.float64)


def modulator_response_dev(E, out, dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1, tgt_v=None, ext=None):
    """
    ``modulator_response`` of the reference on (nmodes, L) complex DeviceArrays, one point-wise launch; ``out`` may be ``E``.  ``dcbias``,
    ``gfactr`` and ``cfactr`` real (both arms alike) or complex (I, Q).  ``tgt_v``: ``ideal_amplifier_response(E, tgt_v)`` first, in the same
    launch - ``E / max * tgt_v`` with the maximum over all rows read from ``ext`` (:func:`row_extrema_dev`; None: formed here, two more
    launches).  Every angle is formed in double and reduced modulo one turn before the sine and cosine, in both precisions.
    """
    c = resident(E, "modulator_response_dev")
    same_as(E, out, "modulator_response_dev")
    modes_upto(E, "modulator_response_dev", TX_MAXMODES)
    prm = _mod_params(dcbias, gfactr, cfactr, dcbias_out, gfactr_out)
    if tgt_v is not None and not np.isfinite(float(tgt_v)):
        raise ValueError("tgt_v must be finite")
    buffer(ext, "modulator_response_dev", "ext", (E.shape[0], 2), np.float64, optional=True)
    _lib.call("qh_modulator_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr if ext is not None else None, int(tgt_v is not None),
              0.0 if tgt_v is None else float(tgt_v), _lib.ptr(prm), out.ptr)
    return out


def _dac_filter(dac_params):
    """The sections of ``apply_DAC_filter(**dac_params)``, or None without parameters."""
    if not dac_params:
        return None
    prm = dict(dac_params)
    if prm.pop("fn", None) is not None:
        raise NotImplementedError("a measured DAC response (fn=...) multiplies the spectrum of the whole row, which is not implemented")
    prm.pop("ch", None)
    cutoff = prm.pop("cutoff", 18e9)
    if prm:
        raise TypeError("unknown DAC parameters: %s" % ", ".join(sorted(prm)))
    return cutoff


def sim_dac_response_dev(E, out, fs, enob=5, clip_rat=1, quant_bits=0, seed=0, ext=None, **dac_params):
    """``sim_DAC_response`` on (nmodes, L) complex DeviceArrays: :func:`dac_pointwise_dev`, then - if any ``dac_params`` are given - the DAC's
    second-order Bessel low-pass at ``cutoff`` (default 18 GHz; :func:`filter_signal_dev`).  ``out`` may be ``E``."""
    resident(E, "sim_dac_response_dev")
    same_as(E, out, "sim_dac_response_dev")
    _dac_stages(clip_rat, quant_bits, enob)
    cutoff = _dac_filter(dac_params)
    sos = None if cutoff is None else design_lowpass_sos(fs, cutoff, "bessel", 2)
    dac_pointwise_dev(E, out, clip_rat=clip_rat, quant_bits=quant_bits, enob=enob, seed=seed, ext=ext)
    if sos is not None:
        sosfilt_dev(out, out, sos)
    return out


_DAC_DEFAULT = {"cutoff": 18e9}


def sim_tx_response_check(E, out, fs, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_DAC_DEFAULT, seed=0, **mod_prms):
    """Every check of :func:`sim_tx_response_dev`, without touching the device: TypeError / ValueError / NotImplementedError, else None."""
    resident(E, "sim_tx_response_dev")
    same_as(E, out, "sim_tx_response_dev")
    modes_upto(E, "sim_tx_response_dev", TX_MAXMODES)
    _dac_stages(clip_rat, quant_bits, enob)
    _mod_params(**mod_prms)
    if not np.isfinite(float(tgt_v)):
        raise ValueError("tgt_v must be finite")
    seed64(seed)
    cutoff = _dac_filter(dac_params)
    if cutoff is not None:
        design_lowpass_sos(fs, cutoff, "bessel", 2)


def sim_tx_response_dev(E, out, fs, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_DAC_DEFAULT, seed=0, **mod_prms):
    """
    ``sim_tx_response`` on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one: the DAC
    (:func:`sim_dac_response_dev`), the ideal amplifier to ``tgt_v`` (in fractions of Vpi) and the IQ modulator
    (:func:`modulator_response_dev`) with ``mod_prms``.  Every argument is checked before the first launch
    (:func:`sim_tx_response_check`).  At most nine launches - extrema (2), DAC point-wise pass (1), filter (3), extrema of the filtered
    field (2), amplifier and modulator (1) - on the current library stream, nothing read back.
    """
    sim_tx_response_check(E, out, fs, enob=enob, tgt_v=tgt_v, clip_rat=clip_rat, quant_bits=quant_bits, dac_params=dac_params, seed=seed, **mod_prms)
    if E.shape[1] == 0:
        return out
    sim_dac_response_dev(E, out, fs, enob=enob, clip_rat=clip_rat, quant_bits=quant_bits, seed=seed, **(dac_params or {}))
    return modulator_response_dev(out, out, tgt_v=tgt_v, **mod_prms)
