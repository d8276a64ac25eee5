"""
Nonlinear fibre on a resident field: split-step Fourier propagation of the (Manakov) nonlinear Schroedinger equation and digital
back-propagation; kernels in qampy_amd/csrc/fibre.hip, the model in include/qampy_hip.h and DESIGN.md 3.22.
"""
import numpy as np

from ... import _lib
from ._args import buffer, resident, same_as, seed64
from .frontend import fft_plan

FIBRE_MAX = 4096                       # most steps per span, most spans (csrc/fibre.hip FIB_MAX)
H_PLANCK = 6.62607015e-34              # J s
C_LIGHT = 2.99792458e8                 # m / s (core/filter.py)


def fibre_alpha(alpha_db_km):
    """Power loss in 1 / m of a loss in dB / km: ``alpha_db_km 1e-3 ln(10) / 10``."""
    return float(alpha_db_km) * 1e-3 * np.log(10) / 10


def ase_power(nf_db, alpha, span_length, fs, wl0=1550e-9):
    """Noise power in watts per mode that an amplifier of noise figure ``nf_db`` adds within the sampled band ``fs`` when it makes up the loss
    ``alpha`` (1 / m) of ``span_length`` metres: ``n_sp h (c / wl0) (G - 1) fs`` with ``n_sp = 10**(nf_db / 10) / 2`` and ``G = exp(alpha span_length)``."""
    n_sp = 10 ** (float(nf_db) / 10) / 2
    G = np.exp(float(alpha) * float(span_length))
    return float(n_sp * H_PLANCK * (C_LIGHT / float(wl0)) * (G - 1) * float(fs))


def _fibre_steps(steps, span_length):
    """The step lengths of one span as a list of floats: ``steps`` equal ones, or the given sequence, which must add up to the span."""
    span = float(span_length)
    if not (np.isfinite(span) and span > 0):
        raise ValueError("span_length must be finite and positive")
    if np.ndim(steps) == 0:
        if isinstance(steps, (bool, np.bool_)) or int(steps) != steps:
            raise ValueError("steps is a whole number of equal steps, or a sequence of step lengths")
        n = int(steps)
        if not 1 <= n <= FIBRE_MAX:
            raise ValueError("a span takes 1 to %d steps" % FIBRE_MAX)
        return [span / n] * n
    dz = [float(v) for v in np.asarray(steps, dtype=np.float64).ravel()]
    if not 1 <= len(dz) <= FIBRE_MAX:
        raise ValueError("a span takes 1 to %d steps" % FIBRE_MAX)
    if not all(np.isfinite(v) and v > 0 for v in dz):
        raise ValueError("every step length must be finite and positive")
    if abs(sum(dz) - span) > 1e-9 * span:
        raise ValueError("the steps add up to %r m, the span is %r m" % (sum(dz), span))
    return dz


def _fibre_spans(nspans):
    if isinstance(nspans, (bool, np.bool_)) or np.ndim(nspans) != 0 or int(nspans) != nspans or not 1 <= int(nspans) <= FIBRE_MAX:
        raise ValueError("nspans is a whole number from 1 to %d" % FIBRE_MAX)
    return int(nspans)


def fibre_plan(L, steps, nspans=1, span_length=1.0, power_dbm=None, backward=False):
    """What one call of :func:`ssfm_dev` / :func:`dbp_dev` launches on rows of ``L`` samples, as a dict: ``filters`` - whole-row spectral filters, a
    transform pair each, ``steps + 1`` per span; ``nonlinear`` - launches of the point-wise kernel, ``steps`` per span; ``tables`` - launches that
    form a dispersion table: two tables live on the device and the one used longest ago is formed again when a new length comes up, so equal
    steps form two per call and only a list of three or more different half-step sums forms more; ``power`` - launches that fix ``pscale`` (2 when it
    is derived from ``power_dbm``, else 1).  ``steps``, ``span_length``: as the propagation takes them (the counts of equal steps do not depend on the
    span)."""
    fft_plan(L)
    dz = _fibre_steps(steps, span_length)
    nspans = _fibre_spans(nspans)
    if backward:
        dz = dz[::-1]
    n = len(dz)
    held, last, tables = [None, None], 1, 0
    for _ in range(nspans):
        for h in [dz[0] / 2] + [dz[i] / 2 + (dz[i + 1] / 2 if i + 1 < n else 0.0) for i in range(n)]:
            if h in held:
                last = held.index(h)
                continue
            last = 0 if held[0] is None else (1 if held[1] is None else 1 - last)
            held[last] = h
            tables += 1
    return dict(filters=nspans * (n + 1), nonlinear=nspans * n, tables=tables, power=2 if power_dbm is not None else 1)


def _fibre_call(what, E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, backward, ase_w=0.0, seed=0):
    from ..filter import beta2
    c = resident(E, what)
    same_as(E, out, what)
    if E.shape[0] not in (1, 2):
        raise ValueError("%s: one row, or two (Manakov), not %d" % (what, E.shape[0]))
    fft_plan(E.shape[1])
    dz = _fibre_steps(steps, span_length)
    nspans = _fibre_spans(nspans)
    if (power_dbm is None) == (pscale is None):
        raise ValueError("%s: give exactly one of power_dbm (the launch power over all rows) and pscale (watts per unit of |E|**2)" % what)
    mode, power = (1, 1e-3 * 10 ** (float(power_dbm) / 10)) if pscale is None else (0, float(pscale))
    fs, gamma, alpha, b2 = float(fs), float(gamma), fibre_alpha(alpha_db_km), float(beta2(float(D), float(wl0)))
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("%s: fs must be finite and positive" % what)
    if not all(np.isfinite(v) for v in (gamma, alpha, b2)):
        raise ValueError("%s: D, wl0, gamma and alpha_db_km must be finite" % what)
    if not (np.isfinite(power) and power > 0):
        raise ValueError("%s: the power must be finite and positive" % what)
    if not (np.isfinite(ase_w) and ase_w >= 0):
        raise ValueError("%s: the amplifier noise power must be finite and not negative" % what)
    if abs(alpha) * sum(dz) > 709:                                           # exp overflows in double
        raise ValueError("%s: the loss of a span overflows" % what)
    arr = (_lib.C.c_double * len(dz))(*dz)
    _lib.call("qh_fibre_ssfm_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], fs, b2, gamma, alpha, arr, len(dz), nspans, int(backward), int(bool(amplify)), mode,
              power, float(ase_w), seed64(seed), out.ptr)
    return out


def fibre_nl_dev(E, out, a, coef, pscale, sigma_w=0.0, seed=0):
    """The nonlinear step of :func:`ssfm_dev` on its own, one launch: ``out[m, n] = a exp(1j coef pscale[0] P[n]) E[m, n]`` with
    ``P[n] = sum_m |E[m, n]|**2``, plus - ``sigma_w > 0`` - noise of standard deviation ``sigma_w / sqrt(pscale[0])`` drawn under ``seed``.
    ``pscale``: a float64 DeviceArray of one value.  One or two rows of 1 to 2**24 samples; ``out`` may be ``E``."""
    c = resident(E, "fibre_nl_dev")
    same_as(E, out, "fibre_nl_dev")
    if E.shape[0] not in (1, 2) or not 1 <= E.shape[1] <= 1 << 24:
        raise ValueError("fibre_nl_dev: one or two rows of 1 to 2**24 samples")
    buffer(pscale, "fibre_nl_dev", "pscale", (1,), np.float64, by_size=True)
    a, coef, sigma_w = float(a), float(coef), float(sigma_w)
    if not (np.isfinite(a) and np.isfinite(coef) and np.isfinite(sigma_w) and sigma_w >= 0):
        raise ValueError("fibre_nl_dev: a and coef must be finite, sigma_w finite and not negative")
    _lib.call("qh_fibre_nl_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], a, coef, pscale.ptr, sigma_w, seed64(seed), out.ptr)
    return out


def ssfm_dev(E, out, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, nf_db=None,
             wl0=1550e-9, seed=0):
    """
    Propagate the (nmodes, L) complex DeviceArray ``E`` (one row, or two: Manakov with 8 / 9) through ``nspans`` identical spans of ``span_length``
    metres by the symmetric split-step Fourier method, into ``out`` (same shape and dtype; it may be ``E``).  ``fs``: sampling rate; ``D``:
    dispersion in s / m / m at ``wl0`` (``beta2`` as ``add_dispersion`` forms it); ``gamma`` in 1 / (W m); ``alpha_db_km`` in dB / km; ``steps``: the
    number of equal steps of a span, or a sequence of step lengths that add up to the span within 1e-9 relative.

    A span is ``D(dz[0] / 2)``, then for every step ``N(dz[i])`` and ``D(dz[i] / 2 + dz[i + 1] / 2)`` (the last ``D(dz[-1] / 2)``), with::

        D(h):  row <- ifft(exp(-0.5j (2 pi f)**2 beta2 h) fft(row)),  f = fftfreq(L, 1 / fs), the phase formed and reduced in double
        N(h):  E[m, n] <- exp(-alpha h / 2) exp(1j kappa gamma pscale h_eff sum_m |E[m, n]|**2) E[m, n],  h_eff = (1 - exp(-alpha h)) / alpha

    ``amplify``: the last ``N`` of a span also multiplies by ``exp(alpha span_length / 2)``, so the power at the end of a span is the launch power.
    ``nf_db``: that amplifier's noise figure - the launch adds white noise of :func:`ase_power` watts per mode, a function of ``seed + s`` for
    span ``s`` (the unit draws of :func:`impair_pointwise_dev`).  The field keeps its normalisation: exactly one of ``pscale`` - watts per unit
    of ``|E|**2`` - and ``power_dbm`` - the launch power over all rows, from which ``pscale = P / sum_m mean_n |E[m, n]|**2`` is formed on the
    device - says what it means in watts.  Every check raises before a launch; the whole loop is enqueued on the current library stream, nothing
    is read back, and a repeated call is bit-identical.  :func:`fibre_plan` counts the launches.
    """
    ase = 0.0
    if nf_db is not None:
        if not np.isfinite(float(nf_db)):
            raise ValueError("ssfm_dev: nf_db must be finite")
        ase = ase_power(nf_db, fibre_alpha(alpha_db_km), span_length, fs, wl0)
    return _fibre_call("ssfm_dev", E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, False, ase, seed)


def dbp_dev(E, out, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, wl0=1550e-9, **kw):
    """
    Digital back-propagation: the algebraic inverse of the noise-free :func:`ssfm_dev` with the same arguments - the steps walked in reverse with
    ``beta2``, ``gamma`` and ``alpha`` negated, and with ``amplify`` the factor ``exp(-alpha span_length / 2)`` in front of the first nonlinear step
    of a span, before its power is taken.  With fewer steps than the link, or a scaled ``gamma``, it is the usual practical back-propagation.
    ``power_dbm`` is then the power of the field as it arrives, which with ``amplify`` is the launch power.  It adds no noise: ``nf_db`` raises
    ValueError.
    """
    if "nf_db" in kw:
        if kw.pop("nf_db") is not None:
            raise ValueError("dbp_dev: back-propagation adds no amplifier noise (nf_db)")
    if kw:
        raise TypeError("dbp_dev: unexpected arguments %s" % sorted(kw))
    return _fibre_call("dbp_dev", E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, True)
