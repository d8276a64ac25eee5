"""
Constellation tables, equaliser constants and the theory curves: the call surface of QAMpy's ``theory`` module.

First the tables whose *values* are inputs of the equaliser and BPS kernels (also the constants of
``core.equalisation``), pinned bit-for-bit by ``tests/golden/constants.npz`` which was captured from the reference.  Then, under the reference's
names, the closed-form SER / BER curves (host numpy / scipy), the probabilistic-shaping pair and the Monte-Carlo GMI / MI curves, which run on the
GPU (``core.hip_dsp.awgn_mc``); they are held to the reference's values by ``tests/golden/theory.npz``.

Reference behaviour restated (file:line in /root/reference):
  * ``cal_symbols_qam``            qampy/theory.py:111-118, 150-177
  * ``cal_scaling_factor_qam``     qampy/theory.py:139-148
  * ``gray_code_qam``              qampy/theory.py:180-192, qampy/core/utils.py:195-200
  * Gray-label ordered alphabet    qampy/signals.py:831-845 (``coded_symbols``)
  * CMA / MCMA constants           qampy/core/equalisation/equalisation.py:271-281
  * RDE / MRDE codes + partitions  qampy/core/equalisation/equalisation.py:311-359
"""
import numpy as np


def _is_cross(M):
    nbits = int(round(np.log2(M)))
    if 2 ** nbits != M:
        raise ValueError("M must be a power of two, got %r" % (M,))
    return bool(nbits % 2)


def _square_points(M):
    side = int(round(np.sqrt(M)))
    lev = np.arange(-(side - 1), side, 2, dtype=np.float64)
    # raster order of the reference: real part is the slow axis, imaginary part the fast axis
    re = np.repeat(lev, side)
    im = np.tile(lev, side)
    return re + 1j * im


def _cross_points(M):
    nbits = int(round(np.log2(M)))
    n = (nbits - 1) // 2
    if n < 1:
        raise ValueError("cross QAM needs M >= 8")
    s = 2.0 ** (n - 1)
    wide = 2 ** (n + 1)
    tall = 2 ** n
    re = np.repeat(np.arange(-(wide - 1), wide, 2, dtype=np.float64), tall)
    im = np.tile(np.arange(-(tall - 1), tall, 2, dtype=np.float64), wide)
    are, aim = np.abs(re), np.abs(im)
    outer = are > 3 * s
    corner = outer & (aim > s)
    edge = outer & (aim <= s)
    new_re = np.where(corner, np.sign(re) * (are - 2 * s), np.where(edge, np.sign(re) * (4 * s - are), re))
    new_im = np.where(corner, np.sign(im) * (4 * s - aim), np.where(edge, np.sign(im) * (aim + 2 * s), im))
    return new_re + 1j * new_im


def cal_symbols_qam(M):
    """Un-normalised M-QAM constellation in the reference's raster order (qampy/theory.py:111-118)."""
    return _cross_points(M) if _is_cross(M) else _square_points(M)


def cal_scaling_factor_qam(M):
    """Mean power of the un-normalised constellation (qampy/theory.py:139-148)."""
    if _is_cross(M):
        return (np.abs(cal_symbols_qam(M)) ** 2).mean()
    return 2 / 3 * (M - 1)


def normalised_symbols_qam(M):
    """``cal_symbols_qam(M)/sqrt(scale)`` exactly as equalisation.py:117-125 evaluates it (complex / real)."""
    syms = cal_symbols_qam(M)
    syms /= np.sqrt(cal_scaling_factor_qam(M))
    return syms


def gray_code_qam(M):
    """Gray labels of the raster-ordered constellation (qampy/theory.py:180-192)."""
    nbits = int(round(np.log2(M)))
    n_im = nbits // 2
    n_re = nbits - n_im
    a = np.repeat(np.arange(2 ** n_re), 2 ** n_im)
    b = np.tile(np.arange(2 ** n_im), 2 ** n_re)
    ga = a ^ (a >> 1)
    gb = b ^ (b >> 1)
    return (ga << n_im) | gb


def coded_symbols_qam(M, dtype=np.complex128):
    """
    Unit-power alphabet in Gray-label order, i.e. what ``SignalQAMGrayCoded.coded_symbols`` holds
    (qampy/signals.py:831-845, :662).  Entry ``g`` is the point whose Gray label is ``g``.
    """
    syms = cal_symbols_qam(M).astype(dtype)
    syms /= np.sqrt(cal_scaling_factor_qam(M))
    code = gray_code_qam(M)
    inv = np.zeros_like(code)
    inv[code] = np.arange(code.size)
    return syms[inv]


# --------------------------------------------------------------------------- equaliser constants
def cal_Rconstant(M):
    """CMA radius <|s|^4>/<|s|^2> (equalisation.py:271-275)."""
    s = normalised_symbols_qam(M)
    return np.mean(abs(s) ** 4) / np.mean(abs(s) ** 2)


def cal_Rconstant_complex(M):
    """MCMA per-quadrature radius (equalisation.py:277-281)."""
    s = normalised_symbols_qam(M)
    return np.mean(s.real ** 4) / np.mean(s.real ** 2) + 1.j * np.mean(s.imag ** 4) / np.mean(s.imag ** 2)


def generate_partition_codes_complex(M):
    """MRDE codes then partitions, real axis in .real and imaginary axis in .imag (equalisation.py:311-336)."""
    s = normalised_symbols_qam(M)
    # NB: the reference forms |x|^4/|x|^2 (not |x|^2) before np.unique, which leaves float-duplicates for
    # some M; the tables are pinned by golden constants, so the same expression is evaluated here.
    cr = np.unique(abs(s.real) ** 4 / abs(s.real) ** 2)
    ci = np.unique(abs(s.imag) ** 4 / abs(s.imag) ** 2)
    codes = cr + 1.j * ci
    pr = cr[:-1] + np.diff(cr) / 2
    pi = ci[:-1] + np.diff(ci) / 2
    return np.hstack([codes, pr + 1.j * pi])


def generate_partition_codes_radius(M):
    """RDE codes then partitions on |s|^2 (equalisation.py:338-359)."""
    s = normalised_symbols_qam(M)
    codes = np.unique(abs(s) ** 4 / abs(s) ** 2)
    parts = codes[:-1] + np.diff(codes) / 2
    return np.hstack([codes, parts])


# --------------------------------------------------------------------------- theory curves
# The analytic and Monte-Carlo curves of qampy/theory.py (:34-109, :120-137, :195-334) under the reference's names.  The closed forms are host
# numpy / scipy, written from the formulas (they agree with the reference's values to 1e-12); the Monte-Carlo curves (cal_gmi, sim_mi_mc) run on the GPU only (hip_dsp.awgn_mc, one
# launch for all SNR points), like the other drop-ins of the compiled module.  Three functions of the reference cannot run as written -
# generate_ps_symbols(normalize=True) and hybrid_qam_ber_vs_esn0 raise NameError, sim_mi_mc rescales its argument in place - and are built here
# to their evident intent; their docstrings say how.
def cal_symbols_square_qam(M):
    """Un-normalised square M-QAM points in the reference's raster order (qampy/theory.py:151-158)."""
    return _square_points(M)


def cal_symbols_cross_qam(M):
    """Un-normalised cross M-QAM points in the reference's raster order (qampy/theory.py:161-178)."""
    return _cross_points(M)


def cal_symbols_psk(M):
    """M-PSK points of unit power, counter-clockwise from phase 0; QPSK alone sits on the diagonals (first point at pi / 4), as the reference's."""
    phase = 2 * np.pi * np.arange(M) / M
    if M == 4:
        phase = phase + np.pi / 4
    return np.exp(1j * phase)


def _rail_argument(snr, M):
    """``d / (2 sigma)`` of one rail of square M-QAM at the linear Es / N0 ``snr``: half the level spacing over the rail's noise deviation,
    ``sqrt(3 snr / (M - 1))``."""
    return np.sqrt(3 * np.asarray(snr, dtype=np.float64) / (M - 1))


def _ber_square_qam(snr, M):
    """Shafik's (2006) nearest-neighbour bit error rate of Gray-coded square M-QAM: the share ``1 - 1 / sqrt(M)`` of rail levels with a neighbour on
    a given side, two sides, one bit of the rail's ``log2 sqrt(M)`` per error, times the tail ``Q(d / sigma)``."""
    from .core.special_fcts import q_function
    side = np.sqrt(M)
    return 2 * (1 - 1 / side) / np.log2(side) * q_function(_rail_argument(snr, M))


def ser_vs_es_over_n0_qam(snr, M):
    """Symbol error rate of square M-QAM against the linear Es / N0 (the reference's ``ser_vs_es_over_n0_qam``; right for M > 4 only): a rail
    errs with ``P = (1 - 1 / sqrt(M)) erfc(sqrt(3 snr / (2 (M - 1))))`` and the symbol with ``1 - (1 - P)**2``."""
    from scipy.special import erfc
    rail = (1 - 1 / np.sqrt(M)) * erfc(_rail_argument(snr, M) / np.sqrt(2))
    return rail * (2 - rail)


def ber_vs_evm_qam(evm_dB, M):
    """Bit error rate of M-QAM against the EVM in dB, ``10 log10(P_error / P_reference)`` (the reference's ``ber_vs_evm_qam``, after Shafik 2006):
    :func:`ber_vs_es_over_n0_qam` at the SNR ``1 / EVM``."""
    from .helpers import dB2lin
    return _ber_square_qam(1 / dB2lin(np.asarray(evm_dB, dtype=np.float64)), M)


def ber_vs_es_over_n0_qam(snr, M):
    """Bit error rate of M-QAM against the linear SNR (the reference's ``ber_vs_es_over_n0_qam``, after Shafik 2006)."""
    return _ber_square_qam(snr, M)


def ser_vs_es_over_n0_psk(snr, M):
    """Symbol error rate of M-PSK against the linear Es / N0: the tail beyond the half-distance ``sqrt(snr) sin(pi / M)`` to either neighbour."""
    from scipy.special import erfc
    half_distance = np.sin(np.pi / M) * np.sqrt(snr)
    return erfc(half_distance)


def ser_vs_es_over_n0_4pam(snr):
    """Symbol error rate of 4-PAM against the linear Es / N0: levels -3 .. 3 (mean power 5), six of the eight level sides have a neighbour."""
    from scipy.special import erfc
    return 6 / 8 * erfc(np.sqrt(np.asarray(snr, dtype=np.float64) / 5))


def hybrid_qam_ber_vs_esn0(snr, pr, fr, M1, M2):
    """
    Bit error rate of time-domain hybrid QAM against the SNR in dB (qampy/theory.py:250-280, after Curri et al., OFC 2014): ``pr`` the ratio of the
    mean powers of the M1 and the M2 symbols, ``fr`` the fraction of M2 symbols in the frame.

    The reference's body calls ``theory.MQAM_BERvsEsN0``, a name that does not exist (``NameError``); the formula is written here with
    :func:`ber_vs_es_over_n0_qam`, the function that name evidently stood for.
    """
    snr = 10 ** (np.asarray(snr, dtype=np.float64) / 10)
    bps1, bps2 = np.log2(M1), np.log2(M2)
    mix = (1 - fr) + fr * pr
    return 1 / ((1 - fr) * bps1 + fr * bps2) * ((1 - fr) * bps1 * ber_vs_es_over_n0_qam(snr / mix, M1) + fr * bps2 * ber_vs_es_over_n0_qam(pr * snr / mix, M2))


def cal_ps_probablts(symbols, nu):
    """``(levels, px)`` of probabilistic shaping: the distinct real parts of ``symbols``, ascending, and their Maxwell-Boltzmann probabilities
    ``exp(-nu level**2)`` normalised to sum 1 (the reference's function of this name)."""
    levels = np.unique(np.real(symbols))
    weight = np.exp(-nu * levels ** 2)
    return levels, weight / weight.sum()


def generate_ps_symbols(N, symbs, px, normalize=True, seed=None, method="pyt"):
    """
    ``N`` probabilistically shaped symbols (an int, or ``(nmodes, N)`` for rows): real and imaginary part each one of the levels ``symbs`` with the
    probabilities ``px`` (qampy/theory.py:224-248).

    ``method="pyt"``: numpy, ``np.random.default_rng(seed).choice`` for the real, then for the imaginary parts (the reference draws from numpy's
    global generator and takes no seed).  ``method="hip"``: the counter-based device source (``hip_dsp.ps_symbols_dev``, complex128), read back.
    ``normalize``: every row minus its mean, scaled to unit power.  The reference calls ``utils.normalise_and_center`` without importing ``utils``
    (``NameError``); :func:`qampy_amd.helpers.normalise_and_center` is what it meant - on the device path the resampler's row moments and
    centre-and-scale kernels do the same on the resident rows.
    """
    shape = (int(N),) if np.ndim(N) == 0 else tuple(int(n) for n in N)
    if len(shape) not in (1, 2) or min(shape) < 1:
        raise ValueError("generate_ps_symbols: N is a positive length or (nmodes, N)")
    symbs, px = np.asarray(symbs, dtype=np.float64), np.asarray(px, dtype=np.float64)
    if symbs.ndim != 1 or symbs.shape != px.shape:
        raise ValueError("generate_ps_symbols: one probability per level")
    if method == "pyt":
        rng = np.random.default_rng(seed)
        out = rng.choice(symbs, shape, p=px) + 1j * rng.choice(symbs, shape, p=px)
        if normalize:
            from .helpers import normalise_and_center
            out = normalise_and_center(out).reshape(shape)
        return out
    if method != "hip":
        raise ValueError("generate_ps_symbols: method is 'pyt' (numpy) or 'hip' (device), not %r" % (method,))
    from ._lib import DeviceArray
    from .core import hip_dsp, resample
    hip_dsp.ps_cdf(px)                                       # the checks, before the device is touched
    out = DeviceArray(shape, np.complex128)
    hip_dsp.ps_symbols_dev(out, symbs, px, seed)
    if normalize:
        resample.center_scale_dev(out, resample.row_moments_dev(out))
    return out.to_host()


def cal_gmi(M, snr, N=10 ** 3, seed=None, dtype=np.complex128, per_bit=False):
    """
    Soft-decision GMI of Gray-coded M-QAM over AWGN by the Monte-Carlo method of ``pythran_dsp.cal_gmi_mc`` (qampy/theory.py:282-310): ``snr`` in
    dB, a scalar or an array; the result is an array with one value per SNR, as the reference's.  ``N`` noise draws per SNR point, every point with
    draws of its own; all points go through one launch (``hip_dsp.awgn_mc``).  ``seed``: the draws are a function of (seed, point, draw) - None
    takes a fresh seed, as the reference's unseeded ``randn``.  ``dtype``: the precision of the kernel.  ``per_bit``: return ``(gmi, gmi_per_bit)``,
    the second ``(nsnr, nbits)``.  GPU only.
    """
    from .core import hip_dsp
    snr = np.atleast_1d(np.asarray(snr, dtype=np.float64))
    res = hip_dsp.awgn_mc(np.ascontiguousarray(coded_symbols_qam(M, dtype=dtype)), 10 ** (snr / 10), N, seed=seed)
    return (res[:, 0], res[:, 2:]) if per_bit else res[:, 0]


def sim_mi_mc(symbols, snr, N, seed=None):
    """
    Monte-Carlo mutual information of the alphabet ``symbols`` over AWGN at ``snr`` dB with ``N`` noise draws (qampy/theory.py:312-334): a float
    for a scalar ``snr``, an array for an array.  The alphabet (complex, or real as the reference also takes) is normalised to unit power - a copy
    of it: the reference divides the caller's array in place, so a second call sees other symbols, which is not reproduced.  ``seed`` as in
    :func:`cal_gmi`.  GPU only.  ``2**nbits`` points (up to 1024) take the Monte-Carlo kernel's MI column, all SNRs in one launch.

    Beyond the reference's use with QAM alphabets: the reference's loop takes any number of points, so an alphabet that is no power of two (up to
    1024 points) is served too, by the same draws (``hip_dsp.awgn_mc_noise_dev``, read back) through the general ``hip_dsp.cal_mi_mc`` kernel, one
    call per SNR.
    """
    from . import _lib
    from .core import hip_dsp
    sy = np.array(symbols, copy=True)
    if sy.ndim != 1 or sy.size < 1 or sy.dtype.kind not in "fciu":
        raise TypeError("sim_mi_mc: symbols is a 1-d numeric alphabet")
    if sy.dtype != np.complex64:
        sy = sy.astype(np.complex128)
    sy /= np.sqrt(np.mean(abs(sy) ** 2))
    snr_db = np.asarray(snr, dtype=np.float64)
    lin = 10 ** (np.atleast_1d(snr_db) / 10)
    M = sy.size
    if M & (M - 1) == 0 and 2 <= M <= 1024:
        mi = hip_dsp.awgn_mc(sy, lin, N, seed=seed)[:, 1]
    else:
        lin = hip_dsp.theory._mc_snr(lin, "sim_mi_mc")
        z = hip_dsp.awgn_mc_noise_dev(_lib.DeviceArray((lin.size, int(N)), sy.dtype), lin, seed).to_host()
        mi = np.array([hip_dsp.cal_mi_mc(z[p], sy, 1 / lin[p]) for p in range(lin.size)])
    return float(mi[0]) if snr_db.ndim == 0 else mi
