"""numpy restatement, in float64, of the theory kernels: the Monte-Carlo GMI / MI of csrc/metrics.hip (awgn_mc_kernel) and the shaped source of
csrc/source.hip (ps_symbols_kernel).

``gmi_mc`` is ``pythran_dsp.cal_gmi_mc`` and ``cal_mi_mc`` on given draws (tests/test_theory_ref.py holds it to the reference's values): with
``y = s_i + conj(z_l)`` the reference's exponent ``|s_i - s_j|^2 + 2 Re(z_l (s_i - s_j))`` is ``|y - s_j|^2 - |z_l|^2``.  Every sum of
exponentials is a log-sum-exp about its own largest exponent, so the result is finite at any SNR and for any draw."""
import numpy as np

import impair_ref as ir

STREAM_MC, STREAM_SHAPE = 3, 4
CHUNK = 1 << 22                    # distances held at once


def nbits(M):
    nb = int(round(np.log2(M)))
    assert 2 ** nb == M
    return nb


def _lse2(a, axis=-1, where=None):
    """log2 sum 2^a along the axis (over the entries where ``where`` holds), about the largest exponent"""
    if where is not None:
        a = np.where(where, a, -np.inf)
    m = a.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log2(np.sum(np.exp2(a - m), axis=axis))


def gmi_mc(alphabet, snr, z):
    """``(gmi, gmi_per_bit, mi)`` of the alphabet (label order: point g carries label g, bit k MSB first) at the linear ``snr`` over the draws
    ``z``: gmi = nbits - sum_k sum_(i, l) log2(S_all / S_(k, side of i)) / (M ns), mi = log2 M - sum_(i, l) log2(S_all / e_i) / (M ns)."""
    s = np.asarray(alphabet, np.complex128).ravel()
    z = np.asarray(z, np.complex128).ravel()
    M, ns = s.size, z.size
    nb = nbits(M)
    g = np.arange(M)
    own = [(((g[:, None] ^ g[None, :]) >> (nb - 1 - k)) & 1) == 0 for k in range(nb)]         # [k][i, g]: g on the side of i
    bit_sums, mi_sum = np.zeros(nb), 0.0
    step = max(1, CHUNK // (M * M))
    for a in range(0, ns, step):
        y = s[:, None] + np.conj(z[None, a:a + step])                                          # (M, c)
        e = -float(snr) * np.abs(y[:, :, None] - s[None, None, :]) ** 2 * np.log2(np.e)       # (M, c, M): exponents to base 2
        all_ = _lse2(e)
        mi_sum += np.sum(all_ - e[g, :, g])
        for k in range(nb):
            bit_sums[k] += np.sum(all_ - _lse2(e, where=own[k][:, None, :]))
    per_bit = 1 - bit_sums / (M * ns)
    return nb - bit_sums.sum() / (M * ns), per_bit, np.log2(M) - mi_sum / (M * ns)


def mc_noise(seed, snr, ns, wide):
    """The draws of awgn_mc_noise_kernel in float64: z[p, l] = (g0 + 1j g1) sqrt(1 / (2 snr_p)) from counter (l, p, STREAM_MC); also the radii."""
    snr = np.atleast_1d(np.asarray(snr, np.float64))
    z, r = np.empty((snr.size, ns), np.complex128), np.empty((snr.size, ns))
    for p in range(snr.size):
        g0, g1, r[p] = ir.gauss(seed, p, np.arange(ns), STREAM_MC, wide)
        z[p] = (g0 + 1j * g1) * np.sqrt(1.0 / (2.0 * snr[p]))
    return z, r


def shaped_cdf(px):
    px = np.asarray(px, np.float64)
    cdf = np.cumsum(px) / px.sum()
    cdf[-1] = 1.0
    return cdf


def shaped_indices(seed, mode, n, px):
    """(I index, Q index) of the samples ``n`` of ``mode``: words x and y of counter (n, mode, STREAM_SHAPE) -> u = word 2^-32 -> the number of
    cumulative entries <= u."""
    x, y, _, _ = ir.words(seed, mode, n, STREAM_SHAPE)
    cdf = shaped_cdf(px)
    return (np.searchsorted(cdf, x.astype(np.float64) * 2.0 ** -32, side="right"),
            np.searchsorted(cdf, y.astype(np.float64) * 2.0 ** -32, side="right"))
