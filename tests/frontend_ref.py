"""Float64 numpy restatement of the device algorithms of csrc/fft.hip and csrc/iq.hip: the same splits, the same integer chirp, the same
closed forms - what the kernels compute, written so that numpy can be held against it on a machine without a GPU."""
import numpy as np

FH_BRICK, FH_BAND, FH_TWORAIL, FH_RAMP = 1, 2, 3, 4


def plan(L):
    """(M, N1, N2, bluestein) as csrc/fft.hip's fft_plan."""
    L = int(L)
    pow2 = L & (L - 1) == 0 and L >= 256
    if L < 2 or (pow2 and L > 2 ** 24) or (not pow2 and L > 2 ** 23):
        raise ValueError("length out of range")
    lg = 8
    while (1 << lg) < (L if pow2 else 2 * L - 1):
        lg += 1
    lg1 = lg // 2 if lg > 13 else 0
    return 1 << lg, 1 << lg1, 1 << (lg - lg1), not pow2


def ramp(turns):
    """exp(-2 pi i t), the turn reduced in double first."""
    t = np.asarray(turns, np.float64)
    t = t - np.rint(t)
    return np.cos(2 * np.pi * t) - 1j * np.sin(2 * np.pi * t)


def four_step(x, N1, N2):
    """FFT of the rows of x (rows, N1 N2): columns n2 of the (N1, N2) view over n1, times W^(k1 n2) with the exact turn k1 n2 / N, rows over
    n2, bin k1 + N1 k2."""
    rows, N = x.shape
    assert N == N1 * N2
    T = np.fft.fft(x.reshape(rows, N1, N2), axis=1)                       # [k1][n2]
    k1n2 = np.arange(N1, dtype=np.int64)[:, None] * np.arange(N2, dtype=np.int64)[None, :]
    T = T * ramp(k1n2.astype(np.float64) / N)
    Y = np.fft.fft(T, axis=2)                                             # [k1][k2]
    return Y.transpose(0, 2, 1).reshape(rows, N)                          # k = k1 + N1 k2


def fft_pow2(x, dtype=np.complex128):
    M, N1, N2, blue = plan(x.shape[1])
    assert not blue
    y = np.fft.fft(x, axis=1) if N1 == 1 else four_step(x, N1, N2)
    return y.astype(dtype)


def chirp(L, dtype=np.complex128):
    """exp(-i pi n^2 / L), n^2 mod 2 L in integers, cast to the signal's precision."""
    n = np.arange(L, dtype=np.uint64)
    m = (n * n) % np.uint64(2 * L)
    return ramp(m.astype(np.float64) / (2 * L)).astype(dtype)


def _fft_M(x, dtype):
    """the size-M transform in the signal's precision (scipy keeps complex64)"""
    import scipy.fft as sf
    M, N1, N2, _ = plan(x.shape[1])
    if dtype == np.complex128 and N1 > 1:
        return four_step(x, N1, N2)
    return sf.fft(x.astype(dtype), axis=1)


def bluestein(x, inverse=False, dtype=np.complex128):
    """DFT (inverse: numpy's ifft) of the rows of x by the chirp transform, step by step as the device takes them."""
    x = np.atleast_2d(x).astype(dtype)
    rows, L = x.shape
    M, _, _, blue = plan(L)
    assert blue
    w = chirp(L, dtype)
    b = np.zeros((1, M), dtype)
    b[0, :L] = np.conj(w)
    b[0, M - L + 1:] = np.conj(w[1:][::-1])
    Bhat = _fft_M(b, dtype).astype(dtype)
    a = np.zeros((rows, M), dtype)
    a[:, :L] = (np.conj(x) if inverse else x) * w
    W = np.conj(_fft_M(a, dtype).astype(dtype) * Bhat).astype(dtype)
    F = _fft_M(W, dtype).astype(dtype)[:, :L]
    if inverse:
        return (F * np.conj(w) * dtype(1).real.dtype.type(1.0 / M / L)).astype(dtype)
    return (np.conj(F * np.conj(w)) * dtype(1).real.dtype.type(1.0 / M)).astype(dtype)


def fft(x, inverse=False, dtype=np.complex128):
    x = np.atleast_2d(x)
    if plan(x.shape[1])[3]:
        return bluestein(x, inverse, dtype)
    if inverse:
        return (np.conj(fft_pow2(np.conj(x))) / x.shape[1]).astype(dtype)
    return fft_pow2(x, dtype)


def signed_bins(L):
    k = np.arange(L, dtype=np.int64)
    return np.where(k < (L - 1) // 2 + 1, k, k - L)


def pre_filter_bins(L, bw):
    c = int(L / (bw / 2))
    lo, hi, _ = slice(c, -c).indices(L)
    return (lo, hi) if hi > lo else (0, 0)


def H_brick(L, bw):
    lo, hi = pre_filter_bins(L, bw)
    j = (np.arange(L) + L // 2) % L
    return ((j >= lo) & (j < hi)).astype(np.float64)


def H_band(L, bw, os, center_freq=0):
    f = signed_bins(L) * (1.0 / (L * (1 / os)))
    return (np.abs(f - center_freq) < bw / 2).astype(np.float64)


def H_ramp(L, delay, sampling_rate):
    f = signed_bins(L) * (1.0 / (L * (sampling_rate / 2)))
    return ramp(delay * f)


def two_rail(X, Hi, Hq):
    """Y[k] = Hi_s[k] (X[k] + conj X[-k]) / 2 + Hq_s[k] (X[k] - conj X[-k]) / 2,  H_s[k] = (H[k] + conj H[-k]) / 2"""
    L = X.shape[-1]
    neg = (-np.arange(L)) % L
    Xm = np.conj(X[..., neg])
    His, Hqs = (Hi + np.conj(Hi[neg])) / 2, (Hq + np.conj(Hq[neg])) / 2
    return His * (X + Xm) / 2 + Hqs * (X - Xm) / 2


def skew(x, delay_i, delay_q, sampling_rate):
    x = np.atleast_2d(x).astype(np.complex128)
    L = x.shape[1]
    Y = two_rail(fft(x), H_ramp(L, delay_i, sampling_rate), H_ramp(L, delay_q, sampling_rate))
    return fft(Y, inverse=True)


def spectral(x, H):
    x = np.atleast_2d(x).astype(np.complex128)
    return fft(fft(x) * H, inverse=True)


def moments(x, os=1):
    """(rows, 10): sum I, Q, I^2, Q^2, IQ over all samples, then over every os-th."""
    x = np.atleast_2d(x).astype(np.complex128)
    out = []
    for v in (x, x[:, ::os]):
        I, Q = v.real, v.imag
        out += [I.sum(1), Q.sum(1), (I * I).sum(1), (Q * Q).sum(1), (I * Q).sum(1)]
    return np.stack(out, axis=1)


def coeffs_orthonormalize(mom, L, os):
    """(rows, 6): a00, a01, a10, a11, b0, b1 of orthonormalize_signal's map."""
    n, ns = float(L), float((L + os - 1) // os)
    m = mom.T
    mI, mQ = m[0] / n, m[1] / n
    PI, PQ, PIQ = m[2] / n - mI * mI, m[3] / n - mQ * mQ, m[4] / n - mI * mQ
    a, d, g = 1 / np.sqrt(PI), 1 / np.sqrt(PQ), PIQ / (PI * np.sqrt(PQ))
    sI, sQ = m[5] / ns, m[6] / ns
    VI, VQ, VIQ = m[7] / ns - sI * sI, m[8] / ns - sQ * sQ, m[9] / ns - sI * sQ
    s = 1 / np.sqrt(a * a * VI + d * d * VQ - 2 * d * g * VIQ + g * g * VI)
    a00, a10, a11 = s * a, -s * g, s * d
    return np.stack([a00, 0 * a00, a10, a11, -a00 * sI, -(a10 * sI + a11 * sQ)], axis=1)


def coeffs_imbalance(mom, L, centre_only=False):
    """the pooled map of comp_IQ_inbalance, the same for every row"""
    rows = mom.shape[0]
    t = mom[:, :5].sum(0)
    n = float(L) * rows
    mI, mQ = t[0] / n, t[1] / n
    c2, c3 = 0.0, 1.0
    if not centre_only:
        SII, SQQ, SIQ = t[2] - n * mI * mI, t[3] - n * mQ * mQ, t[4] - n * mI * mQ
        sn = -(SIQ / SII)
        cs = np.sqrt(1 - sn * sn)
        g = np.sqrt(SII / ((SQQ + 2 * sn * SIQ + sn * sn * SII) / (cs * cs)))
        c2, c3 = g * sn / cs, g / cs
    return np.tile([1.0, 0.0, c2, c3, -mI, -(c2 * mI + c3 * mQ)], (rows, 1))


def affine(x, coef):
    x = np.atleast_2d(x).astype(np.complex128)
    c = coef[:, :, None]
    return (c[:, 0] * x.real + c[:, 1] * x.imag + c[:, 4]) + 1j * (c[:, 2] * x.real + c[:, 3] * x.imag + c[:, 5])


def orthonormalize(x, os=1):
    x = np.atleast_2d(x)
    return affine(x, coeffs_orthonormalize(moments(x, os), x.shape[1], os))


def comp_iq_imbalance(x):
    x = np.atleast_2d(x)
    return affine(x, coeffs_imbalance(moments(x), x.shape[1]))
