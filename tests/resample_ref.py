"""
Float64 numpy restatement of the polyphase resampler (qampy_amd/csrc/resample.hip) and of the filters the reference feeds it
(qampy/core/resample.py, qampy/core/filter.py rrcos_pulseshaping, scipy.signal.resample_poly's default design).

    up, down = Fraction(fnew / fold).limit_denominator();  real taps h[0..T-1];  half = (T - 1) // 2;  x zero outside [0, n)
    n_out = ceil(n up / down)
    y[k]  = g sum_m h[k down + half - m up] x[m]

g = up: resample_poly(x, up, down, window=h) and rrcos_resample(fftconv=False); g = 1: rrcos_resample(fftconv=True), and with
up = down = 1 rrcos_pulseshaping.  Evaluated phase by phase: p = (k down + half) % up, m0 = (k down + half) // up,
y[k] = g (x * h[p::up])[m0].
"""
import fractions

import numpy as np


def factors(fold, fnew):
    r = fractions.Fraction(fnew / fold).limit_denominator()
    return r.numerator, r.denominator


def n_out(n, up, down):
    return -(-n * up // down)


def phase_major(h, up):
    """tab[p, j] = h[p + j up], zero-padded to J = ceil(T / up)."""
    h = np.asarray(h, dtype=np.float64)
    J = -(-h.size // up)
    tab = np.zeros((up, J))
    for p in range(up):
        hp = h[p::up]
        tab[p, :hp.size] = hp
    return tab


def resample(x, h, up, down, gain=1.0, nout=None):
    """What the kernel computes, in float64.  x: (nmodes, n) or (n,); the first ``nout`` outputs of every row."""
    x = np.asarray(x)
    one = x.ndim == 1
    X = np.atleast_2d(x).astype(np.complex128)
    h = np.asarray(h, dtype=np.float64)
    n, half = X.shape[1], (h.size - 1) // 2
    nout = n_out(n, up, down) if nout is None else nout
    a = np.arange(nout, dtype=np.int64) * down + half
    p, m0 = a % up, a // up
    tab = phase_major(h, up)
    out = np.zeros((X.shape[0], nout), np.complex128)
    for r in range(X.shape[0]):
        for ph in range(up):
            c = np.convolve(X[r], tab[ph])                  # c[m] = sum_j tab[ph, j] x[m - j]
            sel = np.nonzero((p == ph) & (m0 < c.size))[0]
            out[r, sel] = c[m0[sel]]
    out *= gain
    return out[0] if one else out


def rrcos_time(t, beta, T):
    """Root-raised-cosine impulse response with its limits at t = 0 and |t| = T / (4 beta).  As in the reference, a sample within a
    quarter of the grid spacing of such a point takes the limit (at 80 GS/s and T = 1 / 28e9 that moves samples +-7, 0.05 T off)."""
    x = np.asarray(t, dtype=np.float64) / T
    out = np.empty_like(x)
    eps = abs(x[1] - x[0]) / 4 if x.size > 1 else 1e-9
    for i, v in enumerate(x):
        if abs(v) < eps:
            out[i] = 1 + beta * (4 / np.pi - 1)
        elif abs(abs(v) - 1 / (4 * beta)) < eps:
            a = np.pi / (4 * beta)
            out[i] = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(a) + (1 - 2 / np.pi) * np.cos(a))
        else:
            out[i] = (np.sin(np.pi * v * (1 - beta)) + 4 * beta * v * np.cos(np.pi * v * (1 + beta))) / (np.pi * v * (1 - (4 * beta * v) ** 2))
    return out / T


def rrcos_taps(taps, fs, T, beta):
    t = (np.arange(taps) - (taps - 1) // 2) / fs
    h = rrcos_time(t, beta, T)
    return h / h.max()


def default_window(up, down):
    """scipy's resample_poly design before its scaling by up: Kaiser(5.0)-windowed sinc, cutoff 1 / max(up, down), unit DC gain."""
    mx = max(up, down)
    m = np.arange(-10 * mx, 10 * mx + 1)
    h = np.sinc(m / mx) / mx * np.kaiser(m.size, 5.0)
    return h / h.sum()


def renormalise(out, x):
    """normalise_and_center(out) * sqrt(mean |x|^2), per row."""
    out, x = np.atleast_2d(out), np.atleast_2d(x)
    c = out - out.mean(axis=1, keepdims=True)
    c /= np.sqrt(np.mean(np.abs(c) ** 2, axis=1, keepdims=True))
    return c * np.sqrt(np.mean(np.abs(x) ** 2, axis=1, keepdims=True))


def rrcos_resample(x, fold, fnew, Ts=None, beta=None, taps=4001, renorm=False, fftconv=True):
    up, down = factors(fold, fnew)
    x = np.asarray(x)
    if beta is None:
        return np.array(x, dtype=np.complex128) if up == down == 1 else resample(x, default_window(up, down), up, down, up)
    Ts = 1 / fold if Ts is None else Ts
    if not fftconv and up == down == 1:
        y = np.array(x, dtype=np.complex128)
    else:
        y = resample(x, rrcos_taps(taps, up * fold, Ts, beta), up, down, 1 if fftconv else up)
    if renorm:
        y = renormalise(y, x).reshape(y.shape)
    return y


def unit_noise(nmodes, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nmodes, n)) + 1j * rng.standard_normal((nmodes, n))
    return x / np.sqrt(np.mean(np.abs(x) ** 2))
