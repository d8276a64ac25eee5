"""
Float64 numpy restatement of the chromatic-dispersion filter (qampy_amd/csrc/cd.hip) and of the map from the reference's
CDcomp / add_dispersion parameters to its coefficients (qampy_amd/core/filter.py).

    H(w) = exp(j (c2 w^2 + c1 w + c0)),   w = 2 pi fftfreq(N)   (rad / sample)

circular: overlap-save, output block j = samples [j n, (j + 1) n) (n = N / 2) of a transform over input positions
          j n - N/4 .. j n + n + N/4 - 1 taken modulo L; N == L: one circular transform.
linear:   the reference's zero-padded overlap-add (CDcomp with N > 0), with H in fftfreq order; output length n (L // n).
"""
import numpy as np

C_LIGHT = 2.99792458e8


def beta2(D, wl):
    return D * wl ** 2 / (2 * np.pi * C_LIGHT)


def spread(fs, D, L, wl=1550e-9):
    """CD spread across the sampled band, in samples: 2 pi |beta2 L| fs^2."""
    return 2 * np.pi * abs(beta2(D, wl) * L) * fs ** 2


def coeffs_exact(fs, D, L, wl=1550e-9):
    """add_dispersion's H = exp(-0.5j beta2 L omega^2) on the fftfreq grid, per sample."""
    return -0.5 * beta2(D, wl) * L * fs ** 2, 0.0, 0.0


def coeffs_linspace(fs, D, L, wl, Ntot):
    """CDcomp's H on pi fs linspace(-1, 1, Ntot), read in fftfreq order: omega_ref = a omega + delta, a = Ntot / (Ntot - 1),
    delta = pi fs / (Ntot - 1) for even Ntot and 0 for odd Ntot (where fftshift puts the zero frequency in the middle)."""
    b = beta2(D, wl) * L
    a = Ntot / (Ntot - 1)
    d = np.pi * fs / (Ntot - 1) if Ntot % 2 == 0 else 0.0
    return -0.5 * b * a * a * fs ** 2, -b * a * d * fs, -0.5 * b * d * d


def response(N, c2, c1, c0):
    w = 2 * np.pi * np.fft.fftfreq(N)
    return np.exp(1j * (c2 * w * w + c1 * w + c0))


def cd_filter(E, N, c2, c1, c0, mode="circular"):
    """What the kernel computes, in float64.  E: (nmodes, L) or (L,)."""
    E = np.asarray(E)
    one = E.ndim == 1
    X = np.atleast_2d(E).astype(np.complex128)
    nm, L = X.shape
    H = response(N, c2, c1, c0)
    n, q = N // 2, N // 4
    if mode == "circular":
        if L == N:
            out = np.fft.ifft(np.fft.fft(X, axis=1) * H, axis=1)
        else:
            nblk = -(-L // n)
            idx = (np.arange(nblk)[:, None] * n - q + np.arange(N)[None, :]) % L
            Y = np.fft.ifft(np.fft.fft(X[:, idx], axis=2) * H, axis=2)[:, :, q:q + n]
            out = Y.reshape(nm, nblk * n)[:, :L]
    elif mode == "linear":
        B = L // n
        blocks = np.zeros((nm, B, N), np.complex128)
        blocks[:, :, q:q + n] = X[:, :B * n].reshape(nm, B, n)
        Y = np.fft.ifft(np.fft.fft(blocks, axis=2) * H, axis=2)
        acc = np.zeros((nm, n * (B + 1)), np.complex128)
        for i in range(B):
            acc[:, i * n:i * n + N] += Y[:, i]
        out = acc[:, q:n * (B + 1) - q]
    else:
        raise ValueError(mode)
    return out[0] if one else out


def cdcomp_exact(E, fs, L, D, wl):
    """The reference's CDcomp with N = 0: one circular transform of the whole row on its linspace grid."""
    E = np.asarray(E).ravel()
    return cd_filter(E, E.size, *coeffs_linspace(fs, D, L, wl, E.size))


def cdcomp_blocks(E, fs, N, L, D, wl):
    """The intended CDcomp with N > 0: the reference's blocks with its H in fftfreq (ifftshift) order."""
    return cd_filter(np.asarray(E).ravel(), N, *coeffs_linspace(fs, D, L, wl, N), mode="linear")


def add_dispersion(sig, fs, D, L, wl0=1550e-9):
    """The reference's add_dispersion per row: circular filtering on the fftfreq grid of the row length."""
    X = np.atleast_2d(np.asarray(sig))
    out = cd_filter(X, X.shape[1], *coeffs_exact(fs, D, L, wl0))
    return out[0] if np.asarray(sig).ndim == 1 else out


def bandlimited(nmodes, L, seed, band=0.55):
    """Unit-power complex noise limited to |f| < band * fs / 2: a stand-in for 2-sample/symbol QAM with roll-off 0.1."""
    rng = np.random.default_rng(seed)
    X = np.fft.fft(rng.standard_normal((nmodes, L)) + 1j * rng.standard_normal((nmodes, L)), axis=1)
    X[:, np.abs(np.fft.fftfreq(L)) >= band / 2] = 0
    x = np.fft.ifft(X, axis=1)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))
