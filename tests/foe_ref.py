"""Float64 NumPy restatement of the blind frequency-offset estimator (csrc/foe.hip), written from its contract:

    X_b = FFT_N(x[b N : (b + 1) N] ** 4), b = 0 .. B - 1      block 0 zero-padded when L < N; of a longer row B = 1 reads the first N samples
    P[k] = sum_b |X_b[k]|**2                                  in block order
    bin  = the first maximum of P;  fo = fftfreq(N, 1 / os)[bin] / 4;  optionally the mean over the rows in every row

and of the removal ``x[n] exp(-2j pi (n + 1) fo / os)`` (qampy/core/phaserecovery.py:435-473)."""
import numpy as np


def n_blocks(L, N, blocks):
    return max(1, L // N) if isinstance(blocks, str) and blocks == "all" else int(blocks)


def power_spectrum(x, N, blocks=1):
    """(nmodes, N) float64: the summed power spectra of the fourth power of ``blocks`` blocks of every row."""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    L = x.shape[1]
    B = n_blocks(L, N, blocks)
    assert B == 1 or B * N <= L
    P = np.zeros((x.shape[0], N))
    for b in range(B):
        blk = np.zeros((x.shape[0], N), np.complex128)
        seg = x[:, b * N:(b + 1) * N]
        blk[:, :seg.shape[1]] = seg ** 4
        P += np.abs(np.fft.fft(blk, axis=1)) ** 2
    return P


def find_freq_offset(x, os=1, fft_size=2 ** 16, blocks=1, average_over_modes=True, full=False):
    """(nmodes,) float64 offsets; ``full``: also the bins, the stats (nmodes, 3) = (bin, P[bin], sum P) and P."""
    P = power_spectrum(x, fft_size, blocks)
    bins = np.argmax(P, axis=1)
    fo = (np.fft.fftfreq(fft_size, 1 / os) / 4)[bins]
    if average_over_modes:
        fo = np.mean(fo) * np.ones(fo.shape)
    if not full:
        return fo
    stats = np.stack([bins.astype(np.float64), P[np.arange(P.shape[0]), bins], P.sum(axis=1)], axis=1)
    return fo, bins, stats, P


def peak_ratio(P):
    """Largest over second-largest bin of every row (inf when the second is zero and the first is not; 1 for an all-zero row)."""
    s = np.sort(np.atleast_2d(P), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = s[:, -1] / s[:, -2]
    return np.where(s[:, -1] == 0, 1.0, r)


def comp_freq_offset(x, fo, os=1):
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    t = np.arange(1, x.shape[1] + 1, dtype=float)
    fo = np.broadcast_to(np.asarray(fo, dtype=np.float64).reshape(-1), (x.shape[0],))
    return x * np.exp(-2j * np.pi * t[None, :] * fo[:, None] / os)


def qam_tone(M, nmodes, L, f, seed, snr_db=25., os=1):
    """(nmodes, L) complex128 test rows: square M-QAM symbols at unit power plus noise at ``snr_db``, rotated by ``exp(2j pi f[row] n)`` (``f`` in
    cycles per sample, one per row or one for all) and rounded to multiples of 2^-12, so that complex64 and complex128 hold the same values."""
    rng = np.random.default_rng(seed)
    m = int(round(np.sqrt(M)))
    lev = 2 * np.arange(m) - (m - 1)
    s = rng.choice(lev, (nmodes, L)) + 1j * rng.choice(lev, (nmodes, L))
    s = s / np.sqrt(np.mean(np.abs(lev) ** 2) * 2)
    s = np.repeat(s[:, :(L + os - 1) // os], os, axis=1)[:, :L] if os > 1 else s
    sig = 10 ** (-snr_db / 20) / np.sqrt(2)
    s = s + sig * (rng.standard_normal((nmodes, L)) + 1j * rng.standard_normal((nmodes, L)))
    f = np.broadcast_to(np.asarray(f, dtype=np.float64).reshape(-1), (nmodes,))
    s = s * np.exp(2j * np.pi * f[:, None] * np.arange(L)[None, :])
    return np.round(s * 4096) / 4096
