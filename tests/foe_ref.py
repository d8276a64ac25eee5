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


def four_step_split(N):
    """``(N1, N2)`` of the kernel's transform of N = 2^8 .. 2^20 points: one transform, (1, N), up to 2^13; above, N = N1 N2 with
    N1 = 2^floor(lg N / 2)."""
    lg = int(N).bit_length() - 1
    assert N == 1 << lg
    if lg <= 13:
        return 1, N
    N1 = 1 << (lg // 2)
    return N1, N // N1


def split_bins(N):
    """Line bins of the rows of a size's test.  Four-step sizes: bins whose k1 = k mod N1 and k2 = k div N1 differ, so that a spectrum stored
    or read back with N1 and N2 exchanged moves them (N - 1 apart, which both forms keep; duplicates at the square sizes dropped)."""
    N1, N2 = four_step_split(N)
    if N1 == 1:
        cand = [1, N - 1, N // 2 + 3, 5, N // 4 + 2, N // 2 - 7, 3 * N // 4 + 1]
    else:
        cand = [N1, N2, N1 + 1, N - 1, (N1 - 1) + N1, 3 + 5 * N1, N // 2 + N1 + 2]
    bins = []
    for k in cand:
        if k not in bins:
            bins.append(k)
    assert all(0 < k < N for k in bins)
    return bins


def swapped_readback(P, N1, N2):
    """What a kernel returns for the spectrum ``P (rows, N1 N2)`` in bin order that stores bin k = k1 + N1 k2 at position k1 N2 + k2, as
    csrc/foe.hip does, and reads position q back with N1 and N2 exchanged: as bin (q div N1) + N2 (q mod N1) in the peak search, or, which
    is the same permutation, out[k] = S[(k mod N2) N1 + k div N2] in the spectrum kernel.  The identity when N1 = N2."""
    P = np.atleast_2d(P)
    S = P.reshape(-1, N2, N1).transpose(0, 2, 1).reshape(P.shape)                    # S[k1 N2 + k2] = P[k1 + N1 k2]
    return S.reshape(-1, N2, N1).transpose(0, 2, 1).reshape(P.shape)                 # out[b N2 + a] = S[a N1 + b]


def swapped_store(P, N1, N2):
    """The other way round: a kernel that stores with N1 and N2 exchanged - bin k = k1' + N2 k2' at position k1' N1 + k2' - and reads
    back correctly, out[k] = S[(k mod N1) N2 + k div N1].  The inverse permutation of :func:`swapped_readback`."""
    P = np.atleast_2d(P)
    S = P.reshape(-1, N1, N2).transpose(0, 2, 1).reshape(P.shape)                    # S[a N1 + b] = P[a + N2 b]
    return S.reshape(-1, N1, N2).transpose(0, 2, 1).reshape(P.shape)                 # out[b N1 + a] = S[a N2 + b]


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
