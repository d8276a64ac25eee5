"""numpy restatement of the channel impairments of qampy_amd/csrc/impair.hip, in float64 / complex128: the deterministic stages
(rotation, PMD whole-row and overlap-save, carrier offset, modal delay, their order) and the counter-based Gaussian draws (Philox4x32-10 +
Box-Muller from the same counters as the device)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_PHASE, STREAM_NOISE = 1, 2
TILE = 1024                       # samples of one mode per workgroup of the point-wise pass
PMD_N = 8192                      # block size of the overlap-save PMD filter


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on arrays (or scalars) of 32-bit words held in uint64; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, mode, n, stream):
    """The four words of sample index ``n`` (array) of ``mode``: counter (n low, n high, mode, stream), key (seed low, seed high)."""
    n = np.asarray(n, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = np.zeros_like(n)
    return philox4x32_10(n & np.uint64(MASK), n >> np.uint64(32), z + np.uint64(mode), z + np.uint64(stream), seed & MASK, seed >> 32)


def gauss(seed, mode, n, stream, wide):
    """Two standard normals per sample by Box-Muller in float64.  ``wide`` (the complex128 pass): uniforms of 53 bits, u from words (0, 1),
    v from words (2, 3); otherwise (the complex64 pass) of 32 bits from words 0 and 1.  Also returns the radius sqrt(-2 ln u)."""
    x, y, z, w = words(seed, mode, n, stream)
    if wide:
        a, b = ((x << np.uint64(32)) | y) >> np.uint64(11), ((z << np.uint64(32)) | w) >> np.uint64(11)
        u, v = (a.astype(np.float64) + 1.0) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53
    else:
        u, v = (x.astype(np.float64) + 1.0) * 2.0 ** -32, y.astype(np.float64) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u))
    ang = 6.283185307179586 * v
    return r * np.cos(ang), r * np.sin(ang), r


def phase_increments(seed, nmodes, L, var, wide):
    return np.stack([np.sqrt(var) * gauss(seed, m, np.arange(L), STREAM_PHASE, wide)[0] for m in range(nmodes)])


def noise(seed, nmodes, L, wide):
    """Unit-variance complex noise (nmodes, L), split over I and Q."""
    out = np.empty((nmodes, L), np.complex128)
    for m in range(nmodes):
        g0, g1, _ = gauss(seed, m, np.arange(L), STREAM_NOISE, wide)
        out[m] = (g0 + 1j * g1) * np.sqrt(0.5)
    return out


def rotate_field(x, theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * x[0] - s * x[1], s * x[0] + c * x[1]])


def _pmd_blocks(y, d):
    """Rows of the rotated field ``y`` (2, ..., N) through H = exp(-1j w d / 2) (row 0) and conj(H) (row 1) on the fftfreq grid of N."""
    N = y.shape[-1]
    k = np.fft.fftfreq(N) * N
    H = np.exp(1j * np.remainder(-np.pi * d * k / N, 2 * np.pi))
    Y = np.fft.fft(y, axis=-1)
    Y[0] *= H
    Y[1] *= np.conj(H)
    return np.fft.ifft(Y, axis=-1)


def pmd_whole(x, theta, d):
    """R(-theta) diag(H, conj H) R(theta) by one transform per row; ``d`` = t_dgd fs in samples."""
    return rotate_field(_pmd_blocks(rotate_field(np.asarray(x, np.complex128), theta), d), -theta)


def pmd_overlap_save(x, theta, d, N=PMD_N):
    """The same in blocks of N: block j keeps outputs [j n, (j + 1) n), n = N / 2, of a transform over the inputs j n - N/4 .. j n + n + N/4 - 1
    taken modulo L."""
    x = np.asarray(x, np.complex128)
    L = x.shape[1]
    n, q = N // 2, N // 4
    nblk = (L + n - 1) // n
    idx = (np.arange(nblk)[:, None] * n - q + np.arange(N)[None, :]) % L
    y = _pmd_blocks(rotate_field(x, theta)[:, idx], d)[:, :, q:q + n].reshape(2, -1)[:, :L]
    return rotate_field(y, -theta)


def pmd(x, theta, d):
    """What the device runs for this row length."""
    L = x.shape[1]
    whole = 256 <= L <= PMD_N and L & (L - 1) == 0
    return pmd_whole(x, theta, d) if whole else pmd_overlap_save(x, theta, d)


def carrier_offset(x, f):
    """x[:, n] exp(2j pi n f), f in turns per sample, the turn reduced before the exponential."""
    t = np.arange(x.shape[-1]) * float(f)
    return x * np.exp(2j * np.pi * (t - np.rint(t)))


def modal_delay(x, delay):
    return np.stack([np.roll(r, int(d)) for r, d in zip(x, delay)])


def simulate(x, fs, freq_off=None, modal=None, dgd=None, theta=np.pi / 3.731):
    """The deterministic stages in the order of simulate_transmission: carrier offset, modal delay, PMD."""
    x = np.asarray(x, np.complex128)
    if freq_off is not None:
        x = carrier_offset(x, freq_off / fs)
    if modal is not None:
        x = modal_delay(x, modal)
    if dgd is not None:
        x = pmd(x, theta, dgd * fs)
    return x


def qam_field(M, nmodes, nsym, os, beta, seed):
    """Band-limited M-QAM test field on a 2^-12 grid: random square-QAM symbols, root-raised-cosine shaped in the frequency domain
    (circular), unit rms before rounding."""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(M))
    lv = 2 * np.arange(side) - side + 1
    s = lv[rng.integers(0, side, (nmodes, nsym))] + 1j * lv[rng.integers(0, side, (nmodes, nsym))]
    L = nsym * os
    up = np.zeros((nmodes, L), np.complex128)
    up[:, ::os] = s
    f = np.abs(np.fft.fftfreq(L) * os)                                   # in units of the symbol rate
    H = np.where(f <= (1 - beta) / 2, 1.0, np.where(f <= (1 + beta) / 2, np.sqrt(0.5 * (1 + np.cos(np.pi / beta * (f - (1 - beta) / 2)))), 0.0))
    x = np.fft.ifft(np.fft.fft(up, axis=1) * H, axis=1)
    x /= np.sqrt(np.mean(np.abs(x) ** 2))
    return (np.round(x.real * 4096) + 1j * np.round(x.imag * 4096)) / 4096
