"""Float64 NumPy restatements of the two feed-forward carrier-recovery estimators (csrc/cpr.hip), written from their contracts, and the
inputs of their tests.

Viterbi-Viterbi (qampy/core/phaserecovery.py:40-79), per row of L samples, window N, order M:

    z_n = (E_n / |E_n|) ** M                              a zero sample gives z = 1 (np.angle(0) = 0)
    s_k = z_k + .. + z_(k + N - 1),  k = 0 .. L - N
    theta_k = angle(s_k);  c_k = -1 where theta_k - theta_(k-1) > pi, +1 where it is < -pi, else 0;  K = cumsum(c)   (np.unwrap)
    trace_k = (theta_k + 2 pi K_k - pi) / M
    Eout[o + k] = E[o + k] exp(-j trace_k),  o = (N - 1) // 2;  the other N - 1 samples are zero

16-QAM by QPSK partitioning (:292-382), per row, blocks of Nblock samples (the last may be short):

    S0 = cal_s0(E, 1.32) with gamma = 25 / 33;  inner = (sqrt(S0 / 5) + sqrt(S0)) / 2;  outer = (sqrt(9 S0 / 5) + sqrt(S0)) / 2
    class 1: |E| < inner or |E| > outer;  S1 = sum over the block's class 1 of E ** 4
    per class-2 sample A = S1 - (E e^(j phi)) ** 4, B = S1 - (E e^(-j phi)) ** 4, phi = pi / 4 + atan(1 / 3); numpy's complex minimum of
    the two (real part first, then imaginary part, a tie keeps A);  theta_b = angle(S1 + sum of the minima)
    K over the blocks as above;  trace_n = theta_b(n) / 4 + (pi / 2) K_b(n) - pi / 4;  Eout = E exp(-j trace)  (every mode by its own trace)

Both functions return ``(field, trace, unwrap_margin, ring_margin)``: ``unwrap_margin = min | |theta_k - theta_(k-1)| - pi |`` (inf where
there is no step) says how far every unwrap decision is from flipping, ``ring_margin = min | |E| - threshold |`` the same for the classes
(inf for V&V).  The partition has a third decision, numpy's complex minimum of A and B, whose real parts differ by 2 |Im(E^4) sin(4 phi)|:
they tie where E lies on an axis or a diagonal, and there the choice moves the block sum by 2 |E|^4 - the estimator is discontinuous, in the
reference too.  ``tie_margin`` measures that distance and ``qam16_rows`` moves the few samples of a row that come too close.  Where all
margins are comfortably above the rounding of a kernel, kernel and restatement must take the same decisions and parity is a matter of
rounding alone."""
import numpy as np

GAMMA_132 = 25.0 / 33.0                  # _cal_gamma(1.32) of the reference's signal_quality
PHI = np.pi / 4 + np.arctan(1 / 3)


def wrap_counts(theta):
    """(c, K, margin) of np.unwrap over a 1-d array of angles: the corrections in units of 2 pi, their running sum, and the margin."""
    d = np.diff(theta)
    c = np.where(d > np.pi, -1, np.where(d < -np.pi, 1, 0)).astype(np.int64)
    K = np.concatenate([[0], np.cumsum(c)])
    margin = float(np.min(np.abs(np.abs(d) - np.pi))) if d.size else np.inf
    return c, K, margin


def viterbiviterbi(x, N, M):
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    nm, L = x.shape
    assert 1 <= N <= L
    nout, o = L - N + 1, (N - 1) // 2
    field, trace, margin = np.zeros((nm, L), np.complex128), np.zeros((nm, nout)), np.inf
    for r in range(nm):
        mag = np.abs(x[r])
        z = np.where(mag == 0, 1.0, x[r] / np.where(mag == 0, 1.0, mag)) ** M
        s = np.zeros(nout, np.complex128)
        for j in range(N):
            s += z[j:j + nout]
        theta = np.angle(s)
        _, K, m = wrap_counts(theta)
        trace[r] = (theta + 2 * np.pi * K - np.pi) / M
        field[r, o:o + nout] = x[r, o:o + nout] * np.exp(-1j * trace[r])
        margin = min(margin, m)
    return field, trace, margin, np.inf


def ring_thresholds(row):
    r2, r4 = np.mean(np.abs(row) ** 2), np.mean(np.abs(row) ** 4)
    S1 = 1 - 2 * r2 ** 2 / r4 - np.sqrt((2 - GAMMA_132) * (2 * r2 ** 4 / r4 ** 2 - r2 ** 2 / r4))
    S2 = GAMMA_132 * r2 ** 2 / r4 - 1
    S0 = r2 / (1 + S2 / S1)
    return (np.sqrt(S0 / 5) + np.sqrt(S0)) / 2, (np.sqrt(9 * S0 / 5) + np.sqrt(S0)) / 2


def phase_partition_16qam(x, Nblock):
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    nm, L = x.shape
    field, trace, umargin, rmargin = np.zeros((nm, L), np.complex128), np.zeros((nm, L)), np.inf, np.inf
    for r in range(nm):
        row = x[r]
        inner, outer = ring_thresholds(row)
        mag = np.abs(row)
        rmargin = min(rmargin, float(np.min(np.minimum(np.abs(mag - inner), np.abs(mag - outer)))))
        c1 = (mag < inner) | (mag > outer)
        e4, ep, em = row ** 4, (row * np.exp(1j * PHI)) ** 4, (row * np.exp(-1j * PHI)) ** 4
        nb = (L + Nblock - 1) // Nblock
        theta = np.zeros(nb)
        for b in range(nb):
            sl = slice(b * Nblock, min(L, (b + 1) * Nblock))
            S1 = np.sum(e4[sl][c1[sl]])
            A, B = S1 - ep[sl][~c1[sl]], S1 - em[sl][~c1[sl]]
            takeB = (B.real < A.real) | ((B.real == A.real) & (B.imag < A.imag))
            theta[b] = np.angle(S1 + np.sum(np.where(takeB, B, A)))
        _, K, m = wrap_counts(theta)
        tb = theta / 4 + (np.pi / 2) * K - np.pi / 4
        trace[r] = np.repeat(tb, Nblock)[:L]
        field[r] = row * np.exp(-1j * trace[r])
        umargin = min(umargin, m)
    return field, trace, umargin, rmargin


def tie_margin(x):
    """min over the class-2 samples of | Re (E e^(j phi))^4 - Re (E e^(-j phi))^4 |: how far numpy's complex minimum of A and B is from
    taking the other one (inf without class-2 samples).  A complex64 fourth power of a 16-QAM sample at unit mean power (|E|^4 <= 4)
    carries about 8 * 2^-24 * 4 = 2e-6 of rounding; the tests ask for 1e-4."""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    m = np.inf
    for row in x:
        inner, outer = ring_thresholds(row)
        mag = np.abs(row)
        c2 = ~((mag < inner) | (mag > outer))
        if c2.any():
            m = min(m, float(np.min(_tie_distance(row[c2]))))
    return m


def _tie_distance(e):
    return np.abs(((e * np.exp(1j * PHI)) ** 4).real - ((e * np.exp(-1j * PHI)) ** 4).real)


# ------------------------------------------------------------------------------------------------ inputs
def _finish(s, snr_db, lw, rng):
    """Noise at ``snr_db`` against unit power, a Wiener phase of linewidth x symbol period ``lw`` per row, rounding to multiples of 2^-12 (so
    that complex64 and complex128 hold the same values: the convention of foe_ref.qam_tone)."""
    nm, L = s.shape
    sig = 10 ** (-snr_db / 20) / np.sqrt(2)
    s = s + sig * (rng.standard_normal((nm, L)) + 1j * rng.standard_normal((nm, L)))
    ph = np.cumsum(np.sqrt(2 * np.pi * lw) * rng.standard_normal((nm, L)), axis=1)
    return np.round(s * np.exp(1j * ph) * 4096) / 4096


def psk_rows(M, nmodes, L, seed, snr_db, lw=1e-4):
    """(nmodes, L) complex128: M-PSK symbols at the angles pi / M + 2 pi k / M, noise, phase noise."""
    rng = np.random.default_rng(seed)
    s = np.exp(1j * (np.pi / M + 2 * np.pi * rng.integers(0, M, (nmodes, L)) / M))
    return _finish(s, snr_db, lw, rng)


def qam16_rows(nmodes, L, seed, snr_db=30., lw=1e-5, rotation=0.):
    """(nmodes, L) complex128: 16-QAM symbols at unit power, noise, phase noise, a constant rotation."""
    rng = np.random.default_rng(seed)
    lev = np.array([-3., -1., 1., 3.])
    s = (rng.choice(lev, (nmodes, L)) + 1j * rng.choice(lev, (nmodes, L))) / np.sqrt(10)
    x = _finish(s * np.exp(1j * rotation), snr_db, lw, rng)
    # off the ties of the complex minimum (tie_margin): a sample outside the inner ring whose fourth power is real to 1e-3 is moved by
    # (16, 5) grid steps - off every axis and diagonal - a fifth of the noise's standard deviation at 30 dB - on the 2^-12 grid such samples are common
    # (re = +-im exactly), and what the estimator does with them is decided by the last bit of a rounding
    for _ in range(4):
        close = (np.abs(x) > 0.6) & (_tie_distance(x) < 1e-3)
        if not close.any():
            break
        x = x + np.where(close, (16 + 5j) / 4096, 0.)
    return x


def wrap_ramp(L=3079, at=1024):
    """One noiseless QPSK-like row (N = 1, M = 4: output k is sample k) whose raw angle 4 arg(E_k) climbs slowly, so that it wraps every
    ~1570 samples, and flips between +3.0 and -3.0 at the outputs ``at - 1``, ``at`` and ``at + 1``: np.unwrap corrects at each of the three,
    by +1, -1 and +1 turns.  Returns ``(row (1, L), the three indices)``."""
    k = np.arange(L)
    U = 3.0 + 0.004 * (k - (at - 2))
    U[at - 1] = U[at - 2] + 0.28
    U[at] = U[at - 2]
    U[at + 1:] = U[at - 2] + 0.28 + 0.004 * (k[at + 1:] - (at + 1))
    row = np.round(np.exp(1j * U / 4) * 4096) / 4096
    return row.reshape(1, -1), (at - 1, at, at + 1)


VV_SNR = {2: 12., 4: 18., 8: 24.}          # dB, one per order
VV_N = (1, 2, 10, 11, 64, 1024)
P16_NBLOCK = (32, 48, 64, 100, 1000)


# the cases of tests/golden/cpr.npz (gen_golden_cpr.py): (name, M, N, nmodes, L, seed) and (name, Nblock, nmodes, L, seed)
GOLDEN_VV = (("4_11_2_1025", 4, 11, 2, 1025, 11), ("2_1_1_300", 2, 1, 1, 300, 12), ("8_64_1_1100", 8, 64, 1, 1100, 13), ("4_10_3_1030", 4, 10, 3, 1030, 14),
             ("4_1024_1_2100", 4, 1024, 1, 2100, 15))
GOLDEN_P16 = (("64_2_4099", 64, 2, 4099, 21), ("100_1_1000", 100, 1, 1000, 22), ("32_3_1000", 32, 3, 1000, 23), ("1000_1_1000", 1000, 1, 1000, 24))


def cases():
    """The shared case list: dicts with ``kind`` "vv" (``N``, ``M``) or "p16" (``Nblock``), ``name`` and ``make()`` -> the (nmodes, L) complex128
    input.  Small shapes that cross what the kernels tile by: one output and two, rows around one and three unwrap chunks of 1024, windows from 1
    to the limit, a short last block, a block length that is no power of two, one block only."""
    out = []
    i = 0
    for N in VV_N:
        for L in sorted({N, N + 1, 1023, 1024, 1025, 3 * 1024 + 7, 5000}):
            if L < N or (L == 5000 and N not in (1, 11, 1024)):
                continue
            M, nm = (2, 4, 8)[i % 3], (1, 3)[(i // 3) % 2]
            out.append(dict(kind="vv", name="vv-M%d-N%d-L%d-m%d" % (M, N, L, nm), N=N, M=M,
                            make=lambda M=M, nm=nm, L=L, i=i: psk_rows(M, nm, L, 1000 + i, VV_SNR[M])))
            i += 1

    def with_zero():
        x = psk_rows(4, 1, 1500, 77, 18.)
        x[0, 1030] = 0
        return x
    out.append(dict(kind="vv", name="vv-zero-sample", N=11, M=4, make=with_zero))
    out.append(dict(kind="vv", name="vv-wrap-ramp", N=1, M=4, make=lambda: wrap_ramp()[0]))
    i = 0
    for Nb in P16_NBLOCK:
        for L in sorted({Nb, 1000, 4099, 20000}):
            if L < Nb:
                continue
            nm = (1, 2)[i % 2]
            out.append(dict(kind="p16", name="p16-B%d-L%d-m%d" % (Nb, L, nm), Nblock=Nb,
                            make=lambda nm=nm, L=L, i=i: qam16_rows(nm, L, 2000 + i)))
            i += 1
    out.append(dict(kind="p16", name="p16-rotated", Nblock=64, make=lambda: qam16_rows(1, 4099, 2100, rotation=0.3)))
    return out


def long_vv_row(extra=0):
    """2^20 + 3 (+ ``extra``) samples of QPSK at 18 dB with linewidth x symbol period 3e-4, for N = 11: a trace of tens of radians over 1024 unwrap
    chunks (2^20 - 7 outputs, the last chunk short).  ``extra=1024`` makes it 1025 chunks: then every thread of the scan of the chunk sums holds
    more than one chunk."""
    return psk_rows(4, 1, 2 ** 20 + 3 + extra, 4242, 18., lw=3e-4)


def long_p16_row():
    """2^18 samples of 16-QAM at 30 dB: 4096 blocks of 64, i.e. four unwrap chunks of blocks."""
    return qam16_rows(1, 2 ** 18, 4343)


def run(case, x=None):
    """The restatement of a case: ``(field, trace, unwrap_margin, ring_margin)``."""
    x = case["make"]() if x is None else x
    return viterbiviterbi(x, case["N"], case["M"]) if case["kind"] == "vv" else phase_partition_16qam(x, case["Nblock"])
