"""float64 numpy restatement of the digital pre-compensation (qampy/core/digital_pre_compensation.py, pythran_dsp.cal_lut_avg) and the shared
test cases.  Nothing here imports the reference or the package: tests/golden/gen_golden_precomp.py holds it against the reference, the GPU tests
hold the kernels against it.

Case inputs are multiples of 2^-10 with |tx - rx| <= 1 per rail and at most 4099 samples per row: complex64 and complex128 hold the same
values, and every sum is exact in float32, in double and in 64-bit fixed point, whatever the order of accumulation.  Indices, counts and the
whole table can then be compared bit for bit."""
import numpy as np

Q = 1024.0                               # inputs are multiples of 1 / Q
RAIL = {"r2": 2, "r4": 4, "r8": 8, "r32": 32}
ALPHABET = {"c16": 4, "c64": 8}


# ------------------------------------------------------------------------------------------------ the five operations
def rail_levels(m):
    return np.arange(-(m - 1), m, 2).astype(np.float64)


def qam(m):
    """The square alphabet of m x m points as cal_lut is handed it (any order: it takes np.unique)."""
    lv = rail_levels(m)
    return (lv[:, None] + 1j * lv[None, :]).ravel()[::-1].copy()


def levels_of(kind):
    """(lev_I, lev_Q, None) for a rail kind, (None, None, sorted complex alphabet) for an alphabet kind."""
    if kind in RAIL:
        lv = rail_levels(RAIL[kind])
        return lv, lv.copy(), None
    return None, None, np.unique(qam(ALPHABET[kind]))


def ref_sym_of(kind):
    """ref_sym and real_ptrns as cal_lut takes them"""
    if kind in RAIL:
        return qam(RAIL[kind]), True
    return qam(ALPHABET[kind]), False


def decide(x, levels):
    """np.argmin(|x - levels|): the first minimum wins a tie, a NaN sample gets 0"""
    x, levels = np.asarray(x), np.asarray(levels)
    return np.argmin(np.abs(x.reshape(1, -1).astype(np.result_type(x.dtype, np.float64)) - levels.reshape(-1, 1)), axis=0)


def margin(x, levels):
    """second smallest minus smallest distance of every sample, halved: how far the sample is from changing its decision"""
    d = np.sort(np.abs(np.asarray(x).reshape(1, -1) - np.asarray(levels).reshape(-1, 1)), axis=0)
    return (d[1] - d[0]) / 2


def window_index(lev, M, mem_len):
    """p[i] = sum_j lev[(i - mem_len // 2 + j) % L] M**(mem_len - 1 - j)"""
    L = lev.size
    i = np.arange(L)
    p = np.zeros(L, np.int64)
    for j in range(mem_len):
        p = p * M + lev[(i - mem_len // 2 + j) % L]
    return p


def pattern_index(x, lev_I, lev_Q, alphabet, mem_len):
    """(idx_I, idx_Q) int64 of one row"""
    x = np.asarray(x)
    if alphabet is None:
        return window_index(decide(x.real, lev_I), lev_I.size, mem_len), window_index(decide(x.imag, lev_Q), lev_Q.size, mem_len)
    p = window_index(decide(x, alphabet), alphabet.size, mem_len)
    return p, p


def lut(tx, rx, idx_I, idx_Q, N, mask=None):
    """(ea complex128, nI, nQ) of one row; err in float64"""
    err = np.asarray(tx).astype(np.complex128) - np.asarray(rx).astype(np.complex128)
    sel = np.ones(err.size, bool) if mask is None else np.asarray(mask, bool)
    sI, sQ = np.zeros(N), np.zeros(N)
    np.add.at(sI, idx_I[sel], err.real[sel])
    np.add.at(sQ, idx_Q[sel], err.imag[sel])
    nI, nQ = np.bincount(idx_I[sel], minlength=N), np.bincount(idx_Q[sel], minlength=N)
    # the reference's own expression: numpy divides the COMPLEX product 1j * sQ by the counts, which it does as a product with the reciprocal
    # 1 / n - the imaginary parts are sQ * (1 / n), rounded twice, not sQ / n
    return sI / np.maximum(nI, 1) + 1j * sQ / np.maximum(nQ, 1), nI, nQ


def apply_lut(sig, ea, idx_I, idx_Q, gain=1.0):
    return np.asarray(sig).astype(np.complex128) + gain * (ea[idx_I].real + 1j * ea[idx_Q].imag)


def comp_mod_sin(x, vpi=1.14, clip=0):
    x = np.asarray(x).astype(np.complex128)
    vpi = vpi if np.iscomplexobj(vpi) else vpi + 1j * vpi
    re, im = x.real, x.imag
    if clip:
        re, im = np.clip(re, -clip, clip), np.clip(im, -clip, clip)
    with np.errstate(invalid="ignore"):
        return 2 * vpi.real * np.arcsin(re) + 1j * (2 * vpi.imag * np.arcsin(im))


def comp_dac_resp(dpe_fb, sim_len, rrc_beta, PAPR=9, prms_dac=(16e9, 2, "sos", 6), os=2):
    """p_f: raised-cosine power response over the regularised Bessel response"""
    import scipy.signal as scisig
    fs = dpe_fb * os
    T = 1 / dpe_fb
    f = np.abs(np.fft.fftfreq(sim_len) * fs)
    lo, hi = (1 - rrc_beta) / (2 * T), (1 + rrc_beta) / (2 * T)
    n_f = np.zeros(sim_len)
    n_f[f <= lo] = 1
    tr = (f > lo) & (f <= hi)
    n_f[tr] = 0.5 * (1 + np.cos(np.pi * T / rrc_beta * (f[tr] - lo))) if rrc_beta else 0
    cutoff, order, frmt, enob = prms_dac
    sos = scisig.bessel(order, cutoff, "low", analog=False, output="sos", norm="mag", fs=fs)
    z = np.exp(-2j * np.pi * np.arange(sim_len) / sim_len)
    d_f = np.ones(sim_len, complex)
    for b0, b1, b2, a0, a1, a2 in sos:
        d_f *= (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
    alpha = 10 ** (PAPR / 10) / (6 * dpe_fb * 2 ** (2 * enob)) * np.sum(np.abs(d_f) ** 2 * n_f * (fs / sim_len))
    return n_f * np.conj(d_f) / (n_f * np.abs(d_f) ** 2 + alpha)


# ------------------------------------------------------------------------------------------------ cases
def dyadic(rng, n, bound):
    """n multiples of 1 / Q in [-bound, bound]"""
    return rng.integers(-int(bound * Q), int(bound * Q) + 1, n) / Q


def symbols(kind, L, seed):
    """One row: a level of the kind per rail plus an offset of at most 1/4 - at least 3/4 away from the next decision boundary"""
    rng = np.random.default_rng(seed)
    m = RAIL.get(kind) or ALPHABET[kind]
    lv = rail_levels(m)
    return (lv[rng.integers(0, m, L)] + dyadic(rng, L, 0.25)) + 1j * (lv[rng.integers(0, m, L)] + dyadic(rng, L, 0.25))


def capture(kind, L, seed):
    """(tx, rx) of one row: rx = tx - err, every rail of err a multiple of 1 / Q in [-1, 1]"""
    tx = symbols(kind, L, seed)
    rng = np.random.default_rng(seed + 1000)
    return tx, tx - (dyadic(rng, L, 1) + 1j * dyadic(rng, L, 1))


def mask_of(which, L):
    """None (all), every third symbol, one symbol, none"""
    if which == "full":
        return None
    m = np.zeros(L, bool)
    if which == "third":
        m[1::3] = True
    elif which == "single":
        m[L // 2] = True
    elif which != "empty":
        raise ValueError(which)
    return m


#: (kind, mem_len, L, seed) of the pattern-index cases: every level count and alphabet of the issue, mem_len 1, 2, 3, 5 and 7, L = 1, L < mem_len,
#: both sides of the 256-thread workgroup and of the 1024-symbol tile, more than one tile
INDEX_CASES = [("r2", 1, 1, 1), ("r2", 7, 5, 2), ("r2", 7, 4099, 3), ("r4", 3, 255, 4), ("r4", 2, 256, 5), ("r4", 5, 256, 6), ("r4", 7, 257, 7), ("r8", 3, 257, 8),
               ("r8", 5, 4099, 9), ("r32", 2, 4099, 10), ("r32", 3, 257, 11), ("c16", 1, 256, 12), ("c16", 3, 257, 13), ("c64", 2, 255, 14), ("c64", 3, 4099, 15),
               ("c16", 5, 5, 16), ("r4", 3, 1023, 17), ("r4", 3, 1025, 18)]

#: (name, kind, mem_len, L, seed): table sizes 64 (kept in LDS), 32768 and 64**3 = 262144 (global atomics), and one small complex one
LUT_CASES = [("lds", "r4", 3, 4099, 21), ("mid", "r8", 5, 4099, 22), ("big", "c64", 3, 4099, 23), ("cplx", "c16", 3, 257, 24)]
LUT_MASKS = ("full", "third", "single", "empty")


def tie_row():
    """r4, every sample of a stretch exactly midway between two levels on one rail or both: the lower level must win"""
    x = symbols("r4", 257, 31)
    x[10:20] = np.array([-2, 0, 2, -2, 0, 2, 0, 0, -2, 2]) + 1j * x[10:20].imag
    x[30:36] = x[30:36].real + 1j * np.array([0, 2, -2, 0, 2, -2])
    x[40] = 0
    return x


def nan_row():
    """r4 with one NaN real part, one NaN imaginary part and one sample NaN in both"""
    x = symbols("r4", 256, 32)
    x[7] = complex(np.nan, x[7].imag)
    x[100] = complex(x[100].real, np.nan)
    x[255] = complex(np.nan, np.nan)
    return x


def nonzero_table(ea):
    """(positions, values) of the entries of a table that are not 0 - how the large tables are stored"""
    at = np.flatnonzero(ea)
    return at.astype(np.int64), ea[at]


def cases():
    """dict(index=[...], lut=[...], tie=..., nan=...) of the shared cases, the inputs made anew on every call (they are never changed)"""
    index = [dict(kind=k, mem_len=m, L=L, x=symbols(k, L, s)) for k, m, L, s in INDEX_CASES]
    lut_cases = []
    for name, k, m, L, s in LUT_CASES:
        tx, rx = capture(k, L, s)
        lut_cases.append(dict(name=name, kind=k, mem_len=m, L=L, tx=tx, rx=rx))
    return dict(index=index, lut=lut_cases, tie=tie_row(), nan=nan_row())


#: comp_dac_resp: (name, dpe_fb, sim_len, rrc_beta, PAPR, prms_dac, os)
DAC_CASES = [("d256", 20e9, 256, 0.1, 9, (16e9, 2, "sos", 6), 2), ("d1000", 20e9, 1000, 0.1, 9, (16e9, 2, "sos", 6), 2),
             ("d8192", 20e9, 8192, 0.1, 9, (16e9, 2, "sos", 6), 2), ("d256b0", 20e9, 256, 0, 9, (16e9, 2, "sos", 6), 2),
             ("d1000alt", 32e9, 1000, 0.2, 7, (18e9, 4, "sos", 5), 2), ("d8192b0alt", 32e9, 8192, 0, 7, (18e9, 4, "sos", 5), 2)]


def mod_sin_input():
    """Values across (-1, 1), +-1 exactly, the next float32 and the next float64 beyond +-1 (NaN there), on both rails"""
    v = np.concatenate([np.linspace(-0.999, 0.999, 249), [1.0, -1.0, 0.0, float(np.nextafter(np.float32(1), np.float32(2))), -float(np.nextafter(np.float32(1), np.float32(2))),
                                                          np.nextafter(1.0, 2.0), -np.nextafter(1.0, 2.0), 1.5]])
    return v + 1j * v[::-1]
