"""A float64 restatement of what the signal-quality kernels (qampy_amd/csrc/metrics.hip) compute, written in numpy from the
definitions (not from the kernels), for the tests: tests/test_metrics_ref.py checks it against the reference's own numbers
(tests/golden/metrics.npz), tests/test_gpu_metrics_edges.py checks the kernels against it.

Conventions as in the kernels: point g of ``alphabet`` carries the label g, bit k (MSB first) of g is ``(g >> (nb - 1 - k)) & 1``,
``d_g = |x - s_g|^2``.  Everything is evaluated in float64 on the samples the kernel saw (complex64 rows are widened exactly)
and in chunks of symbols, so memory stays bounded at any length."""
import numpy as np

LN2 = np.log(2.)
CHUNK = 1 << 22                     # symbols x points per chunk


def nbits(M):
    nb = int(M).bit_length() - 1
    assert M == 1 << nb, M
    return nb


def bit_table(M):
    """(M, nb) int: bit k of label g."""
    nb = nbits(M)
    return (np.arange(M)[:, None] >> np.arange(nb - 1, -1, -1)[None, :]) & 1


def _chunks(n, M):
    step = max(1, CHUNK // M)
    for a in range(0, n, step):
        yield slice(a, min(n, a + step))


def _c128(a):
    return np.asarray(a).astype(np.complex128)


def dist2(x, alphabet):
    d = x[:, None] - alphabet[None, :]
    return d.real ** 2 + d.imag ** 2


def overlap(N, ntx, lag, trim):
    """Length of the aligned overlap [max(trim, lag), min(N - trim, ntx + lag)): the class fractions' denominator."""
    return max(0, min(N - trim, ntx + lag) - max(trim, lag))


def aligned(row, tx_labels, M, rot=0, lag=0, trim=0, ntx=None):
    """(x, t): the compared symbols ``row[i] * j^rot`` and their labels, for i in [trim, N - trim) with 0 <= i - lag < ntx and
    0 <= tx_labels[i - lag] < M, in index order."""
    row = _c128(row)
    t = np.asarray(tx_labels).astype(np.int64)
    ntx = t.size if ntx is None else int(ntx)
    i = np.arange(trim, row.size - trim)
    i = i[(i - lag >= 0) & (i - lag < ntx)]
    lab = t[i - lag]
    keep = (lab >= 0) & (lab < M)
    return row[i[keep]] * (1j ** (rot & 3)), lab[keep]


def decide(x, alphabet):
    """First index of the smallest |x - s_g| (np.argmin of hypot distances)."""
    al = _c128(alphabet)
    out = np.empty(x.size, np.int64)
    for s in _chunks(x.size, al.size):
        out[s] = np.argmin(np.abs(x[s, None] - al[None, :]), axis=1)
    return out


def near_ties(x, alphabet, rel=1e-6):
    """Number of symbols whose best and second-best distance |x - s_g| lie within ``rel`` of each other (where a float32
    decision may legitimately differ from this one)."""
    al = _c128(alphabet)
    n = 0
    for s in _chunks(x.size, al.size):
        h = np.partition(np.abs(x[s, None] - al[None, :]), 1, axis=1) if al.size > 1 else np.zeros((s.stop - s.start, 2))
        n += int(np.count_nonzero(h[:, 1] - h[:, 0] <= rel * h[:, 1]))
    return n


def _split(d, nb, k):
    """d (n, M) viewed so that axis 2 is bit k: (n, 2^k, 2, 2^(nb-1-k))."""
    return d.reshape(d.shape[0], 1 << k, 2, 1 << (nb - 1 - k))


def llr_maxlog(x, alphabet, snr):
    """(n, nb) ``snr (min_{bit k = 0} d - min_{bit k = 1} d)``."""
    al = _c128(alphabet)
    nb = nbits(al.size)
    L = np.empty((x.size, nb))
    for s in _chunks(x.size, al.size):
        d = dist2(x[s], al)
        for k in range(nb):
            m = _split(d, nb, k).min(axis=(1, 3))
            L[s, k] = snr * (m[:, 0] - m[:, 1])
    return L


def llr_exact(x, alphabet, snr):
    """(n, nb) ``ln sum_{bit k = 1} exp(-snr d) - ln sum_{bit k = 0} exp(-snr d)``, each side's log-sum-exp shifted by its own
    largest exponent (finite for every finite input)."""
    al = _c128(alphabet)
    nb = nbits(al.size)
    bits = bit_table(al.size).astype(np.float64)
    L = np.empty((x.size, nb))
    for s in _chunks(x.size, al.size):
        d = dist2(x[s], al)
        # one exp per distance, shifted by the global minimum; a side whose own largest term is below 1e-250 there (its sum
        # would lose digits to underflow) is redone below with its own shift
        dmin = d.min(axis=1, keepdims=True)
        e = np.exp(-snr * (d - dmin))
        s1, s0 = e @ bits, e @ (1 - bits)
        with np.errstate(divide="ignore"):
            L[s] = np.log(s1) - np.log(s0)
        for k in range(nb):
            m = _split(d, nb, k).min(axis=(1, 3))
            redo = np.nonzero(snr * (m.max(axis=1) - dmin[:, 0]) > 575)[0]
            if redo.size:
                a = -snr * _split(d[redo], nb, k)
                mx = a.max(axis=(1, 3), keepdims=True)
                lse = np.log(np.exp(a - mx).sum(axis=(1, 3))) + mx[:, :, :, 0].reshape(-1, 2)
                L[s.start + redo, k] = lse[:, 1] - lse[:, 0]
    return L


def side_sums_global_shift(x, alphabet, snr):
    """(n, nb, 2) ``sum_{bit k = b} exp(-snr (d - dmin))`` in float64: the complex128 kernel's sums (its LLR is finite and
    accurate where both are normal numbers)."""
    al = _c128(alphabet)
    bits = bit_table(al.size).astype(np.float64)
    out = np.empty((x.size, bits.shape[1], 2))
    for s in _chunks(x.size, al.size):
        d = dist2(x[s], al)
        e = np.exp(-snr * (d - d.min(axis=1, keepdims=True)))
        out[s, :, 0], out[s, :, 1] = e @ (1 - bits), e @ bits
    return out


def softplus2(y):
    """log2(1 + exp(y)) without overflow."""
    return np.logaddexp(0., y) / LN2


def gmi_sums(L, t, nb):
    """(nb,) per bit sum over symbols of log2(1 + exp((-1)^b L)), b the transmitted bit (GMI_k = 1 - sum / n)."""
    b = (np.asarray(t)[:, None] >> np.arange(nb - 1, -1, -1)[None, :]) & 1
    return softplus2(np.where(b == 1, -L, L)).sum(axis=0)


def mi_fast_sum(x, tx_points, alphabet, snr):
    """sum over symbols of log2 sum_j exp(-snr (|x - s_j|^2 - |x - t|^2)) (cal_mi_mc_fast: MI = log2 M - sum / n)."""
    al = _c128(alphabet)
    tx_points = _c128(tx_points)
    tot = 0.
    for s in _chunks(x.size, al.size):
        dt = np.abs(x[s] - tx_points[s]) ** 2
        a = -snr * (dist2(x[s], al) - dt[:, None])
        mx = a.max(axis=1)
        tot += float(np.sum((np.log(np.exp(a - mx[:, None]).sum(axis=1)) + mx) / LN2))
    return tot


def snr_estimate(x, t, M, L):
    """(snr, S0, N0) from the per-class means and variances, class fractions K_g / L; an empty class gives NaN."""
    t = np.asarray(t)
    K = np.bincount(t, minlength=M).astype(np.float64)
    if np.any(K == 0):
        return np.nan, np.nan, np.nan
    mu = (np.bincount(t, x.real, M) + 1j * np.bincount(t, x.imag, M)) / K
    var = np.bincount(t, np.abs(x - mu[t]) ** 2, M) / K
    P = K / L
    s0, n0 = float(np.sum(P * np.abs(mu) ** 2)), float(np.sum(P * var))
    return s0 / n0, s0, n0


def mi_mc(noise, alphabet, N0):
    """cal_mi_mc: log2 M - mean over (l, i) of log2 sum_j exp(-(|s_i - s_j|^2 + 2 Re((s_i - s_j) n_l)) / N0)."""
    al = _c128(alphabet)
    n = _c128(noise)
    dd = al[:, None] - al[None, :]                                         # (i, j)
    tot = 0.
    for s in _chunks(n.size, al.size * al.size):
        a = -(np.abs(dd) ** 2 + 2 * (dd[None] * n[s, None, None]).real) / N0    # (l, i, j)
        mx = a.max(axis=2)
        tot += float(np.sum((np.log(np.exp(a - mx[:, :, None]).sum(axis=2)) + mx) / LN2))
    return np.log2(al.size) - tot / al.size / n.size


def metrics(row, tx_labels, alphabet, rot=0, lag=0, trim=0, ntx=None, snr=None, minmax=False):
    """Everything the fused pass and the SNR estimate report for one aligned row:
    ``errors, bit_errors, compared`` (ints), ``err_pow`` (sum |x - s_t|^2), ``mi_sum`` (see mi_fast_sum), ``gmi_sums`` (nb,),
    ``snr, s0, n0`` (estimated when ``snr`` is None, else s0 = n0 = NaN) and ``ser, ber, evm, gmi, gmi_per_bit, mi`` as
    cal_metrics_dev derives them, plus ``near_ties`` and ``x`` / ``t`` (the compared symbols)."""
    al = _c128(alphabet)
    M, nb = al.size, nbits(al.size)
    ntx = np.asarray(tx_labels).size if ntx is None else int(ntx)
    x, t = aligned(row, tx_labels, M, rot, lag, trim, ntx)
    if snr is None:
        snr_v, s0, n0 = snr_estimate(x, t, M, overlap(np.asarray(row).size, ntx, lag, trim))
    else:
        snr_v, s0, n0 = float(snr), np.nan, np.nan
    dec = decide(x, al)
    n = x.size
    L = llr_maxlog(x, al, snr_v) if minmax else llr_exact(x, al, snr_v)
    err_pow = float(np.sum(np.abs(x - al[t]) ** 2))
    gs = gmi_sums(L, t, nb)
    mis = mi_fast_sum(x, al[t], al, snr_v)
    nn = max(n, 1)
    per_bit = 1 - gs / nn
    errors, bit_errors = int(np.count_nonzero(dec != t)), int(bit_table(M)[dec ^ t].sum())
    return dict(errors=errors, bit_errors=bit_errors, compared=int(n), err_pow=err_pow, mi_sum=mis, gmi_sums=gs, snr=snr_v, s0=s0, n0=n0,
                ser=errors / nn, ber=bit_errors / (nn * nb), evm=np.sqrt(err_pow / nn), gmi=float(per_bit.sum()), gmi_per_bit=per_bit,
                mi=np.log2(M) - mis / nn, near_ties=near_ties(x, al), x=x, t=t, dec=dec)
