"""Float64 NumPy restatement of the device symbol-error harness (qh_ser_c64_dev / qh_ser_c128_dev, csrc/ser.hip) and of the bare error
counter (qh_count_errors_dev, csrc/bps.hip), written from their contract in include/qampy_hip.h, and the inputs of their tests.

The harness, for one received row ``rx`` (N,), the labels ``idx_tx`` (nmodes, ntx) of the transmitted symbols and an alphabet (M,):

    decide(x)_i = first arg-min over k of |x_i - s_k|                         (np.abs, not its square)
    W = window if window > 0 else 4096, then W = min(W, N - 2 trim);          start = trim + (N - 2 trim - W) // 2
    counts[m, k, l] = #{ i < W : 0 <= start + i - lag < ntx  and  decide(rx j^k)[start + i] == idx_tx[m, start + i - lag] },  lag = l - maxlag
    (mode, k, lag) = the first maximum of counts in C order
    errors, compared over i in [trim, N - trim) with 0 <= i - lag < ntx:  compared counts them, errors those with
    decide(rx j^k)[i] != idx_tx[mode, i - lag]

and the seven numbers of ``result`` are errors, compared, mode, k, lag, counts[mode, k, lag], W.  All of them are integers, so a kernel and
this restatement agree exactly as soon as they take the same decisions.  A float32 kernel does when no sample lies close to a decision
boundary: ``margin`` (second-smallest minus smallest distance) says how close, and ``clear_of_ties`` moves the few samples of a row whose
margin under any of the four quarter turns is below ``BAR`` = 1e-4.  At unit power |x - s| <= ~4; hypotf, the two float32 subtractions and
the float32 cast of the alphabet together carry about 5e-7 of error per distance, and 1e-4 is 200 times that (the reasoning of
cpr_ref.tie_margin).  Samples are rounded to multiples of 2^-12 so that complex64 and complex128 hold the same numbers (the convention of
cpr_ref / foe_ref)."""
import functools

import numpy as np

from qampy_amd import theory

BAR = 1e-4
GRID = 4096.
TRIP = 2048 * 256                 # symbols one pass of the counting kernels covers: the grid is capped at 2048 blocks of 256 threads


# ------------------------------------------------------------------------------------------------ the restatement
def decide(x, alphabet, chunk=1 << 14):
    """(idx int32, margin): first arg-min of |x - s_k| per sample, and second-smallest minus smallest distance (inf for M = 1)."""
    x = np.asarray(x, np.complex128).ravel()
    al = np.asarray(alphabet, np.complex128).ravel()
    idx, margin = np.empty(x.size, np.int32), np.full(x.size, np.inf)
    for a in range(0, x.size, chunk):
        d = np.abs(x[a:a + chunk, None] - al[None, :])
        idx[a:a + chunk] = np.argmin(d, axis=1)
        if al.size > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            margin[a:a + chunk] = two[:, 1] - two[:, 0]
    return idx, margin


def window_of(N, window, trim):
    """(W, start) of the search window."""
    W = window if window > 0 else 4096
    W = min(W, N - 2 * trim)
    return W, trim + (N - 2 * trim - W) // 2


def ser(rx_row, idx_tx, alphabet, maxlag, window, trim, detail=False):
    """The seven numbers of ``result`` as a tuple of ints.  ``detail``: also the positions compared and the positions in error (two index
    arrays into the row)."""
    rx = np.asarray(rx_row, np.complex128).ravel()
    tx = np.atleast_2d(np.asarray(idx_tx)).astype(np.int64)
    N, (nmodes, ntx) = rx.size, tx.shape
    assert N > 0 and 1 <= nmodes <= 16 and 0 <= maxlag <= 4096 and trim >= 0 and 2 * trim < N
    W, start = window_of(N, window, trim)
    pos = start + np.arange(W)
    counts = np.zeros((nmodes, 4, 2 * maxlag + 1), np.int64)
    for k in range(4):
        d = decide(rx[start:start + W] * 1j ** k, alphabet)[0]
        for l in range(2 * maxlag + 1):
            it = pos - (l - maxlag)
            ok = (it >= 0) & (it < ntx)
            for m in range(nmodes):
                counts[m, k, l] = np.count_nonzero(d[ok] == tx[m, it[ok]])
    mode, k, l = np.unravel_index(np.argmax(counts), counts.shape)          # np.argmax: the first maximum of the flattened (C order) array
    lag = int(l) - maxlag
    i = np.arange(trim, N - trim)
    i = i[(i - lag >= 0) & (i - lag < ntx)]
    wrong = decide(rx[i] * 1j ** int(k), alphabet)[0] != tx[mode, i - lag]
    res = (int(np.count_nonzero(wrong)), int(i.size), int(mode), int(k), lag, int(counts[mode, k, l]), int(W))
    return (res, i, i[wrong]) if detail else res


def count_errors(idx_rx, idx_tx, n, lag):
    """#{ i < n : 0 <= i - lag < ntx and idx_rx[i] != idx_tx[i - lag] }, what qh_count_errors_dev ADDS to its counter."""
    rx, tx = np.asarray(idx_rx).ravel(), np.asarray(idx_tx).ravel()
    i = np.arange(n)
    i = i[(i - lag >= 0) & (i - lag < tx.size)]
    return int(np.count_nonzero(rx[i] != tx[i - lag]))


# ------------------------------------------------------------------------------------------------ inputs
def alphabet(name):
    """complex128 alphabets by name: "qam4" .. "qam1024" (theory.coded_symbols_qam at unit power; 32 is the cross), "qam16_shifted" and
    "irregular16" as tests/test_gpu_parity.py builds them, and "one", a single point."""
    q16 = theory.coded_symbols_qam(16)
    if name == "qam16_shifted":
        return q16 + (0.11 - 0.07j)
    if name == "irregular16":
        jit = np.random.default_rng(5).normal(size=(16, 2)) * 0.04
        return q16 + jit[:, 0] + 1j * jit[:, 1]
    if name == "one":
        return np.array([0.75 + 0.5j])
    return theory.coded_symbols_qam(int(name[3:]))


def labels(nmodes, ntx, M, seed):
    return np.random.default_rng(seed).integers(0, M, (nmodes, ntx)).astype(np.int32)


def snr_for(M):
    """dB at which an M-QAM row counts one or two per cent of symbol errors: 10 log10(M - 1) + 3."""
    return 10 * np.log10(max(M - 1, 1)) + 3.


def received(labels_row, alphabet, turns, lag, N, snr_db, seed):
    """(row (N,) complex128, share of samples moved by clear_of_ties): ``row[i] = alphabet[labels_row[i - lag]] j^turns`` + noise at ``snr_db``
    against unit power (None: no noise).  A linear shift, not np.roll: where no symbol was transmitted the row holds an independent random
    alphabet point.  Rounded to multiples of 2^-12, then kept clear of ties."""
    rng = np.random.default_rng(seed)
    al = np.asarray(alphabet, np.complex128)
    lab = np.asarray(labels_row)
    it = np.arange(N) - lag
    have = (it >= 0) & (it < lab.size)
    sent = rng.integers(0, al.size, N)
    sent[have] = lab[it[have]]
    x = al[sent] * 1j ** turns
    if snr_db is not None:
        x = x + 10 ** (-snr_db / 20) / np.sqrt(2) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    x = np.round(x * GRID) / GRID
    return clear_of_ties(x, al)


def min_margin(x, alphabet):
    """Smallest decision margin of the samples under the four quarter turns."""
    return min(float(np.min(decide(x * 1j ** k, alphabet)[1])) for k in range(4))


def clear_of_ties(x, alphabet, bar=BAR):
    """(x with every sample whose margin under any of the four quarter turns is below ``bar`` replaced by the 2^-12-grid point nearest its own
    decided symbol, share of samples moved)."""
    al = np.asarray(alphabet, np.complex128)
    idx, margin = decide(x, al)
    close = margin < bar
    for k in (1, 2, 3):
        close |= decide(x * 1j ** k, al)[1] < bar
    x = np.where(close, np.round(al[idx] * GRID) / GRID, x)
    return x, float(np.mean(close))


# ------------------------------------------------------------------------------------------------ the shared case list
def _case(name, al="qam16", N=4097, nmodes=2, ntx=None, mode=None, turns=3, lag=7, maxlag=64, window=0, trim=0, snr="auto", band=True,
          identical=False, bad=0., ties=False, c64_only=False):
    """Defaults: 16-QAM, two transmitted modes, the row carries the last one turned by -j (found with rotation 1) at lag 7, maxlag 64.
    ``band``: the case is aligned and long enough for its error share to lie in [1e-4, 0.1]."""
    return dict(name=name, al=al, N=N, nmodes=nmodes, ntx=N if ntx is None else ntx, mode=nmodes - 1 if mode is None else mode, turns=turns,
                lag=lag, maxlag=maxlag, window=window, trim=trim, snr=snr, band=band, identical=identical, bad=bad, ties=ties,
                c64_only=c64_only)


def cases():
    out = []
    # lengths and the window.  Short rows get a lower SNR so that a few per cent of a few hundred symbols are in error; one or two symbols
    # cannot lie in the band at all
    for N in (1, 2):
        out.append(_case("N%d" % N, N=N, lag=0, snr=None, band=False))
    for N in (255, 256, 257):
        out.append(_case("N%d" % N, N=N, snr=13.5))
    for N in (4095, 4096, 4097):
        out.append(_case("N%d" % N, N=N))
    out.append(_case("window1", window=1, band=False))                          # one symbol cannot align anything
    for w in (255, 257, 4096, 4097, 4098, -5):
        out.append(_case("window%d" % w, window=w))
    out.append(_case("trim1", trim=1))
    out.append(_case("trim2048", trim=2048, band=False))                        # one symbol compared
    out.append(_case("odd-start", trim=1, window=1000))                         # 4095 - 1000 is odd
    # the counting trip: QPSK, 6 dB so that the last 300 symbols hold errors too
    for name, n in (("trip-1", TRIP - 1), ("trip", TRIP), ("trip+1", TRIP + 1), ("2trip+300", 2 * TRIP + 300)):
        out.append(_case(name, al="qam4", N=n + 200, trim=100, snr=6., c64_only=name == "2trip+300"))
    # lags
    for lag in (-64, -63, 0, 63, 64):
        out.append(_case("lag%d" % lag, N=6000, window=2048, lag=lag))
    out.append(_case("lag65", N=6000, window=2048, lag=65, band=False))          # outside the search: whatever the restatement gives
    out.append(_case("maxlag0", N=6000, window=2048, lag=0, maxlag=0))
    for lag in (-4096, 4096):
        out.append(_case("maxlag4096-lag%d" % lag, N=12000, window=2048, nmodes=1, lag=lag, maxlag=4096))
    # geometry of the transmitted side
    out.append(_case("ntx-short", N=6000, ntx=5000))
    out.append(_case("ntx-long", N=6000, ntx=7000))
    out.append(_case("ntx1", N=6000, ntx=1, band=False))
    for nm in (1, 3, 16):
        out.append(_case("nmodes%d" % nm, N=6000, nmodes=nm))
    out.append(_case("identical-modes", N=6000, identical=True))
    for t in (0, 1, 2, 3):
        out.append(_case("turns%d" % t, N=6000, turns=t))
    # alphabets
    for al in ("qam4", "qam16", "qam32", "qam64", "qam256", "qam1024", "qam16_shifted", "irregular16"):
        out.append(_case("al-" + al, al=al, N=20000))
    out.append(_case("al-one", al="one", N=20000, band=False))                   # nothing to get wrong
    # exact decision ties and labels outside [0, M)
    out.append(_case("ties-qam4", al="qam4", N=6000, ties=True))
    out.append(_case("ties-qam16", al="qam16", N=6000, ties=True))
    out.append(_case("bad-labels", N=6000, bad=0.01))
    return out


CASES = {c["name"]: c for c in cases()}
TIE_AT = 2900                          # first of the exact-tie samples of a ``ties`` case (inside the default window of a 6000-symbol row)


def tie_samples(al):
    """Samples with re == 0, with im == 0, and 0 + 0j: equidistant from mirror-image points of a mirror-symmetric alphabet in any precision
    (hypot takes absolute values), so only the order of the alphabet decides.  The other coordinate sits on the alphabet's levels and 16 grid steps
    outside them, far from every other boundary."""
    lev = np.unique(np.round(np.abs(np.asarray(al).real) * GRID) / GRID)
    off = np.concatenate([lev, -lev, lev + 16 / GRID, -lev - 16 / GRID])
    return np.concatenate([1j * off, off, [0j]]).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def make(name):
    """The inputs of a case: dict with ``rx`` (N,) complex128, ``labels`` (nmodes, ntx) int32, ``alphabet`` complex128, ``moved`` (the share
    clear_of_ties moved), ``exempt`` (positions of the exact-tie samples) and the case's own fields.  Cached: treat the arrays as read-only."""
    import zlib
    c = dict(CASES[name])
    seed = zlib.crc32(name.encode())
    al = alphabet(c["al"])
    lab = labels(c["nmodes"], c["ntx"], al.size, seed)
    if c["identical"]:
        lab[1] = lab[0]
    snr = snr_for(al.size) if c["snr"] == "auto" else c["snr"]
    rx, moved = received(lab[c["mode"]], al, c["turns"], c["lag"], c["N"], snr, seed + 1)
    exempt = np.zeros(0, np.int64)
    n = c["N"] - 2 * c["trim"]
    if n >= TRIP - 1:
        # noise alone leaves a pass of one symbol without an error: the first symbol of every pass after the first and the last symbol
        # compared carry a neighbouring label's point
        at = np.unique(np.r_[c["trim"] + TRIP * np.arange(1, (n + TRIP - 1) // TRIP), c["N"] - c["trim"] - 1])
        rx = rx.copy()
        rx[at] = np.round(al[(lab[c["mode"], at - c["lag"]] + 1) % al.size] * 1j ** c["turns"] * GRID) / GRID
    if c["ties"]:
        t = tie_samples(al)
        exempt = TIE_AT + np.arange(t.size)
        rx = rx.copy()
        rx[exempt] = t
        # every other tie sample was "sent" as the point the first-minimum rule decides: another rule turns these into errors
        want = decide(t * 1j ** ((-c["turns"]) % 4), al)[0]
        lab[c["mode"], exempt[::2] - c["lag"]] = want[::2]
    if c["bad"]:
        rng = np.random.default_rng(seed + 2)
        hit = rng.random(lab.shape) < c["bad"]
        lab[hit] = np.where(rng.random(np.count_nonzero(hit)) < 0.5, -1, al.size)
    for a in (rx, lab, al):
        a.setflags(write=False)
    c.update(rx=rx, labels=lab, alphabet=al, moved=moved, exempt=exempt)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement of a case: the seven numbers."""
    c = make(name)
    return ser(c["rx"], c["labels"], c["alphabet"], c["maxlag"], c["window"], c["trim"])
