"""
Sequence alignment helpers of the pilot receiver / SER harness, behaviour of ``qampy.core.ber_functions``
(qampy/core/ber_functions.py:33-106): delay of one sequence inside another from the peak of their full cross-correlation,
trying the four quarter-turn rotations for complex data.  Host-side numpy/scipy (a few thousand samples per call).  :func:`cal_ser_dev` is the device-resident counterpart of
``SignalQAM.cal_ser`` (qampy/core/signals.py:295-335) for captures that stay in HBM.
"""
import numpy as np
from scipy.signal import fftconvolve


def find_sequence_offset(x, y, show_cc=False):
    """Index by which ``y`` has to be shifted to line up with ``x`` (peak of the full cross-correlation, :33-69)."""
    X = 1. * np.asarray(x)
    Y = 1. * np.asarray(y)
    rev = Y.conj()[::-1] if np.iscomplexobj(Y) else Y[::-1]
    cc = fftconvolve(X, rev, "full")
    idx = abs(cc).argmax() - (Y.shape[0] - 1)
    return (idx, cc) if show_cc else idx


def find_sequence_offset_complex(x, y):
    """``(offset, rotated y, quarter turns, peak)`` over the rotations ``1j**i`` of the received sequence ``y`` (:71-106)."""
    if not np.iscomplexobj(x) and not np.iscomplexobj(y):
        idx, cc = find_sequence_offset(x, y, show_cc=True)
        return idx, y, 0, cc
    # turning y by 1j**i turns the whole cross-correlation by (-1j)**i: one correlation serves the four hypotheses, and its
    # magnitude peak - the offset - is the same for all of them
    idx, cc = find_sequence_offset(x, y, show_cc=True)
    peaks = np.array([cc.real.max(), cc.imag.max(), (-cc.real).max(), (-cc.imag).max()])      # max Re((-1j)**i cc), i = 0..3
    if not peaks.max() > 0:
        return 0, y, 0, 0.
    turns = int(np.argmax(peaks))
    return idx, y * 1.j ** turns, turns, float(peaks[turns])


def tx_indices_dev(symbols_tx, alphabet):
    """Decided indices of the transmitted symbols ``(nmodes, Nsym)`` as an int32 DeviceArray (once per capture)."""
    from .. import _lib
    from .equalisation import hip_equalisation as hk
    tx = symbols_tx if isinstance(symbols_tx, _lib.DeviceArray) else _lib.DeviceArray.from_host(np.ascontiguousarray(symbols_tx))
    alpha = alphabet if isinstance(alphabet, _lib.DeviceArray) else _lib.DeviceArray.from_host(
        np.ascontiguousarray(alphabet, dtype=tx.dtype))
    idx = _lib.DeviceArray(tx.shape, np.int32)
    hk.make_decision_dev(tx, alpha, None, None, idx)
    return idx


def cal_ser_dev(out, idx_tx, alphabet, maxlag=256, window=4096, trim=0):
    """
    Symbol error rate of recovered rows that live in HBM, without moving them to the host.

    What ``cal_ser`` does on the host - synchronise with the transmitted sequence over the four quarter-turn rotations
    (``sync_and_adjust`` / ``find_sequence_offset_complex``, ber_functions.py:33-160), decide, compare - as a bounded-lag
    search on decided indices plus one counting pass (``qh_ser_*_dev``).

    Parameters
    ----------
    out : DeviceArray (nrows, N) complex
    idx_tx : DeviceArray (nmodes, Nsym) int32 from :func:`tx_indices_dev`
    alphabet : DeviceArray (M,) complex, same dtype as ``out``
    maxlag : largest |lag| (symbols) searched;  window : symbols used for the search;  trim : symbols ignored at both ends

    Returns
    -------
    list of dicts per row: ``errors, compared, ser, tx_mode, rotation, lag, window_matches, window``
    """
    from .. import _lib
    suf = "c64" if np.dtype(out.dtype) == np.complex64 else "c128"
    nrows, N = out.shape
    nmodes, ntx = idx_tx.shape
    res = []
    for r in range(nrows):
        h = np.zeros(7, np.int64)
        _lib.call("qh_ser_%s_dev" % suf, out.row(r).ptr, N, idx_tx.ptr, nmodes, ntx, alphabet.ptr, int(np.prod(alphabet.shape)),
                  int(maxlag), int(window), int(trim), _lib.ptr(h))
        res.append(dict(errors=int(h[0]), compared=int(h[1]), ser=float(h[0]) / max(int(h[1]), 1), tx_mode=int(h[2]),
                        rotation=int(h[3]), lag=int(h[4]), window_matches=int(h[5]), window=int(h[6])))
    return res


# ------------------------------------------------------------------------------------------------ alignment of tx and rx
def _adjust_to(data, N, back=True):
    """``data`` repeated to ``N`` samples (ber_functions.py:309-320): whole copies, then the first ``N mod len`` samples
    behind them (``back``) or the last ``N mod len`` samples in front of them.  As in the reference, a remainder of 0 in
    front puts a whole copy there (``data[-0:]`` is all of ``data``), and ``N < 0`` gives the remainder alone."""
    n = data.shape[0]
    copies, rem = N // n, N % n
    body = np.concatenate([data] * copies) if copies > 0 else np.array([], dtype=data.dtype)
    return np.hstack([body, data[:rem]]) if back else np.hstack([data[-rem:], body])


def _extend_to(short, N, offset):
    """``short`` made periodic to ``N`` samples with its start ``offset`` samples in."""
    if offset == 0:
        return _adjust_to(short, N)
    head = _adjust_to(short, offset, back=False)
    return np.hstack([head, _adjust_to(short, N - head.shape[0])])


def adjust_data_length(data_tx, data_rx, method=None, offset=0):
    """
    Bring ``data_tx`` and ``data_rx`` to a common length (ber_functions.py:248-307).

    ``"truncate"``: cut the longer one.  ``"extend"``: repeat the shorter one periodically, its start ``offset`` samples into
    the other.  ``None``: only ``data_tx`` changes - cut if longer, repeated if shorter.
    """
    ntx, nrx = len(data_tx), len(data_rx)
    if method is None:
        if ntx > nrx:
            return data_tx[:nrx], data_rx
        if ntx < nrx:
            if offset == 0:
                return _adjust_to(data_tx, nrx), data_rx
            return np.hstack([_adjust_to(data_tx, offset, back=False), _adjust_to(data_tx, nrx - offset)]), data_rx
        return data_tx, data_rx
    if method == "truncate":
        n = min(ntx, nrx)
        return (data_tx[:n] if ntx > n else data_tx), (data_rx[:n] if nrx > n else data_rx)
    if method == "extend":
        if ntx > nrx:
            return data_tx, _extend_to(data_rx, ntx, offset)
        if ntx < nrx:
            return _extend_to(data_tx, nrx, offset), data_rx
        return data_tx, data_rx
    return None


def sync_and_adjust(data_tx, data_rx, adjust="tx"):
    """
    Line up one received row with one transmitted row and give them a common length (ber_functions.py:108-160).

    The offset and the quarter turn come from :func:`find_sequence_offset_complex`; the sequence named by ``adjust`` is
    rotated, rolled or made periodic around the other one.  Returns ``((tx, rx), peak)``, ``peak`` the correlation
    maximum the mode assignment of ``SignalQAM._sync_and_adjust`` compares.
    """
    assert adjust in ("tx", "rx"), "adjust need to be either 'tx' or 'rx'"
    ntx, nrx = data_tx.shape[0], data_rx.shape[0]
    if adjust == "tx":
        offset, tx, _, peak = find_sequence_offset_complex(data_rx, data_tx)
        if ntx > nrx:
            return adjust_data_length(np.roll(tx, offset), data_rx, method="truncate"), peak
        if ntx < nrx:
            return adjust_data_length(tx, data_rx, method="extend", offset=offset), peak
        return (np.roll(tx, offset), data_rx), peak
    offset, rx, _, peak = find_sequence_offset_complex(data_tx, data_rx)
    if ntx > nrx:
        return adjust_data_length(data_tx, rx, method="extend", offset=offset), peak
    if ntx < nrx:
        return adjust_data_length(data_tx, np.roll(rx, offset), method="truncate"), peak
    return (data_tx, np.roll(rx, offset)), peak


# ------------------------------------------------------------------------------------------------ device-resident metrics
def cal_metrics_dev(out, idx_tx, alphabet, snr_db=None, maxlag=256, window=4096, trim=0, llr_minmax=False):
    """
    Signal-quality metrics of recovered rows that live in HBM: SER, BER, EVM, SNR estimate, GMI (exact or max-log LLRs) and
    the fast MI, without moving the rows or any LLR to the host.

    Each row is aligned as :func:`cal_ser_dev` aligns it (its tx mode, quarter turn and lag); then, over the compared
    overlap, the SNR is estimated from the known symbols (``qh_estimate_snr_*_dev``, what ``SignalQAM.est_snr`` does) unless
    ``snr_db`` is given, and one fused pass (``qh_metrics_*_dev``) counts symbol / bit errors and sums the error power,
    the per-bit GMI terms at that SNR and the MI terms at ``N0 = 1 / snr`` (what ``cal_gmi`` / ``cal_mi`` do).

    Returns one dict per row: ``ser, ber, evm, snr, s0, n0, gmi, gmi_per_bit, mi, errors, bit_errors, compared, tx_mode,
    rotation, lag`` (``snr`` linear; ``s0`` / ``n0`` NaN when ``snr_db`` is given).
    """
    from .. import _lib
    suf = "c64" if np.dtype(out.dtype) == np.complex64 else "c128"
    nrows, N = out.shape
    nmodes, ntx = idx_tx.shape
    M = int(np.prod(alphabet.shape))
    nbits = int(np.log2(M))
    res = []
    for r, al in enumerate(cal_ser_dev(out, idx_tx, alphabet, maxlag, window, trim)):
        row, tx = out.row(r).ptr, idx_tx.row(al["tx_mode"]).ptr
        aligned = (al["rotation"], al["lag"], int(trim))
        if snr_db is None:
            est = np.zeros(3, np.float64)
            _lib.call("qh_estimate_snr_%s_dev" % suf, row, N, tx, ntx, alphabet.ptr, M, *aligned, _lib.ptr(est))
            snr, s0, n0 = (float(v) for v in est)
        else:
            snr, s0, n0 = 10 ** (float(snr_db) / 10), float("nan"), float("nan")
        counts, sums = np.zeros(3, np.int64), np.zeros(2 + nbits, np.float64)
        _lib.call("qh_metrics_%s_dev" % suf, row, N, tx, ntx, alphabet.ptr, M, *aligned, snr, int(bool(llr_minmax)), _lib.ptr(counts),
                  _lib.ptr(sums))
        n = max(int(counts[2]), 1)
        gmi_per_bit = 1 - sums[2:] / n
        res.append(dict(ser=int(counts[0]) / n, ber=int(counts[1]) / (n * nbits), evm=float(np.sqrt(sums[0] / n)), snr=snr, s0=s0, n0=n0,
                        gmi=float(np.sum(gmi_per_bit)), gmi_per_bit=gmi_per_bit, mi=float(np.log2(M) - sums[1] / n),
                        errors=int(counts[0]), bit_errors=int(counts[1]), compared=int(counts[2]), tx_mode=al["tx_mode"],
                        rotation=al["rotation"], lag=al["lag"]))
    return res
