"""
Sequence alignment helpers of the pilot receiver / SER harness, behaviour of ``qampy.core.ber_functions``
(qampy/core/ber_functions.py:33-106): delay of one sequence inside another from the peak of their full cross-correlation,
trying the four quarter-turn rotations for complex data.  ``method="pyt"`` (the default) is the reference's host form, numpy / scipy: a few
thousand samples per call in the pilot receiver, but one full-length double-precision correlation per (received mode, free transmitted
mode) pair under the ``SignalQAM`` metrics.  ``method="hip"`` runs the same correlation, peak search and alignment on the device
(csrc/sync.hip).  :func:`cal_ser_dev` and :func:`cal_metrics_dev` are the device-resident counterparts of ``SignalQAM.cal_ser`` and its
siblings (qampy/core/signals.py:295-335) for captures that stay in HBM: ``sync="window"`` aligns by a bounded search
on decided indices, ``sync="full"`` by the full correlation as the host form does.
"""
import numpy as np
from scipy.signal import fftconvolve


def _method(method, name="method"):
    if method not in ("pyt", "hip"):
        raise ValueError("%s must be 'pyt' (host) or 'hip' (device), not %r" % (name, method))
    return method == "hip"


def _sync(sync):
    if sync not in ("window", "full"):
        raise ValueError("sync must be 'window' (bounded search on decisions) or 'full' (full cross-correlation), not %r" % (sync,))
    return sync == "full"


def _xcorr_hip(X, Y):
    """``(argmax |cc|, cc, result row of the peak search)`` of two host rows through csrc/sync.hip; ``cc`` in the dtype the host form
    gives (real for two real rows, single precision for two single-precision ones)."""
    from .. import _lib
    from . import hip_dsp
    if X.ndim != 1 or Y.ndim != 1 or X.shape[0] < 1 or Y.shape[0] < 1:
        raise ValueError("find_sequence_offset works on two non-empty 1-d sequences")
    n = X.shape[0] + Y.shape[0] - 1
    if n > hip_dsp.XCORR_MAX:
        raise ValueError("the full correlation of %d and %d samples is longer than 2**24" % (X.shape[0], Y.shape[0]))
    rt = np.result_type(X.dtype, Y.dtype)
    ct = np.complex64 if rt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128
    dx, dy = (_lib.DeviceArray.from_host(np.ascontiguousarray(v, dtype=ct)) for v in (X, Y))
    cc, res = _lib.DeviceArray((n,), ct), _lib.DeviceArray((hip_dsp.PEAK_FIELDS,), np.float64)
    hip_dsp.xcorr_dev(dx, dy, cc)
    hip_dsp.xcorr_peak_dev(cc, n, res)
    res, cc = res.to_host(), cc.to_host()
    if not np.iscomplexobj(X) and not np.iscomplexobj(Y):
        cc = np.ascontiguousarray(cc.real)
    return int(res[0]), cc, res


def find_sequence_offset(x, y, show_cc=False, method="pyt"):
    """Index by which ``y`` has to be shifted to line up with ``x`` (peak of the full cross-correlation, :33-69).  ``method="hip"``: the
    correlation and its peak search run on the device; ``show_cc`` then returns the device's correlation."""
    hip = _method(method)
    X = 1. * np.asarray(x)
    Y = 1. * np.asarray(y)
    if hip:
        k, cc, _ = _xcorr_hip(X, Y)
        idx = np.int64(k - (Y.shape[0] - 1))
        return (idx, cc) if show_cc else idx
    rev = Y.conj()[::-1] if np.iscomplexobj(Y) else Y[::-1]
    cc = fftconvolve(X, rev, "full")
    idx = abs(cc).argmax() - (Y.shape[0] - 1)
    return (idx, cc) if show_cc else idx


def find_sequence_offset_complex(x, y, method="pyt"):
    """``(offset, rotated y, quarter turns, peak)`` over the rotations ``1j**i`` of the received sequence ``y`` (:71-106).
    ``method="hip"``: correlation, peak search and the four directional maxima on the device; six scalars come back."""
    hip = _method(method)
    if not np.iscomplexobj(x) and not np.iscomplexobj(y):
        idx, cc = find_sequence_offset(x, y, show_cc=True, method=method)
        return idx, y, 0, cc
    if hip:
        from . import hip_dsp
        Y = 1. * np.asarray(y)
        _, _, res = _xcorr_hip(1. * np.asarray(x), Y)
        offset, turns, peak = hip_dsp.peak_decision(res, Y.shape[0])
        if not peak > 0:
            return 0, y, 0, 0.
        return np.int64(offset), y * 1.j ** turns, turns, peak
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


def _ws_buffer(ws, name, shape, dtype):
    """Buffer ``name`` of the workspace dict ``ws`` a caller keeps between calls (allocated again only when shape or dtype change);
    without a workspace, a fresh DeviceArray."""
    from .. import _lib
    if ws is None:
        return _lib.DeviceArray(shape, dtype)
    buf = ws.get(name)
    if buf is None or tuple(buf.shape) != tuple(int(v) for v in shape) or np.dtype(buf.dtype) != np.dtype(dtype):
        buf = ws[name] = _lib.DeviceArray(shape, dtype)
    return buf


def full_alignment_dev(out, idx_tx, alphabet, ws=None):
    """
    Alignment of recovered rows in HBM by the full cross-correlation, what ``SignalQAM._sync_and_adjust`` does on the host
    (qampy/signals.py:245-266): the transmitted symbols are rebuilt from ``alphabet[idx_tx]``, every received row is correlated with
    every transmitted mode (csrc/sync.hip), the small table of peaks is read back, and each row in turn takes the still-free mode with
    the largest peak; the labels of that mode are then rolled, cut or continued periodically to the row's length.

    Returns one dict per row: ``tx_mode, lag`` (the reference's offset), ``turns`` (quarter turns of the transmitted row), ``peak`` and
    ``labels``, the aligned (N,) int32 DeviceArray.  More rows than modes raises ``ValueError``.

    ``ws``: a dict the caller keeps (``ResidentReceiver`` does); the symbols, the correlation, the peak table and the label rows then
    live in it, so that a call at a shape seen before allocates nothing - and ``labels`` is good until the next call with that dict.
    """
    from .. import _lib
    from . import hip_dsp
    if len(out.shape) != 2 or len(idx_tx.shape) != 2:
        raise ValueError("the received rows and the transmitted indices must be 2-d")
    nrows, N = out.shape
    nmodes, ntx = idx_tx.shape
    if nrows > nmodes:
        raise ValueError("%d received rows but only %d transmitted modes to assign" % (nrows, nmodes))
    if N + ntx - 1 > hip_dsp.XCORR_MAX:
        raise ValueError("the full correlation of %d and %d symbols is longer than 2**24" % (N, ntx))
    if np.dtype(idx_tx.dtype) != np.int32 or np.dtype(alphabet.dtype) != np.dtype(out.dtype):
        raise TypeError("idx_tx must be int32 and the alphabet of the rows' dtype")
    n = N + ntx - 1
    sym = hip_dsp.labels_to_symbols_dev(idx_tx, alphabet, _ws_buffer(ws, "symbols", idx_tx.shape, out.dtype))
    cc, res = _ws_buffer(ws, "cc", (nrows, n), out.dtype), _ws_buffer(ws, "peaks", (nmodes, nrows, hip_dsp.PEAK_FIELDS), np.float64)
    for m in range(nmodes):
        hip_dsp.xcorr_dev(out, sym.row(m), cc)
        hip_dsp.xcorr_peak_dev(cc, n, res.row(m))
    table = res.to_host()
    free, aligned = list(range(nmodes)), []
    for r in range(nrows):
        best, pick = -100., None
        for m in free:
            cand = hip_dsp.peak_decision(table[m, r], ntx)
            if cand[2] > best:
                best, pick, chosen = cand[2], m, cand
        free.remove(pick)
        labels = hip_dsp.cyclic_gather_dev(idx_tx.row(pick), chosen[0], 0, _ws_buffer(ws, "labels%d" % r, (N,), np.int32))
        aligned.append(dict(tx_mode=pick, lag=chosen[0], turns=chosen[1], peak=chosen[2], labels=labels))
    return aligned


def _ser_full(out, idx_tx, alphabet, trim, ws=None):
    """:func:`cal_ser_dev` with ``sync="full"``: the fused counting pass on the aligned labels, at lag 0 and the matching rotation."""
    from .. import _lib
    suf = "c64" if np.dtype(out.dtype) == np.complex64 else "c128"
    N, M = out.shape[1], int(np.prod(alphabet.shape))
    res = []
    for r, al in enumerate(full_alignment_dev(out, idx_tx, alphabet, ws)):
        rot = (-al["turns"]) % 4                   # tx turned by 1j**turns: the received row is turned back instead
        counts, sums = np.zeros(3, np.int64), np.zeros(2 + int(np.log2(M)), np.float64)
        _lib.call("qh_metrics_%s_dev" % suf, out.row(r).ptr, N, al["labels"].ptr, N, alphabet.ptr, M, rot, 0, int(trim), 1., 0, _lib.ptr(counts),
                  _lib.ptr(sums))
        res.append(dict(errors=int(counts[0]), compared=int(counts[2]), ser=float(counts[0]) / max(int(counts[2]), 1), tx_mode=al["tx_mode"],
                        rotation=rot, lag=al["lag"], window_matches=None, window=None, peak=al["peak"]))
    return res


def cal_ser_dev(out, idx_tx, alphabet, maxlag=256, window=4096, trim=0, sync="window", sync_ws=None):
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
    sync : ``"window"`` - the bounded search above, linear overlap only;  ``"full"`` - the full cross-correlation of every row with
        every transmitted mode (:func:`full_alignment_dev`): any delay, the pattern rolled or continued periodically, every symbol of
        ``[trim, N - trim)`` compared, as ``SignalQAM.cal_ser`` does on the host (``maxlag`` and ``window`` are not used)
    sync_ws : workspace dict of ``sync="full"`` kept by the caller (:func:`full_alignment_dev`); None: buffers allocated per call

    Returns
    -------
    list of dicts per row: ``errors, compared, ser, tx_mode, rotation, lag, window_matches, window``; ``sync="full"``: ``lag`` is the
    reference's offset, ``window_matches`` and ``window`` are None, and ``peak`` (the correlation maximum) is added
    """
    from .. import _lib
    if _sync(sync):
        return _ser_full(out, idx_tx, alphabet, trim, sync_ws)
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


def _sync_and_adjust_hip(data_tx, data_rx, adjust):
    """``sync_and_adjust`` of two complex host rows on the device: upload, ``hip_dsp.sync_and_adjust_dev``, the adjusted row back."""
    from .. import _lib
    from . import hip_dsp
    tx, rx = np.asarray(data_tx), np.asarray(data_rx)
    if tx.ndim != 1 or rx.ndim != 1 or tx.shape[0] < 1 or rx.shape[0] < 1:
        raise ValueError("sync_and_adjust works on two non-empty 1-d sequences")
    if tx.shape[0] + rx.shape[0] - 1 > hip_dsp.XCORR_MAX:
        raise ValueError("the full correlation of %d and %d samples is longer than 2**24" % (tx.shape[0], rx.shape[0]))
    rt = np.result_type((1. * tx[:1]).dtype, (1. * rx[:1]).dtype)
    ct = np.complex64 if rt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128
    dtx, drx = (_lib.DeviceArray.from_host(np.ascontiguousarray(v, dtype=ct)) for v in (tx, rx))
    (atx, arx), peak = hip_dsp.sync_and_adjust_dev(dtx, drx, adjust)
    moved = tx if adjust == "tx" else rx
    out = (atx if adjust == "tx" else arx).to_host().astype((moved[:1] * 1.j).dtype, copy=False)      # the dtype of the host form's y * 1j**turns
    return ((out, data_rx) if adjust == "tx" else (data_tx, out)), peak


def sync_and_adjust(data_tx, data_rx, adjust="tx", method="pyt"):
    """
    Line up one received row with one transmitted row and give them a common length (ber_functions.py:108-160).

    The offset and the quarter turn come from :func:`find_sequence_offset_complex`; the sequence named by ``adjust`` is
    rotated, rolled or made periodic around the other one.  Returns ``((tx, rx), peak)``, ``peak`` the correlation
    maximum the mode assignment of ``SignalQAM._sync_and_adjust`` compares.  ``method="hip"``: correlation, peak search, rotation and
    roll / extension run on the device (csrc/sync.hip) and the adjusted row comes back; two real rows keep the host's arrangement around
    the device's offset.
    """
    assert adjust in ("tx", "rx"), "adjust need to be either 'tx' or 'rx'"
    if _method(method) and (np.iscomplexobj(data_tx) or np.iscomplexobj(data_rx)):
        return _sync_and_adjust_hip(data_tx, data_rx, adjust)
    ntx, nrx = data_tx.shape[0], data_rx.shape[0]
    if adjust == "tx":
        offset, tx, _, peak = find_sequence_offset_complex(data_rx, data_tx, method)
        if ntx > nrx:
            return adjust_data_length(np.roll(tx, offset), data_rx, method="truncate"), peak
        if ntx < nrx:
            return adjust_data_length(tx, data_rx, method="extend", offset=offset), peak
        return (np.roll(tx, offset), data_rx), peak
    offset, rx, _, peak = find_sequence_offset_complex(data_tx, data_rx, method)
    if ntx > nrx:
        return adjust_data_length(data_tx, rx, method="extend", offset=offset), peak
    if ntx < nrx:
        return adjust_data_length(data_tx, np.roll(rx, offset), method="truncate"), peak
    return (data_tx, np.roll(rx, offset)), peak


# ------------------------------------------------------------------------------------------------ device-resident metrics
def cal_metrics_dev(out, idx_tx, alphabet, snr_db=None, maxlag=256, window=4096, trim=0, llr_minmax=False, sync="window", sync_ws=None):
    """
    Signal-quality metrics of recovered rows that live in HBM: SER, BER, EVM, SNR estimate, GMI (exact or max-log LLRs) and
    the fast MI, without moving the rows or any LLR to the host.

    Each row is aligned as :func:`cal_ser_dev` aligns it (its tx mode, quarter turn and lag; ``sync="full"``: by the full
    cross-correlation, :func:`full_alignment_dev`, the labels rolled or continued periodically to the row's length); then, over the compared
    overlap, the SNR is estimated from the known symbols (``qh_estimate_snr_*_dev``, what ``SignalQAM.est_snr`` does) unless
    ``snr_db`` is given, and one fused pass (``qh_metrics_*_dev``) counts symbol / bit errors and sums the error power,
    the per-bit GMI terms at that SNR and the MI terms at ``N0 = 1 / snr`` (what ``cal_gmi`` / ``cal_mi`` do).

    Returns one dict per row: ``ser, ber, evm, snr, s0, n0, gmi, gmi_per_bit, mi, errors, bit_errors, compared, tx_mode,
    rotation, lag`` (``snr`` linear; ``s0`` / ``n0`` NaN when ``snr_db`` is given); ``sync="full"`` adds ``peak``, ``window_matches`` and
    ``window`` (both None) and ``lag`` is the reference's offset (``sync_ws``: as in :func:`cal_ser_dev`).  ``rotation`` turns the received row onto the transmitted labels (the
    host form turns the transmitted row instead): every figure is the host's, but ``gmi_per_bit`` is ordered by the transmitted labels -
    with an odd ``rotation`` the in-phase and quadrature halves of a square alphabet's bits trade places against ``SignalQAM.cal_gmi``.
    """
    from .. import _lib
    suf = "c64" if np.dtype(out.dtype) == np.complex64 else "c128"
    nrows, N = out.shape
    nmodes, ntx = idx_tx.shape
    M = int(np.prod(alphabet.shape))
    nbits = int(np.log2(M))
    res = []
    full = _sync(sync)
    alignment = [dict(al, rotation=(-al["turns"]) % 4) for al in full_alignment_dev(out, idx_tx, alphabet, sync_ws)] if full else cal_ser_dev(
        out, idx_tx, alphabet, maxlag, window, trim)
    for r, al in enumerate(alignment):
        row, tx = out.row(r).ptr, idx_tx.row(al["tx_mode"]).ptr
        aligned = (al["rotation"], al["lag"], int(trim))
        if full:                                   # the labels already lie on the row: its own length, lag 0
            tx, ntx, aligned = al["labels"].ptr, N, (al["rotation"], 0, int(trim))
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
        if full:
            res[-1].update(peak=al["peak"], window_matches=None, window=None)
    return res
