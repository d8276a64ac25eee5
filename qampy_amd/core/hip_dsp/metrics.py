"""
Signal-quality metrics: the last exports of pythran_dsp (qampy/core/pythran_dsp.py:87-131, :244-313) that
qampy/core/signal_quality.py:27-29 binds; kernels in qampy_amd/csrc/metrics.hip.
"""
import numpy as np

from ... import _lib


def bits_map_labels(bits_map):
    """
    Invert the reference's ``bits_map`` ``(nbits, M/2, 2)`` (``generate_bitmapping_mtx``: ``[k, :, b]`` are the points whose
    bit ``k`` is ``b``) into the alphabet in label order: entry ``g`` is the point whose bits, MSB first, spell ``g``.
    Raises ValueError if the map is not a labelling of one alphabet of ``M = 2^nbits`` distinct points.
    """
    bm = np.asarray(bits_map)
    if bm.ndim != 3 or bm.shape[2] != 2:
        raise ValueError("bits_map must have the shape (nbits, M/2, 2)")
    nbits, half = bm.shape[0], bm.shape[1]
    M = 2 * half
    if nbits < 1 or M != 1 << nbits:
        raise ValueError("bits_map of %d bits holds %d points, not 2**%d" % (nbits, M, nbits))
    points = np.concatenate([bm[0, :, 0], bm[0, :, 1]])
    if np.unique(points).size != M:
        raise ValueError("bits_map: the points of bit 0 are not %d distinct points" % M)
    labels = np.zeros(M, dtype=np.int64)
    for k in range(nbits):
        on, off = np.isin(points, bm[k, :, 1]), np.isin(points, bm[k, :, 0])
        if not np.all(on ^ off) or np.count_nonzero(on) != half:
            raise ValueError("bits_map: bit %d does not split the alphabet into two halves" % k)
        labels |= on.astype(np.int64) << (nbits - 1 - k)
    if not np.array_equal(np.sort(labels), np.arange(M)):
        raise ValueError("bits_map: the bit patterns are not a labelling (two points share a label)")
    alphabet = np.empty(M, dtype=bm.dtype)
    alphabet[labels] = points
    return alphabet


def _demapper(rx_symbs, num_bits, snr, bits_map, minmax):
    rx = np.ascontiguousarray(rx_symbs)
    if rx.ndim != 1 or not np.iscomplexobj(rx):
        raise TypeError("the demapper works on a 1-d complex array")
    suf, rt, ct = _lib.suffix(rx.dtype)
    alphabet = np.ascontiguousarray(bits_map_labels(bits_map), dtype=ct)
    nbits = int(np.log2(alphabet.size))
    if not 1 <= int(num_bits) <= nbits:
        raise ValueError("num_bits must be 1 .. bits_map.shape[0]")
    L = np.zeros((rx.size, nbits), dtype=np.float64)
    name = "qh_soft_l_value_demapper_" + ("minmax_" if minmax else "") + _lib.cname(suf)
    _lib.call(name, _lib.ptr(rx), rx.size, nbits, float(snr), _lib.ptr(alphabet), alphabet.size, _lib.ptr(L))
    return L if int(num_bits) == nbits else np.ascontiguousarray(L[:, :int(num_bits)])


def soft_l_value_demapper(rx_symbs, num_bits, snr, bits_map):
    """``(N, num_bits)`` float64 LLRs ``ln sum_{bit=1} exp(-snr |s - r|^2) - ln sum_{bit=0} ...`` (pythran_dsp.py:87-104)."""
    return _demapper(rx_symbs, num_bits, snr, bits_map, False)


def soft_l_value_demapper_minmax(rx_symbs, num_bits, snr, bits_map):
    """Max-log LLRs ``snr (min_{bit=0} |s - r|^2 - min_{bit=1} |s - r|^2)`` (pythran_dsp.py:106-131)."""
    return _demapper(rx_symbs, num_bits, snr, bits_map, True)


def estimate_snr(signal_rx, symbols_tx, gray_symbols):
    """``(snr, S0, N0)`` linear, from the per-point means and spreads of the received symbols (pythran_dsp.py:244-286).
    A point of ``gray_symbols`` that ``symbols_tx`` never equals gives NaN, as in the reference."""
    rx = np.ascontiguousarray(signal_rx)
    suf, rt, ct = _lib.suffix(rx.dtype)
    tx = np.ascontiguousarray(symbols_tx, dtype=ct)
    al = np.ascontiguousarray(gray_symbols, dtype=ct)
    if rx.ndim != 1 or tx.shape != rx.shape:
        raise ValueError("signal_rx and symbols_tx must be 1-d arrays of the same length")
    res = np.zeros(3, np.float64)
    _lib.call("qh_estimate_snr_" + _lib.cname(suf), _lib.ptr(rx), rx.size, _lib.ptr(tx), tx.size, _lib.ptr(al), al.size, _lib.ptr(res))
    return float(res[0]), float(res[1]), float(res[2])


def cal_mi_mc(noise, symbols, N0):
    """Mutual information from the noise samples, averaged over every transmitted point (pythran_dsp.py:289-300)."""
    n = np.ascontiguousarray(noise)
    suf, rt, ct = _lib.suffix(n.dtype)
    al = np.ascontiguousarray(symbols, dtype=ct)
    mi = np.zeros(1, np.float64)
    _lib.call("qh_cal_mi_mc_" + _lib.cname(suf), _lib.ptr(n), n.size, _lib.ptr(al), al.size, float(N0), _lib.ptr(mi))
    return float(mi[0])


def cal_mi_mc_fast(sig, sig_tx, symbols, N0):
    """Mutual information from received / transmitted pairs (pythran_dsp.py:303-313)."""
    x = np.ascontiguousarray(sig)
    suf, rt, ct = _lib.suffix(x.dtype)
    tx = np.ascontiguousarray(sig_tx, dtype=ct)
    al = np.ascontiguousarray(symbols, dtype=ct)
    if tx.shape != x.shape or x.ndim != 1:
        raise ValueError("sig and sig_tx must be 1-d arrays of the same length")
    mi = np.zeros(1, np.float64)
    _lib.call("qh_cal_mi_mc_fast_" + _lib.cname(suf), _lib.ptr(x), _lib.ptr(tx), x.size, _lib.ptr(al), al.size, float(N0), _lib.ptr(mi))
    return float(mi[0])
