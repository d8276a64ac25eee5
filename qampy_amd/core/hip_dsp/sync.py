"""
Synchronisation of rx and tx rows: csrc/sync.hip on DeviceArrays, for find_sequence_offset / find_sequence_offset_complex /
sync_and_adjust of qampy/core/ber_functions.py:33-160.
"""
import numpy as np

from ... import _lib
from ._args import buffer, cplx, field

XCORR_MAX = 2 ** 24                # longest full correlation, nx + ny - 1 (the largest power-of-two transform of csrc/fft.hip)
PEAK_TILE, PEAK_FIELDS = 4096, 6   # values per workgroup of the peak search's first stage; doubles per row of its result
SYNC_ROW_MAX = 2 ** 31             # longest row of the gather and the label kernels


def xcorr_dev(x, y, out):
    """Full cross-correlation ``fftconvolve(x, conj(y)[::-1], "full")`` of every row of ``x`` ((nx,) or (rows, nx)) with the row ``y`` (ny,)
    into ``out`` ((nx + ny - 1,) or (rows, nx + ny - 1)), all complex DeviceArrays of one dtype: the peak of ``|out|`` at index ``k`` puts
    ``y`` ``k - (ny - 1)`` samples into ``x`` (qampy/core/ber_functions.py:60-68).  ``nx + ny - 1`` at most 2**24.  Nothing is read back."""
    c, rows, nx = field(x, "xcorr_dev", "x", ndim=(1, 2))
    if len(y.shape) != 1 or y.shape[0] < 1:
        raise ValueError("xcorr_dev: y must be one non-empty row")
    ny = y.shape[0]
    if np.dtype(y.dtype) != np.dtype(x.dtype) or np.dtype(out.dtype) != np.dtype(x.dtype):
        raise TypeError("xcorr_dev: x, y and out must have one dtype")
    n = nx + ny - 1
    if n > XCORR_MAX:
        raise ValueError("xcorr_dev: nx + ny - 1 = %d is above 2**24" % n)
    if rows > 65535:
        raise ValueError("xcorr_dev: at most 65535 rows")
    if tuple(out.shape) != tuple(x.shape[:-1]) + (n,):
        raise ValueError("xcorr_dev: out must be %s" % (tuple(x.shape[:-1]) + (n,),))
    _lib.call("qh_xcorr_%s_dev" % c, x.ptr, rows, nx, y.ptr, ny, out.ptr)
    return out


def xcorr_peak_dev(cc, n, res):
    """Peak search of a correlation (csrc/sync.hip): per row of ``cc`` the (6,) doubles ``res`` = index of the first maximum of ``|cc|`` over
    ``[0, n)`` (``np.argmax``'s, a NaN included), ``max Re, max Im, max -Re, max -Im`` (the four quarter-turn hypotheses; NaN if the row holds
    one) and ``|cc|`` there.  ``cc``: one row of at least ``n`` values, or (rows, n); ``res``: (6,) or (rows, 6) float64.  Nothing is read back."""
    c, rows, length = field(cc, "xcorr_peak_dev", "cc", ndim=(1, 2))
    n = int(n)
    if n < 1 or n > length or (rows > 1 and n != length):
        raise ValueError("xcorr_peak_dev: n must be in [1, %d]%s" % (length, " and the row length of a stack" if rows > 1 else ""))
    if n > 2 * XCORR_MAX or rows > 65535:
        raise ValueError("xcorr_peak_dev: at most 2**25 values per row and 65535 rows")
    if np.dtype(res.dtype) != np.float64 or int(np.prod(res.shape)) != rows * PEAK_FIELDS or res.shape[-1] != PEAK_FIELDS:
        raise ValueError("xcorr_peak_dev: res must be float64 (%d, %d)" % (rows, PEAK_FIELDS))
    _lib.call("qh_xcorr_peak_%s_dev" % c, cc.ptr, rows, n, res.ptr)
    return res


def cyclic_gather_dev(src, offset, turns, out):
    """``out[i] = 1j**turns * src[(i - offset) % len(src)]`` for every ``i`` of ``out`` (1-d DeviceArrays of one dtype, complex or int32;
    ``turns`` must be 0 for int32): ``np.roll(src, offset)``, cut or continued periodically to ``out``'s length - the three arrangements of
    ``sync_and_adjust``.  The rotation is exact.  ``out`` must not be ``src``."""
    if len(src.shape) != 1 or len(out.shape) != 1 or src.shape[0] < 1 or out.shape[0] < 1:
        raise ValueError("cyclic_gather_dev: src and out must be non-empty 1-d rows")
    if np.dtype(src.dtype) != np.dtype(out.dtype):
        raise TypeError("cyclic_gather_dev: src and out must have one dtype")
    if int(offset) != offset or int(turns) != turns:
        raise ValueError("cyclic_gather_dev: offset and turns must be integers")
    offset, turns = int(offset), int(turns)
    if max(src.shape[0], out.shape[0], abs(offset)) > SYNC_ROW_MAX:
        raise ValueError("cyclic_gather_dev: lengths and |offset| at most 2**31")
    if src.ptr == out.ptr:
        raise ValueError("cyclic_gather_dev: out must be another buffer than src")
    if np.dtype(src.dtype) == np.int32:
        if turns % 4:
            raise ValueError("cyclic_gather_dev: labels cannot be rotated")
        _lib.call("qh_cyclic_gather_i32_dev", src.ptr, src.shape[0], offset, out.shape[0], out.ptr)
        return out
    if np.dtype(src.dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise TypeError("cyclic_gather_dev works on complex64, complex128 or int32 rows")
    c = cplx(src, "cyclic_gather_dev", "src")
    _lib.call("qh_cyclic_gather_%s_dev" % c, src.ptr, src.shape[0], offset, turns % 4, out.shape[0], out.ptr)
    return out


def labels_to_symbols_dev(idx, alphabet, out):
    """``out = alphabet[idx]`` for int32 labels of any shape (0 for a label outside the alphabet); ``out``: ``idx``'s shape, ``alphabet``'s dtype."""
    c = cplx(alphabet, "labels_to_symbols_dev", "alphabet")
    n, M = int(np.prod(idx.shape)), int(np.prod(alphabet.shape))
    if np.dtype(idx.dtype) != np.int32:
        raise TypeError("labels_to_symbols_dev: idx must be int32")
    buffer(out, "labels_to_symbols_dev", "out", idx.shape, alphabet.dtype)
    if n < 1 or n > SYNC_ROW_MAX or M < 1:
        raise ValueError("labels_to_symbols_dev: between 1 and 2**31 labels, at least one alphabet point")
    _lib.call("qh_labels_to_symbols_%s_dev" % c, idx.ptr, n, alphabet.ptr, M, out.ptr)
    return out


def peak_decision(res, ny):
    """``(offset, turns, peak)`` of one row of :func:`xcorr_peak_dev`'s result, the rule of ``find_sequence_offset_complex``
    (qampy/core/ber_functions.py:71-106): the turn with the largest directional maximum; ``(0, 0, 0.)`` unless that maximum is positive."""
    peaks = np.asarray(res, dtype=np.float64)[1:5]
    if not peaks.max() > 0:
        return 0, 0, 0.
    turns = int(np.argmax(peaks))
    return int(res[0]) - (int(ny) - 1), turns, float(peaks[turns])


def _sync_pair(x, y, what):
    c = cplx(x, what, "the first row")
    if len(x.shape) != 1 or len(y.shape) != 1 or x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError("%s works on two non-empty 1-d rows" % what)
    if np.dtype(y.dtype) != np.dtype(x.dtype):
        raise TypeError("%s: both rows must have one dtype" % what)
    if x.shape[0] + y.shape[0] - 1 > XCORR_MAX:
        raise ValueError("%s: the full correlation of %d and %d samples is longer than 2**24" % (what, x.shape[0], y.shape[0]))
    return c


def find_sequence_offset_complex_dev(x, y, cc=None, res=None):
    """``(offset, turns, peak)`` of ``find_sequence_offset_complex(x, y)`` for two 1-d complex DeviceArrays: ``y * 1j**turns`` rolled by
    ``offset`` lines up with ``x``.  Full correlation, peak search, and only the (6,) result is read back.  ``cc`` / ``res``: buffers to
    reuse ((nx + ny - 1,) of the rows' dtype; (6,) float64)."""
    _sync_pair(x, y, "find_sequence_offset_complex_dev")
    n = x.shape[0] + y.shape[0] - 1
    cc = _lib.DeviceArray((n,), x.dtype) if cc is None else cc
    res = _lib.DeviceArray((PEAK_FIELDS,), np.float64) if res is None else res
    xcorr_dev(x, y, cc)
    xcorr_peak_dev(cc, n, res)
    return peak_decision(res.to_host(), y.shape[0])


def sync_and_adjust_dev(tx, rx, adjust="tx", out=None):
    """``sync_and_adjust`` (qampy/core/ber_functions.py:108-160) on two 1-d complex DeviceArrays: the row named by ``adjust`` is turned by
    the quarter turns, rolled by the offset of the correlation peak and cut or continued periodically to the other row's length, into
    ``out`` (the other row's length; allocated when None).  Returns ``((tx, rx), peak)`` with the adjusted row replaced by ``out``."""
    if adjust not in ("tx", "rx"):
        raise ValueError("adjust need to be either 'tx' or 'rx'")
    _sync_pair(tx, rx, "sync_and_adjust_dev")
    fixed, moved = (rx, tx) if adjust == "tx" else (tx, rx)
    buffer(out, "sync_and_adjust_dev", "out", fixed.shape, moved.dtype, optional=True)          # (the length of the row that stays)
    offset, turns, peak = find_sequence_offset_complex_dev(fixed, moved)
    out = _lib.DeviceArray(fixed.shape, moved.dtype) if out is None else out
    cyclic_gather_dev(moved, offset, turns, out)
    return ((out, rx) if adjust == "tx" else (tx, out)), peak
