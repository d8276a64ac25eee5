"""Feed-forward carrier recovery: Viterbi-Viterbi and QPSK partitioning (qampy_amd/csrc/cpr.hip), and the pilot phase trace (csrc/bps.hip)."""
import numpy as np

from ... import _lib
from ._args import buffer, field

VV_NMAX, VV_MMAX, P16_NBLOCK_MAX = 1024, 64, 4096          # limits of csrc/cpr.hip


def _cpr_check(name, E, trace, Eout, trace_len):
    """``c`` of the field; here a wrong dtype or rank is a ValueError like a wrong shape."""
    c = field(E, name, empty=True, exc=ValueError)[0]
    buffer(Eout, name, "Eout", E.shape, E.dtype)
    buffer(trace, name, "trace", (E.shape[0], trace_len), _lib.suffix(E.dtype)[1])
    return c


def vv_recover_dev(E, N, M, trace, Eout):
    """
    Viterbi-Viterbi carrier recovery of every row of the (nmodes, L) complex DeviceArray ``E`` in HBM (csrc/cpr.hip; host layer
    qampy/core/phaserecovery.py:40-79): ``M``-PSK, ``2 <= M <= 64``, windows of ``N`` samples, ``1 <= N <= min(L, 1024)``.  ``trace``:
    (nmodes, L - N + 1) DeviceArray in the signal's real type, ``(unwrap(angle(window sums)) - pi) / M``; ``Eout``: (nmodes, L) like ``E``,
    ``E[:, o + k] * exp(-1j * trace[:, k])`` with ``o = (N - 1) // 2`` and zeros on the other ``N - 1`` samples.  ValueError for sizes out
    of range and for wrong shapes or dtypes.  Nothing is read back; enqueued on the current library stream.
    """
    N, M = int(N), int(M)
    if len(E.shape) != 2:
        raise ValueError("vv_recover_dev works on a 2-d complex array")
    L = E.shape[1]
    if not 1 <= N <= VV_NMAX:
        raise ValueError("N must be between 1 and %d" % VV_NMAX)
    if N > L:
        raise ValueError("a window of %d samples does not fit a signal of %d" % (N, L))
    if not 2 <= M <= VV_MMAX:
        raise ValueError("M must be between 2 and %d" % VV_MMAX)
    c = _cpr_check("vv_recover_dev", E, trace, Eout, L - N + 1)
    _lib.call("qh_vv_recover_%s_dev" % c, E.ptr, E.shape[0], L, N, M, trace.ptr, Eout.ptr)


def partition16_recover_dev(E, Nblock, trace, Eout):
    """
    16-QAM carrier recovery by QPSK partitioning of every row of the (nmodes, L) complex DeviceArray ``E`` in HBM (csrc/cpr.hip; host layer
    qampy/core/phaserecovery.py:292-382) in blocks of ``Nblock`` samples, ``1 <= Nblock <= 4096``.  ``trace``: (nmodes, L) DeviceArray in
    the signal's real type, the reference's trace; ``Eout = E * exp(-1j * trace)``, every mode by its own trace (the reference rotates every
    mode by four times the last mode's raw estimate: INTEGRATION.md).  ValueError for ``Nblock`` out of range and for wrong shapes or dtypes.
    Nothing is read back; enqueued on the current library stream.
    """
    Nblock = int(Nblock)
    if not 1 <= Nblock <= P16_NBLOCK_MAX:
        raise ValueError("Nblock must be between 1 and %d" % P16_NBLOCK_MAX)
    if len(E.shape) != 2 or E.shape[1] < 1:
        raise ValueError("partition16_recover_dev works on a 2-d complex array")
    c = _cpr_check("partition16_recover_dev", E, trace, Eout, E.shape[1])
    _lib.call("qh_partition16_recover_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], Nblock, trace.ptr, Eout.ptr)


def _cpr_host(E, run, trace_len):
    """Rows of a host array up, ``run(dE, trace, out)``, ``(Eout, trace)`` back."""
    E = np.asarray(E)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("carrier recovery works on a 2-d complex array")
    suf, rt, ct = _lib.suffix(E.dtype)
    D = _lib.DeviceArray
    dE = D.from_host(np.ascontiguousarray(E))
    trace, out = D((E.shape[0], trace_len), rt), D(E.shape, ct)
    run(dE, trace, out)
    return out.to_host(), trace.to_host()


def vv_recover(E, N, M):
    """:func:`vv_recover_dev` for a host array ``E (nmodes, L)``: ``(Eout, trace)`` with the trace of every row."""
    E = np.asarray(E)
    N, M = int(N), int(M)
    if E.ndim != 2:
        raise TypeError("vv_recover works on a 2-d complex array")
    if not 1 <= N <= VV_NMAX:
        raise ValueError("N must be between 1 and %d" % VV_NMAX)
    if N > E.shape[1]:
        raise ValueError("a window of %d samples does not fit a signal of %d" % (N, E.shape[1]))
    if not 2 <= M <= VV_MMAX:
        raise ValueError("M must be between 2 and %d" % VV_MMAX)
    return _cpr_host(E, lambda dE, tr, out: vv_recover_dev(dE, N, M, tr, out), E.shape[1] - N + 1)


def partition16_recover(E, Nblock):
    """:func:`partition16_recover_dev` for a host array ``E (nmodes, L)``: ``(Eout, trace)``."""
    E = np.asarray(E)
    Nblock = int(Nblock)
    if E.ndim != 2 or E.shape[1] < 1:
        raise TypeError("partition16_recover works on a non-empty 2-d complex array")
    if not 1 <= Nblock <= P16_NBLOCK_MAX:
        raise ValueError("Nblock must be between 1 and %d" % P16_NBLOCK_MAX)
    return _cpr_host(E, lambda dE, tr, out: partition16_recover_dev(dE, Nblock, tr, out), E.shape[1])


def pilot_phase_trace(E, knots, knot_phase):
    """Linear interpolation of the pilot phases ``knot_phase (nmodes, nk)`` at the symbol positions ``knots`` to every symbol of ``E
    (nmodes, L)`` (np.interp) and its removal, on the device: ``(E * exp(-1j trace), trace)``, the trace in E's complex dtype as the
    reference returns it (qampy/core/pilotbased_receiver.py:318-327)."""
    suf, rt, ct = _lib.suffix(E.dtype)
    E = np.ascontiguousarray(E)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("pilot_phase_trace works on a 2-d complex array")
    knots = np.ascontiguousarray(knots, dtype=np.int64)
    kph = np.ascontiguousarray(knot_phase, dtype=np.float64)
    if kph.shape != (E.shape[0], knots.size) or knots.size < 1:
        raise ValueError("one phase per mode and knot")
    if np.any(np.diff(knots.ravel()) <= 0):                       # (the kernel divides by the distance of two knots)
        raise ValueError("knots must be strictly increasing")
    big = E.nbytes >= _lib.PINNED_MIN_BYTES                       # results through the pinned pool: one DMA at the link rate each
    out = _lib.pinned_empty(E.shape, E.dtype) if big else np.empty_like(E)
    trace = _lib.pinned_empty(E.shape, E.dtype) if big else np.empty_like(E)
    _lib.call("qh_pilot_phase_trace_" + _lib.cname(suf), _lib.ptr(E), E.shape[0], E.shape[1], _lib.ptr(knots), _lib.ptr(kph), knots.size,
              _lib.ptr(out), _lib.ptr(trace))
    return out, trace
