"""
Drop-in for the BPS entry points of the compiled module ``qampy.core.pythran_dsp`` on MI355X.

``bps`` and ``select_angles`` keep the signatures of the ``#pythran export`` lines qampy/core/pythran_dsp.py:45-46 and
:133-136; the kernels live in qampy_amd/csrc/bps.hip.
"""
import threading

import numpy as np

from .. import _lib


def bps(E, testangles, symbols, N):
    """
    Blind phase search: int32 index of the best test angle for every symbol of ONE mode (pythran_dsp.py:45-85 with
    select_angle_index :26-42).  ``testangles`` is ``(1, A)`` (one grid) or ``(L, A)`` (per-symbol grid).
    """
    suf, rt, ct = _lib.suffix(E.dtype)
    if E.ndim != 1 or not np.iscomplexobj(E):
        raise TypeError("bps works on a 1-d complex array")
    E = np.ascontiguousarray(E)
    if testangles.ndim != 2 or testangles.dtype != rt:
        raise TypeError("testangles must be a 2-d %s array" % np.dtype(rt).name)
    symbols = np.ascontiguousarray(symbols)
    if symbols.dtype != ct:
        raise TypeError("symbols must be %s" % np.dtype(ct).name)
    testangles = np.ascontiguousarray(testangles)
    p, A = testangles.shape
    L = E.shape[0]
    if not (p == 1 or p == L):
        raise ValueError("p must be either 1 or the length of the input signal")
    idx = np.zeros(L, dtype=np.int32)
    _lib.call("qh_bps_" + _lib.cname(suf), _lib.ptr(E), L, _lib.ptr(testangles), p, A, _lib.ptr(symbols),
              symbols.size, int(N), _lib.ptr(idx))
    return idx


def select_angles(angles, idx):
    """``angles[0, idx[i]]`` (one grid) or ``angles[i, idx[i]]`` (per-symbol grid), pythran_dsp.py:133-153."""
    suf, rt, ct = _lib.suffix(angles.dtype)
    angles = np.ascontiguousarray(angles)
    if angles.ndim != 2:
        raise TypeError("angles must be 2-d")
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    p, A = angles.shape
    L = idx.shape[0] if p <= 1 else p
    if idx.shape[0] < L:
        raise ValueError("a per-symbol grid of %d rows needs as many indices (got %d)" % (p, idx.shape[0]))
    if idx.size and (idx.max() >= A or idx.min() < 0):
        raise ValueError("angle index out of range")
    out = np.zeros(L, dtype=rt)
    _lib.call("qh_select_angles_f" + suf, _lib.ptr(angles), p, A, _lib.ptr(idx), L, _lib.ptr(out))
    return out


def test_angle_grid(Mtestangles, rt):
    """The ``(1, A)`` grid of the host layer: ``np.linspace(-pi/4, pi/4, A, endpoint=False)`` formed in double and cast
    (qampy/core/phaserecovery.py:145)."""
    return np.linspace(-np.pi / 4, np.pi / 4, int(Mtestangles), endpoint=False, dtype=rt).reshape(1, -1)


def bps_recover_dev(E, Mtestangles, symbols, N, idx, ph, Eout, angles=None, part=0, nparts=1):
    """
    Device-resident carrier recovery of all modes at once: BPS index, grid look-up, ``np.unwrap`` of the interior and
    de-rotation (host layer qampy/core/phaserecovery.py:145-159) without leaving HBM.  All arguments except the integers
    are DeviceArrays: E, Eout (nmodes, L) complex; ph (nmodes, L) real; idx (nmodes, L) int32; ``angles`` the (A,) grid of
    :func:`test_angle_grid` (``None``: formed on the device in the signal's precision).

    ``part`` / ``nparts``: the work in ``nparts`` calls (``qh_bps_recover_part_*_dev``) - parts ``0 .. nparts - 2`` search a run of the signal each,
    the last one searches the rest, unwraps and de-rotates; same results, see ``ResidentReceiver.run(overlap=True)`` for what it is good for.
    """
    suf, rt, ct = _lib.suffix(E.dtype)
    nm, L = E.shape
    if nparts == 1:
        _lib.call("qh_bps_recover_" + _lib.cname(suf) + "_dev", E.ptr, nm, L, angles.ptr if angles is not None else None,
                  int(Mtestangles), symbols.ptr, int(np.prod(symbols.shape)), int(N), idx.ptr, ph.ptr, Eout.ptr)
    else:
        _lib.call("qh_bps_recover_part_" + _lib.cname(suf) + "_dev", E.ptr, nm, L, angles.ptr if angles is not None else None,
                  int(Mtestangles), symbols.ptr, int(np.prod(symbols.shape)), int(N), idx.ptr, ph.ptr, Eout.ptr, int(part), int(nparts))


def bps_recover(E, Mtestangles, symbols, N):
    """
    Carrier recovery of every row of ``E (nmodes, L)`` in one go: upload once, blind phase search + unwrap + de-rotation in
    HBM, ``(Eout, ph)`` back.  What the host layer of the reference does mode by mode with three compiled / numpy passes.
    """
    suf, rt, ct = _lib.suffix(E.dtype)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("bps_recover works on a 2-d complex array")
    symbols = np.ascontiguousarray(symbols)
    if symbols.dtype != ct:
        raise TypeError("symbols must be %s" % np.dtype(ct).name)
    nm, L = E.shape
    if L == 0:
        return np.zeros((nm, 0), ct), np.zeros((nm, 0), rt)
    D = _lib.DeviceArray
    E = np.ascontiguousarray(E)
    dsy, dang = D.from_host(symbols), D.from_host(test_angle_grid(Mtestangles, rt))
    dE, idx, ph, out = D((nm, L), ct), D((nm, L), np.int32), D((nm, L), rt), D((nm, L), ct)
    if E.nbytes < _lib.PINNED_MIN_BYTES:
        dE.set(E)
        bps_recover_dev(dE, Mtestangles, dsy, N, idx, ph, out, angles=dang)
        return out.to_host(), ph.to_host()
    return _row_pipeline(E, dE, (out, ph), lambda r: bps_recover_dev(_row2d(dE, r), Mtestangles, dsy, N, _row2d(idx, r), _row2d(ph, r), _row2d(out, r),
                                                                    angles=dang))


def twostage_offsets(Mtestangles, B):
    """Offsets ``off[a]`` of the ``B`` fine angles of the two-stage search around a coarse estimate, in double, by the reference's
    expression (qampy/core/phaserecovery.py:278-279): symbol ``j`` is searched at ``(rt)(float64(coarse[j]) + off[a])``.  The library forms
    the same table with the same double operations (csrc/bps.hip); the tests hold it to this one."""
    return np.linspace(-B / 2, B / 2, B) / (B * Mtestangles) * np.pi / 2


def bps_twostage_recover_dev(E, Mtestangles, B, symbols, N, idx1, idx2, ph, Eout, angles=None):
    """
    Device-resident two-stage carrier recovery of all modes at once (host layer qampy/core/phaserecovery.py:222-288): coarse search over
    ``Mtestangles`` angles, ``B`` fine angles around each symbol's coarse estimate (:func:`twostage_offsets`; the ``(L, B)`` grid of the
    reference is never formed), ``np.unwrap`` of the whole row and de-rotation without leaving HBM.  All arguments except the integers are
    DeviceArrays: E, Eout (nmodes, L) complex, not the same buffer; ph (nmodes, L) real; idx1, idx2 (nmodes, L) int32 - the coarse and the
    fine index; ``angles`` the (A,) grid of :func:`test_angle_grid` (``None``: formed on the device in the signal's precision).
    ``1 <= B <= 64``.
    """
    suf, rt, ct = _lib.suffix(E.dtype)
    nm, L = E.shape
    _lib.call("qh_bps_twostage_recover_" + _lib.cname(suf) + "_dev", E.ptr, nm, L, angles.ptr if angles is not None else None,
              int(Mtestangles), int(B), symbols.ptr, int(np.prod(symbols.shape)), int(N), idx1.ptr, idx2.ptr, ph.ptr, Eout.ptr)


def bps_twostage_recover(E, Mtestangles, symbols, N, B=4):
    """
    Two-stage carrier recovery of every row of ``E (nmodes, L)`` in one go: upload once, :func:`bps_twostage_recover_dev` in HBM,
    ``(Eout, ph)`` back - where the composed host layer makes two uploads, two index downloads and an ``(L, B)`` grid per mode.
    """
    E = np.asarray(E)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("bps_twostage_recover works on a 2-d complex array")
    suf, rt, ct = _lib.suffix(E.dtype)
    symbols = np.ascontiguousarray(symbols)
    if symbols.dtype != ct:
        raise TypeError("symbols must be %s" % np.dtype(ct).name)
    nm, L = E.shape
    if L == 0:
        return np.zeros((nm, 0), ct), np.zeros((nm, 0), rt)
    D = _lib.DeviceArray
    E = np.ascontiguousarray(E)
    dsy, dang = D.from_host(symbols), D.from_host(test_angle_grid(Mtestangles, rt))
    dE, idx1, idx2, ph, out = D((nm, L), ct), D((nm, L), np.int32), D((nm, L), np.int32), D((nm, L), rt), D((nm, L), ct)
    if E.nbytes < _lib.PINNED_MIN_BYTES:
        dE.set(E)
        bps_twostage_recover_dev(dE, Mtestangles, B, dsy, N, idx1, idx2, ph, out, angles=dang)
        return out.to_host(), ph.to_host()
    return _row_pipeline(E, dE, (out, ph), lambda r: bps_twostage_recover_dev(_row2d(dE, r), Mtestangles, B, dsy, N, _row2d(idx1, r), _row2d(idx2, r),
                                                                             _row2d(ph, r), _row2d(out, r), angles=dang))


def _row_pipeline(E, dE, results, search):
    """Rows (modes) are independent: row r + 1 of the host array ``E`` goes up into ``dE`` (stream 1) while ``search(r)`` enqueues the search of
    row r (stream 0) and row r - 1 of every DeviceArray in ``results`` comes back (stream 2, into pooled pinned memory) - PCIe carries both
    directions at once; all searches on ONE stream (they share the library's scratch buffers).  Returns the host arrays, complete."""
    nm = E.shape[0]
    back = [_lib.pinned_empty(d.shape, d.dtype) for d in results]
    ev_up, ev_done = [_lib.Event() for _ in range(nm)], [_lib.Event() for _ in range(nm)]
    for r in range(nm):
        with _lib.on_stream(1):
            _lib.call("qh_memcpy_h2d_async", dE.row(r).ptr, E[r].ctypes.data, E[r].nbytes)
            ev_up[r].record()
        _lib.call("qh_stream_wait_event", ev_up[r].ptr)
        search(r)
        ev_done[r].record()
        with _lib.on_stream(2):
            _lib.call("qh_stream_wait_event", ev_done[r].ptr)
            for h, d in zip(back, results):
                _lib.call("qh_memcpy_d2h_async", h[r].ctypes.data, d.row(r).ptr, h[r].nbytes)
    _lib.sync()
    return tuple(back)


def _row2d(a, r):
    """Row ``r`` of a 2-d DeviceArray as a (1, L) view."""
    v = a.row(r)
    v.shape = (1,) + tuple(v.shape)
    return v


def comp_freq_offset(E, freq_offset, os=1):
    """``E[k, n] * exp(-2j pi (n + 1) freq_offset[k] / os)`` for every row (qampy/core/phaserecovery.py:435-473) on the device."""
    suf, rt, ct = _lib.suffix(E.dtype)
    E = np.ascontiguousarray(E)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("comp_freq_offset works on a 2-d complex array")
    fo = np.ascontiguousarray(np.broadcast_to(np.asarray(freq_offset, dtype=np.float64).reshape(-1), (E.shape[0],)) if np.size(freq_offset) == 1
                              else np.asarray(freq_offset, dtype=np.float64).reshape(-1))
    if fo.size != E.shape[0]:
        raise ValueError("one frequency offset per mode (or one for all)")
    out = np.empty_like(E)
    _lib.call("qh_comp_freq_offset_" + _lib.cname(suf), _lib.ptr(E), E.shape[0], E.shape[1], _lib.ptr(fo), int(os), _lib.ptr(out))
    return out


def comp_freq_offset_dev(E, fo, os, out):
    """:func:`comp_freq_offset` with everything in HBM: E, out (nmodes, L) complex DeviceArrays - the same buffer for removal in place -
    and ``fo`` the (nmodes,) float64 DeviceArray :func:`find_freq_offset_dev` wrote.  Enqueued on the current library stream."""
    suf, rt, ct = _lib.suffix(E.dtype)
    if len(E.shape) != 2 or np.dtype(E.dtype) != ct:
        raise TypeError("comp_freq_offset_dev works on a 2-d complex array")
    if tuple(out.shape) != tuple(E.shape) or np.dtype(out.dtype) != np.dtype(E.dtype):
        raise ValueError("out must have E's shape and dtype")
    if np.dtype(fo.dtype) != np.float64 or int(np.prod(fo.shape)) != E.shape[0]:
        raise ValueError("fo: one float64 offset per mode")
    _lib.call("qh_comp_freq_offset_" + _lib.cname(suf) + "_dev", E.ptr, E.shape[0], E.shape[1], fo.ptr, int(os), out.ptr)


# ------------------------------------------------------------------------------------------------ blind frequency-offset estimate
FOE_NMIN, FOE_NMAX = 2 ** 8, 2 ** 20          # transform sizes of csrc/foe.hip


def foe_plan(L, fft_size, blocks=1):
    """``(N, B)`` of a frequency-offset estimate over rows of ``L`` samples, checked on the host: ``fft_size`` rounded up to a power of two
    as the reference rounds it (qampy/core/phaserecovery.py:414-415), ``blocks`` an integer or ``"all"`` (``max(1, L // N)``).  ValueError for
    a size outside ``2**8 .. 2**20``, for ``blocks < 1`` and for more than one block with ``blocks * N > L``."""
    if not fft_size >= 1:
        raise ValueError("fft_size must be positive")
    N = 2 ** int(np.ceil(np.log2(fft_size)))
    if not FOE_NMIN <= N <= FOE_NMAX:
        raise ValueError("fft_size %d (rounded up to a power of two) is outside %d .. %d" % (N, FOE_NMIN, FOE_NMAX))
    L = int(L)
    if L < 1:
        raise ValueError("an empty signal has no frequency offset")
    if isinstance(blocks, str):
        if blocks != "all":
            raise ValueError("blocks is an integer or 'all'")
        return N, max(1, L // N)
    B = int(blocks)
    if B != blocks or B < 1:
        raise ValueError("blocks is a positive integer or 'all'")
    if B > 1 and B * N > L:
        raise ValueError("%d blocks of %d samples do not fit a signal of %d" % (B, N, L))
    return N, B


def _foe_os(os):
    if int(os) != os or os < 1:
        raise ValueError("the device estimator takes a whole number of samples per symbol")
    return int(os)


def find_freq_offset_dev(E, os, fft_size, blocks, average_over_modes, fo, stats=None, spectrum=None):
    """
    Blind frequency-offset estimate of every row of the (nmodes, L) complex DeviceArray ``E`` in HBM (csrc/foe.hip): the peak of
    ``sum_b |FFT_N(E[row, b N:(b + 1) N] ** 4)|**2`` over ``blocks`` blocks of ``N = fft_size`` samples (see :func:`foe_plan`), divided by 4,
    on numpy's ``fftfreq(N, 1 / os)`` grid, written to the (nmodes,) float64 DeviceArray ``fo`` - the mean over the rows in every entry with
    ``average_over_modes``.  Optional DeviceArrays: ``stats`` (nmodes, 3) float64 - bin, peak power, total power - and ``spectrum``
    (nmodes, N) in the signal's real type.  Nothing is read back; enqueued on the current library stream.
    """
    suf, rt, ct = _lib.suffix(E.dtype)
    if len(E.shape) != 2 or np.dtype(E.dtype) != ct:
        raise TypeError("find_freq_offset_dev works on a 2-d complex array")
    nm, L = E.shape
    N, B = foe_plan(L, fft_size, blocks)
    os = _foe_os(os)
    if np.dtype(fo.dtype) != np.float64 or int(np.prod(fo.shape)) != nm:
        raise ValueError("fo: one float64 offset per mode")
    if stats is not None and (np.dtype(stats.dtype) != np.float64 or tuple(stats.shape) != (nm, 3)):
        raise ValueError("stats must be (nmodes, 3) float64")
    if spectrum is not None and (np.dtype(spectrum.dtype) != rt or tuple(spectrum.shape) != (nm, N)):
        raise ValueError("spectrum must be (nmodes, %d) %s" % (N, np.dtype(rt).name))
    _lib.call("qh_find_freq_offset_" + _lib.cname(suf) + "_dev", E.ptr, nm, L, os, N, B, int(bool(average_over_modes)), fo.ptr,
              stats.ptr if stats is not None else None, spectrum.ptr if spectrum is not None else None)


def find_freq_offset(E, os=1, fft_size=2 ** 16, blocks=1, average_over_modes=True):
    """:func:`find_freq_offset_dev` for a host array: ``E (nmodes, L)`` up, the (nmodes,) float64 offsets back."""
    E = np.asarray(E)
    if E.ndim != 2 or not np.iscomplexobj(E):
        raise TypeError("find_freq_offset works on a 2-d complex array")
    suf, rt, ct = _lib.suffix(E.dtype)
    N, B = foe_plan(E.shape[1], fft_size, blocks)
    os = _foe_os(os)
    E = np.ascontiguousarray(E)
    fo = np.zeros(E.shape[0], dtype=np.float64)
    _lib.call("qh_find_freq_offset_" + _lib.cname(suf), _lib.ptr(E), E.shape[0], E.shape[1], os, N, B, int(bool(average_over_modes)),
              _lib.ptr(fo), None, None)
    return fo


# ------------------------------------------------------------------------------------------------ feed-forward carrier recovery
VV_NMAX, VV_MMAX, P16_NBLOCK_MAX = 1024, 64, 4096          # limits of csrc/cpr.hip


def _cpr_check(name, E, trace, Eout, trace_len):
    suf, rt, ct = _lib.suffix(E.dtype)
    if len(E.shape) != 2 or np.dtype(E.dtype) != ct:
        raise ValueError("%s works on a 2-d complex array" % name)
    if tuple(Eout.shape) != tuple(E.shape) or np.dtype(Eout.dtype) != np.dtype(E.dtype):
        raise ValueError("Eout must have E's shape and dtype")
    if tuple(trace.shape) != (E.shape[0], trace_len) or np.dtype(trace.dtype) != rt:
        raise ValueError("trace must be (%d, %d) %s" % (E.shape[0], trace_len, np.dtype(rt).name))
    return _lib.cname(suf)


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
    big = E.nbytes >= _lib.PINNED_MIN_BYTES                       # results through the pinned pool: one DMA at the link rate each
    out = _lib.pinned_empty(E.shape, E.dtype) if big else np.empty_like(E)
    trace = _lib.pinned_empty(E.shape, E.dtype) if big else np.empty_like(E)
    _lib.call("qh_pilot_phase_trace_" + _lib.cname(suf), _lib.ptr(E), E.shape[0], E.shape[1], _lib.ptr(knots), _lib.ptr(kph), knots.size,
              _lib.ptr(out), _lib.ptr(trace))
    return out, trace


# ------------------------------------------------------------------------------------------------ signal-quality metrics
# The last exports of pythran_dsp (qampy/core/pythran_dsp.py:87-131, :244-313) that qampy/core/signal_quality.py:27-29 binds;
# kernels in qampy_amd/csrc/metrics.hip.

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


# ------------------------------------------------------------------------------------------------ channel impairments on a resident field
# The channel part of qampy/core/impairments.py (:29-328) on DeviceArrays; kernels in qampy_amd/csrc/impair.hip.
IMPAIR_TILE = 1024                 # samples of one mode per workgroup of the point-wise pass (csrc/impair.hip IMP_TILE)
PMD_NMIN, PMD_N = 256, 8192        # whole-row transform sizes; block size of the overlap-save form


def _impair_field(E, what):
    suf, rt, ct = _lib.suffix(E.dtype)
    if len(E.shape) != 2 or np.dtype(E.dtype) != ct:
        raise TypeError("%s works on a 2-d complex64 or complex128 DeviceArray" % what)
    return "c64" if suf == "32" else "c128"


def _same_as(E, out, what):
    if tuple(out.shape) != tuple(E.shape) or np.dtype(out.dtype) != np.dtype(E.dtype):
        raise ValueError("%s: out must have E's shape and dtype" % what)


def _seed64(seed):
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def snr_noise_factor(snr_db, os):
    """``sigma / sqrt(p)`` of the reference's ``change_snr`` (qampy/core/impairments.py:230-233): ``10**(-snr/20) sqrt(fs/fb)``."""
    if not os > 0:
        raise ValueError("the oversampling fs / fb must be positive")
    return 10 ** (-float(snr_db) / 20) * np.sqrt(float(os))


def snr_power_factor(snr_db, os):
    """Factor by which ``change_snr`` at ``snr_db`` and ``os = fs / fb`` samples per symbol raises the mean power of a noiseless signal:
    ``1 + os 10**(-snr/10)``."""
    return 1.0 + float(os) * 10 ** (-float(snr_db) / 10)


def impair_pointwise_dev(E, out, *, sigma=None, snr=None, phase=None, freq=None, seed=0, trace=None):
    """
    The fused point-wise impairment pass on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one::

        out[m, n] = E[m, n] exp(j (phi[m, n] + 2 pi n fo / fs)) + sigma w[m, n]

    ``sigma``: noise strength as ``add_awgn`` takes it; or ``snr=(snr_db, os)``: ``sigma = sqrt(p) 10**(-snr_db/20) sqrt(os)`` with
    ``p = mean |E|**2`` over all modes together, reduced on the device (``change_snr``); neither: no noise (``sigma=0`` too: the field comes
    back bit for bit).  ``phase=(df, fs)``: a Wiener phase per mode with increments of variance ``2 pi df / fs`` (``apply_phase_noise``);
    ``trace``, an (nmodes, L) float64 DeviceArray, receives it.  ``freq=(fo, fs)``: carrier offset (``add_carrier_offset``); ``2 pi n fo / fs``
    is formed in double and reduced modulo one turn for both precisions - the reference's complex64 path builds ``np.arange`` in float32 and
    loses the sample index above 2**24, which is not reproduced.

    The noise is counter-based (Philox4x32-10 keyed by ``seed``): a draw depends on (seed, mode, n) only, noise and phase noise of one
    seed are independent, and a repeated call is bit-identical.  At most three launches on the current library stream, nothing read back.
    """
    c = _impair_field(E, "impair_pointwise_dev")
    _same_as(E, out, "impair_pointwise_dev")
    if sigma is not None and snr is not None:
        raise ValueError("give sigma or snr, not both")
    mode, noise = 0, 0.0
    if sigma is not None:
        mode, noise = 1, float(sigma)
    elif snr is not None:
        mode, noise = 2, snr_noise_factor(*snr)
    if mode and not (np.isfinite(noise) and noise >= 0):
        raise ValueError("the noise strength must be finite and not negative")
    var = 0.0
    if phase is not None:
        df, fs = phase
        var = 2 * np.pi * float(df) / float(fs)
        if not (np.isfinite(var) and var >= 0):
            raise ValueError("the linewidth must be finite and not negative")
    ft = 0.0
    if freq is not None:
        fo, fs = freq
        ft = float(fo) / float(fs)
        if not np.isfinite(ft):
            raise ValueError("the carrier offset must be finite")
    if trace is not None:
        if phase is None:
            raise ValueError("a trace needs phase=(df, fs)")
        if np.dtype(trace.dtype) != np.float64 or tuple(trace.shape) != tuple(E.shape):
            raise ValueError("trace must be an (nmodes, L) float64 DeviceArray")
    _lib.call("qh_impair_pointwise_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], mode, noise, int(phase is not None), var, int(freq is not None), ft,
              _seed64(seed), trace.ptr if trace is not None else None, out.ptr)
    return out


def phase_noise_dev(out, df, fs, seed, cumulative=True, draws=np.complex128):
    """The Wiener phase of :func:`impair_pointwise_dev` on its own, into the (nmodes, L) float64 DeviceArray ``out`` (``phase_noise`` of the
    reference); ``cumulative=False`` writes the raw increments instead of their running sum.  ``draws``: the precision of the pass whose
    draws are wanted - complex64 draws in float with the fast intrinsics, complex128 in double; the sums are double in both."""
    if len(out.shape) != 2 or np.dtype(out.dtype) != np.float64:
        raise TypeError("phase_noise_dev writes an (nmodes, L) float64 DeviceArray")
    c = {np.dtype(np.complex64): "c64", np.dtype(np.complex128): "c128"}.get(np.dtype(draws))
    if c is None:
        raise TypeError("draws is complex64 or complex128")
    var = 2 * np.pi * float(df) / float(fs)
    if not (np.isfinite(var) and var >= 0):
        raise ValueError("the linewidth must be finite and not negative")
    _lib.call("qh_phase_noise_%s_dev" % c, out.ptr, out.shape[0], out.shape[1], var, _seed64(seed), int(bool(cumulative)))
    return out


def _two_modes(E, what):
    if E.shape[0] != 2:
        raise ValueError("%s needs two modes" % what)


def rotate_field_dev(E, out, theta):
    """``[[cos, -sin], [sin, cos]] @ E`` for a (2, L) field (``rotate_field``); ``out`` may be ``E``."""
    c = _impair_field(E, "rotate_field_dev")
    _same_as(E, out, "rotate_field_dev")
    _two_modes(E, "rotate_field_dev")
    _lib.call("qh_rotate_field_%s_dev" % c, E.ptr, 2, E.shape[1], float(theta), out.ptr)
    return out


def apply_pmd_dev(E, out, theta, t_dgd, fs):
    """
    First-order PMD on a (2, L) field in HBM (``apply_PMD_to_field``): ``R(-theta) diag(H, conj H) R(theta)`` with ``H = exp(-j omega t_dgd / 2)``,
    into ``out`` (not ``E``).  Two launches on the current library stream.

    A row length that is a power of two from 256 to 8192 is one exact circular transform per row - the reference's operation.  Every other
    length runs as overlap-save blocks of 8192 samples (4096 kept, 2048 of halo either side, the field taken modulo L), which is NOT the
    reference's operation: a delay of a fraction of a sample has a 1/n tail that the block cuts off and wraps.  On 16-QAM at 2 samples per
    symbol, roll-off 0.1, 40 GS/s, theta = pi/5.6, against the full-length transform: 30 ps (+-0.6 sample) deviates by 2.2e-4 of the rms at
    most (rms 1.1e-4), a delay of whole samples (200 ps) by 4e-15; at one sample per symbol 30 ps deviates by 1.3e-2.  For an odd row
    length the reference's own frequency grid is off numpy's fftfreq grid by half a bin; the blocks use the fftfreq grid.
    """
    c = _impair_field(E, "apply_pmd_dev")
    _same_as(E, out, "apply_pmd_dev")
    _two_modes(E, "apply_pmd_dev")
    if out.ptr == E.ptr:
        raise ValueError("apply_pmd_dev is out of place: out must not be E")
    d = float(t_dgd) * float(fs)
    if not (np.isfinite(d) and np.isfinite(float(theta))):
        raise ValueError("theta and the delay must be finite")
    _lib.call("qh_apply_pmd_%s_dev" % c, E.ptr, 2, E.shape[1], float(theta), d, out.ptr)
    return out


def _delays(delay, nmodes):
    d = np.asarray(delay)
    if d.ndim != 1 or d.shape[0] != nmodes:
        raise ValueError("Delay array must have the same length as number of modes of signal")
    if not np.all(np.equal(np.mod(d, 1), 0)):
        raise ValueError("the modal delays are whole numbers of samples")
    return np.ascontiguousarray(d, dtype=np.int64)


def modal_delay_dev(E, out, delay):
    """Row m of ``E`` rolled by ``delay[m]`` samples into ``out`` (``add_modal_delay``: ``np.roll`` per mode); ``out`` is not ``E``."""
    c = _impair_field(E, "modal_delay_dev")
    _same_as(E, out, "modal_delay_dev")
    if out.ptr == E.ptr:
        raise ValueError("modal_delay_dev is out of place: out must not be E")
    d = _delays(delay, E.shape[0])
    _lib.call("qh_modal_delay_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], _lib.ptr(d), out.ptr)
    return out


def simulate_transmission_dev(E, out, fb, fs, snr=None, freq_off=None, lwdth=None, dgd=None, theta=np.pi / 3.731, modal_delay=None, seed=0, tmp=None):
    """
    ``simulate_transmission`` of the reference on (nmodes, L) DeviceArrays, in its order: phase noise, carrier offset and SNR - one fused
    pass (:func:`impair_pointwise_dev`) - then the modal delay, then PMD (:func:`apply_pmd_dev`).  ``out`` may be ``E``.  The two
    out-of-place stages alternate between ``out`` and ``tmp``, a DeviceArray like ``E`` (allocated here when one is needed and none is
    given), so that the last one writes ``out``.  Returns ``out``.
    """
    _impair_field(E, "simulate_transmission_dev")
    _same_as(E, out, "simulate_transmission_dev")
    nfilt = int(modal_delay is not None) + int(dgd is not None)
    if dgd is not None:
        _two_modes(E, "PMD")
    if nfilt and tmp is None:
        tmp = _lib.DeviceArray(E.shape, E.dtype)
    # the out-of-place stages alternate between tmp and out so that the last one writes out
    first = out if nfilt != 1 else tmp
    impair_pointwise_dev(E, first, snr=None if snr is None else (snr, fs / fb), phase=None if lwdth is None else (lwdth, fs),
                         freq=None if freq_off is None else (freq_off, fs), seed=seed)
    cur = first
    if modal_delay is not None:
        nxt = tmp if cur is out else out
        modal_delay_dev(cur, nxt, modal_delay)
        cur = nxt
    if dgd is not None:
        nxt = tmp if cur is out else out
        apply_pmd_dev(cur, nxt, theta, dgd, fs)
        cur = nxt
    assert cur is out
    return out


# ------------------------------------------------------------------------------------------------ transmitter response on a resident field
# The transmitter part of qampy/core/impairments.py (:370-671) and filter_signal (qampy/core/filter.py:86-147) on DeviceArrays; kernels in
# qampy_amd/csrc/txresp.hip.
SOS_CHUNK, SOS_TILE = 128, 8192     # samples per lane and per workgroup of the sections filter (csrc/txresp.hip SOS_C, SOS_T; qh_sos_geometry)
SOS_MAXSEC = 4
TX_MAXMODES = 1024


def _tx_modes(E, what):
    if not 1 <= E.shape[0] <= TX_MAXMODES:
        raise ValueError("%s works on 1 to %d modes" % (what, TX_MAXMODES))


def row_extrema_dev(E, ext=None):
    """``(max |re|, max |im|)`` of every row of the (nmodes, L) complex DeviceArray ``E`` into the (nmodes, 2) float64 DeviceArray ``ext``
    (made when None); two launches, nothing read back, bit-reproducible.  The later stages read their scale factors from it on the device."""
    c = _impair_field(E, "row_extrema_dev")
    _tx_modes(E, "row_extrema_dev")
    if E.shape[1] < 1:
        raise ValueError("row_extrema_dev needs at least one sample per row")
    if ext is None:
        ext = _lib.DeviceArray((E.shape[0], 2), np.float64)
    elif tuple(ext.shape) != (E.shape[0], 2) or np.dtype(ext.dtype) != np.float64:
        raise ValueError("ext must be an (nmodes, 2) float64 DeviceArray")
    _lib.call("qh_row_extrema_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr)
    return ext


def _dac_stages(clip_rat, quant_bits, enob):
    """(mask, clip_rat, bits, enob) of the DAC's point-wise stages, checked; a stage is off where the reference's ``np.isclose`` says so."""
    clip_rat, enob = float(clip_rat), float(enob)
    if not (np.isfinite(clip_rat) and clip_rat > 0):
        raise ValueError("clip_rat must be positive")
    if not (np.isfinite(enob) and enob >= 0):
        raise ValueError("enob must not be negative")
    qb = float(quant_bits)
    bits = 0
    if not np.isclose(qb, 0):
        if not (np.isfinite(qb) and qb == int(qb) and 1 <= qb <= 16):
            raise ValueError("quant_bits must be 0 or a whole number from 1 to 16")
        bits = int(qb)
    stages = (0 if np.isclose(clip_rat, 1) else 1) | (2 if bits else 0) | (0 if np.isclose(enob, 0) else 4)
    return stages, clip_rat, bits, enob


def dac_pointwise_dev(E, out, clip_rat=1, quant_bits=0, enob=0, seed=0, ext=None):
    """
    The point-wise part of ``sim_DAC_response`` on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one: clip,
    then quantise, then ENOB noise, each optional, in the reference's order and with its conventions.

    Clip (unless ``np.isclose(clip_rat, 1)``): every row scaled to ``+-1 / clip_rat`` by its own maximum, re and im clamped to ``+-1``.
    Quantise (unless ``np.isclose(quant_bits, 0)``; ``quantize_signal_New``): every row scaled to ``+-1`` by its own maximum, the level index
    the number of thresholds ``-1 + k d`` (``d = 2 / 2**bits``) that are <= the value - a value on a threshold goes up -, the output level
    ``-1 + d / 2 + index d`` times the maximum over all rows of the quantiser's input.  Noise (unless ``np.isclose(enob, 0)``;
    ``apply_enob_as_awgn``): ``sigma = sqrt(2 (x_max / 2**(enob - 1))**2 / 12)`` with ``x_max`` over all rows of the stage's input, added
    exactly as ``impair_pointwise_dev(sigma=sigma, seed=seed)`` adds it.

    ``ext``: the row extrema of ``E`` (:func:`row_extrema_dev`); None: formed here.  One extrema pass serves all three stages - after
    clipping every row's maximum is ``min(1 / clip_rat, 1)``, after quantising ``(1 - d / 2) max_swing``.  Launches: 1, plus 2 for the
    extrema when ``ext`` is None; with nothing to do none (``out is E``) or one copy, and the field comes back bit for bit.
    """
    c = _impair_field(E, "dac_pointwise_dev")
    _same_as(E, out, "dac_pointwise_dev")
    _tx_modes(E, "dac_pointwise_dev")
    stages, clip_rat, bits, enob = _dac_stages(clip_rat, quant_bits, enob)
    if ext is not None and (tuple(ext.shape) != (E.shape[0], 2) or np.dtype(ext.dtype) != np.float64):
        raise ValueError("ext must be an (nmodes, 2) float64 DeviceArray")
    _lib.call("qh_dac_pointwise_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr if ext is not None else None, stages, clip_rat, bits, enob,
              _seed64(seed), out.ptr)
    return out


def enob_sigma(x_max, enob):
    """The noise strength of ``apply_enob_as_awgn``: ``sqrt(2 (x_max / 2**(enob - 1))**2 / 12)``."""
    return np.sqrt(2 * (float(x_max) / 2 ** (float(enob) - 1)) ** 2 / 12)


def _check_sos(sos):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= SOS_MAXSEC:
        raise ValueError("sos must be (n_sections, 6) with 1 to %d sections" % SOS_MAXSEC)
    if not np.all(np.isfinite(sos)):
        raise ValueError("the section coefficients must be finite")
    if not np.all(sos[:, 3] == 1.0):
        raise ValueError("every section must be normalised to a0 = 1")
    return sos


def sos_transition(sos, C):
    """The (2 nsec, 2 nsec) matrix that maps the state of the cascade ``sos`` - (z0, z1) of section 0, then of section 1, ... as
    ``scipy.signal.sosfilt`` keeps them - over ``C`` samples of zero input: ``M**C`` with ``M`` the map over one sample.  The power is
    formed in ``np.longdouble`` and rounded to float64 once: for a narrow low-pass the entries reach 1e9 and cancel in every product, and a
    power formed in float64 is off by 1e-9 of its largest entry - 3e-12 of the input's rms in the filtered field instead of 5e-14."""
    sos = _check_sos(sos)
    C = int(C)
    if C < 0:
        raise ValueError("C must not be negative")
    n = 2 * sos.shape[0]
    M = np.zeros((n, n), np.longdouble)
    for j in range(n):
        z = np.zeros(n, np.longdouble)
        z[j] = 1
        x = np.longdouble(0)
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos.astype(np.longdouble)):
            y = b0 * x + z[2 * s]
            z[2 * s] = b1 * x - a1 * y + z[2 * s + 1]
            z[2 * s + 1] = b2 * x - a2 * y
            x = y
        M[:, j] = z
    P = np.eye(n, dtype=np.longdouble)
    while C:
        if C & 1:
            P = P @ M
        M = M @ M
        C >>= 1
    return P.astype(np.float64)


_TRANSITIONS = {}


def _chunk_transition(key, nsec):
    """``sos_transition(sos, SOS_CHUNK)`` of the sections whose bytes are ``key``, kept for the next call: a sweep filters with the same
    sections again and again, and the extended-precision power costs more host time than the filter takes on the device."""
    P = _TRANSITIONS.get(key)
    if P is None:
        if len(_TRANSITIONS) >= 64:
            _TRANSITIONS.clear()
        P = _TRANSITIONS[key] = np.ascontiguousarray(sos_transition(np.frombuffer(key, np.float64).reshape(nsec, 6), SOS_CHUNK))
    return P


def sosfilt_dev(E, out, sos):
    """
    ``scipy.signal.sosfilt(sos, E, axis=-1)`` on (nmodes, L) complex DeviceArrays: zero initial state, every row on its own, real
    coefficients (re and im are filtered alike), up to 4 sections; ``out`` may be ``E``.  Coefficients and state are double in both
    precisions; only the samples are complex64 in the complex64 form.

    Exact and parallel in time: a lane filters ``SOS_CHUNK`` consecutive samples from a zero state, the chunks' start states follow from
    ``s[k + 1] = P s[k] + f[k]`` with ``P = sos_transition(sos, SOS_CHUNK)`` by a log-step scan inside a workgroup (``SOS_TILE`` samples) and a
    second one across workgroups, and every lane runs its chunk again from its true start state.  Three launches, one when a row fits a tile.
    """
    c = _impair_field(E, "sosfilt_dev")
    _same_as(E, out, "sosfilt_dev")
    sos = _check_sos(sos)
    P = _chunk_transition(sos.tobytes(), sos.shape[0])
    _lib.call("qh_sosfilt_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], _lib.ptr(sos), sos.shape[0], _lib.ptr(P), out.ptr)
    return out


_DESIGNS = {}            # sections by (fs, cutoff, ftype, order): scipy's design takes longer than the filter on the device


def design_lowpass_sos(fs, cutoff, ftype="bessel", order=2):
    """The sections of the reference's digital low-pass (``filter_signal``, qampy/core/filter.py:129-135): ``scipy.signal.bessel(order,
    cutoff, 'low', norm='mag', output='sos', fs=fs)`` or ``scipy.signal.butter(order, cutoff, 'low', output='sos', fs=fs)``, checked."""
    if ftype in ("gauss", "exp"):
        raise NotImplementedError("ftype=%r filters the whole row in the frequency domain, which is not implemented: 'bessel' or 'butter'" % ftype)
    if ftype not in ("bessel", "butter"):
        raise ValueError("ftype is 'bessel' or 'butter'")
    if int(order) != order or not 1 <= int(order) <= 2 * SOS_MAXSEC:
        raise ValueError("order must be a whole number from 1 to %d" % (2 * SOS_MAXSEC))
    fs, cutoff = float(fs), float(cutoff)
    if not (np.isfinite(fs) and np.isfinite(cutoff) and 0 < cutoff < fs / 2):
        raise ValueError("the cutoff must lie between 0 and fs / 2")
    key = (fs, cutoff, ftype, int(order))
    sos = _DESIGNS.get(key)
    if sos is None:
        import scipy.signal as scisig
        if len(_DESIGNS) >= 64:
            _DESIGNS.clear()
        if ftype == "bessel":
            sos = scisig.bessel(int(order), cutoff, "low", norm="mag", output="sos", fs=fs)
        else:
            sos = scisig.butter(int(order), cutoff, "low", output="sos", fs=fs)
        _DESIGNS[key] = sos
    return sos.copy()


def filter_signal_dev(E, out, fs, cutoff, ftype="bessel", order=2):
    """``filter_signal`` of the reference on (nmodes, L) complex DeviceArrays: a digital Bessel (``norm='mag'``) or Butterworth low-pass of
    ``order`` 1 to 8 with the 3 dB ``cutoff``, designed on the host (:func:`design_lowpass_sos`) and run by :func:`sosfilt_dev`; ``out`` may be
    ``E``.  ``ftype`` 'gauss' and 'exp' raise NotImplementedError."""
    _impair_field(E, "filter_signal_dev")
    _same_as(E, out, "filter_signal_dev")
    return sosfilt_dev(E, out, design_lowpass_sos(fs, cutoff, ftype, order))


def _iq(v, name):
    """(I, Q) of a modulator parameter: a real value serves both arms (``np.iscomplex`` of the reference: an imaginary part of 0 is real)."""
    v = complex(v)
    if not (np.isfinite(v.real) and np.isfinite(v.imag)):
        raise ValueError("%s must be finite" % name)
    return (v.real, v.imag) if v.imag != 0 else (v.real, v.real)


def _mod_params(dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1):
    d, g, c = _iq(dcbias, "dcbias"), _iq(gfactr, "gfactr"), _iq(cfactr, "cfactr")
    for name, v in (("dcbias_out", dcbias_out), ("gfactr_out", gfactr_out)):
        if np.iscomplexobj(v) or not np.isfinite(float(v)):
            raise ValueError("%s must be real and finite" % name)
    return np.array([d[0], d[1], g[0], g[1], c[0], c[1], float(dcbias_out), float(gfactr_out)], np.float64)


def modulator_response_dev(E, out, dcbias=1, gfactr=1, cfactr=0, dcbias_out=0.5, gfactr_out=1, tgt_v=None, ext=None):
    """
    ``modulator_response`` of the reference on (nmodes, L) complex DeviceArrays, one point-wise launch; ``out`` may be ``E``.  ``dcbias``,
    ``gfactr`` and ``cfactr`` real (both arms alike) or complex (I, Q).  ``tgt_v``: ``ideal_amplifier_response(E, tgt_v)`` first, in the same
    launch - ``E / max * tgt_v`` with the maximum over all rows read from ``ext`` (:func:`row_extrema_dev`; None: formed here, two more
    launches).  Every angle is formed in double and reduced modulo one turn before the sine and cosine, in both precisions.
    """
    c = _impair_field(E, "modulator_response_dev")
    _same_as(E, out, "modulator_response_dev")
    _tx_modes(E, "modulator_response_dev")
    prm = _mod_params(dcbias, gfactr, cfactr, dcbias_out, gfactr_out)
    if tgt_v is not None and not np.isfinite(float(tgt_v)):
        raise ValueError("tgt_v must be finite")
    if ext is not None and (tuple(ext.shape) != (E.shape[0], 2) or np.dtype(ext.dtype) != np.float64):
        raise ValueError("ext must be an (nmodes, 2) float64 DeviceArray")
    _lib.call("qh_modulator_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], ext.ptr if ext is not None else None, int(tgt_v is not None),
              0.0 if tgt_v is None else float(tgt_v), _lib.ptr(prm), out.ptr)
    return out


def _dac_filter(dac_params):
    """The sections of ``apply_DAC_filter(**dac_params)``, or None without parameters."""
    if not dac_params:
        return None
    prm = dict(dac_params)
    if prm.pop("fn", None) is not None:
        raise NotImplementedError("a measured DAC response (fn=...) multiplies the spectrum of the whole row, which is not implemented")
    prm.pop("ch", None)
    cutoff = prm.pop("cutoff", 18e9)
    if prm:
        raise TypeError("unknown DAC parameters: %s" % ", ".join(sorted(prm)))
    return cutoff


def sim_dac_response_dev(E, out, fs, enob=5, clip_rat=1, quant_bits=0, seed=0, ext=None, **dac_params):
    """``sim_DAC_response`` on (nmodes, L) complex DeviceArrays: :func:`dac_pointwise_dev`, then - if any ``dac_params`` are given - the DAC's
    second-order Bessel low-pass at ``cutoff`` (default 18 GHz; :func:`filter_signal_dev`).  ``out`` may be ``E``."""
    _impair_field(E, "sim_dac_response_dev")
    _same_as(E, out, "sim_dac_response_dev")
    _dac_stages(clip_rat, quant_bits, enob)
    cutoff = _dac_filter(dac_params)
    sos = None if cutoff is None else design_lowpass_sos(fs, cutoff, "bessel", 2)
    dac_pointwise_dev(E, out, clip_rat=clip_rat, quant_bits=quant_bits, enob=enob, seed=seed, ext=ext)
    if sos is not None:
        sosfilt_dev(out, out, sos)
    return out


_DAC_DEFAULT = {"cutoff": 18e9}


def sim_tx_response_check(E, out, fs, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_DAC_DEFAULT, seed=0, **mod_prms):
    """Every check of :func:`sim_tx_response_dev`, without touching the device: TypeError / ValueError / NotImplementedError, else None."""
    _impair_field(E, "sim_tx_response_dev")
    _same_as(E, out, "sim_tx_response_dev")
    _tx_modes(E, "sim_tx_response_dev")
    _dac_stages(clip_rat, quant_bits, enob)
    _mod_params(**mod_prms)
    if not np.isfinite(float(tgt_v)):
        raise ValueError("tgt_v must be finite")
    _seed64(seed)
    cutoff = _dac_filter(dac_params)
    if cutoff is not None:
        design_lowpass_sos(fs, cutoff, "bessel", 2)


def sim_tx_response_dev(E, out, fs, enob=6, tgt_v=1, clip_rat=1, quant_bits=0, dac_params=_DAC_DEFAULT, seed=0, **mod_prms):
    """
    ``sim_tx_response`` on (nmodes, L) complex DeviceArrays, ``out`` the same buffer as ``E`` or another one: the DAC
    (:func:`sim_dac_response_dev`), the ideal amplifier to ``tgt_v`` (in fractions of Vpi) and the IQ modulator
    (:func:`modulator_response_dev`) with ``mod_prms``.  Every argument is checked before the first launch
    (:func:`sim_tx_response_check`).  At most nine launches - extrema (2), DAC point-wise pass (1), filter (3), extrema of the filtered
    field (2), amplifier and modulator (1) - on the current library stream, nothing read back.
    """
    sim_tx_response_check(E, out, fs, enob=enob, tgt_v=tgt_v, clip_rat=clip_rat, quant_bits=quant_bits, dac_params=dac_params, seed=seed, **mod_prms)
    if E.shape[1] == 0:
        return out
    sim_dac_response_dev(E, out, fs, enob=enob, clip_rat=clip_rat, quant_bits=quant_bits, seed=seed, **(dac_params or {}))
    return modulator_response_dev(out, out, tgt_v=tgt_v, **mod_prms)


# ------------------------------------------------------------------------------------------------ whole-row transforms and the analog front end
# csrc/fft.hip and csrc/iq.hip on DeviceArrays: qampy/core/analog_frontend.py and pre_filter / pre_filter_wdm of qampy/core/filter.py.
FFT_POW2_MIN, FFT_POW2_MAX, FFT_ANY_MAX = 2 ** 8, 2 ** 24, 2 ** 23       # limits of csrc/fft.hip
IQ_TILE = 4096                                                           # samples per workgroup of the moments pass (csrc/iq.hip)
FH_BRICK, FH_BAND, FH_TWORAIL, FH_RAMP, FH_REAL, FH_COMPLEX = 1, 2, 3, 4, 5, 6
IQ_ORTHONORMALIZE, IQ_IMBALANCE, IQ_CENTRE = 0, 1, 2


def fft_length_ok(L):
    """Whether csrc/fft.hip transforms rows of ``L`` samples: a power of two from 2**8 to 2**24, or any other length from 2 to 2**23."""
    L = int(L)
    if L < 2:
        return False
    if L & (L - 1) == 0 and L >= FFT_POW2_MIN:
        return L <= FFT_POW2_MAX
    return L <= FFT_ANY_MAX


def fft_plan(L):
    """``(M, N1, N2, bluestein)`` of a row length: the power-of-two transform size, its four-step split (``N1 = 1``: one workgroup per row)
    and whether the row goes through Bluestein's chirp transform."""
    L = int(L)
    if not fft_length_ok(L):
        raise ValueError("a row of %d samples: the whole-row transform takes a power of two from 2**8 to 2**24, or any other length from 2 to 2**23" % L)
    blue = not (L & (L - 1) == 0 and L >= FFT_POW2_MIN)
    lg = 8
    while (1 << lg) < (2 * L - 1 if blue else L):
        lg += 1
    lg1 = lg // 2 if lg > 13 else 0
    return 1 << lg, 1 << lg1, 1 << (lg - lg1), blue


def _fft_field(E, out, what):
    c = _impair_field(E, what)
    _same_as(E, out, what)
    fft_plan(E.shape[1])
    return c


def fft_dev(E, out):
    """``np.fft.fft`` along the last axis of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (same shape and dtype; it may be ``E``),
    csrc/fft.hip.  ``L``: a power of two from 2**8 to 2**24 or any other length from 2 to 2**23; ValueError otherwise, before a launch.
    Nothing is read back; enqueued on the current library stream; a repeated call is bit-identical."""
    c = _fft_field(E, out, "fft_dev")
    _lib.call("qh_fft_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], 0, out.ptr)
    return out


def ifft_dev(E, out):
    """``np.fft.ifft`` along the last axis: see :func:`fft_dev`."""
    c = _fft_field(E, out, "ifft_dev")
    _lib.call("qh_fft_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], 1, out.ptr)
    return out


def _spectral(E, out, what, kind, p0=0.0, p1=0.0, p2=0.0, i0=0, i1=0, H=None):
    c = _fft_field(E, out, what)
    p = [float(v) for v in (p0, p1, p2)]
    if not all(np.isfinite(p)):
        raise ValueError("%s: parameters must be finite" % what)
    _lib.call("qh_spectral_filter_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], kind, p[0], p[1], p[2], int(i0), int(i1), None if H is None else H.ptr, out.ptr)
    return out


def spectral_filter_dev(E, out, H):
    """``ifft(H * fft(E))`` of every row of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (it may be ``E``).  ``H``: an (L,)
    DeviceArray in ``fftfreq`` order, real in the field's real type or complex in the field's dtype."""
    suf, rt, ct = _lib.suffix(E.dtype)
    _impair_field(E, "spectral_filter_dev")
    if tuple(H.shape) != (E.shape[1],):
        raise ValueError("H must hold one value per bin: (%d,)" % E.shape[1])
    if np.dtype(H.dtype) == np.dtype(rt):
        kind = FH_REAL
    elif np.dtype(H.dtype) == np.dtype(ct):
        kind = FH_COMPLEX
    else:
        raise TypeError("H must be %s or %s for a %s field" % (np.dtype(rt).name, np.dtype(ct).name, np.dtype(ct).name))
    return _spectral(E, out, "spectral_filter_dev", kind, H=H)


def pre_filter_bins(L, bw):
    """``(lo, hi)``: the reference's ``h[:, int(L / (bw / 2)):-int(L / (bw / 2))] = 1`` keeps the positions ``lo <= j < hi`` after
    ``fftshift`` (qampy/core/filter.py:44, as written: ``bw`` is no fraction, and an empty slice - ``bw=0.01``, or a count of 0 - keeps
    nothing)."""
    if not (np.isfinite(bw) and bw != 0):
        raise ValueError("bw must be finite and not zero")
    c = L / (bw / 2)
    if not abs(c) < 2.0 ** 62:
        return 0, 0
    c = int(c)
    lo, hi, _ = slice(c, -c).indices(int(L))
    return (lo, hi) if hi > lo else (0, 0)


def pre_filter_dev(E, out, bw):
    """The brick-wall ``pre_filter(signal, bw)`` of qampy/core/filter.py:28-49 on every row of the (nmodes, L) complex DeviceArray ``E``, into
    ``out`` (it may be ``E``): see :func:`pre_filter_bins` for the bins that survive."""
    _impair_field(E, "pre_filter_dev")
    fft_plan(E.shape[1])
    lo, hi = pre_filter_bins(E.shape[1], float(bw))
    return _spectral(E, out, "pre_filter_dev", FH_BRICK, i0=lo, i1=hi)


def pre_filter_wdm_dev(E, out, bw, os, center_freq=0):
    """Band selection on every row: keep the bins where ``abs(fftfreq(L, 1 / os) - center_freq) < bw / 2`` (``pre_filter_wdm`` of
    qampy/core/filter.py:51-84, restated for rows along the last axis)."""
    _impair_field(E, "pre_filter_wdm_dev")
    fft_plan(E.shape[1])
    if not (np.isfinite(os) and os > 0):
        raise ValueError("os must be positive")
    L = E.shape[1]
    val = 1.0 / (L * (1 / os))                                           # numpy's fftfreq: k * (1 / (n d))
    return _spectral(E, out, "pre_filter_wdm_dev", FH_BAND, p0=val, p1=center_freq, p2=bw / 2)


def _skew_step(L, sampling_rate):
    if not (np.isfinite(sampling_rate) and sampling_rate > 0):
        raise ValueError("sampling_rate must be positive")
    return 1.0 / (L * (sampling_rate / 2))                               # fftfreq(L, sampling_rate / 2), the reference's grid as written


def skew_dev(E, out, delay_i, delay_q, sampling_rate):
    """Delay the rails of every row of the (nmodes, L) complex DeviceArray ``E`` separately: ``out = comp_rf_delay(E.real, delay_i,
    sampling_rate) + 1j * comp_rf_delay(E.imag, delay_q, sampling_rate)`` (qampy/core/analog_frontend.py:54-88, its frequency grid
    ``fftfreq(L, sampling_rate / 2)`` as written), one forward and one inverse transform for both rails.  ``out`` may be ``E``."""
    _impair_field(E, "skew_dev")
    fft_plan(E.shape[1])
    return _spectral(E, out, "skew_dev", FH_TWORAIL, p0=_skew_step(E.shape[1], sampling_rate), p1=delay_i, p2=delay_q)


def delay_dev(E, out, delay, sampling_rate):
    """``ifft(exp(-2j pi delay f) * fft(E))`` with ``f = fftfreq(L, sampling_rate / 2)``: the complex output of ``comp_rf_delay`` before its
    real part is taken."""
    _impair_field(E, "delay_dev")
    fft_plan(E.shape[1])
    return _spectral(E, out, "delay_dev", FH_RAMP, p0=_skew_step(E.shape[1], sampling_rate), p1=delay)


def _iq_field(E, what, os=1):
    c = _impair_field(E, what)
    if int(os) != os or int(os) < 1:
        raise ValueError("os must be a positive integer")
    if E.shape[1] < 1:
        raise ValueError("%s needs at least one sample" % what)
    return c


def _iq_buf(buf, shape, name):
    if buf is None:
        return _lib.DeviceArray(shape, np.float64)
    if tuple(buf.shape) != tuple(shape) or np.dtype(buf.dtype) != np.dtype(np.float64):
        raise ValueError("%s must be a %s float64 DeviceArray" % (name, shape))
    return buf


def iq_moments_dev(E, os=1, mom=None):
    """Per row of the (nmodes, L) complex DeviceArray ``E``: sum I, sum Q, sum I**2, sum Q**2, sum I Q over all samples and the same five
    over ``E[:, ::os]``, in double, into ``mom`` (nmodes, 10) float64 (allocated if None; returned).  Two launches, bit-reproducible."""
    c = _iq_field(E, "iq_moments_dev", os)
    mom = _iq_buf(mom, (E.shape[0], 10), "mom")
    _lib.call("qh_iq_moments_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], int(os), mom.ptr)
    return mom


def iq_coeffs_dev(mom, L, os, kind, coef=None):
    """The coefficients ``(a00, a01, a10, a11, b0, b1)`` per row of ``y = A (I, Q)^T + b`` from the moments of :func:`iq_moments_dev`, formed on
    the device: ``kind`` IQ_ORTHONORMALIZE, IQ_IMBALANCE (pooled over the rows) or IQ_CENTRE."""
    if len(mom.shape) != 2 or mom.shape[1] != 10 or np.dtype(mom.dtype) != np.dtype(np.float64):
        raise ValueError("mom must be an (nmodes, 10) float64 DeviceArray")
    if kind not in (IQ_ORTHONORMALIZE, IQ_IMBALANCE, IQ_CENTRE):
        raise ValueError("unknown kind")
    coef = _iq_buf(coef, (mom.shape[0], 6), "coef")
    _lib.call("qh_iq_coeffs_dev", mom.ptr, mom.shape[0], int(L), int(os), kind, coef.ptr)
    return coef


def iq_affine_dev(E, out, coef):
    """``out = A (E.real, E.imag)^T + b`` per row, evaluated in double; ``out`` may be ``E``."""
    c = _iq_field(E, "iq_affine_dev")
    _same_as(E, out, "iq_affine_dev")
    _iq_buf(coef, (E.shape[0], 6), "coef")
    _lib.call("qh_iq_affine_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], coef.ptr, out.ptr)
    return out


def orthonormalize_dev(E, out, os=1, mom=None, coef=None):
    """``orthonormalize_signal(E, os)`` (qampy/core/analog_frontend.py:91-132) of the (nmodes, L) complex DeviceArray ``E`` into ``out`` (it may
    be ``E``): one moments pass, the closed-form map, one affine pass; nothing is read back."""
    _iq_field(E, "orthonormalize_dev", os)
    _same_as(E, out, "orthonormalize_dev")
    mom = iq_moments_dev(E, os, mom)
    coef = iq_coeffs_dev(mom, E.shape[1], os, IQ_ORTHONORMALIZE, coef)
    return iq_affine_dev(E, out, coef)


def comp_iq_imbalance_dev(E, out, mom=None, coef=None):
    """``comp_IQ_inbalance(E)`` (qampy/core/analog_frontend.py:30-52) into ``out``, which must not be ``E``: mean, sum I Q and sum I**2 pooled
    over the whole array as the reference pools them, and ``E`` itself centred in place as the reference centres its argument."""
    _iq_field(E, "comp_iq_imbalance_dev")
    _same_as(E, out, "comp_iq_imbalance_dev")
    if out.ptr == E.ptr:
        raise ValueError("comp_iq_imbalance_dev centres E in place: out must be another buffer")
    mom = iq_moments_dev(E, 1, mom)
    coef = iq_coeffs_dev(mom, E.shape[1], 1, IQ_IMBALANCE, coef)
    iq_affine_dev(E, out, coef)
    iq_affine_dev(E, E, iq_coeffs_dev(mom, E.shape[1], 1, IQ_CENTRE, coef))
    return out


# ---------------------------------------------------------------------------------------------- synchronisation of rx and tx rows
# csrc/sync.hip on DeviceArrays: find_sequence_offset / find_sequence_offset_complex / sync_and_adjust of qampy/core/ber_functions.py:33-160.
XCORR_MAX = 2 ** 24                # longest full correlation, nx + ny - 1 (the largest power-of-two transform of csrc/fft.hip)
PEAK_TILE, PEAK_FIELDS = 4096, 6   # values per workgroup of the peak search's first stage; doubles per row of its result
SYNC_ROW_MAX = 2 ** 31             # longest row of the gather and the label kernels


def _sync_cplx(a, what, name):
    suf, rt, ct = _lib.suffix(a.dtype)
    if np.dtype(a.dtype) != ct:
        raise TypeError("%s: %s must be a complex64 or complex128 DeviceArray" % (what, name))
    return "c64" if suf == "32" else "c128"


def _sync_rows(a, what, name):
    """``(rows, length)`` of a 1-d row or a 2-d stack of rows."""
    if len(a.shape) not in (1, 2) or min(a.shape) < 1:
        raise ValueError("%s: %s must be a non-empty 1-d row or 2-d stack of rows" % (what, name))
    return (1, a.shape[0]) if len(a.shape) == 1 else tuple(a.shape)


def xcorr_dev(x, y, out):
    """Full cross-correlation ``fftconvolve(x, conj(y)[::-1], "full")`` of every row of ``x`` ((nx,) or (rows, nx)) with the row ``y`` (ny,)
    into ``out`` ((nx + ny - 1,) or (rows, nx + ny - 1)), all complex DeviceArrays of one dtype: the peak of ``|out|`` at index ``k`` puts
    ``y`` ``k - (ny - 1)`` samples into ``x`` (qampy/core/ber_functions.py:60-68).  ``nx + ny - 1`` at most 2**24.  Nothing is read back."""
    c = _sync_cplx(x, "xcorr_dev", "x")
    rows, nx = _sync_rows(x, "xcorr_dev", "x")
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
    c = _sync_cplx(cc, "xcorr_peak_dev", "cc")
    rows, length = _sync_rows(cc, "xcorr_peak_dev", "cc")
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
    c = _sync_cplx(src, "cyclic_gather_dev", "src")
    _lib.call("qh_cyclic_gather_%s_dev" % c, src.ptr, src.shape[0], offset, turns % 4, out.shape[0], out.ptr)
    return out


def labels_to_symbols_dev(idx, alphabet, out):
    """``out = alphabet[idx]`` for int32 labels of any shape (0 for a label outside the alphabet); ``out``: ``idx``'s shape, ``alphabet``'s dtype."""
    c = _sync_cplx(alphabet, "labels_to_symbols_dev", "alphabet")
    n, M = int(np.prod(idx.shape)), int(np.prod(alphabet.shape))
    if np.dtype(idx.dtype) != np.int32:
        raise TypeError("labels_to_symbols_dev: idx must be int32")
    if tuple(out.shape) != tuple(idx.shape) or np.dtype(out.dtype) != np.dtype(alphabet.dtype):
        raise ValueError("labels_to_symbols_dev: out must have idx's shape and the alphabet's dtype")
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
    c = _sync_cplx(x, what, "the first row")
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
    if out is not None and (tuple(out.shape) != tuple(fixed.shape) or np.dtype(out.dtype) != np.dtype(moved.dtype)):
        raise ValueError("sync_and_adjust_dev: out must have the length of the row that stays and the rows' dtype")
    offset, turns, peak = find_sequence_offset_complex_dev(fixed, moved)
    out = _lib.DeviceArray(fixed.shape, moved.dtype) if out is None else out
    cyclic_gather_dev(moved, offset, turns, out)
    return ((out, rx) if adjust == "tx" else (tx, out)), peak


# ---------------------------------------------------------------------------------------------- bit source and Gray mapper
# csrc/source.hip on DeviceArrays: qampy.core.prbs, PRBSBits and SignalQAMGrayCoded._modulate / _demodulate (qampy/signals.py:89-137, :678-731).
# Bits are one byte each (uint8 or bool DeviceArrays, 0 / 1); labels are int32, the first bit of a symbol the most significant.
PRBS_ORDERS = (7, 15, 23, 31)
PRBS_KINDS = {"ext": 0, "int": 1}  # external (Fibonacci) / internal (Galois) XOR
PRBS_W = 65536                     # bits per workgroup of prbs_bits_dev (csrc/source.hip SRC_W)
SOURCE_SYMS = 8192                 # symbols per workgroup of prbs_symbols_dev, 32 per thread, whatever the bits per symbol (SRC_SYMS)
PRBS_ROW_MAX = 2 ** 31             # most bits of a row, most symbols of a mapping call
PRBS_START_MAX = 2 ** 62
SOURCE_NB = (2, 10)                # bits per symbol


def prbs_seed(order, seed=None):
    """The seed of a PRBS as an integer in ``[0, 2**order)``: ``None`` is all ones, a bool array is read as the reference's ``bool2bin`` reads
    it (element 0 is bit 0).  Anything outside the range raises ``ValueError`` (in the reference the stray high bits drift into the taps)."""
    if order not in PRBS_ORDERS:
        raise ValueError("Only orders 7, 15, 23, 31 are implemented")
    if seed is None:
        return 2 ** order - 1
    if np.ndim(seed) > 0:
        seed = sum(int(bool(v)) << i for i, v in enumerate(np.asarray(seed).ravel()))
    if int(seed) != seed:
        raise ValueError("the seed must be an integer or an array of bools")
    seed = int(seed)
    if not 0 <= seed < 2 ** order:
        raise ValueError("the seed of a PRBS of order %d must lie in [0, 2**%d), got %d" % (order, order, seed))
    return seed


def _prbs_args(order, seed, kind, start):
    seed = prbs_seed(order, seed)
    if kind not in PRBS_KINDS:
        raise ValueError("kind must be 'ext' (external XOR) or 'int' (internal XOR), not %r" % (kind,))
    if int(start) != start or not 0 <= int(start) <= PRBS_START_MAX:
        raise ValueError("start must be an integer in [0, 2**62]")
    return int(order), PRBS_KINDS[kind], seed, int(start)


def _bit_rows(a, what, name):
    if np.dtype(a.dtype) not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError("%s: %s must be a uint8 or bool DeviceArray" % (what, name))
    return _sync_rows(a, what, name)


def _bits_per_symbol(nb, what):
    if int(nb) != nb or not SOURCE_NB[0] <= nb <= SOURCE_NB[1]:
        raise ValueError("%s: between %d and %d bits per symbol" % ((what,) + SOURCE_NB))
    return int(nb)


def _alphabet_bits(alphabet, what):
    M = int(np.prod(alphabet.shape))
    nb = int(round(np.log2(M))) if M >= 1 else 0
    if 2 ** nb != M:
        raise ValueError("%s: the alphabet must have a power of two of points, got %d" % (what, M))
    return M, _bits_per_symbol(nb, what)


def prbs_bits_dev(out, order, seed=None, kind="ext", start=0, invert=False):
    """Bits ``start .. start + n - 1`` of the PRBS of ``order`` (7, 15, 23, 31) into the 1-d uint8 / bool DeviceArray ``out`` of ``n`` bits:
    ``kind="ext"`` what ``make_prbs_extXOR(order, start + n, seed)[start:]`` holds, ``"int"`` the internal-XOR form.  ``seed``: None (all
    ones), an int in ``[0, 2**order)`` or a bool array (element 0 is bit 0); ``start`` up to 2**62 at no extra cost (every workgroup jumps to
    its first bit); ``invert`` complements the output.  Nothing is read back."""
    order, k, seed, start = _prbs_args(order, seed, kind, start)
    if len(out.shape) != 1:
        raise ValueError("prbs_bits_dev: out must be one row (use DeviceArray.row for a stack)")
    rows, n = _bit_rows(out, "prbs_bits_dev", "out")
    if n > PRBS_ROW_MAX:
        raise ValueError("prbs_bits_dev: at most 2**31 bits per call")
    _lib.call("qh_prbs_bits_dev", order, k, seed, start, int(bool(invert)), n, out.ptr)
    return out


def _map_shapes(bits, labels, nb, what):
    """Number of symbols of ``bits`` (rows of whole symbols) and the check of ``labels`` against it."""
    rows, n = _bit_rows(bits, what, "bits")
    if n % nb:
        raise ValueError("%s: the rows of bits must hold whole symbols of %d bits" % (what, nb))
    shape = tuple(bits.shape[:-1]) + (n // nb,)
    if labels is not None:
        if np.dtype(labels.dtype) != np.int32:
            raise TypeError("%s: labels must be int32" % what)
        if tuple(labels.shape) != shape:
            raise ValueError("%s: labels must be %s" % (what, shape))
    if rows * (n // nb) > PRBS_ROW_MAX:
        raise ValueError("%s: at most 2**31 symbols per call" % what)
    return rows * (n // nb), shape


def bits_to_labels_dev(bits, nb, labels):
    """``labels = bits.reshape(..., -1, nb) @ 2**arange(nb - 1, -1, -1)`` (``_modulate``'s index, MSB first) for a row or a stack of rows of
    whole symbols; ``labels`` int32, one per symbol."""
    nb = _bits_per_symbol(nb, "bits_to_labels_dev")
    if labels is None:
        raise ValueError("bits_to_labels_dev: labels must be given")
    nsym, _ = _map_shapes(bits, labels, nb, "bits_to_labels_dev")
    _lib.call("qh_bits_to_labels_dev", bits.ptr, nsym, nb, labels.ptr)
    return labels


def labels_to_bits_dev(labels, nb, bits):
    """The inverse of :func:`bits_to_labels_dev`: the low ``nb`` bits of every int32 label, most significant first, one byte each."""
    nb = _bits_per_symbol(nb, "labels_to_bits_dev")
    if labels is None:
        raise ValueError("labels_to_bits_dev: labels must be given")
    nsym, _ = _map_shapes(bits, labels, nb, "labels_to_bits_dev")
    _lib.call("qh_labels_to_bits_dev", labels.ptr, nsym, nb, bits.ptr)
    return bits


def modulate_bits_dev(bits, alphabet, symbols, labels=None, nb=None):
    """``symbols = alphabet[label]`` of every ``nb`` bits of ``bits`` (``SignalQAMGrayCoded._modulate`` with ``alphabet`` the coded symbols):
    one launch, ``labels`` written too when given.  ``nb``: ``log2`` of the alphabet's size; given explicitly, the alphabet may be shorter than
    ``2**nb`` and a label outside it gives 0, as in :func:`labels_to_symbols_dev`."""
    c = _sync_cplx(alphabet, "modulate_bits_dev", "alphabet")
    M = int(np.prod(alphabet.shape))
    nb = _alphabet_bits(alphabet, "modulate_bits_dev")[1] if nb is None else _bits_per_symbol(nb, "modulate_bits_dev")
    if M < 1:
        raise ValueError("modulate_bits_dev: at least one alphabet point")
    nsym, shape = _map_shapes(bits, labels, nb, "modulate_bits_dev")
    if tuple(symbols.shape) != shape or np.dtype(symbols.dtype) != np.dtype(alphabet.dtype):
        raise ValueError("modulate_bits_dev: symbols must be %s of the alphabet's dtype" % (shape,))
    _lib.call("qh_modulate_bits_%s_dev" % c, bits.ptr, nsym, nb, alphabet.ptr, M, symbols.ptr, None if labels is None else labels.ptr)
    return symbols


def prbs_symbols_dev(symbols, alphabet, order, seed=None, kind="ext", start=0, labels=None, bits=None):
    """The fused source of one row: PRBS bits ``start .. start + nsym * nb - 1`` (arguments as :func:`prbs_bits_dev`) -> labels -> ``symbols
    = alphabet[label]`` in one launch.  ``symbols``: 1-d, ``nsym`` values of the alphabet's dtype; ``alphabet``: ``2**nb`` points; ``labels``
    (nsym,) int32 and ``bits`` (nsym * nb,) uint8 / bool are written only when given - symbols alone cost no bit traffic."""
    c = _sync_cplx(alphabet, "prbs_symbols_dev", "alphabet")
    M, nb = _alphabet_bits(alphabet, "prbs_symbols_dev")
    order, k, seed, start = _prbs_args(order, seed, kind, start)
    if len(symbols.shape) != 1 or symbols.shape[0] < 1 or np.dtype(symbols.dtype) != np.dtype(alphabet.dtype):
        raise ValueError("prbs_symbols_dev: symbols must be one non-empty row of the alphabet's dtype")
    nsym = symbols.shape[0]
    if nsym * nb > PRBS_ROW_MAX:
        raise ValueError("prbs_symbols_dev: at most 2**31 bits per row")
    if labels is not None and (np.dtype(labels.dtype) != np.int32 or tuple(labels.shape) != (nsym,)):
        raise ValueError("prbs_symbols_dev: labels must be int32 (%d,)" % nsym)
    if bits is not None and (_bit_rows(bits, "prbs_symbols_dev", "bits") != (1, nsym * nb) or len(bits.shape) != 1):
        raise ValueError("prbs_symbols_dev: bits must be (%d,)" % (nsym * nb))
    _lib.call("qh_prbs_symbols_%s_dev" % c, order, k, seed, start, nsym, nb, alphabet.ptr, M, symbols.ptr, None if labels is None else labels.ptr,
              None if bits is None else bits.ptr)
    return symbols


def demodulate_dev(E, alphabet, bits, labels=None):
    """Bits of the decisions of ``E`` (a row or a stack of rows): the nearest alphabet point of every sample (``qh_make_decision_*_dev``), then
    its label's bits, MSB first, into ``bits`` (``E``'s shape with the last axis times ``nb``).  ``labels``: the int32 decisions, kept when
    given (a buffer of ``E``'s shape)."""
    from .equalisation import hip_equalisation as hk
    _sync_cplx(alphabet, "demodulate_dev", "alphabet")
    M, nb = _alphabet_bits(alphabet, "demodulate_dev")
    if np.dtype(E.dtype) != np.dtype(alphabet.dtype):
        raise TypeError("demodulate_dev: E and the alphabet must have one dtype")
    _sync_rows(E, "demodulate_dev", "E")
    if tuple(bits.shape) != tuple(E.shape[:-1]) + (E.shape[-1] * nb,):
        raise ValueError("demodulate_dev: bits must be %s" % (tuple(E.shape[:-1]) + (E.shape[-1] * nb,),))
    if labels is None:
        _map_shapes(bits, None, nb, "demodulate_dev")
        labels = _lib.DeviceArray(E.shape, np.int32)
    else:
        _map_shapes(bits, labels, nb, "demodulate_dev")
    hk.make_decision_dev(E, alphabet, None, None, labels)
    return labels_to_bits_dev(labels, nb, bits)


# ---------------------------------------------------------------------------------------------- pilot frames
# csrc/pilot.hip on DeviceArrays: SignalWithPilots' frame (qampy/signals.py:1494-1545), get_data / extract_pilots (:1753-1804), pilot_based_cpe_new and
# pilot_based_foe (qampy/core/pilotbased_receiver.py:258-327, :32-73) and find_pilot_const_phase (qampy/phaserec.py:194-218).  A frame of ``F`` symbols
# is ``S`` pilots (the sequence) followed by payload with one phase pilot every ``R`` symbols, the first at position ``S`` (``R`` 0 or None: the
# sequence only); the kernels compute this rule, they read no index table.
PILOT_NMAX = 1023                  # longest moving average of csrc/pilot.hip (PILOT_NMAX)
PILOT_ROW_MAX = 2 ** 40            # most symbols of a row of frames


def _pilot_geometry(F, S, R):
    R = 0 if R is None else R
    if int(F) != F or int(S) != S or int(R) != R:
        raise ValueError("frame length, sequence length and insertion ratio are whole numbers")
    F, S, R = int(F), int(S), int(R)
    if F < 1:
        raise ValueError("a frame holds at least one symbol")
    if S < 0:
        raise ValueError("the pilot sequence cannot have a negative length")
    if S > F:
        raise ValueError("a pilot sequence of %d symbols does not fit a frame of %d" % (S, F))
    if R < 0:
        raise ValueError("the pilot insertion ratio cannot be negative")
    if R == 1:
        raise ValueError("an insertion ratio of 1 leaves no payload")
    if R and (F - S) % R:
        raise ValueError("Frame without pilot sequence divided by pilot rate needs to be an integer")
    return F, S, R


def pilot_counts(F, S, R):
    """``(NP, ND)``: pilots and payload symbols of one frame of ``F`` symbols with a sequence of ``S`` pilots and one phase pilot every ``R``
    symbols behind it (``R`` 0 or None: none).  ValueError for ``S < 0``, ``S > F``, ``R == 1`` (no payload) and ``(F - S) % R != 0``."""
    F, S, R = _pilot_geometry(F, S, R)
    NP = S + ((F - S) // R if R else 0)
    return NP, F - NP


def pilot_ordinals(F, S, R):
    """The rule the kernels compute, on the host: ``(is_pilot (F,) bool, ordinal (F,) int64)`` - whether position ``i`` of a frame is a pilot
    and its place among the pilots, respectively among the payload symbols, of the frame."""
    F, S, R = _pilot_geometry(F, S, R)
    i = np.arange(F, dtype=np.int64)
    b = i - S
    if R:
        pil = (i < S) | (b % R == 0)
        ordinal = np.where(i < S, i, np.where(b % R == 0, S + b // R, (b // R) * (R - 1) + b % R - 1))
    else:
        pil = i < S
        ordinal = np.where(pil, i, b)
    return pil, ordinal


def pilot_positions(F, S, R):
    """The inverse maps: ``(positions of the NP pilots, positions of the ND payload symbols)`` inside a frame, by rule."""
    F, S, R = _pilot_geometry(F, S, R)
    NP, ND = pilot_counts(F, S, R)
    k = np.arange(NP, dtype=np.int64)
    pil = np.where(k < S, k, S + (k - S) * R)
    d = np.arange(ND, dtype=np.int64)
    dat = S + (d // (R - 1)) * R + d % (R - 1) + 1 if R else S + d
    return pil, dat


def _pilot_field(a, what, name, rows=None, dtype=None):
    c = _sync_cplx(a, what, name)
    if len(a.shape) != 2 or min(a.shape) < 1:
        raise ValueError("%s: %s must be a non-empty 2-d complex DeviceArray" % (what, name))
    if rows is not None and a.shape[0] != rows:
        raise ValueError("%s: %s must have %d rows" % (what, name, rows))
    if dtype is not None and np.dtype(a.dtype) != np.dtype(dtype):
        raise TypeError("%s: %s must be %s like the field" % (what, name, np.dtype(dtype).name))
    if a.shape[0] > 65535 or a.shape[1] > PILOT_ROW_MAX:
        raise ValueError("%s: %s is too large" % (what, name))
    return c


def _pilot_buf(a, what, name, shape, dtype):
    if a is None or tuple(a.shape) != tuple(shape) or np.dtype(a.dtype) != np.dtype(dtype):
        raise ValueError("%s: %s must be %s %s" % (what, name, tuple(shape), np.dtype(dtype).name))


def pilot_frame_dev(pilots, payload, F, S, R, nframes, frame, pilot_scale=1, repeat_data=True, labels=None, idx_frame=None):
    """
    Assemble ``frame (nmodes, nframes * F)`` in one launch from ``pilots (nmodes, NP)``, multiplied by ``pilot_scale``, and ``payload``:
    ``(nmodes, ND)`` repeated in every frame (``repeat_data``, the reference's default) or ``(nmodes, nframes * ND)``, ``ND`` symbols per frame.
    With ``labels`` (int32, the payload's shape) and ``idx_frame (nmodes, nframes * F)`` int32 the labels are laid out like the frame in the same
    launch, -1 at the pilots.  All DeviceArrays of one complex dtype; nothing is read back.
    """
    what = "pilot_frame_dev"
    F, S, R = _pilot_geometry(F, S, R)
    NP, ND = pilot_counts(F, S, R)
    if int(nframes) != nframes or nframes < 1 or nframes * F > PILOT_ROW_MAX:
        raise ValueError("%s: nframes must be a positive whole number" % what)
    nframes = int(nframes)
    if NP < 1 or ND < 1:
        raise ValueError("%s: a frame needs at least one pilot and one payload symbol" % what)
    c = _pilot_field(frame, what, "frame")
    nm = frame.shape[0]
    _pilot_buf(frame, what, "frame", (nm, nframes * F), frame.dtype)
    _pilot_buf(pilots, what, "pilots", (nm, NP), frame.dtype)
    pay = (nm, ND if repeat_data else nframes * ND)
    _pilot_buf(payload, what, "payload", pay, frame.dtype)
    if (labels is None) != (idx_frame is None):
        raise ValueError("%s: labels and idx_frame come together" % what)
    if labels is not None:
        _pilot_buf(labels, what, "labels", pay, np.int32)
        _pilot_buf(idx_frame, what, "idx_frame", (nm, nframes * F), np.int32)
    scale = float(pilot_scale)
    if not np.isfinite(scale):
        raise ValueError("%s: pilot_scale must be finite" % what)
    _lib.call("qh_pilot_frame_%s_dev" % c, pilots.ptr, payload.ptr, None if labels is None else labels.ptr, nm, F, S, R, nframes, int(not repeat_data), scale,
              frame.ptr, None if idx_frame is None else idx_frame.ptr)
    return frame


def pilot_frame_list(frames, L, F):
    """The int32 table of frame numbers ``pilot_split_dev`` takes: ``None`` is every whole frame of a row of ``L`` symbols.  ValueError for a
    frame that does not lie whole inside ``L``."""
    whole = int(L) // int(F)
    fr = np.arange(whole, dtype=np.int64) if frames is None else np.atleast_1d(np.asarray(frames))
    if fr.ndim != 1 or fr.size < 1 or not np.issubdtype(fr.dtype, np.integer):
        raise ValueError("frames: a non-empty list of whole numbers (a row of %d symbols holds %d whole frames of %d)" % (L, whole, F))
    if fr.min() < 0 or fr.max() >= whole:
        raise ValueError("every requested frame must lie whole inside the %d symbols of the signal (%d frames of %d)" % (L, whole, F))
    return np.ascontiguousarray(fr, dtype=np.int32)


_PILOT_TABLES = threading.local()
PILOT_TABLES_KEPT = 16


def _pilot_table(arr):
    """The device copy of a small host table (frame numbers, pilot positions), kept per host thread by content for the last few tables: a sweep
    that asks for the same frames and positions again uploads nothing - an upload is a blocking copy, and releasing its buffer waits for the
    device."""
    kept = getattr(_PILOT_TABLES, "kept", None)
    if kept is None:
        kept = _PILOT_TABLES.kept = {}
    key = (arr.dtype.str, arr.tobytes())
    if key not in kept:
        while len(kept) >= PILOT_TABLES_KEPT:
            kept.pop(next(iter(kept)))
        kept[key] = _lib.DeviceArray.from_host(arr)
    return kept[key]


def pilot_split_dev(E, F, S, R, frames=None, payload=None, pilots=None):
    """
    Take the frames ``frames`` (a list of frame numbers, in that order; None: every whole frame) of the frame-aligned 1 sample/symbol rows
    ``E (nmodes, L)`` apart in one launch: ``payload (nmodes, nfr * ND)`` and / or ``pilots (nmodes, nfr * NP)``, DeviceArrays of E's dtype.
    The frame numbers are a small host list, uploaded; nothing is read back.  ValueError for a frame that does not lie whole inside ``L``.
    """
    what = "pilot_split_dev"
    F, S, R = _pilot_geometry(F, S, R)
    NP, ND = pilot_counts(F, S, R)
    c = _pilot_field(E, what, "E")
    nm, L = E.shape
    fr = pilot_frame_list(frames, L, F)
    if payload is None and pilots is None:
        raise ValueError("%s: give payload, pilots or both" % what)
    if payload is not None:
        if ND < 1:
            raise ValueError("%s: this frame has no payload" % what)
        _pilot_buf(payload, what, "payload", (nm, fr.size * ND), E.dtype)
    if pilots is not None:
        if NP < 1:
            raise ValueError("%s: this frame has no pilots" % what)
        _pilot_buf(pilots, what, "pilots", (nm, fr.size * NP), E.dtype)
    table = _pilot_table(fr)
    _lib.call("qh_pilot_split_%s_dev" % c, E.ptr, nm, L, F, S, R, table.ptr, fr.size, None if payload is None else payload.ptr, None if pilots is None else pilots.ptr)
    return fr.size


def pilot_used(where, F, nframes, span):
    """Number of used pilots: positions ``where + f * F``, ``f < nframes``, below ``span`` (``where`` strictly increasing inside ``[0, F)``)."""
    where = np.asarray(where)
    full, rem = divmod(int(span), int(F))
    full = min(full, int(nframes))
    return full * where.size + (int(np.count_nonzero(where < rem)) if full < nframes else 0)


def _pilot_plan(what, E, where, F, nframes, sent, span):
    c = _pilot_field(E, what, "E")
    nm, L = E.shape
    _pilot_field(sent, what, "sent", rows=nm, dtype=E.dtype)
    if int(F) != F or F < 1 or int(nframes) != nframes or nframes < 1 or nframes * F > PILOT_ROW_MAX:
        raise ValueError("%s: frame_len and nframes must be positive whole numbers" % what)
    F, nframes = int(F), int(nframes)
    where = np.asarray(where)
    if where.ndim != 1 or where.size < 1 or not np.issubdtype(where.dtype, np.integer):
        raise ValueError("%s: where must be a non-empty 1-d list of positions inside a frame" % what)
    where = np.ascontiguousarray(where, dtype=np.int64)
    if where[0] < 0 or where[-1] >= F or np.any(np.diff(where) <= 0):
        raise ValueError("%s: where must be strictly increasing inside [0, %d)" % (what, F))
    span = min(nframes * F, L) if span is None else span
    if int(span) != span or not 1 <= span <= min(nframes * F, L):
        raise ValueError("%s: span must lie between 1 and min(nframes * frame_len, L) = %d" % (what, min(nframes * F, L)))
    span = int(span)
    n = pilot_used(where, F, nframes, span)
    if n < 1:
        raise ValueError("%s: no pilot lies inside the first %d symbols" % (what, span))
    return c, nm, L, where, F, nframes, span, n


def pilot_phase_dev(E, where, F, nframes, sent, phase, span=None):
    """
    Unwrapped pilot phase ``unwrap(angle(E[:, pos] * conj(sent)))`` of every mode of ``E (nmodes, L)`` into ``phase (nmodes, n)`` float64.  Used
    pilot ``j`` sits at ``where[j % npf] + (j // npf) * F`` - ``where``: the ``npf`` positions inside a frame, a small host array, strictly
    increasing - as far as ``span`` (default ``min(nframes * F, L)``) goes, and is paired with ``sent[:, j % nref]``, ``sent (nmodes, nref)``: the
    reference's ``np.tile(...)[:, :n]``.  ``n = pilot_used(where, F, nframes, span)`` is returned.  Nothing is read back.
    """
    what = "pilot_phase_dev"
    c, nm, L, where, F, nframes, span, n = _pilot_plan(what, E, where, F, nframes, sent, span)
    _pilot_buf(phase, what, "phase", (nm, n), np.float64)
    table = _pilot_table(where)
    _lib.call("qh_pilot_phase_%s_dev" % c, E.ptr, nm, L, table.ptr, where.size, nframes, F, span, n, sent.ptr, sent.shape[1], phase.ptr)
    return n


def _pilot_window(what, N, n):
    if int(N) != N or N % 2 == 0 or not 3 <= N <= PILOT_NMAX:
        raise ValueError("%s: the moving average takes an odd number of pilots between 3 and %d" % (what, PILOT_NMAX))
    if N > n:
        raise ValueError("%s: an average over %d pilots does not fit %d used pilots" % (what, N, n))
    return int(N)


def pilot_knots_dev(phase, N, knot_phase, knot_pos=None, where=None, F=None):
    """Centred moving average over ``N`` (odd, 3 .. 1023) of the ``n`` unwrapped phases ``phase (nmodes, n)`` float64, every output a direct sum:
    ``knot_phase (nmodes, n - N + 1)`` float64 and, when given, ``knot_pos (n - N + 1)`` int64 - the position of the pilot in the middle of every
    window (``where``, ``F`` as in :func:`pilot_phase_dev`; without them pilot ``j`` sits at ``j``)."""
    what = "pilot_knots_dev"
    if len(phase.shape) != 2 or np.dtype(phase.dtype) != np.float64 or min(phase.shape) < 1:
        raise ValueError("%s: phase must be a non-empty (nmodes, n) float64 DeviceArray" % what)
    nm, n = phase.shape
    N = _pilot_window(what, N, n)
    _pilot_buf(knot_phase, what, "knot_phase", (nm, n - N + 1), np.float64)
    table, npf = None, 1
    if knot_pos is not None:
        _pilot_buf(knot_pos, what, "knot_pos", (n - N + 1,), np.int64)
        if where is not None:
            where = np.ascontiguousarray(where, dtype=np.int64)
            if F is None or where.ndim != 1 or where.size < 1 or where[0] < 0 or where[-1] >= F or np.any(np.diff(where) <= 0):
                raise ValueError("%s: where must be strictly increasing inside [0, F)" % what)
            table, npf = _pilot_table(where), where.size
    _lib.call("qh_pilot_knots_dev", phase.ptr, nm, n, N, None if table is None else table.ptr, npf, int(F) if table is not None else 1, knot_phase.ptr,
              None if knot_pos is None else knot_pos.ptr)
    return knot_phase


def pilot_cpe_dev(E, where, F, nframes, sent, N, Eout, trace, span=None):
    """
    Pilot-aided carrier-phase estimate and its removal with everything in HBM (``pilot_based_cpe_new`` behind its selection of pilots): the
    unwrapped pilot phase of :func:`pilot_phase_dev`, its moving average over ``N`` pilots (odd, 3 .. 1023, at most the used pilots), ``np.interp``
    of these knots to every symbol of ``[0, span)`` - constant outside the knots - and ``Eout = E[:, :span] * exp(-1j * trace)``.  ``Eout (nmodes,
    span)`` of E's dtype, ``trace (nmodes, span)`` in its real type.  Returns the number of used pilots; nothing is read back.
    """
    what = "pilot_cpe_dev"
    c, nm, L, where, F, nframes, span, n = _pilot_plan(what, E, where, F, nframes, sent, span)
    N = _pilot_window(what, N, n)
    rt = _lib.suffix(E.dtype)[1]
    _pilot_buf(Eout, what, "Eout", (nm, span), E.dtype)
    _pilot_buf(trace, what, "trace", (nm, span), rt)
    table = _pilot_table(where)
    _lib.call("qh_pilot_cpe_%s_dev" % c, E.ptr, nm, L, table.ptr, where.size, nframes, F, span, n, sent.ptr, sent.shape[1], N, Eout.ptr, trace.ptr)
    return n


def _pilot_pair(what, rec, ref, nmin):
    c = _pilot_field(rec, what, "rec")
    _pilot_field(ref, what, "ref", rows=rec.shape[0], dtype=rec.dtype)
    if ref.shape[1] != rec.shape[1]:
        raise ValueError("%s: received and transmitted pilots must have one length" % what)
    if rec.shape[1] < nmin:
        raise ValueError("%s: at least %d pilots" % (what, nmin))
    return c


def pilot_foe_dev(rec, ref, fit, fo, average=False):
    """Frequency offset from the pilots (``pilot_based_foe``): least-squares line through the unwrapped phase of ``rec`` against ``ref`` (both
    ``(nmodes, n)``, ``n >= 2``) per mode.  ``fit (nmodes, 2)`` float64: ``[slope / (2 pi), intercept]``; ``fo (nmodes,)`` float64, what
    :func:`comp_freq_offset_dev` takes: every mode's own estimate, or - ``average`` - the mean over the modes in every entry."""
    what = "pilot_foe_dev"
    c = _pilot_pair(what, rec, ref, 2)
    nm, n = rec.shape
    _pilot_buf(fit, what, "fit", (nm, 2), np.float64)
    if fo is None or np.dtype(fo.dtype) != np.float64 or int(np.prod(fo.shape)) != nm:
        raise ValueError("%s: fo: one float64 offset per mode" % what)
    _lib.call("qh_pilot_foe_%s_dev" % c, rec.ptr, ref.ptr, nm, n, int(bool(average)), fit.ptr, fo.ptr)
    return fo


def pilot_const_phase_dev(rec, ref, phase):
    """``phase (nmodes,)`` float64: the mean of the unwrapped phase of ``rec`` against ``ref`` per mode (``find_pilot_const_phase``)."""
    what = "pilot_const_phase_dev"
    c = _pilot_pair(what, rec, ref, 1)
    nm, n = rec.shape
    if phase is None or np.dtype(phase.dtype) != np.float64 or int(np.prod(phase.shape)) != nm:
        raise ValueError("%s: phase: one float64 value per mode" % what)
    _lib.call("qh_pilot_const_phase_%s_dev" % c, rec.ptr, ref.ptr, nm, n, phase.ptr)
    return phase


def rotate_rows_dev(E, phi, out):
    """``out[m] = E[m] * exp(-1j * phi[m])`` with ``phi (nmodes,)`` float64 read from HBM (``correct_pilot_const_phase``); ``out`` may be ``E``."""
    what = "rotate_rows_dev"
    c = _pilot_field(E, what, "E")
    _pilot_buf(out, what, "out", E.shape, E.dtype)
    if phi is None or np.dtype(phi.dtype) != np.float64 or int(np.prod(phi.shape)) != E.shape[0]:
        raise ValueError("%s: phi: one float64 phase per mode" % what)
    _lib.call("qh_rotate_rows_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], phi.ptr, out.ptr)
    return out


def _pilot_host(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or not np.iscomplexobj(a):
        raise TypeError("%s must be a 2-d complex array" % name)
    return a


_PILOT_STAGING = threading.local()


def _pilot_staging(key, bufs):
    """Device buffers of the host-array forms, kept per host thread for the shapes of the last call: a frame-by-frame loop over one capture
    then allocates nothing (an allocation that follows a release can stall for tens of milliseconds while the runtime maps memory anew)."""
    if getattr(_PILOT_STAGING, "key", None) != key:
        _PILOT_STAGING.key, _PILOT_STAGING.bufs = None, None                    # (release the old ones first)
        _PILOT_STAGING.bufs = tuple(_lib.DeviceArray(shape, dtype) for shape, dtype in bufs)
        _PILOT_STAGING.key = key
    return _PILOT_STAGING.bufs


def pilot_cpe(E, sent, where, F, nframes, N, span=None):
    """:func:`pilot_cpe_dev` for host arrays: ``E (nmodes, L)`` and ``sent (nmodes, nref)`` up, ``(Eout, trace)`` - both ``(nmodes, span)``, the
    trace in the real type - back."""
    E, sent = _pilot_host(E, "E"), _pilot_host(sent, "sent")
    suf, rt, ct = _lib.suffix(E.dtype)
    E, sent = np.ascontiguousarray(E), np.ascontiguousarray(sent, dtype=ct)
    plan = _pilot_plan("pilot_cpe", E, where, F, nframes, sent, span)          # (the checks, before anything is uploaded)
    _pilot_window("pilot_cpe", N, plan[-1])
    dE, dS, out, trace = _pilot_staging(("cpe", E.shape, sent.shape, plan[-2], ct),
                                        ((E.shape, ct), (sent.shape, ct), ((E.shape[0], plan[-2]), ct), ((E.shape[0], plan[-2]), rt)))
    dE.set(E)
    dS.set(sent)
    pilot_cpe_dev(dE, where, F, nframes, dS, N, out, trace, span=span)
    return out.to_host(pinned=True), trace.to_host(pinned=True)


def pilot_foe(rec, ref, average=False):
    """:func:`pilot_foe_dev` for host arrays ``rec``, ``ref (nmodes, n)``: ``(fit (nmodes, 2), fo (nmodes,))``."""
    rec, ref = _pilot_host(rec, "rec"), _pilot_host(ref, "ref")
    suf, rt, ct = _lib.suffix(rec.dtype)
    rec, ref = np.ascontiguousarray(rec), np.ascontiguousarray(ref, dtype=ct)
    _pilot_pair("pilot_foe", rec, ref, 2)
    D = _lib.DeviceArray
    dr, df = D.from_host(rec), D.from_host(ref)
    fit, fo = D((rec.shape[0], 2), np.float64), D((rec.shape[0],), np.float64)
    pilot_foe_dev(dr, df, fit, fo, average=average)
    return fit.to_host(), fo.to_host()


def pilot_const_phase(rec, ref):
    """:func:`pilot_const_phase_dev` for host arrays: the ``(nmodes,)`` float64 mean phases."""
    rec, ref = _pilot_host(rec, "rec"), _pilot_host(ref, "ref")
    ct = _lib.suffix(rec.dtype)[2]
    rec, ref = np.ascontiguousarray(rec), np.ascontiguousarray(ref, dtype=ct)
    _pilot_pair("pilot_const_phase", rec, ref, 1)
    D = _lib.DeviceArray
    dr, df = D.from_host(rec), D.from_host(ref)
    ph = D((rec.shape[0],), np.float64)
    pilot_const_phase_dev(dr, df, ph)
    return ph.to_host()


# ------------------------------------------------------------------------------------------------ digital pre-compensation
# qampy/core/digital_pre_compensation.py on DeviceArrays; kernels in qampy_amd/csrc/precomp.hip.
PRECOMP_MEM_MAX = 15               # longest pattern
PRECOMP_M_MAX = 4096               # most levels of a rail, most points of a complex alphabet
PRECOMP_N_MAX = 2 ** 24            # largest table, M**mem_len
PRECOMP_LDS_N = 2048               # largest table a workgroup accumulates privately in LDS (csrc/precomp.hip PC_LDS_N)
PRECOMP_LUT_LMAX = 2 ** 24         # longest row of the table's accumulation: 37 bits per sample are left below the largest error
PRECOMP_ROW_MAX = 2 ** 40
PRECOMP_LEN_MAX = 2 ** 24          # most bins of the pre-emphasis table


class PatternLevels:
    """What a symbol is decided against (:func:`pattern_levels`): two rail tables ``lev_I`` / ``lev_Q`` (float64, strictly increasing), or one
    complex ``alphabet`` (complex128); ``M`` is the base of the pattern number and ``N(mem_len) = M**mem_len`` the table size.  The object owns
    the device copies of its tables: they go up at the first launch that needs them and live as long as the object, so a loop that keeps its
    levels uploads nothing, and no launch can be handed a table that something else has released."""
    __slots__ = ("lev_I", "lev_Q", "alphabet", "M", "_dev")

    def __init__(self, lev_I=None, lev_Q=None, alphabet=None):
        if alphabet is None:
            lev = []
            for name, v in (("lev_I", lev_I), ("lev_Q", lev_Q)):
                v = np.ascontiguousarray(v, dtype=np.float64)
                if v.ndim != 1 or not 2 <= v.size <= PRECOMP_M_MAX or not np.all(np.isfinite(v)) or not np.all(np.diff(v) > 0):
                    raise ValueError("%s: 2 to %d finite levels, strictly increasing" % (name, PRECOMP_M_MAX))
                lev.append(v)
            if lev[1].size > lev[0].size:
                raise ValueError("the quadrature rail has more levels than the in-phase rail: its patterns do not fit a table of M_I**mem_len entries")
            self.lev_I, self.lev_Q, self.alphabet, self.M = lev[0], lev[1], None, lev[0].size
            self._dev = None
        else:
            if lev_I is not None or lev_Q is not None:
                raise ValueError("rail tables or an alphabet, not both")
            a = np.ascontiguousarray(alphabet, dtype=np.complex128)
            if a.ndim != 1 or not 2 <= a.size <= PRECOMP_M_MAX or not np.all(np.isfinite(a)):
                raise ValueError("alphabet: 2 to %d finite points" % PRECOMP_M_MAX)
            self.lev_I, self.lev_Q, self.alphabet, self.M = None, None, a, a.size
            self._dev = None

    def N(self, mem_len):
        """``M**mem_len``, checked: ``1 <= mem_len <= 15`` and at most 2**24 entries."""
        if isinstance(mem_len, bool) or int(mem_len) != mem_len or not 1 <= int(mem_len) <= PRECOMP_MEM_MAX:
            raise ValueError("mem_len must be a whole number from 1 to %d" % PRECOMP_MEM_MAX)
        n = self.M ** int(mem_len)
        if n > PRECOMP_N_MAX:
            raise ValueError("M**mem_len = %d**%d exceeds the largest table, 2**24 entries" % (self.M, int(mem_len)))
        return n

    def _tables(self):
        """The device copies of the tables, (lev_I, lev_Q) or (alphabet,): uploaded once, owned by this object."""
        if self._dev is None:
            host = (self.lev_I, self.lev_Q) if self.alphabet is None else (self.alphabet,)
            self._dev = tuple(_lib.DeviceArray.from_host(t) for t in host)
        return self._dev

    def _abi(self, mem_len):
        """The level arguments of the C entry points; the pointers are those of :meth:`_tables`, alive while this object is."""
        dev = self._tables()
        if self.alphabet is None:
            return (dev[0].ptr, self.lev_I.size, dev[1].ptr, self.lev_Q.size, None, 0, int(mem_len))
        return (None, 0, None, 0, dev[0].ptr, self.alphabet.size, int(mem_len))


def pattern_levels(ref_sym, real_ptrns=True):
    """The levels ``cal_lut`` decides against, from the symbol alphabet ``ref_sym``: ``np.unique`` of its real and of its imaginary parts
    (``real_ptrns``), or ``np.unique(ref_sym)`` - complex, sorted by real part then imaginary part."""
    ref = np.asarray(ref_sym)
    if ref.ndim != 1 or ref.size < 1:
        raise ValueError("ref_sym must be a non-empty 1-d array")
    if real_ptrns:
        return PatternLevels(np.unique(ref.real), np.unique(ref.imag))
    return PatternLevels(alphabet=np.unique(ref))


def _precomp_levels(levels, what):
    if not isinstance(levels, PatternLevels):
        raise TypeError("%s: levels come from pattern_levels() or PatternLevels()" % what)
    return levels


def _precomp_gain(gain, what):
    if np.iscomplexobj(gain) or not np.isfinite(float(gain)):
        raise ValueError("%s: gain must be real and finite" % what)
    return float(gain)


def pattern_index_dev(E, levels, mem_len, idx_I=None, idx_Q=None):
    """
    The pattern number of every symbol of the (nmodes, L) complex DeviceArray ``E`` (``find_sym_patterns`` as ``cal_lut`` uses it), one launch:
    ``lev[k] = argmin |x[k] - levels|`` - the first minimum wins a tie, a NaN sample gets level 0 - and
    ``p[i] = sum_j lev[(i - mem_len // 2 + j) % L] * M**(mem_len - 1 - j)``; the window wraps as often as it must (``L < mem_len``).  With rail
    levels the real parts give ``idx_I`` and the imaginary parts ``idx_Q`` (each to the base of its own level count); with a complex alphabet both
    get the same numbers.  ``idx_I`` / ``idx_Q``: (nmodes, L) int32 DeviceArrays, made when both are None.  Returns ``(idx_I, idx_Q)``.
    """
    what = "pattern_index_dev"
    c = _pilot_field(E, what, "E")
    lv = _precomp_levels(levels, what)
    lv.N(mem_len)
    if idx_I is None and idx_Q is None:
        idx_I, idx_Q = _lib.DeviceArray(E.shape, np.int32), _lib.DeviceArray(E.shape, np.int32)
    for name, a in (("idx_I", idx_I), ("idx_Q", idx_Q)):
        if a is not None:
            _pilot_buf(a, what, name, E.shape, np.int32)
    _lib.call("qh_pattern_index_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], *lv._abi(mem_len), None if idx_I is None else idx_I.ptr, None if idx_Q is None else idx_Q.ptr)
    return idx_I, idx_Q


def lut_accumulate_dev(tx, rx, idx_I, idx_Q, N, idx_data=None, ea=None, nI=None, nQ=None):
    """
    The average error per pattern (``pythran_dsp.cal_lut_avg``): ``err = tx - rx`` at the positions where ``idx_data`` - a uint8 DeviceArray
    ``(L,)`` for all rows or ``(nmodes, L)``, None: everywhere - is not 0, summed per entry of ``idx_I`` (real parts) and ``idx_Q`` (imaginary
    parts): ``ea (nmodes, N)`` complex128 ``= sum_I / max(nI, 1) + 1j sum_Q / max(nQ, 1)`` - always complex128, as the reference's division by an
    integer array leaves it - and the counts ``nI``, ``nQ (nmodes, N)`` int32, with which tables of several captures can be merged.  A pattern
    that never occurs, and every entry under an empty mask, is 0.

    Bit-identical on every call: the sums are 64-bit integers in fixed point at the power-of-two scale that leaves ``ceil(log2(L + 1))`` bits of
    headroom above the row's largest error - with ``L <= 2**24`` at least 37 bits, 7.3e-12 of ``max |err|`` per sample.  Values whose sums are
    exact in double (dyadic errors) give the reference's table bit for bit.  Returns ``(ea, nI, nQ)``.
    """
    what = "lut_accumulate_dev"
    c = _pilot_field(tx, what, "tx")
    _pilot_buf(rx, what, "rx", tx.shape, tx.dtype)
    nm, L = tx.shape
    if L > PRECOMP_LUT_LMAX:
        raise ValueError("%s: a row of at most 2**24 symbols (split a longer capture and merge the tables by their counts)" % what)
    if isinstance(N, bool) or int(N) != N or not 1 <= int(N) <= PRECOMP_N_MAX:
        raise ValueError("%s: N must be a whole number from 1 to 2**24" % what)
    N = int(N)
    _pilot_buf(idx_I, what, "idx_I", tx.shape, np.int32)
    _pilot_buf(idx_Q, what, "idx_Q", tx.shape, np.int32)
    rows = 0
    if idx_data is not None:
        if np.dtype(idx_data.dtype) != np.uint8 or tuple(idx_data.shape) not in ((L,), (nm, L)):
            raise ValueError("%s: idx_data must be a uint8 DeviceArray of shape (L,) or (nmodes, L)" % what)
        rows = 1 if len(idx_data.shape) == 1 else nm
    for name, a, dt in (("ea", ea, np.complex128), ("nI", nI, np.int32), ("nQ", nQ, np.int32)):
        if a is not None:
            _pilot_buf(a, what, name, (nm, N), dt)
    ea = _lib.DeviceArray((nm, N), np.complex128) if ea is None else ea
    nI = _lib.DeviceArray((nm, N), np.int32) if nI is None else nI
    nQ = _lib.DeviceArray((nm, N), np.int32) if nQ is None else nQ
    _lib.call("qh_lut_accumulate_%s_dev" % c, tx.ptr, rx.ptr, nm, L, idx_I.ptr, idx_Q.ptr, None if idx_data is None else idx_data.ptr, rows, N, ea.ptr, nI.ptr, nQ.ptr)
    return ea, nI, nQ


def cal_lut_dev(tx, rx, levels, mem_len=3, idx_data=None, ea=None, idx_I=None, idx_Q=None, nI=None, nQ=None):
    """``cal_lut`` on (nmodes, L) complex DeviceArrays, every row on its own: :func:`pattern_index_dev` of ``tx``, then
    :func:`lut_accumulate_dev` with ``N = levels.N(mem_len)``.  The index rows stay whole (the reference cuts them to the positions of
    ``idx_data``).  Returns ``(ea, idx_I, idx_Q, nI, nQ)``."""
    what = "cal_lut_dev"
    _pilot_field(tx, what, "tx")
    _pilot_buf(rx, what, "rx", tx.shape, tx.dtype)
    N = _precomp_levels(levels, what).N(mem_len)
    if tx.shape[1] > PRECOMP_LUT_LMAX:
        raise ValueError("%s: a row of at most 2**24 symbols (split a longer capture and merge the tables by their counts)" % what)
    for name, a, shape, dt in (("idx_I", idx_I, tx.shape, np.int32), ("idx_Q", idx_Q, tx.shape, np.int32), ("ea", ea, (tx.shape[0], N), np.complex128),
                               ("nI", nI, (tx.shape[0], N), np.int32), ("nQ", nQ, (tx.shape[0], N), np.int32)):
        if a is not None:
            _pilot_buf(a, what, name, shape, dt)
    if idx_data is not None and (np.dtype(idx_data.dtype) != np.uint8 or tuple(idx_data.shape) not in ((tx.shape[1],), tuple(tx.shape))):
        raise ValueError("%s: idx_data must be a uint8 DeviceArray of shape (L,) or (nmodes, L)" % what)
    if idx_I is None:
        idx_I = _lib.DeviceArray(tx.shape, np.int32)
    if idx_Q is None:
        idx_Q = _lib.DeviceArray(tx.shape, np.int32)
    pattern_index_dev(tx, levels, mem_len, idx_I, idx_Q)
    ea, nI, nQ = lut_accumulate_dev(tx, rx, idx_I, idx_Q, N, idx_data=idx_data, ea=ea, nI=nI, nQ=nQ)
    return ea, idx_I, idx_Q, nI, nQ


def _precomp_table(ea, what, nmodes):
    if ea is None or len(ea.shape) != 2 or ea.shape[0] != nmodes or np.dtype(ea.dtype) != np.complex128 or not 1 <= ea.shape[1] <= PRECOMP_N_MAX:
        raise ValueError("%s: ea must be an (nmodes, N) complex128 DeviceArray, N at most 2**24" % what)
    return ea.shape[1]


def lut_apply_dev(sig, ea, idx_I, idx_Q, out, gain=1.0):
    """``out = sig + gain * (ea[idx_I].real + 1j * ea[idx_Q].imag)`` row by row on (nmodes, L) complex DeviceArrays, formed in double and rounded
    once to the field's precision; ``out`` may be ``sig``.  An index outside the table adds nothing."""
    what = "lut_apply_dev"
    c = _pilot_field(sig, what, "sig")
    _pilot_buf(out, what, "out", sig.shape, sig.dtype)
    N = _precomp_table(ea, what, sig.shape[0])
    _pilot_buf(idx_I, what, "idx_I", sig.shape, np.int32)
    _pilot_buf(idx_Q, what, "idx_Q", sig.shape, np.int32)
    gain = _precomp_gain(gain, what)
    _lib.call("qh_lut_apply_%s_dev" % c, sig.ptr, sig.shape[0], sig.shape[1], ea.ptr, N, idx_I.ptr, idx_Q.ptr, gain, out.ptr)
    return out


def lut_predistort_dev(sig, levels, mem_len, ea, out, gain=1.0):
    """:func:`pattern_index_dev` of ``sig`` and :func:`lut_apply_dev` in one launch: the pattern numbers are formed on the fly and no index row is
    written.  ``ea (nmodes, levels.N(mem_len))``; ``out`` must be another buffer than ``sig``, because a symbol's window reads its neighbours."""
    what = "lut_predistort_dev"
    c = _pilot_field(sig, what, "sig")
    _pilot_buf(out, what, "out", sig.shape, sig.dtype)
    if out is sig or out.ptr == sig.ptr:
        raise ValueError("%s: out must be another buffer than sig" % what)
    N = _precomp_levels(levels, what).N(mem_len)
    if _precomp_table(ea, what, sig.shape[0]) != N:
        raise ValueError("%s: ea must hold M**mem_len = %d entries per row" % (what, N))
    gain = _precomp_gain(gain, what)
    _lib.call("qh_lut_predistort_%s_dev" % c, sig.ptr, sig.shape[0], sig.shape[1], *levels._abi(mem_len), ea.ptr, N, gain, out.ptr)
    return out


def _vpi_rails(vpi):
    """(I, Q) of ``vpi`` as ``comp_mod_sin`` reads it: a value that is not complex serves both rails."""
    v = np.asarray(vpi)
    if v.ndim != 0:
        raise ValueError("vpi must be one real or complex number")
    v = complex(v) if np.iscomplexobj(v) else complex(float(v), float(v))
    if not (np.isfinite(v.real) and np.isfinite(v.imag)):
        raise ValueError("vpi must be finite")
    return v.real, v.imag


def comp_mod_sin_dev(E, out, vpi=1.14, clip=0):
    """``2 * vpi.real * arcsin(E.real) + 1j * 2 * vpi.imag * arcsin(E.imag)`` on (nmodes, L) complex DeviceArrays (``comp_mod_sin``; a ``vpi``
    that is not complex serves both rails), in double, rounded once; NaN in a rail whose input lies outside [-1, 1], as numpy gives.  ``clip > 0``:
    ``clipper(E, clip)`` first, in the same launch; 0: no clamp.  ``out`` may be ``E``."""
    what = "comp_mod_sin_dev"
    c = _pilot_field(E, what, "E")
    _pilot_buf(out, what, "out", E.shape, E.dtype)
    vr, vi = _vpi_rails(vpi)
    if np.iscomplexobj(clip) or not (np.isfinite(float(clip)) and float(clip) >= 0):
        raise ValueError("%s: clip must be 0 (no clamp) or a positive level" % what)
    _lib.call("qh_comp_mod_sin_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], vr, vi, float(clip), out.ptr)
    return out


def _dac_preemphasis_args(dpe_fb, sim_len, rrc_beta, PAPR, prms_dac, os):
    """(fb, fs, beta, noise factor, sections) of ``comp_dac_resp``, checked."""
    try:
        cutoff, order, frmt, enob = prms_dac
    except (TypeError, ValueError):
        raise ValueError("prms_dac is (cutoff, order, 'sos', enob)")
    if frmt != "sos":
        raise ValueError("prms_dac: the filter format must be 'sos'")
    if isinstance(sim_len, bool) or int(sim_len) != sim_len or not 1 <= int(sim_len) <= PRECOMP_LEN_MAX:
        raise ValueError("sim_len must be a whole number from 1 to 2**24")
    fb, osf, beta, papr, enob = float(dpe_fb), float(os), float(rrc_beta), float(PAPR), float(enob)
    if not (np.isfinite(fb) and fb > 0 and np.isfinite(osf) and osf > 0):
        raise ValueError("the symbol rate and the oversampling must be positive")
    if not 0 <= beta <= 1:
        raise ValueError("rrc_beta must lie between 0 and 1")
    if not (np.isfinite(papr) and np.isfinite(enob)):
        raise ValueError("PAPR and the ENOB must be finite")
    fs = dpe_fb * os
    sos = np.ascontiguousarray(design_lowpass_sos(fs, cutoff, "bessel", order), dtype=np.float64)
    try:
        noise = float(10 ** (PAPR / 10) / (6 * dpe_fb * 2 ** (2 * enob)))
    except OverflowError:
        noise = np.inf
    if not np.isfinite(noise):
        raise ValueError("PAPR and the ENOB give no finite noise factor")
    return fb, float(fs), beta, float(noise), sos


def comp_dac_resp_dev(dpe_fb, sim_len, rrc_beta, PAPR=9, prms_dac=(16e9, 2, "sos", 6), os=2, dtype=np.complex128, out=None):
    """
    ``p_f`` of ``comp_dac_resp`` - the regularised inverse of the DAC's Bessel low-pass under a root-raised-cosine signal - as a ``(sim_len,)``
    DeviceArray of ``dtype`` (complex64 or complex128) in ``fftfreq`` order, built on the device in double (three launches): the raised-cosine power
    response ``n_f``, the response ``d_f`` of the low-pass's second-order sections (designed on the host, :func:`design_lowpass_sos`), ``alpha``
    from one ordered sum, ``p_f = n_f conj(d_f) / (n_f |d_f|**2 + alpha)``.  ``prms_dac = (cutoff, order, 'sos', enob)``: another format raises
    ValueError.  ``out``: the table's buffer, made when None.
    """
    suf, rt, ct = _lib.suffix(dtype)
    if np.dtype(dtype) != ct:
        raise TypeError("comp_dac_resp_dev: the table is complex64 or complex128")
    fb, fs, beta, noise, sos = _dac_preemphasis_args(dpe_fb, sim_len, rrc_beta, PAPR, prms_dac, os)
    if out is None:
        out = _lib.DeviceArray((int(sim_len),), ct)
    else:
        _pilot_buf(out, "comp_dac_resp_dev", "out", (int(sim_len),), ct)
    _lib.call("qh_dac_preemphasis_table_%s_dev" % _lib.cname(suf), int(sim_len), fb, fs, beta, noise, _lib.ptr(sos), sos.shape[0], out.ptr)
    return out


def dac_preemphasis_dev(E, out, dpe_fb, rrc_beta, PAPR=9, prms_dac=(16e9, 2, "sos", 6), os=2, table=None):
    """``ifft(p_f * fft(E))`` of every row of the (nmodes, L) complex DeviceArray ``E``, ``p_f = comp_dac_resp(dpe_fb, L, rrc_beta, ...)``:
    :func:`comp_dac_resp_dev` into ``table`` (an ``(L,)`` DeviceArray of E's dtype; made when None), then :func:`spectral_filter_dev`.  ``out``
    may be ``E``."""
    _fft_field(E, out, "dac_preemphasis_dev")
    table = comp_dac_resp_dev(dpe_fb, E.shape[1], rrc_beta, PAPR=PAPR, prms_dac=prms_dac, os=os, dtype=E.dtype, out=table)
    return spectral_filter_dev(E, out, table)


# ---------------------------------------------------------------------------------------------- theory curves
# The last loop of pythran_dsp without a device form, cal_gmi_mc (qampy/core/pythran_dsp.py:181-197, behind qampy.theory.cal_gmi), and the shaped
# source of qampy.theory.generate_ps_symbols; kernels in csrc/metrics.hip (awgn_mc_*) and csrc/source.hip (ps_symbols_kernel).
MC_TILE = 256                      # (sent point, draw) pairs per workgroup of the Monte-Carlo kernel (csrc/metrics.hip MET_THREADS)
MC_TRIP = 1024 * MC_TILE           # pairs of one SNR point the capped grid covers in one trip (MET_MAXBLK workgroups)
MC_NSNR_MAX = 65535                # SNR points of one launch
MC_NS_MAX = 2 ** 31                # draws per SNR point
PS_TILE = 1024                     # samples of one mode per workgroup of the shaped source (csrc/source.hip PS_TILE)
PS_LMAX = 64                       # most levels of a rail
PS_ROW_MAX = 2 ** 31               # most samples of a row of the shaped source: one workgroup per tile, no stride (csrc/source.hip SRC_NMAX)


def fresh_seed():
    """A 64-bit seed from the operating system's entropy: what ``seed=None`` means to the Monte-Carlo curves and the shaped source."""
    import os
    return int.from_bytes(os.urandom(8), "little")


def _mc_seed(seed):
    return fresh_seed() if seed is None else _seed64(seed)


def _mc_snr(snr, what):
    """The linear SNR points as a contiguous 1-d float64 host array, every one finite and positive."""
    s = np.atleast_1d(np.asarray(snr, dtype=np.float64))
    if s.ndim != 1 or not 1 <= s.size <= MC_NSNR_MAX:
        raise ValueError("%s: between 1 and %d SNR points in one array" % (what, MC_NSNR_MAX))
    if not np.all(np.isfinite(s) & (s > 0)):
        raise ValueError("%s: every linear SNR must be finite and positive" % what)
    return np.ascontiguousarray(s)


def _mc_snr_dev(snr, what):
    """``snr`` on the device: a 1-d float64 DeviceArray as it is (its values are the caller's business), host values checked and uploaded."""
    if hasattr(snr, "ptr"):
        if len(snr.shape) != 1 or np.dtype(snr.dtype) != np.float64 or not 1 <= snr.shape[0] <= MC_NSNR_MAX:
            raise TypeError("%s: snr on the device must be a 1-d float64 DeviceArray of at most %d points" % (what, MC_NSNR_MAX))
        return snr, None
    host = _mc_snr(snr, what)
    return None, host


def _mc_draws(z, nsnr, what):
    c = _sync_cplx(z, what, "z")
    if len(z.shape) != 2 or z.shape[0] != nsnr or not 1 <= z.shape[1] <= MC_NS_MAX:
        raise ValueError("%s: z must be (%d, ns) with 1 <= ns <= 2**31" % (what, nsnr))
    return c


def awgn_mc_noise_dev(z, snr, seed):
    """The Monte-Carlo noise of :func:`awgn_mc_dev` into the ``(nsnr, ns)`` complex DeviceArray ``z``: ``z[p, l] = (g0 + 1j g1) sqrt(1 / (2 snr[p]))``
    with ``(g0, g1)`` the two standard normals of Philox counter ``(l, p, stream 3)`` under ``seed`` - what ``cal_gmi_mc`` draws with
    ``np.random.randn``, here a function of ``(seed, p, l)`` alone, every SNR point with draws of its own.  ``snr``: the linear SNRs, host values
    or a float64 DeviceArray; ``seed=None``: a fresh one.  Nothing is read back.  With ``snr`` on the device the call only enqueues one launch;
    host values go up in a temporary buffer whose release, when the call returns, waits for the device - keep a DeviceArray of the SNRs to stay
    asynchronous."""
    dev, host = _mc_snr_dev(snr, "awgn_mc_noise_dev")
    nsnr = dev.shape[0] if host is None else host.size
    c = _mc_draws(z, nsnr, "awgn_mc_noise_dev")
    seed = _mc_seed(seed)
    if dev is None:
        dev = _lib.DeviceArray.from_host(host)
    _lib.call("qh_awgn_mc_noise_%s_dev" % c, z.ptr, dev.ptr, nsnr, z.shape[1], seed)
    return z


def awgn_mc_dev(alphabet, snr, z, out):
    """Monte-Carlo GMI and MI of ``alphabet`` (``M = 2**nbits`` points in label order, a complex DeviceArray) over AWGN at every linear SNR of
    ``snr`` with the draws ``z`` ``(nsnr, ns)`` of the alphabet's dtype: ``out`` ``(nsnr, 2 + nbits)`` float64 DeviceArray receives ``[gmi, mi,
    gmi of bit 0 .. nbits - 1]`` per point, ``gmi`` what ``pythran_dsp.cal_gmi_mc`` returns for the draws ``z[p]`` and ``mi`` what
    ``cal_mi_mc(z[p], alphabet, 1 / snr[p])`` returns, from one pass (``M**2 ns`` exponentials per point).  All points in one launch of the kernel
    (three launches with the two reductions; beyond 32 MiB of workgroup partials - hundreds of points - in batches of that size); nothing is read
    back; a repeated call is bit-identical.  ``snr`` as host values is uploaded to a temporary buffer whose release waits for the device when the
    call returns: pass a float64 DeviceArray to only enqueue.  The partials live in the calling thread's scratch, which ``cal_metrics_dev`` uses
    too: on two library streams of one thread (``_lib.on_stream``) the two must be ordered by the caller."""
    c = _sync_cplx(alphabet, "awgn_mc_dev", "alphabet")
    if len(alphabet.shape) != 1:
        raise ValueError("awgn_mc_dev: the alphabet must be 1-d")
    M = alphabet.shape[0]
    nb = int(round(np.log2(M))) if M >= 1 else 0
    if 2 ** nb != M or not 1 <= nb <= 10:
        raise ValueError("awgn_mc_dev: the alphabet must have 2**nbits points, nbits in 1..10, got %d" % M)
    dev, host = _mc_snr_dev(snr, "awgn_mc_dev")
    nsnr = dev.shape[0] if host is None else host.size
    if _mc_draws(z, nsnr, "awgn_mc_dev") != c:
        raise TypeError("awgn_mc_dev: z and the alphabet must have one dtype")
    if np.dtype(out.dtype) != np.float64 or tuple(out.shape) != (nsnr, 2 + nb):
        raise ValueError("awgn_mc_dev: out must be a (%d, %d) float64 DeviceArray" % (nsnr, 2 + nb))
    if dev is None:
        dev = _lib.DeviceArray.from_host(host)
    _lib.call("qh_awgn_mc_%s_dev" % c, alphabet.ptr, M, dev.ptr, nsnr, z.ptr, z.shape[1], out.ptr)
    return out


def awgn_mc(alphabet, snr, ns, noise=None, seed=None, return_noise=False):
    """:func:`awgn_mc_dev` for a host alphabet (complex64 or complex128, label order): the ``(nsnr, 2 + nbits)`` result on the host.  ``noise``:
    explicit draws ``(nsnr, ns)`` instead of the seeded ones of :func:`awgn_mc_noise_dev`; ``return_noise``: also the draws that were used."""
    al = np.ascontiguousarray(alphabet)
    suf, rt, ct = _lib.suffix(al.dtype)
    if al.ndim != 1 or al.dtype != ct:
        raise TypeError("awgn_mc: the alphabet must be a 1-d complex64 or complex128 array")
    nb = int(round(np.log2(al.size))) if al.size else 0
    if 2 ** nb != al.size or not 1 <= nb <= 10:
        raise ValueError("awgn_mc: the alphabet must have 2**nbits points, nbits in 1..10, got %d" % al.size)
    s = _mc_snr(snr, "awgn_mc")
    if int(ns) != ns or not 1 <= int(ns) <= MC_NS_MAX:
        raise ValueError("awgn_mc: ns must be a whole number in [1, 2**31]")
    ns = int(ns)
    if noise is not None:
        if np.size(noise) != s.size * ns:
            raise ValueError("awgn_mc: noise must hold %d x %d draws" % (s.size, ns))
        noise = np.ascontiguousarray(noise, dtype=ct).reshape(s.size, ns)
    else:
        seed = _mc_seed(seed)
    A, S = _lib.DeviceArray.from_host(al), _lib.DeviceArray.from_host(s)
    if noise is not None:
        Z = _lib.DeviceArray.from_host(noise)
    else:
        Z = awgn_mc_noise_dev(_lib.DeviceArray((s.size, ns), ct), S, seed)
    out = awgn_mc_dev(A, S, Z, _lib.DeviceArray((s.size, 2 + nb), np.float64)).to_host()
    return (out, Z.to_host()) if return_noise else out


def cal_gmi_mc(symbols, snr, ns, bit_map, noise=None, seed=None):
    """Monte-Carlo soft-decision GMI of a labelled alphabet at the linear ``snr`` (``pythran_dsp.cal_gmi_mc``, pythran_dsp.py:181-197): ``nbits -
    sum / (M ns)`` over ``ns`` noise draws ``z = sqrt(1 / snr) (randn + 1j randn) / sqrt(2)``.  ``bit_map`` ``(nbits, M / 2, 2)`` labels the points
    (:func:`bits_map_labels`); the precision is that of ``symbols``.  The reference draws from numpy's global generator inside the function; here
    the draws are counter-based under ``seed`` (None: a fresh one), or ``noise`` gives the ``ns`` values of ``z`` explicitly - with the reference's
    own draws the result is the reference's."""
    sy = np.asarray(symbols)
    suf, rt, ct = _lib.suffix(sy.dtype)
    if sy.ndim != 1 or sy.dtype != ct:
        raise TypeError("cal_gmi_mc: symbols must be a 1-d complex64 or complex128 array")
    alphabet = np.ascontiguousarray(bits_map_labels(bit_map), dtype=ct)
    if alphabet.size != sy.size:
        raise ValueError("cal_gmi_mc: bit_map labels %d points, symbols holds %d" % (alphabet.size, sy.size))
    if np.ndim(snr) != 0:
        raise ValueError("cal_gmi_mc: one linear SNR (theory.cal_gmi takes an array)")
    if noise is not None and np.size(noise) != ns:
        raise ValueError("cal_gmi_mc: noise must hold ns = %d draws" % ns)
    return float(awgn_mc(alphabet, snr, ns, noise=noise, seed=seed)[0, 0])


def ps_cdf(px):
    """The cumulative table of the shaped source: ``cumsum(px) / sum(px)`` in float64, its last entry forced to 1."""
    p = np.asarray(px, dtype=np.float64).ravel()
    if not 1 <= p.size <= PS_LMAX:
        raise ValueError("ps_symbols: between 1 and %d levels" % PS_LMAX)
    if not np.all(np.isfinite(p) & (p >= 0)) or not p.sum() > 0:
        raise ValueError("ps_symbols: the probabilities must be finite, not negative and not all zero")
    cdf = np.cumsum(p) / p.sum()
    cdf[-1] = 1.0
    return np.ascontiguousarray(np.minimum(cdf, 1.0))


def ps_symbols_dev(out, levels, px, seed, labels=None, label_table=None):
    """Probabilistically shaped symbols into the complex DeviceArray ``out`` ``(nmodes, N)`` or ``(N,)``: ``out[m, n] = levels[i] + 1j levels[q]``,
    ``i`` and ``q`` drawn with the probabilities ``px`` - the number of entries of :func:`ps_cdf` that are ``<= u``, ``u = word 2**-32`` of the
    Philox words x (I) and y (Q) of counter ``(n, m, stream 4)`` under ``seed`` (None: a fresh one).  ``levels`` (at most 64) are rounded to the
    row's precision once.  ``labels``: an int32 DeviceArray of ``out``'s shape for ``label_table[i, q]``, ``label_table`` an ``(L, L)`` int32 host
    array or DeviceArray.  At most 2**31 samples per row.  One launch, nothing read back; a host ``label_table`` goes up in a temporary buffer
    whose release waits for the device when the call returns - pass a DeviceArray to only enqueue."""
    c = _sync_cplx(out, "ps_symbols_dev", "out")
    rows, N = _sync_rows(out, "ps_symbols_dev", "out")
    if N > PS_ROW_MAX or rows > 65535:
        raise ValueError("ps_symbols_dev: at most 65535 rows of 2**31 samples")
    lev = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).ravel())
    cdf = ps_cdf(px)
    if lev.size != cdf.size or not np.all(np.isfinite(lev)):
        raise ValueError("ps_symbols_dev: one finite level per probability")
    L = lev.size
    if (labels is None) != (label_table is None):
        raise ValueError("ps_symbols_dev: labels and label_table go together")
    if labels is not None:
        if np.dtype(labels.dtype) != np.int32 or tuple(labels.shape) != tuple(out.shape):
            raise ValueError("ps_symbols_dev: labels must be int32 of out's shape")
        if np.dtype(label_table.dtype) != np.int32 or tuple(label_table.shape) != (L, L):
            raise ValueError("ps_symbols_dev: label_table must be int32 (%d, %d)" % (L, L))
    seed = _mc_seed(seed)
    if label_table is not None and not hasattr(label_table, "ptr"):
        label_table = _lib.DeviceArray.from_host(np.ascontiguousarray(label_table))
    _lib.call("qh_ps_symbols_%s_dev" % c, out.ptr, rows, N, _lib.ptr(lev), _lib.ptr(cdf), L, seed, None if labels is None else labels.ptr,
              None if label_table is None else label_table.ptr)
    return out


# ------------------------------------------------------------------------------------------------ blind signal quality
# qampy/core/signal_quality.py:122-271 (norm_to_s0, cal_evm, cal_snr_qam, cal_s0, cal_snr_blind_qpsk) on DeviceArrays; kernels in
# qampy_amd/csrc/blind.hip.  Nothing here needs the transmitted symbols.
BLIND_M_MAX = 1024                 # most alphabet points of the distance search (csrc/blind.hip BL_M_MAX)
BLIND_SLICE = 1024                 # fewest samples a workgroup sums before a row or block is cut (BL_MIN)
BLIND_SLICES = 256                 # most workgroups per row or block (BL_NB)
BLIND_STATS = ("r2", "r4", "S1", "S2", "snr", "s0")


def cal_gamma(M):
    """``mean |a|^4`` of the unit-power M-QAM alphabet, the reference's ``_cal_gamma`` (signal_quality.py:227-231) on the host."""
    from .. import theory
    M = int(M)
    if M < 2:
        raise ValueError("cal_gamma: M must be at least 2")
    A = abs(theory.cal_symbols_qam(M)) / np.sqrt(theory.cal_scaling_factor_qam(M))
    uniq, counts = np.unique(A, return_counts=True)
    return float(np.sum(uniq ** 4 * counts / M))


def stats_from_moments(r2, r4, gamma):
    """``(S1, S2, snr, s0)`` of the moment estimator from ``mean |E|^2`` and ``mean |E|^4`` in host arithmetic (signal_quality.py:218-224,
    :251-258); arrays or scalars."""
    with np.errstate(all="ignore"):
        S1 = 1 - 2 * r2 ** 2 / r4 - np.sqrt((2 - gamma) * (2 * r2 ** 4 / r4 ** 2 - r2 ** 2 / r4))
        S2 = gamma * r2 ** 2 / r4 - 1
        return S1, S2, S1 / S2, r2 / (1 + S2 / S1)


_BLIND_IDEAL = {}


def blind_ideal(M):
    """``(Pi, mean |Pi|^2, gamma)`` of M-QAM on the host in double: the ideal alphabet normalised by its own moment estimate of the signal power,
    ``Pi = ideal / sqrt(cal_s0(ideal, M))`` (signal_quality.py:158-159), kept per M."""
    from .. import theory
    M = int(M)
    if M not in _BLIND_IDEAL:
        gamma = cal_gamma(M)
        ideal = np.asarray(theory.cal_symbols_qam(M), dtype=np.complex128).ravel()
        a2 = abs(ideal) ** 2
        s0 = stats_from_moments(np.mean(a2), np.mean(a2 ** 2), gamma)[3]
        Pi = ideal / np.sqrt(s0)
        _BLIND_IDEAL[M] = (Pi, float(np.mean(abs(Pi) ** 2)), gamma)
    return _BLIND_IDEAL[M]


_BLIND_TABLES = threading.local()


def _blind_alphabet_dev(M, dtype):
    """The device copy of :func:`blind_ideal`'s alphabet in ``dtype``, uploaded once per (M, dtype) and host thread."""
    kept = getattr(_BLIND_TABLES, "kept", None)
    if kept is None:
        kept = _BLIND_TABLES.kept = {}
    key = (int(M), np.dtype(dtype).str)
    if key not in kept:
        kept[key] = _lib.DeviceArray.from_host(np.ascontiguousarray(blind_ideal(M)[0], dtype=dtype))
    return kept[key]


def _blind_field(E, what, name="E"):
    if not hasattr(E, "ptr") or np.dtype(E.dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise TypeError("%s: %s must be a complex64 or complex128 DeviceArray" % (what, name))
    rows, L = _sync_rows(E, what, name)
    if rows > 65535:
        raise ValueError("%s: at most 65535 rows" % what)
    return _sync_cplx(E, what, name), rows, L


def _blind_block(what, block, L):
    """``(block argument of the library, blocks per row)``; ``block`` None or 0: whole rows."""
    if block is None or block == 0:
        return 0, 1
    if int(block) != block or block < 0:
        raise ValueError("%s: block must be a positive whole number of samples" % what)
    if block > L:
        raise ValueError("%s: block = %d is longer than a row of %d samples" % (what, block, L))
    return int(block), L // int(block)


def _blind_M(what, M):
    if int(M) != M or not 2 <= M <= BLIND_M_MAX:
        raise ValueError("%s: M from 2 to %d" % (what, BLIND_M_MAX))
    return int(M)


def _blind_buf(buf, what, name, shape):
    if buf is None:
        return _lib.DeviceArray(shape, np.float64)
    if np.dtype(buf.dtype) != np.float64 or int(np.prod(buf.shape)) != int(np.prod(shape)):
        raise ValueError("%s: %s must be float64 %s" % (what, name, tuple(shape)))
    return buf


def blind_moments_dev(E, block=None, mom=None):
    """``mean |E|^2, mean |E|^4, mean re, mean im`` of every row of the complex DeviceArray ``E`` ((L,) or (nrows, L)) into the float64 DeviceArray
    ``mom (nrows, 4)`` (made when None) - or, with ``block``, of every whole block of ``block`` samples into ``mom (nrows, L // block, 4)``; a
    shorter tail is left out.  Terms and sums in double, in a fixed order: two calls give the same bits.  Nothing is read back."""
    what = "blind_moments_dev"
    c, rows, L = _blind_field(E, what)
    blk, nblocks = _blind_block(what, block, L)
    mom = _blind_buf(mom, what, "mom", (rows, 4) if not blk else (rows, nblocks, 4))
    _lib.call("qh_blind_moments_%s_dev" % c, E.ptr, rows, L, blk, mom.ptr)
    return mom


def blind_stats_dev(E, M, block=None, stats=None, mom=None):
    """The moment estimator of an M-QAM signal (Gao and Tepedelenlioglu; ``cal_snr_qam`` / ``cal_s0``) per row - or per block - of ``E``: the
    float64 DeviceArray ``stats (nrows, 6)`` / ``(nrows, L // block, 6)`` = ``(r2, r4, S1, S2, snr, s0)`` (:data:`BLIND_STATS`), ``snr`` linear.
    ``stats`` and the intermediate ``mom`` are made when None.  NaN / inf where the formula gives them.  Nothing is read back."""
    what = "blind_stats_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    blk, nblocks = _blind_block(what, block, L)
    shape = (rows,) if not blk else (rows, nblocks)
    stats = _blind_buf(stats, what, "stats", shape + (6,))
    mom = blind_moments_dev(E, block, mom)
    _lib.call("qh_blind_finish_dev", mom.ptr, rows * nblocks, blind_ideal(M)[2], stats.ptr)
    return stats


def _blind_row_stats(what, E, M, stats, rows):
    if stats is None:
        return blind_stats_dev(E, M)
    if np.dtype(stats.dtype) != np.float64 or tuple(stats.shape) != (rows, 6):
        raise ValueError("%s: stats must be the float64 (%d, 6) of blind_stats_dev on whole rows" % (what, rows))
    return stats


def norm_to_s0_dev(E, M, out, stats=None):
    """``out = E / sqrt(s0)`` per row, ``s0`` the moment estimate of the signal power read from ``stats`` in HBM (``blind_stats_dev(E, M)``, formed
    here when None): the reference's ``norm_to_s0``.  ``out`` has E's shape and dtype and may be ``E``.  Nothing is read back."""
    what = "norm_to_s0_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    if not hasattr(out, "ptr") or tuple(out.shape) != tuple(E.shape) or np.dtype(out.dtype) != np.dtype(E.dtype):
        raise ValueError("%s: out must have E's shape and dtype" % what)
    stats = _blind_row_stats(what, E, M, stats, rows)
    _lib.call("qh_scale_by_stat_%s_dev" % c, E.ptr, rows, L, stats.ptr, out.ptr)
    return out


def blind_evm_dev(E, M, known=None, stats=None, stats_known=None, evm_sum=None):
    """The reference's ``cal_evm(sig, M, known)`` per row of ``E`` as a host array ``(nrows,)``: the RMS distance of ``E / sqrt(s0)`` to the
    nearest point of the equally normalised ideal M-QAM alphabet, relative to that alphabet's RMS - or, with ``known`` (a DeviceArray of E's
    shape and dtype), to ``known / sqrt(s0(known))``, relative to its RMS.  ``stats`` / ``stats_known``: ``blind_stats_dev`` of E / known when at
    hand; ``evm_sum``: a float64 ``(nrows,)`` work buffer.  Reads back ``nrows`` sums (and the stats of ``known``)."""
    what = "blind_evm_dev"
    c, rows, L = _blind_field(E, what)
    M = _blind_M(what, M)
    if known is not None:
        ck, rk, Lk = _blind_field(known, what, "known")
        if (ck, rk, Lk) != (c, rows, L):
            raise ValueError("%s: known must have E's shape and dtype" % what)
    stats = _blind_row_stats(what, E, M, stats, rows)
    evm_sum = _blind_buf(evm_sum, what, "evm_sum", (rows,))
    if known is None:
        pi2 = blind_ideal(M)[1]
        _lib.call("qh_blind_evm_%s_dev" % c, E.ptr, rows, L, stats.ptr, _blind_alphabet_dev(M, E.dtype).ptr, M, None, None, evm_sum.ptr)
    else:
        stats_known = _blind_row_stats(what, known, M, stats_known, rows)
        _lib.call("qh_blind_evm_%s_dev" % c, E.ptr, rows, L, stats.ptr, None, 0, known.ptr, stats_known.ptr, evm_sum.ptr)
        sk = stats_known.to_host().reshape(rows, 6)
        with np.errstate(all="ignore"):
            pi2 = sk[:, 0] / sk[:, 5]                   # mean |known|^2 / s0(known)
    with np.errstate(all="ignore"):
        return np.sqrt(evm_sum.to_host().reshape(rows) / L / pi2)


def qpsk_blind_snr_dev(E, block=None, out=None):
    """The reference's ``cal_snr_blind_qpsk`` per row - or per block - of ``E``: the float64 DeviceArray ``out (nrows, 3)`` / ``(nrows, L // block,
    3)`` = ``(P, var, 10 log10(P / var))`` with ``Eref = (-E**4)**(1/4)`` on the principal branch, ``P = mean |Eref|^2``, ``var = P - |mean
    Eref|^2``.  Nothing is read back."""
    what = "qpsk_blind_snr_dev"
    c, rows, L = _blind_field(E, what)
    blk, nblocks = _blind_block(what, block, L)
    out = _blind_buf(out, what, "out", (rows, 3) if not blk else (rows, nblocks, 3))
    _lib.call("qh_qpsk_blind_%s_dev" % c, E.ptr, rows, L, blk, out.ptr)
    return out


# ---------------------------------------------------------------------------------------------- time-domain hybrid QAM
# csrc/hybrid.hip on DeviceArrays: TDHQAMSymbols (qampy/signals.py:1182-1427) built, taken apart and measured on resident rows.  A frame of ``fM``
# symbols holds ``fM1`` symbols of format 1 followed by ``fM2`` of format 2; format-2 symbols are stored divided by ``sqrt(powratio)``.  The
# reference's own split and metrics raise; DESIGN.md 3.21 fixes what they mean here.
TDH_FM_MAX = 256                   # longest frame of the device forms (csrc/hybrid.hip TDH_FM_MAX)
TDH_TILE = 4096                    # samples of a row per workgroup of the class sums (TDH_TILE)
TDH_M_MAX = 1024                   # most points of an alphabet of the metrics pass (TDH_M_MAX)
TDH_ROW_MAX = 2 ** 31 - 1          # longest row
TDH_SUMS = ("symbol_errors", "bit_errors", "compared", "squared_error")


def tdh_geometry(fr):
    """``(f_M, f_M1, f_M2)`` of a hybrid frame in which the second format takes the fraction ``fr``: ``Fraction(fr).limit_denominator()`` is
    ``f_M2 / f_M`` (``TDHQAMSymbols._cal_fractions``).  Position ``n`` of a row carries format 1 when ``n % f_M < f_M1``."""
    import fractions
    rat = fractions.Fraction(fr).limit_denominator()
    return rat.denominator, rat.denominator - rat.numerator, rat.numerator


def tdh_power_ratio(alphabet1, alphabet2, method="dist"):
    """The power ratio that gives two alphabets the same spacing (``calculate_power_ratio(..., "dist")``): ``(d2 / d1)**2`` with ``d`` the smallest
    distance between neighbours of the alphabet's distinct points in ``np.unique``'s order.  Format-2 symbols are stored over its root."""
    if method != "dist":
        raise NotImplementedError("Only 'dist' method is currently implemented")
    d1, d2 = (np.abs(np.diff(np.unique(np.asarray(a)))).min() for a in (alphabet1, alphabet2))
    return (d2 / d1) ** 2


def _tdh_frame(what, fM, fM1):
    if int(fM) != fM or int(fM1) != fM1:
        raise ValueError("%s: the frame lengths are whole numbers" % what)
    fM, fM1 = int(fM), int(fM1)
    if not 2 <= fM <= TDH_FM_MAX:
        raise ValueError("%s: the device forms take frames of 2 .. %d symbols, got f_M = %d" % (what, TDH_FM_MAX, fM))
    if not 1 <= fM1 < fM:
        raise ValueError("%s: both formats need a place in the frame (1 <= f_M1 < f_M)" % what)
    return fM, fM1


def _tdh_powratio(what, powratio):
    powratio = float(powratio)
    if not (np.isfinite(powratio) and powratio > 0):
        raise ValueError("%s: powratio must be positive and finite" % what)
    return powratio


def _tdh_field(E, what, name, fM):
    """``(c, nmodes, L)`` of a 2-d complex DeviceArray of whole frames."""
    c = _sync_cplx(E, what, name)
    if len(E.shape) != 2 or min(E.shape) < 1:
        raise ValueError("%s: %s must be a non-empty 2-d complex DeviceArray" % (what, name))
    nm, L = E.shape
    if nm > 65535 or L > TDH_ROW_MAX:
        raise ValueError("%s: %s is too large" % (what, name))
    if L % fM:
        raise ValueError("%s: a row of %d symbols does not hold whole frames of %d (the cyclic shift is only meaningful on whole frames)" % (what, L, fM))
    return c, nm, L


def _tdh_buf(a, what, name, shape, dtype, make=False):
    if a is None and make:
        return _lib.DeviceArray(shape, dtype)
    if a is None or tuple(a.shape) != tuple(shape):
        raise ValueError("%s: %s must be %s %s" % (what, name, tuple(shape), np.dtype(dtype).name))
    if np.dtype(a.dtype) != np.dtype(dtype):
        raise ValueError("%s: %s must be %s" % (what, name, np.dtype(dtype).name))
    return a


def _tdh_shift(what, shift, nm):
    """``(device pointer or None, host value)`` of a shift given as an int32 DeviceArray ``(nmodes,)`` or as one whole number."""
    if hasattr(shift, "ptr"):
        _tdh_buf(shift, what, "shift", (nm,), np.int32)
        return shift.ptr, 0
    if np.ndim(shift) != 0 or int(shift) != shift or abs(int(shift)) > TDH_ROW_MAX:
        raise ValueError("%s: shift is an int32 DeviceArray (nmodes,) or one whole number" % what)
    return None, int(shift)


def tdh_assemble_dev(part1, part2, fM, fM1, powratio, out, labels1=None, labels2=None, idx_out=None):
    """Interleave ``part1 (nmodes, nframes * fM1)`` and ``part2 (nmodes, nframes * fM2)`` into ``out (nmodes, nframes * fM)`` in one launch,
    part 2 times ``1 / sqrt(powratio)`` (the product numpy's in-place ``/=`` forms).  With ``labels1``, ``labels2`` (int32, the parts' shapes) and
    ``idx_out (nmodes, nframes * fM)`` int32 the labels are laid out like the symbols: the label of the format at every position.  All
    DeviceArrays of one complex dtype; nothing is read back."""
    what = "tdh_assemble_dev"
    fM, fM1 = _tdh_frame(what, fM, fM1)
    powratio = _tdh_powratio(what, powratio)
    c, nm, L = _tdh_field(out, what, "out", fM)
    nframes = L // fM
    for a, name, n in ((part1, "part1", fM1), (part2, "part2", fM - fM1)):
        _tdh_buf(a, what, name, (nm, nframes * n), out.dtype)
    given = [a is not None for a in (labels1, labels2, idx_out)]
    if any(given) and not all(given):
        raise ValueError("%s: labels1, labels2 and idx_out come together" % what)
    if all(given):
        _tdh_buf(labels1, what, "labels1", part1.shape, np.int32)
        _tdh_buf(labels2, what, "labels2", part2.shape, np.int32)
        _tdh_buf(idx_out, what, "idx_out", out.shape, np.int32)
    _lib.call("qh_tdh_assemble_%s_dev" % c, part1.ptr, part2.ptr, labels1.ptr if all(given) else None, labels2.ptr if all(given) else None, nm, nframes,
              fM, fM1, powratio, out.ptr, idx_out.ptr if all(given) else None)
    return out


def tdh_class_sums_dev(E, fM, sums=None):
    """``sums[m, r] = sum |E[m, n]|`` over ``n % fM == r`` into the float64 DeviceArray ``sums (nmodes, fM)`` (made when None).  Terms and sums
    in double, in a fixed order without atomics: two calls give the same bits.  Nothing is read back."""
    what = "tdh_class_sums_dev"
    fM, _ = _tdh_frame(what, fM, 1)
    c, nm, L = _tdh_field(E, what, "E", fM)
    sums = _tdh_buf(sums, what, "sums", (nm, fM), np.float64, make=True)
    _lib.call("qh_tdh_class_sums_%s_dev" % c, E.ptr, nm, L, fM, sums.ptr)
    return sums


def tdh_align_dev(sums, fM1, M, shift=None):
    """The frame alignment of every row from its class sums, written to the int32 DeviceArray ``shift (nmodes,)`` (made when None): with ``H``
    the residues of the higher-order format - format 1 when ``M[0] > M[1]``, else format 2 - the first ``j`` at which the sum over ``r`` in ``H``
    of ``sums[m, (r + j) % fM]`` is strictly largest.  One small launch; nothing is read back - the split and the metrics take ``shift`` itself."""
    what = "tdh_align_dev"
    if not hasattr(sums, "ptr") or len(sums.shape) != 2 or np.dtype(sums.dtype) != np.float64:
        raise ValueError("%s: sums must be the float64 (nmodes, f_M) of tdh_class_sums_dev" % what)
    nm, fM = sums.shape
    fM, fM1 = _tdh_frame(what, fM, fM1)
    if not 1 <= nm <= 65535:
        raise ValueError("%s: 1 .. 65535 rows" % what)
    shift = _tdh_buf(shift, what, "shift", (nm,), np.int32, make=True)
    _lib.call("qh_tdh_align_dev", sums.ptr, nm, fM, fM1, int(M[0] > M[1]), shift.ptr)
    return shift


def tdh_split_dev(E, fM, fM1, powratio, part1, part2, shift=0):
    """Take the frame-aligned rows apart in one launch: ``part1[m, k] = E[m, (idx1[k] + shift) % L]`` and ``part2[m, k] = E[m, (idx2[k] + shift) %
    L] * sqrt(powratio)``, ``idx1`` / ``idx2`` the positions of the two formats - part 2 sits on its own unit-power alphabet again.  ``shift``:
    the int32 DeviceArray of :func:`tdh_align_dev` (one per row, never read back) or one whole number for every row.  The parts are DeviceArrays
    of E's dtype, ``(nmodes, nframes * fM1)`` and ``(nmodes, nframes * fM2)``, and must not be ``E``."""
    what = "tdh_split_dev"
    fM, fM1 = _tdh_frame(what, fM, fM1)
    powratio = _tdh_powratio(what, powratio)
    c, nm, L = _tdh_field(E, what, "E", fM)
    _tdh_buf(part1, what, "part1", (nm, L // fM * fM1), E.dtype)
    _tdh_buf(part2, what, "part2", (nm, L // fM * (fM - fM1)), E.dtype)
    if part1.ptr == E.ptr or part2.ptr == E.ptr:
        raise ValueError("%s: the parts must not be E (the gather is cyclic)" % what)
    sp, sh = _tdh_shift(what, shift, nm)
    _lib.call("qh_tdh_split_%s_dev" % c, E.ptr, nm, L, fM, fM1, powratio, sp, sh, part1.ptr, part2.ptr)
    return part1, part2


def tdh_metrics_dev(E, idx_tx, fM, fM1, powratio, alphabet1, alphabet2, shift=0, sums=None):
    """The hard metrics of hybrid rows in one fused pass: the float64 DeviceArray ``sums (nmodes, 8)`` (made when None) = ``(symbol errors, bit
    errors, symbols compared, sum |r - s_label|^2)`` of format 1, then of format 2, where ``r = E[m, (n + shift) % L]`` - times
    ``sqrt(powratio)`` in format 2 - is decided against the alphabet of position ``n`` and compared with ``idx_tx[m, n]``, the transmitted label
    into that alphabet (int32, E's shape, as :func:`tdh_assemble_dev` lays them out).  Bit errors are ``popcount(decision ^ label)``: the
    alphabets (1-d DeviceArrays of E's dtype, at most 1024 points) are in bit-label order.  Labels outside the alphabet are skipped.
    :func:`tdh_rates` turns the sums, read back, into SER, BER and EVM."""
    what = "tdh_metrics_dev"
    fM, fM1 = _tdh_frame(what, fM, fM1)
    powratio = _tdh_powratio(what, powratio)
    c, nm, L = _tdh_field(E, what, "E", fM)
    _tdh_buf(idx_tx, what, "idx_tx", (nm, L), np.int32)
    for a, name in ((alphabet1, "alphabet1"), (alphabet2, "alphabet2")):
        if not hasattr(a, "ptr") or len(a.shape) != 1 or not 1 <= a.shape[0] <= TDH_M_MAX:
            raise ValueError("%s: %s must be a 1-d DeviceArray of 1 .. %d points" % (what, name, TDH_M_MAX))
        if np.dtype(a.dtype) != np.dtype(E.dtype):
            raise ValueError("%s: %s must have E's dtype" % (what, name))
    sp, sh = _tdh_shift(what, shift, nm)
    sums = _tdh_buf(sums, what, "sums", (nm, 8), np.float64, make=True)
    _lib.call("qh_tdh_metrics_%s_dev" % c, E.ptr, nm, L, fM, fM1, powratio, sp, sh, idx_tx.ptr, alphabet1.ptr, alphabet1.shape[0], alphabet2.ptr,
              alphabet2.shape[0], sums.ptr)
    return sums


def tdh_rates(sums, M):
    """SER, BER and EVM per mode from the eight sums of the hybrid metrics (a host array ``(nmodes, 8)``): a dict of ``ser``, ``ber`` and ``evm``,
    each ``(per-format (nmodes, 2), combined (nmodes,))``, and ``counts``, the six integer counts ``(nmodes, 2, 3)``.  The combined BER is weighted
    by bits, ``(b1 + b2) / (n1 log2 M1 + n2 log2 M2)``; the EVM is the root of the mean squared error."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 2, 4)
    nbits = np.log2(np.asarray(M, dtype=np.float64))
    se, be, n, sq = (s[:, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        return dict(ser=(se / n, se.sum(axis=1) / n.sum(axis=1)), ber=(be / (n * nbits), be.sum(axis=1) / (n * nbits).sum(axis=1)),
                    evm=(np.sqrt(sq / n), np.sqrt(sq.sum(axis=1) / n.sum(axis=1))), counts=np.rint(s[:, :, :3]).astype(np.int64))


def tdh_align_host(E, fM, fM1, M):
    """The alignment rule in numpy: per row the first ``j < fM`` at which ``mean |E[(H + j) % L]|`` is strictly largest, ``H`` the positions of the
    higher-order format (format 1 when ``M[0] > M[1]``)."""
    E = np.atleast_2d(np.asarray(E))
    L = E.shape[1]
    n = np.arange(L)
    H = n[n % fM < fM1] if M[0] > M[1] else n[n % fM >= fM1]
    mag = np.abs(E)
    shifts = np.zeros(E.shape[0], dtype=np.int32)
    for m in range(E.shape[0]):
        top = -np.inf
        for j in range(fM):
            v = mag[m, (H + j) % L].mean()
            if v > top:
                top, shifts[m] = v, j
    return shifts


def tdh_divide(E, fr, M, powratio, method="pyt"):
    """Take host rows ``E (nmodes, L)`` of a received hybrid signal apart: ``(part1, part2, shifts)`` - every row aligned to its frame by the
    mean magnitude of the higher-order format's positions, then split, part 2 times ``sqrt(powratio)``.  ``method="pyt"``: numpy (the default);
    ``"hip"``: class sums, alignment and split on the device (complex64 / complex128), only the parts and the shifts come back.  ``L`` must be
    a multiple of the frame length."""
    if method not in ("pyt", "hip"):
        raise ValueError("method must be 'pyt' (host) or 'hip' (device), not %r" % (method,))
    fM, fM1, fM2 = tdh_geometry(fr)
    E = np.atleast_2d(np.asarray(E))
    nm, L = E.shape
    if L % fM or L < fM:
        raise ValueError("tdh_divide: a row of %d symbols does not hold whole frames of %d" % (L, fM))
    powratio = _tdh_powratio("tdh_divide", powratio)
    if method == "hip":
        _tdh_frame("tdh_divide", fM, fM1)
        dE = _lib.DeviceArray.from_host(np.ascontiguousarray(E, dtype=_lib.suffix(E.dtype)[2]))
        shift = tdh_align_dev(tdh_class_sums_dev(dE, fM), fM1, M)
        p1, p2 = _lib.DeviceArray((nm, L // fM * fM1), dE.dtype), _lib.DeviceArray((nm, L // fM * fM2), dE.dtype)
        tdh_split_dev(dE, fM, fM1, powratio, p1, p2, shift)
        return p1.to_host(), p2.to_host(), shift.to_host()
    shifts = tdh_align_host(E, fM, fM1, M)
    n = np.arange(L)
    idx1, idx2 = n[n % fM < fM1], n[n % fM >= fM1]
    part1 = np.array([E[m, (idx1 + shifts[m]) % L] for m in range(nm)])
    part2 = np.array([E[m, (idx2 + shifts[m]) % L] for m in range(nm)])
    root = np.sqrt(powratio)
    part2 = (part2.astype(np.complex128) * root).astype(E.dtype) if np.iscomplexobj(E) else part2 * root
    return part1, part2, shifts


# ------------------------------------------------------------------------------------------------ nonlinear fibre on a resident field
# Split-step Fourier propagation of the (Manakov) nonlinear Schroedinger equation and digital back-propagation; kernels in
# qampy_amd/csrc/fibre.hip, the model in include/qampy_hip.h and DESIGN.md 3.22.
FIBRE_MAX = 4096                       # most steps per span, most spans (csrc/fibre.hip FIB_MAX)
H_PLANCK = 6.62607015e-34              # J s
C_LIGHT = 2.99792458e8                 # m / s (core/filter.py)


def fibre_alpha(alpha_db_km):
    """Power loss in 1 / m of a loss in dB / km: ``alpha_db_km 1e-3 ln(10) / 10``."""
    return float(alpha_db_km) * 1e-3 * np.log(10) / 10


def ase_power(nf_db, alpha, span_length, fs, wl0=1550e-9):
    """Noise power in watts per mode that an amplifier of noise figure ``nf_db`` adds within the sampled band ``fs`` when it makes up the loss
    ``alpha`` (1 / m) of ``span_length`` metres: ``n_sp h (c / wl0) (G - 1) fs`` with ``n_sp = 10**(nf_db / 10) / 2`` and ``G = exp(alpha span_length)``."""
    n_sp = 10 ** (float(nf_db) / 10) / 2
    G = np.exp(float(alpha) * float(span_length))
    return float(n_sp * H_PLANCK * (C_LIGHT / float(wl0)) * (G - 1) * float(fs))


def _fibre_steps(steps, span_length):
    """The step lengths of one span as a list of floats: ``steps`` equal ones, or the given sequence, which must add up to the span."""
    span = float(span_length)
    if not (np.isfinite(span) and span > 0):
        raise ValueError("span_length must be finite and positive")
    if np.ndim(steps) == 0:
        if isinstance(steps, (bool, np.bool_)) or int(steps) != steps:
            raise ValueError("steps is a whole number of equal steps, or a sequence of step lengths")
        n = int(steps)
        if not 1 <= n <= FIBRE_MAX:
            raise ValueError("a span takes 1 to %d steps" % FIBRE_MAX)
        return [span / n] * n
    dz = [float(v) for v in np.asarray(steps, dtype=np.float64).ravel()]
    if not 1 <= len(dz) <= FIBRE_MAX:
        raise ValueError("a span takes 1 to %d steps" % FIBRE_MAX)
    if not all(np.isfinite(v) and v > 0 for v in dz):
        raise ValueError("every step length must be finite and positive")
    if abs(sum(dz) - span) > 1e-9 * span:
        raise ValueError("the steps add up to %r m, the span is %r m" % (sum(dz), span))
    return dz


def _fibre_spans(nspans):
    if isinstance(nspans, (bool, np.bool_)) or np.ndim(nspans) != 0 or int(nspans) != nspans or not 1 <= int(nspans) <= FIBRE_MAX:
        raise ValueError("nspans is a whole number from 1 to %d" % FIBRE_MAX)
    return int(nspans)


def fibre_plan(L, steps, nspans=1, span_length=1.0, power_dbm=None, backward=False):
    """What one call of :func:`ssfm_dev` / :func:`dbp_dev` launches on rows of ``L`` samples, as a dict: ``filters`` - whole-row spectral filters, a
    transform pair each, ``steps + 1`` per span; ``nonlinear`` - launches of the point-wise kernel, ``steps`` per span; ``tables`` - launches that
    form a dispersion table: two tables live on the device and the one used longest ago is formed again when a new length comes up, so equal
    steps form two per call and only a list of three or more different half-step sums forms more; ``power`` - launches that fix ``pscale`` (2 when it
    is derived from ``power_dbm``, else 1).  ``steps``, ``span_length``: as the propagation takes them (the counts of equal steps do not depend on the
    span)."""
    fft_plan(L)
    dz = _fibre_steps(steps, span_length)
    nspans = _fibre_spans(nspans)
    if backward:
        dz = dz[::-1]
    n = len(dz)
    held, last, tables = [None, None], 1, 0
    for _ in range(nspans):
        for h in [dz[0] / 2] + [dz[i] / 2 + (dz[i + 1] / 2 if i + 1 < n else 0.0) for i in range(n)]:
            if h in held:
                last = held.index(h)
                continue
            last = 0 if held[0] is None else (1 if held[1] is None else 1 - last)
            held[last] = h
            tables += 1
    return dict(filters=nspans * (n + 1), nonlinear=nspans * n, tables=tables, power=2 if power_dbm is not None else 1)


def _fibre_call(what, E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, backward, ase_w=0.0, seed=0):
    from .filter import beta2
    c = _impair_field(E, what)
    _same_as(E, out, what)
    if E.shape[0] not in (1, 2):
        raise ValueError("%s: one row, or two (Manakov), not %d" % (what, E.shape[0]))
    fft_plan(E.shape[1])
    dz = _fibre_steps(steps, span_length)
    nspans = _fibre_spans(nspans)
    if (power_dbm is None) == (pscale is None):
        raise ValueError("%s: give exactly one of power_dbm (the launch power over all rows) and pscale (watts per unit of |E|**2)" % what)
    mode, power = (1, 1e-3 * 10 ** (float(power_dbm) / 10)) if pscale is None else (0, float(pscale))
    fs, gamma, alpha, b2 = float(fs), float(gamma), fibre_alpha(alpha_db_km), float(beta2(float(D), float(wl0)))
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("%s: fs must be finite and positive" % what)
    if not all(np.isfinite(v) for v in (gamma, alpha, b2)):
        raise ValueError("%s: D, wl0, gamma and alpha_db_km must be finite" % what)
    if not (np.isfinite(power) and power > 0):
        raise ValueError("%s: the power must be finite and positive" % what)
    if not (np.isfinite(ase_w) and ase_w >= 0):
        raise ValueError("%s: the amplifier noise power must be finite and not negative" % what)
    if abs(alpha) * sum(dz) > 709:                                           # exp overflows in double
        raise ValueError("%s: the loss of a span overflows" % what)
    arr = (_lib.C.c_double * len(dz))(*dz)
    _lib.call("qh_fibre_ssfm_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], fs, b2, gamma, alpha, arr, len(dz), nspans, int(backward), int(bool(amplify)), mode,
              power, float(ase_w), _seed64(seed), out.ptr)
    return out


def fibre_nl_dev(E, out, a, coef, pscale, sigma_w=0.0, seed=0):
    """The nonlinear step of :func:`ssfm_dev` on its own, one launch: ``out[m, n] = a exp(1j coef pscale[0] P[n]) E[m, n]`` with
    ``P[n] = sum_m |E[m, n]|**2``, plus - ``sigma_w > 0`` - noise of standard deviation ``sigma_w / sqrt(pscale[0])`` drawn under ``seed``.
    ``pscale``: a float64 DeviceArray of one value.  One or two rows of 1 to 2**24 samples; ``out`` may be ``E``."""
    c = _impair_field(E, "fibre_nl_dev")
    _same_as(E, out, "fibre_nl_dev")
    if E.shape[0] not in (1, 2) or not 1 <= E.shape[1] <= 1 << 24:
        raise ValueError("fibre_nl_dev: one or two rows of 1 to 2**24 samples")
    if np.dtype(pscale.dtype) != np.float64 or int(np.prod(pscale.shape)) != 1:
        raise ValueError("fibre_nl_dev: pscale is a float64 DeviceArray of one value")
    a, coef, sigma_w = float(a), float(coef), float(sigma_w)
    if not (np.isfinite(a) and np.isfinite(coef) and np.isfinite(sigma_w) and sigma_w >= 0):
        raise ValueError("fibre_nl_dev: a and coef must be finite, sigma_w finite and not negative")
    _lib.call("qh_fibre_nl_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], a, coef, pscale.ptr, sigma_w, _seed64(seed), out.ptr)
    return out


def ssfm_dev(E, out, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, nf_db=None,
             wl0=1550e-9, seed=0):
    """
    Propagate the (nmodes, L) complex DeviceArray ``E`` (one row, or two: Manakov with 8 / 9) through ``nspans`` identical spans of ``span_length``
    metres by the symmetric split-step Fourier method, into ``out`` (same shape and dtype; it may be ``E``).  ``fs``: sampling rate; ``D``:
    dispersion in s / m / m at ``wl0`` (``beta2`` as ``add_dispersion`` forms it); ``gamma`` in 1 / (W m); ``alpha_db_km`` in dB / km; ``steps``: the
    number of equal steps of a span, or a sequence of step lengths that add up to the span within 1e-9 relative.

    A span is ``D(dz[0] / 2)``, then for every step ``N(dz[i])`` and ``D(dz[i] / 2 + dz[i + 1] / 2)`` (the last ``D(dz[-1] / 2)``), with::

        D(h):  row <- ifft(exp(-0.5j (2 pi f)**2 beta2 h) fft(row)),  f = fftfreq(L, 1 / fs), the phase formed and reduced in double
        N(h):  E[m, n] <- exp(-alpha h / 2) exp(1j kappa gamma pscale h_eff sum_m |E[m, n]|**2) E[m, n],  h_eff = (1 - exp(-alpha h)) / alpha

    ``amplify``: the last ``N`` of a span also multiplies by ``exp(alpha span_length / 2)``, so the power at the end of a span is the launch power.
    ``nf_db``: that amplifier's noise figure - the launch adds white noise of :func:`ase_power` watts per mode, a function of ``seed + s`` for
    span ``s`` (the unit draws of :func:`impair_pointwise_dev`).  The field keeps its normalisation: exactly one of ``pscale`` - watts per unit
    of ``|E|**2`` - and ``power_dbm`` - the launch power over all rows, from which ``pscale = P / sum_m mean_n |E[m, n]|**2`` is formed on the
    device - says what it means in watts.  Every check raises before a launch; the whole loop is enqueued on the current library stream, nothing
    is read back, and a repeated call is bit-identical.  :func:`fibre_plan` counts the launches.
    """
    ase = 0.0
    if nf_db is not None:
        if not np.isfinite(float(nf_db)):
            raise ValueError("ssfm_dev: nf_db must be finite")
        ase = ase_power(nf_db, fibre_alpha(alpha_db_km), span_length, fs, wl0)
    return _fibre_call("ssfm_dev", E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, False, ase, seed)


def dbp_dev(E, out, fs, D, span_length, nspans=1, gamma=1.3e-3, alpha_db_km=0.2, steps=8, power_dbm=None, pscale=None, amplify=True, wl0=1550e-9, **kw):
    """
    Digital back-propagation: the algebraic inverse of the noise-free :func:`ssfm_dev` with the same arguments - the steps walked in reverse with
    ``beta2``, ``gamma`` and ``alpha`` negated, and with ``amplify`` the factor ``exp(-alpha span_length / 2)`` in front of the first nonlinear step
    of a span, before its power is taken.  With fewer steps than the link, or a scaled ``gamma``, it is the usual practical back-propagation.
    ``power_dbm`` is then the power of the field as it arrives, which with ``amplify`` is the launch power.  It adds no noise: ``nf_db`` raises
    ValueError.
    """
    if "nf_db" in kw:
        if kw.pop("nf_db") is not None:
            raise ValueError("dbp_dev: back-propagation adds no amplifier noise (nf_db)")
    if kw:
        raise TypeError("dbp_dev: unexpected arguments %s" % sorted(kw))
    return _fibre_call("dbp_dev", E, out, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, pscale, amplify, wl0, True)
