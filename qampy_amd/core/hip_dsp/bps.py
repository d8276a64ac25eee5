"""
Drop-in for the BPS entry points of the compiled module ``qampy.core.pythran_dsp`` on MI355X.

``bps`` and ``select_angles`` keep the signatures of the ``#pythran export`` lines qampy/core/pythran_dsp.py:45-46 and
:133-136; the kernels live in qampy_amd/csrc/bps.hip.
"""
import numpy as np

from ... import _lib


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
