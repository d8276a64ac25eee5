"""
Extended-precision numpy restatement of the butterfly FIR (qampy_amd/csrc/apply.hip, pythran_equalisation.py:33-76), the real stacking the host
layer puts around it for real-valued taps (qampy_amd/core/equalisation/equalisation.py apply_filter), and the launch plan of a call
(qh_apply_plan).

    N = max((L - ntaps + 1) // os, 0)
    out[j, i] = sum_k sum_t E[k, i os + t] wx[modes[j], k, t],   i < N            (no conjugate; modes=None: every row of wx)

Complex inputs accumulate in np.clongdouble, real inputs in np.longdouble; the result keeps that type.
"""
import ctypes as C

import numpy as np


def n_out(L, ntaps, os):
    return max((L - ntaps + 1) // os, 0)


def apply_filter(E, os, wx, modes=None):
    E, wx = np.asarray(E), np.asarray(wx)
    acc = np.clongdouble if np.iscomplexobj(E) or np.iscomplexobj(wx) else np.longdouble
    rows = np.arange(wx.shape[0]) if modes is None else np.atleast_1d(modes).astype(np.int64)
    nmodes, L = E.shape
    ntaps = wx.shape[-1]
    N = n_out(L, ntaps, os)
    if N == 0:
        return np.zeros((rows.size, 0), acc)
    win = np.lib.stride_tricks.sliding_window_view(E.astype(acc), ntaps, axis=1)[:, ::os][:, :N]       # (nmodes, N, ntaps), a view
    return np.einsum("kit,jkt->ji", win, wx[rows].astype(acc))


def stack_real(E):
    """``[Re(mode 0..n-1); Im(mode 0..n-1)]``: the field as the real-valued taps see it."""
    return np.ascontiguousarray(np.vstack([E.real, E.imag]))


def unstack_real(out):
    """Back from the stacking: the first half of the rows are real parts, the second half imaginary parts."""
    n = out.shape[0] // 2
    return out[:n] + 1j * out[n:]


def rel_max(got, want):
    """The project's bar: max-abs error over the rms of the expected output."""
    want = np.asarray(want)
    return float(np.abs(got - want).max() / np.sqrt(np.mean(np.abs(want) ** 2)))


def plan(dtype, nmodes, os, ntaps, nsel):
    """``qh_apply_plan`` for arrays of ``dtype``: dict(per_thread, tile, lds, grid_y), or None where the launch's argument check refuses the
    sizes (QH_ERR_ARG).  No device needed."""
    from qampy_amd import _lib
    dtype = np.dtype(dtype)
    p, t, lds, gy = C.c_int(-1), C.c_int(-1), C.c_int64(-1), C.c_int(-1)
    rc = _lib.load().qh_apply_plan(int(dtype.kind == "c"), dtype.itemsize // (2 if dtype.kind == "c" else 1), nmodes, os, ntaps, nsel,
                                   C.byref(p), C.byref(t), C.byref(lds), C.byref(gy))
    if rc == _lib.QH_ERR_ARG:
        assert (p.value, t.value, lds.value, gy.value) == (-1, -1, -1, -1)          # a refused plan writes nothing
        return None
    assert rc == _lib.QH_OK, rc
    return dict(per_thread=p.value, tile=t.value, lds=lds.value, grid_y=gy.value)


def largest_ntaps(dtype, nmodes, os, nsel):
    """The largest tap count the argument check accepts for these sizes, found by bisection on ``plan`` (acceptance is monotone in ntaps)."""
    lo, hi = 1, 1 << 20
    assert plan(dtype, nmodes, os, lo, nsel) is not None and plan(dtype, nmodes, os, hi, nsel) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(dtype, nmodes, os, mid, nsel) is None:
            hi = mid
        else:
            lo = mid
    return lo
