"""Frequency offset: its removal (qampy/core/phaserecovery.py:435-473) and the blind estimate; kernels in qampy_amd/csrc/foe.hip."""
import numpy as np

from ... import _lib
from ._args import buffer, resident, same_as


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
    c = resident(E, "comp_freq_offset_dev")
    same_as(E, out, "comp_freq_offset_dev")
    buffer(fo, "comp_freq_offset_dev", "fo", (E.shape[0],), np.float64, by_size=True)
    _lib.call("qh_comp_freq_offset_%s_dev" % c, E.ptr, E.shape[0], E.shape[1], fo.ptr, int(os), out.ptr)


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
    what = "find_freq_offset_dev"
    c = resident(E, what)
    nm, L = E.shape
    N, B = foe_plan(L, fft_size, blocks)
    os = _foe_os(os)
    buffer(fo, what, "fo", (nm,), np.float64, by_size=True)
    buffer(stats, what, "stats", (nm, 3), np.float64, optional=True)
    buffer(spectrum, what, "spectrum", (nm, N), _lib.suffix(E.dtype)[1], optional=True)
    _lib.call("qh_find_freq_offset_%s_dev" % c, E.ptr, nm, L, os, N, B, int(bool(average_over_modes)), fo.ptr,
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
