"""Digital pre-distortion and compensation of transceiver impairments on plain ndarrays (qampy/core/digital_pre_compensation.py), through the
GPU's kernels (csrc/precomp.hip, :mod:`qampy_amd.core.hip_dsp`): host arrays up, the reference's shapes and dtypes back.  There is no host
fallback.  A loop that stays in device memory uses the ``*_dev`` forms of ``hip_dsp`` instead.

``cal_lut`` follows the reference as it runs compiled (or under ``python -O``): its pure-Python table average asserts that the index arrays
are longer than the error array, which the arrays ``cal_lut`` hands over never are."""
import numpy as np

from . import hip_dsp as _dsp
from .impairments import _on_device, _rows, clipper         # noqa: F401  (clipper: the reference keeps it in this module)


def comp_mod_sin(sig, vpi=1.14):
    """Undo the modulator's sine: ``2 vpi.real arcsin(sig.real) + 1j 2 vpi.imag arcsin(sig.imag)``; a ``vpi`` that is not complex serves both
    rails.  NaN in a rail whose input lies outside [-1, 1], as numpy gives.  complex64 and complex128 keep their dtype."""
    _dsp.precomp._vpi_rails(vpi)
    return _on_device(sig, lambda E, out: _dsp.comp_mod_sin_dev(E, out, vpi=vpi))


def comp_dac_resp(dpe_fb, sim_len, rrc_beta, PAPR=9, prms_dac=(16e9, 2, 'sos', 6), os=2):
    """The pre-emphasis filter ``p_f`` (``sim_len`` bins in ``fftfreq`` order, complex128) against the response of a simulated DAC - a digital
    Bessel low-pass ``prms_dac = (cutoff, order, 'sos', enob)`` - for a root-raised-cosine signal of roll-off ``rrc_beta`` at the symbol rate
    ``dpe_fb`` and ``os`` samples per symbol.  Only the ``'sos'`` format is taken."""
    return _dsp.comp_dac_resp_dev(dpe_fb, sim_len, rrc_beta, PAPR=PAPR, prms_dac=prms_dac, os=os, dtype=np.complex128).to_host()


def _signal_1d(a, name):
    a = np.asarray(a)
    if a.ndim != 1 or a.size < 1:
        raise ValueError("%s must be a non-empty 1-d array (loop over the modes)" % name)
    return a


def find_sym_patterns(sig, ref_sym, N, ret_ptrns=False):
    """Index of the pattern of ``N`` elements of ``ref_sym`` that starts at every element of the 1-d ``sig`` (the signal wraps at its end):
    ``sum_j lev[(i + j) % L] M**(N - 1 - j)`` with ``lev = argmin |sig - ref_sym|``, int64.  ``ret_ptrns``: also the ``(M**N, N)`` array of the
    patterns themselves."""
    from .. import _lib
    sig, ref = _signal_1d(sig, "sig"), _signal_1d(ref_sym, "ref_sym")
    rails = not np.iscomplexobj(sig) and not np.iscomplexobj(ref) and ref.size >= 2 and bool(np.all(np.diff(ref.astype(np.float64)) > 0))
    levels = _dsp.PatternLevels(ref, ref) if rails else _dsp.PatternLevels(alphabet=ref)       # (an unsorted table is scanned in its own order)
    levels.N(N)
    x = sig if sig.dtype in (np.complex64, np.complex128) else sig.astype(np.complex64 if sig.dtype == np.float32 else np.complex128)
    E = _lib.DeviceArray.from_host(x.reshape(1, -1))
    idx, _ = _dsp.pattern_index_dev(E, levels, N, idx_I=_lib.DeviceArray(E.shape, np.int32))
    pattern_idx = np.roll(idx.to_host()[0].astype(np.int64), -(int(N) // 2))              # the device numbers the CENTRED window
    if ret_ptrns:
        M = ref.size
        return pattern_idx, ref[np.array(np.unravel_index(np.arange(M ** int(N)), int(N) * [M])).T]
    return pattern_idx


def cal_lut(tx_sig, rx_sig, ref_sym, mem_len=3, idx_data=None, real_ptrns=True):
    """The look-up table of the average error ``tx_sig - rx_sig`` per pattern of ``mem_len`` symbols around every symbol, a simplified Volterra
    filter; 1-d signals only.  ``idx_data``: a boolean mask of the symbols to use (default all).  ``real_ptrns``: in-phase and quadrature
    patterns on their own (``M**mem_len`` entries, ``M`` the number of in-phase levels) instead of complex patterns.  Returns ``(ea, idx_I,
    idx_Q)``: the complex128 table and the int64 pattern numbers of the used symbols."""
    from .. import _lib
    tx, rx = _signal_1d(tx_sig, "tx_sig"), np.asarray(rx_sig)
    if rx.shape != tx.shape:
        raise ValueError("Tx and Rx signal need to have the same shape")
    ref = _signal_1d(ref_sym, "ref_sym")
    levels = _dsp.pattern_levels(ref, real_ptrns)
    N = levels.N(mem_len)
    if not real_ptrns:
        N = ref.size ** int(mem_len)                                                       # (the reference sizes the table by ref_sym itself)
        if N > _dsp.PRECOMP_N_MAX:
            raise ValueError("ref_sym.size**mem_len exceeds the largest table, 2**24 entries")
    mask = None
    if idx_data is not None:
        mask = np.asarray(idx_data)
        if mask.shape != tx.shape:
            raise ValueError("idx_data must be a mask with one entry per symbol")
        mask = mask.astype(bool)
    ct = np.complex64 if tx.dtype == rx.dtype == np.complex64 else np.complex128          # tx - rx in the wider of the two, as numpy forms it
    D = _lib.DeviceArray
    dtx, drx = D.from_host(np.ascontiguousarray(tx, dtype=ct).reshape(1, -1)), D.from_host(np.ascontiguousarray(rx, dtype=ct).reshape(1, -1))
    dmask = None if mask is None else D.from_host(mask.astype(np.uint8))
    idx_I, idx_Q = _dsp.pattern_index_dev(dtx, levels, mem_len)
    ea, _, _ = _dsp.lut_accumulate_dev(dtx, drx, idx_I, idx_Q, N, idx_data=dmask)
    sel = slice(None) if mask is None else np.flatnonzero(mask)
    return ea.to_host()[0], idx_I.to_host()[0].astype(np.int64)[sel], idx_Q.to_host()[0].astype(np.int64)[sel]


def apply_lut(sig, ea, idx_I, idx_Q, gain=1.0):
    """``sig + gain (ea[idx_I].real + 1j ea[idx_Q].imag)``: what the users of ``cal_lut`` write by hand.  ``sig`` 1-d with a 1-d table, or
    ``(nmodes, L)`` with an ``(nmodes, N)`` table; ``idx_I`` and ``idx_Q`` of sig's shape.  complex64 and complex128 keep their dtype."""
    from .. import _lib
    X, one = _rows(sig)
    T = np.ascontiguousarray(np.atleast_2d(np.asarray(ea)), dtype=np.complex128)
    a, b = np.atleast_2d(np.asarray(idx_I)), np.atleast_2d(np.asarray(idx_Q))
    if X.size == 0 or T.ndim != 2 or T.shape[0] != X.shape[0] or T.shape[1] < 1:
        raise ValueError("sig (L,) with ea (N,), or sig (nmodes, L) with ea (nmodes, N)")
    if a.shape != X.shape or b.shape != X.shape or not (np.issubdtype(a.dtype, np.integer) and np.issubdtype(b.dtype, np.integer)):
        raise ValueError("idx_I and idx_Q hold one whole number per sample of sig")
    if min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= T.shape[1]:
        raise ValueError("a pattern number lies outside the table")
    _dsp.precomp._precomp_gain(gain, "apply_lut")
    D = _lib.DeviceArray
    E = D.from_host(X)
    _dsp.lut_apply_dev(E, D.from_host(T), D.from_host(a.astype(np.int32)), D.from_host(b.astype(np.int32)), E, gain=gain)
    res = E.to_host()
    return res[0] if one else res
