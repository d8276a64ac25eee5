"""Digital pre-compensation: qampy/core/digital_pre_compensation.py on DeviceArrays; kernels in qampy_amd/csrc/precomp.hip."""
import numpy as np

from ... import _lib
from ._args import buffer, field, resident, same_as
from .frontend import fft_plan, spectral_filter_dev
from .txresp import design_lowpass_sos

PRECOMP_MEM_MAX = 15               # longest pattern
PRECOMP_M_MAX = 4096               # most levels of a rail, most points of a complex alphabet
PRECOMP_N_MAX = 2 ** 24            # largest table, M**mem_len
PRECOMP_LDS_N = 2048               # largest table a workgroup accumulates privately in LDS (csrc/precomp.hip PC_LDS_N)
PRECOMP_LUT_LMAX = 2 ** 24         # longest row of the table's accumulation: 37 bits per sample are left below the largest error
PRECOMP_ROW_MAX = 2 ** 40          # most symbols of a row
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


def _precomp_field(a, what, name):
    """``c`` of a non-empty 2-d complex DeviceArray of at most 65535 rows of ``PRECOMP_ROW_MAX`` symbols."""
    return field(a, what, name, max_rows=65535, max_len=PRECOMP_ROW_MAX)[0]


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
    c = _precomp_field(E, what, "E")
    lv = _precomp_levels(levels, what)
    lv.N(mem_len)
    if idx_I is None and idx_Q is None:
        idx_I, idx_Q = _lib.DeviceArray(E.shape, np.int32), _lib.DeviceArray(E.shape, np.int32)
    for name, a in (("idx_I", idx_I), ("idx_Q", idx_Q)):
        buffer(a, what, name, E.shape, np.int32, optional=True)
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
    c = _precomp_field(tx, what, "tx")
    buffer(rx, what, "rx", tx.shape, tx.dtype)
    nm, L = tx.shape
    if L > PRECOMP_LUT_LMAX:
        raise ValueError("%s: a row of at most 2**24 symbols (split a longer capture and merge the tables by their counts)" % what)
    if isinstance(N, bool) or int(N) != N or not 1 <= int(N) <= PRECOMP_N_MAX:
        raise ValueError("%s: N must be a whole number from 1 to 2**24" % what)
    N = int(N)
    buffer(idx_I, what, "idx_I", tx.shape, np.int32)
    buffer(idx_Q, what, "idx_Q", tx.shape, np.int32)
    rows = 0
    if idx_data is not None:
        if np.dtype(idx_data.dtype) != np.uint8 or tuple(idx_data.shape) not in ((L,), (nm, L)):
            raise ValueError("%s: idx_data must be a uint8 DeviceArray of shape (L,) or (nmodes, L)" % what)
        rows = 1 if len(idx_data.shape) == 1 else nm
    for name, a, dt in (("ea", ea, np.complex128), ("nI", nI, np.int32), ("nQ", nQ, np.int32)):
        buffer(a, what, name, (nm, N), dt, optional=True)
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
    _precomp_field(tx, what, "tx")
    buffer(rx, what, "rx", tx.shape, tx.dtype)
    N = _precomp_levels(levels, what).N(mem_len)
    if tx.shape[1] > PRECOMP_LUT_LMAX:
        raise ValueError("%s: a row of at most 2**24 symbols (split a longer capture and merge the tables by their counts)" % what)
    for name, a, shape, dt in (("idx_I", idx_I, tx.shape, np.int32), ("idx_Q", idx_Q, tx.shape, np.int32), ("ea", ea, (tx.shape[0], N), np.complex128),
                               ("nI", nI, (tx.shape[0], N), np.int32), ("nQ", nQ, (tx.shape[0], N), np.int32)):
        buffer(a, what, name, shape, dt, optional=True)
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
    c = _precomp_field(sig, what, "sig")
    buffer(out, what, "out", sig.shape, sig.dtype)
    N = _precomp_table(ea, what, sig.shape[0])
    buffer(idx_I, what, "idx_I", sig.shape, np.int32)
    buffer(idx_Q, what, "idx_Q", sig.shape, np.int32)
    gain = _precomp_gain(gain, what)
    _lib.call("qh_lut_apply_%s_dev" % c, sig.ptr, sig.shape[0], sig.shape[1], ea.ptr, N, idx_I.ptr, idx_Q.ptr, gain, out.ptr)
    return out


def lut_predistort_dev(sig, levels, mem_len, ea, out, gain=1.0):
    """:func:`pattern_index_dev` of ``sig`` and :func:`lut_apply_dev` in one launch: the pattern numbers are formed on the fly and no index row is
    written.  ``ea (nmodes, levels.N(mem_len))``; ``out`` must be another buffer than ``sig``, because a symbol's window reads its neighbours."""
    what = "lut_predistort_dev"
    c = _precomp_field(sig, what, "sig")
    buffer(out, what, "out", sig.shape, sig.dtype)
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
    c = _precomp_field(E, what, "E")
    buffer(out, what, "out", E.shape, E.dtype)
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
    out = buffer(out, "comp_dac_resp_dev", "out", (int(sim_len),), ct, make=True)
    _lib.call("qh_dac_preemphasis_table_%s_dev" % _lib.cname(suf), int(sim_len), fb, fs, beta, noise, _lib.ptr(sos), sos.shape[0], out.ptr)
    return out


def dac_preemphasis_dev(E, out, dpe_fb, rrc_beta, PAPR=9, prms_dac=(16e9, 2, "sos", 6), os=2, table=None):
    """``ifft(p_f * fft(E))`` of every row of the (nmodes, L) complex DeviceArray ``E``, ``p_f = comp_dac_resp(dpe_fb, L, rrc_beta, ...)``:
    :func:`comp_dac_resp_dev` into ``table`` (an ``(L,)`` DeviceArray of E's dtype; made when None), then :func:`spectral_filter_dev`.  ``out``
    may be ``E``."""
    resident(E, "dac_preemphasis_dev")
    same_as(E, out, "dac_preemphasis_dev")
    fft_plan(E.shape[1])
    table = comp_dac_resp_dev(dpe_fb, E.shape[1], rrc_beta, PAPR=PAPR, prms_dac=prms_dac, os=os, dtype=E.dtype, out=table)
    return spectral_filter_dev(E, out, table)
