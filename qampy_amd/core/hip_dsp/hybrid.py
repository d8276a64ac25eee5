"""
Time-domain hybrid QAM: csrc/hybrid.hip on DeviceArrays, TDHQAMSymbols (qampy/signals.py:1182-1427) built, taken apart and measured on
resident rows.  A frame of ``fM`` symbols holds ``fM1`` symbols of format 1 followed by ``fM2`` of format 2; format-2 symbols are stored
divided by ``sqrt(powratio)``.  The reference's own split and metrics raise; DESIGN.md 3.21 fixes what they mean here.
"""
import numpy as np

from ... import _lib
from ._args import buffer, field

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
    c, nm, L = field(E, what, name, max_rows=65535, max_len=TDH_ROW_MAX)
    if L % fM:
        raise ValueError("%s: a row of %d symbols does not hold whole frames of %d (the cyclic shift is only meaningful on whole frames)" % (what, L, fM))
    return c, nm, L


def _tdh_shift(what, shift, nm):
    """``(device pointer or None, host value)`` of a shift given as an int32 DeviceArray ``(nmodes,)`` or as one whole number."""
    if hasattr(shift, "ptr"):
        buffer(shift, what, "shift", (nm,), np.int32)
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
        buffer(a, what, name, (nm, nframes * n), out.dtype)
    given = [a is not None for a in (labels1, labels2, idx_out)]
    if any(given) and not all(given):
        raise ValueError("%s: labels1, labels2 and idx_out come together" % what)
    if all(given):
        buffer(labels1, what, "labels1", part1.shape, np.int32)
        buffer(labels2, what, "labels2", part2.shape, np.int32)
        buffer(idx_out, what, "idx_out", out.shape, np.int32)
    _lib.call("qh_tdh_assemble_%s_dev" % c, part1.ptr, part2.ptr, labels1.ptr if all(given) else None, labels2.ptr if all(given) else None, nm, nframes,
              fM, fM1, powratio, out.ptr, idx_out.ptr if all(given) else None)
    return out


def tdh_class_sums_dev(E, fM, sums=None):
    """``sums[m, r] = sum |E[m, n]|`` over ``n % fM == r`` into the float64 DeviceArray ``sums (nmodes, fM)`` (made when None).  Terms and sums
    in double, in a fixed order without atomics: two calls give the same bits.  Nothing is read back."""
    what = "tdh_class_sums_dev"
    fM, _ = _tdh_frame(what, fM, 1)
    c, nm, L = _tdh_field(E, what, "E", fM)
    sums = buffer(sums, what, "sums", (nm, fM), np.float64, make=True)
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
    shift = buffer(shift, what, "shift", (nm,), np.int32, make=True)
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
    buffer(part1, what, "part1", (nm, L // fM * fM1), E.dtype)
    buffer(part2, what, "part2", (nm, L // fM * (fM - fM1)), E.dtype)
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
    buffer(idx_tx, what, "idx_tx", (nm, L), np.int32)
    for a, name in ((alphabet1, "alphabet1"), (alphabet2, "alphabet2")):
        if not hasattr(a, "ptr") or len(a.shape) != 1 or not 1 <= a.shape[0] <= TDH_M_MAX:
            raise ValueError("%s: %s must be a 1-d DeviceArray of 1 .. %d points" % (what, name, TDH_M_MAX))
        if np.dtype(a.dtype) != np.dtype(E.dtype):
            raise ValueError("%s: %s must have E's dtype" % (what, name))
    sp, sh = _tdh_shift(what, shift, nm)
    sums = buffer(sums, what, "sums", (nm, 8), np.float64, make=True)
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
