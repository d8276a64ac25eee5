"""
Pilot frames: csrc/pilot.hip on DeviceArrays, for SignalWithPilots' frame (qampy/signals.py:1494-1545), get_data / extract_pilots
(:1753-1804), pilot_based_cpe_new and pilot_based_foe (qampy/core/pilotbased_receiver.py:258-327, :32-73) and find_pilot_const_phase
(qampy/phaserec.py:194-218).  A frame of ``F`` symbols is ``S`` pilots (the sequence) followed by payload with one phase pilot every
``R`` symbols, the first at position ``S`` (``R`` 0 or None: the sequence only); the kernels compute this rule, they read no index table.
"""
import threading

import numpy as np

from ... import _lib
from ._args import buffer, field, thread_table

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
    """``c`` of a non-empty 2-d complex DeviceArray of at most 65535 rows of ``PILOT_ROW_MAX`` symbols."""
    return field(a, what, name, rows=rows, like=dtype, max_rows=65535, max_len=PILOT_ROW_MAX)[0]


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
    buffer(frame, what, "frame", (nm, nframes * F), frame.dtype)
    buffer(pilots, what, "pilots", (nm, NP), frame.dtype)
    pay = (nm, ND if repeat_data else nframes * ND)
    buffer(payload, what, "payload", pay, frame.dtype)
    if (labels is None) != (idx_frame is None):
        raise ValueError("%s: labels and idx_frame come together" % what)
    if labels is not None:
        buffer(labels, what, "labels", pay, np.int32)
        buffer(idx_frame, what, "idx_frame", (nm, nframes * F), np.int32)
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
    return thread_table(_PILOT_TABLES, (arr.dtype.str, arr.tobytes()), lambda: _lib.DeviceArray.from_host(arr), keep=PILOT_TABLES_KEPT)


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
        buffer(payload, what, "payload", (nm, fr.size * ND), E.dtype)
    if pilots is not None:
        if NP < 1:
            raise ValueError("%s: this frame has no pilots" % what)
        buffer(pilots, what, "pilots", (nm, fr.size * NP), E.dtype)
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
    buffer(phase, what, "phase", (nm, n), np.float64)
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
    buffer(knot_phase, what, "knot_phase", (nm, n - N + 1), np.float64)
    table, npf = None, 1
    if knot_pos is not None:
        buffer(knot_pos, what, "knot_pos", (n - N + 1,), np.int64)
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
    buffer(Eout, what, "Eout", (nm, span), E.dtype)
    buffer(trace, what, "trace", (nm, span), rt)
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
    buffer(fit, what, "fit", (nm, 2), np.float64)
    buffer(fo, what, "fo", (nm,), np.float64, by_size=True)
    _lib.call("qh_pilot_foe_%s_dev" % c, rec.ptr, ref.ptr, nm, n, int(bool(average)), fit.ptr, fo.ptr)
    return fo


def pilot_const_phase_dev(rec, ref, phase):
    """``phase (nmodes,)`` float64: the mean of the unwrapped phase of ``rec`` against ``ref`` per mode (``find_pilot_const_phase``)."""
    what = "pilot_const_phase_dev"
    c = _pilot_pair(what, rec, ref, 1)
    nm, n = rec.shape
    buffer(phase, what, "phase", (nm,), np.float64, by_size=True)
    _lib.call("qh_pilot_const_phase_%s_dev" % c, rec.ptr, ref.ptr, nm, n, phase.ptr)
    return phase


def rotate_rows_dev(E, phi, out):
    """``out[m] = E[m] * exp(-1j * phi[m])`` with ``phi (nmodes,)`` float64 read from HBM (``correct_pilot_const_phase``); ``out`` may be ``E``."""
    what = "rotate_rows_dev"
    c = _pilot_field(E, what, "E")
    buffer(out, what, "out", E.shape, E.dtype)
    buffer(phi, what, "phi", (E.shape[0],), np.float64, by_size=True)
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
    return thread_table(_PILOT_STAGING, key, lambda: tuple(_lib.DeviceArray(shape, dtype) for shape, dtype in bufs), keep=1)     # (the old set is released first)


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
