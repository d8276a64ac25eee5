"""
Device-resident receiver: dual-mode equalisation + filter application + blind phase search without leaving HBM.

The reference chains ``dual_mode_equalisation`` (qampy/core/equalisation/equalisation.py:400-466) and ``bps``
(qampy/core/phaserecovery.py:93-159) through host ndarrays; on MI355X the capture, the taps, the error traces and the
recovered symbols stay in HBM between the stages (SURVEY.md §8b "optional persistent device buffers") and every stage is
one or a few kernel launches on the library stream.  Host-side logic (constants, tap initialisation, default training
length) is shared with :mod:`qampy_amd.core.equalisation.equalisation`, so both paths take identical decisions.

Layout in HBM (complex64 for the headline configs):
    E        (nmodes, L)            capture, 2 samples/symbol, row-major (coalesced along time)
    wxy      (nmodes, nmodes, Nt)   taps (1312 B at 2x2x41)
    err1/2   (nmodes, TrSyms*Niter) error traces of the two stages
    eq       (nmodes, N)            equalised, decimated signal, N = (L - Nt + 1)//os
    idx, ph, out (nmodes, N)        BPS index, applied phase, phase-recovered symbols
"""
import os as _os

import numpy as np

from . import _lib
from ._lib import DeviceArray
from .core.equalisation import equalisation as _host
from .core.equalisation import hip_equalisation as _k
from .core import hip_dsp as _dsp


# Tier b holds EVERY stage to the same tolerance (library default 1e-3, estimated rms deviation of the equaliser output from
# the sequential recurrence): what a seeding stage leaves in the weakly excited tap directions is handed to the next stage
# undamped, so a looser first stage would show up one-to-one in the result (round 2 used 0.06 there).


def _blind_metrics(rows, M, block, ws):
    """The blind estimators of hip_dsp on the rows of one DeviceArray: what ``blind_metrics`` of a receiver and of a bank return.  ``ws``: the
    caller's dict of work buffers, made again when the shape or the block changes."""
    nrows, N = rows.shape
    block, nblocks = _dsp.blind._blind_block("blind_metrics", block, N)
    key = (nrows, N, block)
    if ws.get("key") != key:
        ws.clear()
        D = DeviceArray
        ws.update(key=key, mom=D((nrows, 4), np.float64), stats=D((nrows, 6), np.float64), evm=D((nrows,), np.float64),
                  qpsk=D((nrows, 3), np.float64) if M == 4 else None)
        if block:
            ws.update(tmom=D((nrows, nblocks, 4), np.float64), tstats=D((nrows, nblocks, 6), np.float64))
    stats = _dsp.blind_stats_dev(rows, M, stats=ws["stats"], mom=ws["mom"])
    evm = _dsp.blind_evm_dev(rows, M, stats=stats, evm_sum=ws["evm"])
    st = stats.to_host()
    qpsk = _dsp.qpsk_blind_snr_dev(rows, out=ws["qpsk"]).to_host() if M == 4 else None
    trace = None
    if block:
        trace = _dsp.blind_stats_dev(rows, M, block=block, stats=ws["tstats"], mom=ws["tmom"]).to_host()
    out = []
    with np.errstate(all="ignore"):
        for i in range(nrows):
            d = dict(snr=float(st[i, 4]), snr_db=float(10 * np.log10(st[i, 4])), s0=float(st[i, 5]), evm_blind=float(evm[i]))
            if qpsk is not None:
                d["snr_qpsk_db"] = float(qpsk[i, 2])
            if trace is not None:
                d["snr_trace"], d["s0_trace"] = trace[i, :, 4].copy(), trace[i, :, 5].copy()
            out.append(d)
    return out


class ResidentReceiver:
    """
    One capture's worth of preallocated device state.

    Parameters mirror ``dual_mode_equalisation`` + ``bps``: ``mu``, ``Niter``, ``methods``, ``adaptive_stepsize`` are
    2-tuples (pass ``methods=("mcma",)`` etc. with 1-tuples for a single stage), ``Mtestangles``/``Nbps`` the BPS
    parameters (``Mtestangles=None`` skips carrier recovery).  ``Bbps=None``: single-stage search over ``Mtestangles`` angles; an integer
    selects the two-stage search - ``Mtestangles`` coarse angles, then ``Bbps`` fine ones around each symbol's coarse estimate
    (``hip_dsp.bps_twostage_recover_dev``; ``idx`` then holds the coarse and ``idx2`` the fine indices) - through the same calls.

    ``carrier``: the carrier-recovery stage - ``"bps"`` (default), the blind phase search above; ``"vv"``, Viterbi-Viterbi for QPSK (``M == 4``)
    with ``Nbps`` as the window (``hip_dsp.vv_recover_dev``): ``out`` keeps its (modes, N) shape with ``Nbps - 1`` zero edge samples and ``ph`` is
    (modes, N - Nbps + 1); ``"partition"``, QPSK partitioning for 16-QAM (``M == 16``) with ``Nbps`` as the block length
    (``hip_dsp.partition16_recover_dev``).  Neither has a test-angle grid or an index array; ``Mtestangles=None`` still skips the stage.
    """

    NONFINAL_TOL_FACTOR = _host.NONFINAL_TOL_FACTOR

    def __init__(self, nmodes, L, os, M, Ntaps, mu, methods=("cma", "mrde"), Niter=(1, 1), adaptive_stepsize=(False, False),
                 TrSyms=(None, None), Mtestangles=64, Nbps=20, dtype=np.complex64, alphabet=None, modes=None, tier="a", pit=None, Bbps=None,
                 carrier="bps"):
        suf, self.rt, self.ct = _lib.suffix(dtype)
        self.carrier = str(carrier).lower()
        if self.carrier not in ("bps", "vv", "partition"):
            raise ValueError("carrier must be 'bps', 'vv' or 'partition'")
        if self.carrier != "bps" and int(M) != {"vv": 4, "partition": 16}[self.carrier]:
            raise ValueError("carrier='vv' recovers QPSK (M = 4) and carrier='partition' 16-QAM (M = 16); M = %d takes carrier='bps'" % int(M))
        if self.carrier != "bps" and Bbps is not None:
            raise ValueError("Bbps belongs to carrier='bps'")
        self.nmodes, self.L, self.os, self.M, self.Ntaps = int(nmodes), int(L), int(os), int(M), int(Ntaps)
        # run(overlap=True), tier b: the pending phase search in parts between the next capture's relaxation passes.  0: as many parts as the previous
        # capture had passes, less one; 1: one launch beside the first passes (rounds 3-4); n > 1: n parts.  (QAMPY_POST_PARTS: initial value, measurements)
        self.post_parts = int(_os.environ.get("QAMPY_POST_PARTS", "0"))
        self.nstage = len(methods)
        self.methods = tuple(m.lower() for m in methods)
        for m in self.methods:
            if m in _host.REAL_VALUED or m in _host.DATA_AIDED:
                raise ValueError("the resident pipeline runs the blind / decision-directed complex methods; %s is not one" % m)
            if m not in _host.TRAINING_FCTS:
                raise ValueError("%s is unknown method" % m)
        self.Niter = tuple(int(n) for n in Niter)
        self.adaptive = tuple(a if isinstance(a, str) else bool(a) for a in adaptive_stepsize)      # True, False or "per-mode"
        self.modes = np.arange(nmodes) if modes is None else np.atleast_1d(modes)
        self.TrSyms = tuple(_host._cal_training_symbol_len(os, Ntaps, L) if t is None else int(t) for t in TrSyms[:self.nstage])
        self.N = (self.L - self.Ntaps + 1) // self.os
        self.Mtestangles, self.Nbps = Mtestangles, Nbps
        self.Bbps = None if Bbps is None else int(Bbps)
        if self.Bbps is not None and not 1 <= self.Bbps <= 64:
            raise ValueError("Bbps: 1 .. 64 fine test angles, or None for the single-stage search")
        # tier "a" (default): the reference's exact sequential recurrence.  tier "b" (opt-in): parallel-in-time training
        #  - concurrently trained segments + waveform relaxation until the boundary defect is below `tol`; the
        # first stage is a cold start (gear-shifted acquisition), later stages start from the previous stage's taps.
        # `pit`: options of hip_equalisation.train_equaliser_dev(pit=...), one dict for all stages or one per stage
        if tier not in ("a", "b"):
            raise ValueError("tier must be 'a' (exact) or 'b' (parallel in time)")
        self.tier = tier
        pit = pit or {}
        self.pit = [dict(p) for p in pit] if isinstance(pit, (tuple, list)) else [dict(pit) for _ in methods]
        for o in self.pit:
            if o.get("acq_chunk"):
                o["_acq_chunk_user"] = True        # the caller fixed the chunk length: load() leaves it alone
        self._owner_thread = None                  # set by ReceiverGroup: the stages of this receiver are enqueued by that thread only
        self.fs = None                             # the receiver's sampling rate (load_resampled)
        self.filter_aside = True                   # run(overlap=True), tier b: the capture's filter on stream 2 (False: on stream 0, for measurements)
        # Tolerance per stage (round 5).  `tol` bounds what the CALL returns: equaliser output <= tol, taps <= 3 tol, error traces <= 3 tol.
        # The device's stop rule holds the estimated output deviation of a sweep to its `tol` - which is what the LAST stage's filter output needs; an
        # earlier stage returns an error trace and hands on taps, both held to 3 tol, so it is certified at NONFINAL_TOL_FACTOR x tol (2: the error
        # functions turn an output deviation into 1.3-1.5 x as much trace deviation, measured).  One `pit` dict per stage overrides this.
        if tier == "b" and not isinstance(pit, (tuple, list)):
            for s_ in range(self.nstage - 1):
                self.pit[s_]["tol"] = self.NONFINAL_TOL_FACTOR * float(self.pit[s_].get("tol") or 1e-3)
        self.pit_report = None
        self.pit_timing = [([], 0.) for _ in methods]
        self.mu0 = tuple(self.rt(m) for m in mu)
        if alphabet is None:
            alphabet = _host.generate_symbols_for_eq("sbd", M, self.ct)[0]
        self.alphabet_host = np.ascontiguousarray(alphabet, dtype=self.ct)
        # ---- device state
        self.E = DeviceArray((nmodes, L), self.ct)
        self.wxy = DeviceArray((nmodes, nmodes, Ntaps), self.ct)
        self.wxy0 = DeviceArray.from_host(_host._init_taps(Ntaps, nmodes, nmodes, self.ct))
        self.mu = [DeviceArray.from_host(np.array([m], dtype=self.rt)) for m in self.mu0]
        self.mu_init = [DeviceArray.from_host(np.array([m], dtype=self.rt)) for m in self.mu0]
        self.symbols = []
        for m in self.methods:
            sy = _host._reshape_symbols(self.alphabet_host if m in _host.DECISION_BASED else None, m, M, self.ct, nmodes)
            self.symbols.append(DeviceArray.from_host(sy))
        self.err = [DeviceArray((nmodes, self.TrSyms[s] * self.Niter[s]), self.ct, zero=True) for s in range(self.nstage)]
        self.eq = DeviceArray((self.modes.size, self.N), self.ct)
        self.alphabet = self.angles = self.idx = self.idx2 = self.ph = self.out = None
        if Mtestangles and self.carrier != "bps":
            lim = min(self.N, _dsp.VV_NMAX) if self.carrier == "vv" else _dsp.P16_NBLOCK_MAX
            if not 1 <= int(Nbps) <= lim:
                raise ValueError("carrier=%r takes Nbps from 1 to %d here" % (self.carrier, lim))
            self.alphabet = DeviceArray.from_host(self.alphabet_host)
            self.ph = DeviceArray((self.modes.size, self.N - int(Nbps) + 1 if self.carrier == "vv" else self.N), self.rt)
            self.out = DeviceArray((self.modes.size, self.N), self.ct)
        elif Mtestangles:
            self.alphabet = DeviceArray.from_host(self.alphabet_host)
            self.angles = DeviceArray.from_host(_dsp.test_angle_grid(Mtestangles, self.rt))
            self.idx = DeviceArray((self.modes.size, self.N), np.int32)
            if self.Bbps is not None:
                self.idx2 = DeviceArray((self.modes.size, self.N), np.int32)
            self.ph = DeviceArray((self.modes.size, self.N), self.rt)
            self.out = DeviceArray((self.modes.size, self.N), self.ct)
        if tier == "b":
            self.pit_report = [_k.PitReportBuffer() for _ in methods]
            for s_, o in enumerate(self.pit):          # segment grid from the host copy of mu: the call then never synchronises
                o.setdefault("acquire", 1 if s_ == 0 else 0)
                if not self.adaptive[s_]:              # fixed step: the host copy spares the call the read-back of *mu (qh_pit_opts.mu_hint)
                    o.setdefault("mu_hint", float(self.mu0[s_]))
                if self.adaptive[s_]:                  # adaptive step: the library's own grid (exact head + 2048-step segments), modes in turn
                    o.setdefault("segments", 0)
                else:
                    o.setdefault("segments", _k.pit_auto_segments(self.TrSyms[s_], float(self.mu0[s_]), self.modes.size, cold=bool(o["acquire"])))
        # ---- what the stages allocate on first use (None until then: nothing is allocated here)
        self.E_next, self._next_loaded = None, False       # the second input buffer (load_next) and whether it holds the capture that follows
        self._cd_buf = self._fe_buf = self._fe_mom = self._fe_coef = self._foe_fo = self._foe_stats = self._tx_mom = self._raw_buf = self._raw_mom = None
        self._idx_tx = self._idx_tx_src = None             # ser() / metrics(): the transmitted indices, cached per symbols_tx object
        self._sync_ws = {}                                 # buffers of sync="full" (symbols, correlation, peak table, label rows), kept from call to call
        self._blind_ws = {}                                # buffers of blind_metrics() (moments, stats, distance sums), kept from call to call
        self._load_power = None                            # tier b: the clean power the last load() read (impair(snr=...) scales it)
        self._acq_asked = [False] * self.nstage            # tier b: the stage's acquisition chunk is known, or the device has been asked for it once
        self._gram = self._basis = None                    # what build_gram() made for this capture
        self._hook_keepalive = self._pass_hook_keepalive = None    # the ctypes callbacks of the training call under way
        # prepared ahead (run(prefetch=True), _prepare_next): two slots, the acquisition and the eigenbasis of the capture that follows; _ev_main is
        # recorded by run() on stream 0 (the capture is in place) and awaited by stream 1, _ev_prep[slot] by stream 1 behind the preparation and
        # awaited by stream 0 when the next run adopts it
        self._prep, self._prep_ready, self._prep_cur = None, [False, False], 0
        self._basis_alt = self._ev_main = self._ev_prep = self._use_prep = None
        # ---- run(overlap=True): the schedule over stream 0 (training), stream 1 (preparation ahead) and stream 2 (filter aside, phase search).
        # The events (created on first use), who records each and who waits for it:
        #   _ev_ready    behind the capture's filter: on stream 2 where the filter went aside, else on stream 0.  Stream 2 waits for it in front of the
        #                pending search, which reads the filter output; stream 0 waits for it (input_free) before an input buffer or the taps copy is
        #                written, which the filter aside reads.  _filter_pending: a filter went aside and stream 0 has not waited since.
        #   _ev_trained  on stream 0 behind the copy of the trained taps into _wxy_f; stream 2 waits for it in front of the filter aside.
        #   _ev_pass     on stream 0 in front of a pass's trainer launch; stream 2 waits for it in front of the part of the search that goes beside it.
        #   _ev_post     on stream 2 behind the last launch of a search.  Stream 0 waits for it in wait_post() and in front of a filter on stream 0, which
        #                overwrites what the search read; stream 1 in front of the next preparation.  A filter aside is behind it by stream 2's order.
        # The pending search: nothing pending -> run(overlap=True): pending (_post_pending, _post_n = 0) -> the next run, tier b, post_parts != 1:
        # in parts (_post_next of _post_n enqueued, one per on_pass, the rest after the training; _post_mark marks the first and the last) -> the last
        # launch enqueued: running (_post_running) -> consumed (stream 0 has waited for _ev_post, or the next filter went aside behind it).
        # _hook_calls: on_pass calls of the run under way; _hook_calls_prev: those of the last run that had any (0: none yet) - the next search's parts.
        self._ev_ready = self._ev_post = self._ev_trained = self._ev_pass = self._wxy_f = None
        self._filter_pending = self._post_pending = self._post_running = False
        self._post_n = self._post_next = self._hook_calls = self._hook_calls_prev = 0
        self._post_mark = None
        _lib.sync()

    # ------------------------------------------------------------------------------------------ data movement
    def load(self, E):
        """Host -> HBM copy of the capture (outside any timed region).  Tier b: the chunk length of a cold stage's acquisition follows the
        capture's power (2 / the gear-shifted step, rounded to a power of two: csrc/train_pit.h) - it is re-derived here for EVERY capture from
        the host copy, by the library's own rule, so that the result of a capture never depends on which capture the receiver saw first and
        no call has to wait for the device to say it."""
        E = np.ascontiguousarray(np.asarray(E), dtype=self.ct)
        assert E.shape == (self.nmodes, self.L)
        self._capture_to_write().set(E)
        self._acq_asked = [False] * self.nstage
        if self.tier == "b":
            self._load_power = float(np.mean(np.abs(E[:, :min(self.L, 4096)].astype(np.complex128)) ** 2))
        self._capture_written(power=self._load_power)

    def _capture_to_write(self, next_capture=False):
        """Start of a stage that writes an input buffer: ``self.E``, or ``self.E_next`` with ``next_capture``, with stream 0 behind a filter that
        may still be reading it on stream 2."""
        buf = self.E_next if next_capture else self.E
        if buf is None:
            raise ValueError("no capture loaded for next_capture=True (load_next first)")
        self.input_free()
        return buf

    def _capture_written(self, next_capture=False, power=None):
        """End of such a stage: what was prepared ahead is dropped.  ``power``, from a stage that changes or first learns the power of the capture
        in ``self.E``: tier b re-derives the acquisition chunk of every cold fixed-step stage from it by the library's own rule (``load``)."""
        if self._prep is not None:
            self.invalidate()
        if self.tier == "b" and power is not None and not next_capture:
            for s_, o in enumerate(self.pit):
                if o.get("acquire") and not self.adaptive[s_] and not o.get("_acq_chunk_user"):
                    o["acq_chunk"] = self._acq_chunk_rule(power, float(self.mu0[s_]), o)
                    self._acq_asked[s_] = True

    def compensate_cd(self, fs, D, L, wl0=1550e-9, N=None, next_capture=False):
        """Take the chromatic dispersion of ``L`` metres of fibre (``D`` in s/m/m) out of the loaded capture in HBM (``self.E``, or
        ``self.E_next`` with ``next_capture``): :func:`qampy_amd.core.filter.cd_filter_dev` with ``-L``, enqueued on stream 0 between
        ``load()`` / ``load_next()`` and ``run()``.  ``L`` is the fibre length the capture went through, as ``add_dispersion`` takes it.
        The filter is all-pass, so the power ``load()`` read for tier b's acquisition rule is still the capture's power."""
        from .core.filter import cd_filter_dev
        buf = self._capture_to_write(next_capture)
        if self._cd_buf is None:
            self._cd_buf = DeviceArray((self.nmodes, self.L), self.ct)
        cd_filter_dev(buf, self._cd_buf, fs, D, -L, wl0=wl0, N=N)
        buf.copy_from(self._cd_buf)
        self._capture_written(next_capture)

    def backpropagate(self, fs, D, span_length, nspans, gamma, alpha_db_km, steps, power_dbm, amplify=True, wl0=1550e-9, next_capture=False):
        """Take ``nspans`` spans of nonlinear fibre out of the loaded capture in HBM (``self.E``, or ``self.E_next`` with ``next_capture``): the
        nonlinear counterpart of ``compensate_cd``, :func:`qampy_amd.core.hip_dsp.dbp_dev` in place on the capture buffer, enqueued on stream 0
        between ``load()`` / ``load_next()`` and ``run()``.  The arguments are those of the link as ``hip_dsp.ssfm_dev`` takes them; ``power_dbm``
        is the launch power over all modes, which is the power of the capture when every span ends in its amplifier; fewer ``steps`` than the
        link, or a scaled ``gamma``, give the usual practical back-propagation.  One or two modes, and a row length csrc/fft.hip takes:
        ValueError otherwise, before a launch.  The filters are all-pass and the Kerr term is a phase; with ``amplify`` the scalars of a span
        multiply to one, so the power ``load()`` read for tier b's acquisition rule is still the capture's power.  With ``amplify=False`` the
        power grows by the loss of the link, ``exp(alpha span_length nspans)``, which is known on the host: tier b's rule is given the new
        power without a read-back (not with ``next_capture``, as in ``impair``)."""
        buf = self._capture_to_write(next_capture)
        _dsp.dbp_dev(buf, buf, fs, D, span_length, nspans=nspans, gamma=gamma, alpha_db_km=alpha_db_km, steps=steps, power_dbm=power_dbm, amplify=amplify,
                     wl0=wl0)
        if not amplify and self._load_power is not None and not next_capture:
            self._load_power *= float(np.exp(_dsp.fibre_alpha(alpha_db_km) * float(span_length) * int(nspans)))
            self._capture_written(power=self._load_power)
        else:
            self._capture_written(next_capture)

    def frontend(self, orthonormalize=True, skew=None, sampling_rate=None, pre_filter_bw=None, next_capture=False):
        """Condition the loaded capture in HBM (``self.E``, or ``self.E_next`` with ``next_capture``) as the analog front end does, between
        ``load()`` / ``load_next()`` and the other compensations, enqueued on stream 0: first the skew between the rails - ``skew=(delay_i,
        delay_q)`` in seconds at ``sampling_rate``, :func:`qampy_amd.core.hip_dsp.skew_dev` - then the brick-wall pre-filter
        ``pre_filter(E, pre_filter_bw)``, then ``orthonormalize_signal(E, os)`` at the receiver's ``os``.  The two filters are whole-row
        transforms (a row of ``L`` samples must be a length csrc/fft.hip takes: ValueError otherwise) into a private buffer.

        This stage changes the power.  Tier b: ``_load_power`` and the acquisition chunk of every cold stage are re-derived by the rule of
        ``load()`` from a read-back of the first ``min(L, 4096)`` conditioned samples of every mode, which waits for the stage (not with
        ``next_capture``, as in ``impair``)."""
        buf = self._capture_to_write(next_capture)
        if skew is not None:
            skew = tuple(float(v) for v in np.atleast_1d(skew))
            if len(skew) != 2 or not all(np.isfinite(skew)):
                raise ValueError("skew is (delay_i, delay_q) in seconds")
            if sampling_rate is None:
                raise ValueError("skew needs the sampling_rate of the capture")
            _dsp.frontend._skew_step(self.L, sampling_rate)
        if pre_filter_bw is not None:
            _dsp.pre_filter_bins(self.L, float(pre_filter_bw))
        if skew is not None or pre_filter_bw is not None:
            _dsp.fft_plan(self.L)
        if (skew is not None or pre_filter_bw is not None) and self._fe_buf is None:
            self._fe_buf = DeviceArray((self.nmodes, self.L), self.ct)
        cur = buf
        if skew is not None:
            cur = _dsp.skew_dev(cur, self._fe_buf, skew[0], skew[1], sampling_rate)
        if pre_filter_bw is not None:
            cur = _dsp.pre_filter_dev(cur, buf if cur is not buf else self._fe_buf, pre_filter_bw)
        if orthonormalize:
            if self._fe_mom is None:
                self._fe_mom = DeviceArray((self.nmodes, 10), np.float64)
                self._fe_coef = DeviceArray((self.nmodes, 6), np.float64)
            _dsp.orthonormalize_dev(cur, buf, self.os, mom=self._fe_mom, coef=self._fe_coef)
        elif cur is not buf:
            buf.copy_from(cur)
        if self.tier == "b" and not next_capture:
            npow = min(self.L, 4096)
            head = np.empty((self.nmodes, npow), self.ct)
            for m in range(self.nmodes):
                _lib.call("qh_memcpy_d2h", head[m].ctypes.data, buf.ptr + m * self.L * head.itemsize, npow * head.itemsize)
            self._load_power = float(np.mean(np.abs(head.astype(np.complex128)) ** 2))
            self._capture_written(power=self._load_power)
        else:
            self._capture_written(next_capture)

    def compensate_foe(self, fft_size=2 ** 16, blocks="all", average_over_modes=True, next_capture=False):
        """Estimate the frequency offset of the loaded capture in HBM (``self.E``, or ``self.E_next`` with ``next_capture``) at the receiver's
        ``os`` and take it out in place: ``hip_dsp.find_freq_offset_dev`` and ``comp_freq_offset_dev``, enqueued on stream 0 between
        ``load()`` / ``load_next()`` (or ``compensate_cd``) and ``run()``, with no read-back between them.  ``fft_size`` and ``blocks`` as in
        ``hip_dsp.foe_plan`` (``"all"``: the spectrum averaged over every whole block of the capture).  The rotation leaves the power as it
        is, so tier b's acquisition rule still holds.  The offsets and the peak statistics stay on the device: :attr:`foe` reads them."""
        buf = self._capture_to_write(next_capture)
        N, B = _dsp.foe_plan(self.L, fft_size, blocks)
        if self._foe_fo is None:
            self._foe_fo = DeviceArray((self.nmodes,), np.float64, zero=True)
            self._foe_stats = DeviceArray((self.nmodes, 3), np.float64, zero=True)
        _dsp.find_freq_offset_dev(buf, self.os, N, B, average_over_modes, self._foe_fo, stats=self._foe_stats)
        _dsp.comp_freq_offset_dev(buf, self._foe_fo, self.os, buf)
        self._capture_written(next_capture)

    def impair(self, fs, snr=None, freq_off=None, lwdth=None, dgd=None, theta=np.pi / 3.731, modal_delay=None, seed=0, source=None,
               next_capture=False, power=None, tx=None):
        """Impair the loaded capture in HBM (``self.E``, or ``self.E_next`` with ``next_capture``) in place, between ``load()`` / ``load_next()``
        and ``run()``: ``hip_dsp.simulate_transmission_dev`` at the sampling rate ``fs`` (symbol rate ``fs / os``) - phase noise of linewidth
        ``lwdth``, carrier offset ``freq_off``, noise to the SNR ``snr`` (dB), ``modal_delay``, PMD of ``dgd`` seconds at ``theta`` - enqueued on
        stream 0 with nothing read back; the noise is a function of ``seed``.  ``source``: a resident (nmodes, L) DeviceArray holding a clean
        field, which is read instead and left as it is - the capture buffer receives its impaired copy, so one clean capture serves a whole
        sweep without crossing PCIe.

        Every stage but the noise keeps the power.  Tier b with ``snr``: the acquisition chunk of a cold stage is re-derived by the rule of
        ``load()`` from the clean power times ``hip_dsp.snr_power_factor(snr, os)``.  The clean power is ``power`` if given, else what the
        last ``load()`` read - with ``source`` that is the power of whatever ``load()`` saw last, so give ``power`` (the mean ``|source|**2``)
        unless the source is a copy of that capture; with neither, ValueError.  The factor is applied to the clean power, not compounded:
        impair a loaded capture once.

        ``tx``: a dict of ``hip_dsp.sim_tx_response_dev`` keywords (``enob``, ``tgt_v``, ``clip_rat``, ``quant_bits``, ``dac_params``, the
        modulator's parameters, ``seed`` - default ``seed + 1``, so that the ENOB noise is not the channel's noise).  The transmitter is
        applied first, to the source or in place, and every mode is then centred and scaled to unit mean power (``row_moments_dev`` /
        ``center_scale_dev``): the modulator's output carries about a tenth of unit power, and the trainers' radii assume unit power.  The
        channel impairments follow on that field; tier b's clean power is then 1."""
        buf = self._capture_to_write(next_capture)
        src = buf if source is None else source
        if tuple(src.shape) != (self.nmodes, self.L) or np.dtype(src.dtype) != np.dtype(self.ct):
            raise ValueError("source must be a (%d, %d) %s DeviceArray" % (self.nmodes, self.L, np.dtype(self.ct).name))
        if source is not None and source.ptr == buf.ptr:
            raise ValueError("source is the capture buffer itself: leave it out to impair in place")
        if tx is not None:
            tx = dict(tx)
            tx.setdefault("seed", int(seed) + 1)
            _dsp.sim_tx_response_check(src, buf, fs, **tx)
        clean = power
        if tx is not None:
            clean = 1.0
        elif self.tier == "b" and snr is not None and not next_capture:
            clean = self._load_power if power is None else float(power)
            if clean is None:
                raise ValueError("tier b needs the clean capture's power for its acquisition rule: power=..., or load() first")
        if (modal_delay is not None or dgd is not None) and self._cd_buf is None:
            self._cd_buf = DeviceArray((self.nmodes, self.L), self.ct)
        if tx is not None:
            from .core import resample as _rs
            if self._tx_mom is None:
                self._tx_mom = DeviceArray((self.nmodes, 3), np.float64)
            _dsp.sim_tx_response_dev(src, buf, fs, **tx)
            _rs.center_scale_dev(buf, _rs.row_moments_dev(buf, self._tx_mom), power=1.0)
            src = buf
        _dsp.simulate_transmission_dev(src, buf, fs / self.os, fs, snr=snr, freq_off=freq_off, lwdth=lwdth, dgd=dgd, theta=theta, modal_delay=modal_delay,
                                       seed=seed, tmp=self._cd_buf)
        noisy = clean * _dsp.snr_power_factor(snr, self.os) if (self.tier == "b" and snr is not None and not next_capture) else None
        self._capture_written(next_capture, power=noisy)

    @property
    def foe(self):
        """``(offset[nmodes], stats[nmodes, 3])`` of the last :meth:`compensate_foe`, read back after a sync: the offset taken out of every
        mode in units of the symbol rate, and per mode the peak's bin, its power and the total power of the fourth-power spectrum."""
        if self._foe_fo is None:
            raise ValueError("compensate_foe has not run")
        _lib.sync()
        return self._foe_fo.to_host(), self._foe_stats.to_host()

    def load_resampled(self, E_raw, fs_in, beta=None, taps=4001, fftconv=True, next_capture=False, fs=None):
        """Load a capture that arrives at the converter's rate: the raw rows ``E_raw`` (nmodes, Lin) at ``fs_in`` go to HBM, are resampled there
        to the receiver's rate ``fs`` (``os`` samples per symbol; keyword, or the attribute ``self.fs``) into ``self.E`` (``self.E_next`` with
        ``next_capture``), of which the first ``self.L`` outputs are kept, and every mode is centred and scaled to unit mean power - three
        launches on stream 0 with no read-back between them (:mod:`qampy_amd.core.resample`).  ``beta=None``: the default Kaiser filter of
        ``resample_poly``; otherwise a root-raised-cosine filter of ``taps`` taps, symbol period ``os / fs`` and roll-off ``beta``, on the
        reference's ``fftconv`` path or its ``resample_poly`` path.  ValueError if the capture yields fewer than ``self.L`` samples.

        Tier b: the loaded capture has unit power by construction, so the acquisition rule of ``load()`` is given the power 1.0 - it stays a
        function of values the host knows."""
        from .core import resample as _rs
        fs = self.fs if fs is None else fs
        if fs is None:
            raise ValueError("load_resampled needs the receiver's sampling rate: fs=..., or set rx.fs")
        E_raw = np.ascontiguousarray(np.asarray(E_raw), dtype=self.ct)
        if E_raw.ndim != 2 or E_raw.shape[0] != self.nmodes:
            raise ValueError("E_raw must be (%d, Lin)" % self.nmodes)
        Lin = E_raw.shape[1]
        up, down = _rs._resamplingfactors(fs_in, fs)
        if _rs.n_out(Lin, up, down) < self.L:
            raise ValueError("%d samples at %g resample to %d at %g, fewer than the receiver's %d" % (Lin, fs_in, _rs.n_out(Lin, up, down), fs, self.L))
        if beta is None:
            h, gain = _rs.default_window(up, down), up
        else:
            if not 0 < beta <= 1:
                raise ValueError("beta needs to be in interval (0,1]")
            h, gain = _rs.rrcos_taps(taps, up * fs_in, self.os / fs, beta), (1 if fftconv else up)
        if next_capture and self.E_next is None:
            self.E_next = DeviceArray((self.nmodes, self.L), self.ct)
        if self._raw_buf is None or self._raw_buf.shape != E_raw.shape:
            self._raw_buf = DeviceArray(E_raw.shape, self.ct)
            self._raw_mom = DeviceArray((self.nmodes, 3), np.float64)
        buf = self._capture_to_write(next_capture)
        self._raw_buf.set(E_raw)
        _rs.resample_dev(self._raw_buf, buf, h, up, down, gain)
        _rs.center_scale_dev(buf, _rs.row_moments_dev(buf, self._raw_mom), power=1.0)
        if next_capture:
            self._next_loaded = True
        else:
            self._acq_asked = [False] * self.nstage
        self._capture_written(next_capture, power=1.0)

    def _acq_chunk_rule(self, power, mu, o):
        return _k.pit_acq_chunk(power, mu, self.nmodes * self.Ntaps, self.rt, o.get("gear"), o.get("acq_bound"))

    # ------------------------------------------------------------------------------------------ stages (enqueue only)
    def reset(self):
        """Centre-spike taps and initial step sizes (start of ``dual_mode_equalisation``)."""
        self.wxy.copy_from(self.wxy0)
        for s_, (m, m0) in enumerate(zip(self.mu, self.mu_init)):
            if self.adaptive[s_]:                  # (a fixed step is only read by the trainers: nothing to restore - a copy is ~6 us of stream 0 between two captures)
                m.copy_from(m0)

    def _bound(self):
        """A receiver of a ReceiverGroup caches state of its worker thread (that thread's library streams, events, scratch slots - a Gram table
        pointer into them): its stages must be enqueued by that thread (``group.map(fn, which=[i])``), or nothing orders them against the
        worker's streams."""
        import threading
        if self._owner_thread is not None and threading.get_ident() != self._owner_thread:
            raise RuntimeError("this receiver belongs to a ReceiverGroup: enqueue its stages on its worker thread (group.map(lambda rx: ..., which=[i]) or group.run)")

    def build_gram(self):
        """Gram terms of the look-ahead trainer: once per capture, shared by all modes, stages and sweeps."""
        self._bound()
        self._gram = None
        if self.tier == "a":
            # shared table only when a block form will read it (>= 128 steps) and it fits the library's scratch budget - otherwise
            # the trainers chunk the sweep themselves (csrc/train_impl.h: gram_budget), which a caller's table would switch off
            budget = _lib.gram_budget_gb() * 2 ** 30
            fits = self.TrSyms[0] * 1024 * (np.dtype(self.ct).itemsize // 8) <= budget
            if len(set(self.TrSyms)) == 1 and self.TrSyms[0] >= 128 and fits and _lib.get_form("trainer") != 1:
                self._gram = _k.gram_build_dev(self.E, self.os, self.Ntaps, self.TrSyms[0])
        elif len(set(self.TrSyms)) == 1 and self.nmodes * self.Ntaps <= 128:
            # tier b builds what its passes need itself (no Gram table in the throughput form, csrc/train_seg.h); what the stages
            # share is the eigenbasis of the capture's input covariance for the coarse correction
            self._basis = _k.pit_basis_dev(self.E, self.os, self.Ntaps, self.TrSyms[0], self._basis, overlap=True)
            for o in self.pit:
                o["basis"] = self._basis.ptr

    def train(self, stage, hook=None, pass_hook=None):
        """``hook`` (tier b): a callable the library invokes once, right after it has enqueued the sweep's first relaxation pass
        (``qh_pit_opts.on_pass0``) - work for the other library streams is enqueued there, while the device is busy, instead of in front of
        this sweep's launches; called after the sweep if the library never got to a first pass (exact form).

        ``pass_hook(sweep, p)`` (tier b): invoked right before the trainer launch of EVERY relaxation pass (``qh_pit_opts.on_pass``) - see
        ``run(overlap=True)``."""
        tb = self.tier == "b"
        self._bound()
        opts = {k: v for k, v in self.pit[stage].items() if not k.startswith("_")} if tb else None
        if tb and stage == 0 and self._use_prep is not None:
            opts["prepared"] = self._use_prep.ptr
            self._use_prep = None
        fired, failed = [False], []
        if pass_hook is not None and tb:
            import ctypes as _C

            def _pcb(_user, sweep, p):
                try:
                    pass_hook(int(sweep), int(p))
                except BaseException as e:            # (never through the C frames: re-raised below)
                    failed.append(e)
                finally:
                    _lib.call("qh_use_stream", 0)
            self._pass_hook_keepalive = _lib.PIT_PASS_HOOK(_pcb)
            opts["on_pass"] = _C.cast(self._pass_hook_keepalive, _C.c_void_p).value
        if hook is not None and tb:
            import ctypes as _C

            def _cb(_user):
                if not fired[0]:
                    fired[0] = True
                    try:
                        hook()
                    except BaseException as e:        # (never through the C frames: re-raised below)
                        failed.append(e)
                    finally:
                        _lib.call("qh_use_stream", 0)
            self._hook_keepalive = _lib.PIT_HOOK(_cb)
            opts["on_pass0"] = _C.cast(self._hook_keepalive, _C.c_void_p).value
        _k.train_equaliser_dev(self.E, self.TrSyms[stage], self.Niter[stage], self.os, self.mu[stage], self.wxy, self.modes,
                               self.adaptive[stage], self.symbols[stage], self.methods[stage], self.err[stage],
                               gram=self._gram, pit=opts, report=self.pit_report[stage] if tb else None)
        if hook is not None and not fired[0]:
            fired[0] = True
            hook()
        if failed:
            raise failed[0]
        if tb:
            self.pit_timing[stage] = _k.pit_last_timing()      # host-side copy of the HIP-event times: no synchronisation
            o = self.pit[stage]
            if o.get("acquire") and not o.get("acq_chunk") and not self.adaptive[stage] and not self._acq_asked[stage]:
                # a capture that was put into self.E directly (device-side synthesis, tests): the chunk length the device derived for it is
                # read back ONCE (this synchronises: the one read of the receiver's life, whatever the report says - a sweep the library
                # sent to the exact form has no acquisition to report and is not asked again); load() derives it on the host instead
                self._acq_asked[stage] = True
                a = self.pit_report[stage].read()["acquisition"]
                if a["chunks"] > 0 and a["steps"] > 0:
                    o["acq_chunk"] = int(a["steps"] // a["chunks"])

    def pit_reports(self):
        """Tier b: what the device decided in the last run, one dict per stage (segments, passes, boundary defects,
        acquisition); synchronises."""
        return [r.read() for r in self.pit_report] if self.pit_report else None

    def apply(self):
        """Filter the capture with the current taps (a phase search still pending from run(overlap=True) is completed first: it reads
        the filter output this call overwrites)."""
        self.wait_post()
        self._apply()

    def recover(self):
        """Phase search, unwrap and de-rotation of the filter output (after a pending one, see apply)."""
        self.wait_post()
        self._recover()

    def _apply(self):
        self._bound()
        _k.apply_filter_to_signal_dev(self.E, self.os, self.wxy, self.modes, self.eq)

    def _recover(self, part=0, nparts=1):
        self._bound()
        if self.carrier != "bps":
            # one pass over the whole row, like the two-stage search: whatever the number of parts, the last one launches it
            if part == nparts - 1 and self.carrier == "vv":
                _dsp.vv_recover_dev(self.eq, self.Nbps, 4, self.ph, self.out)
            elif part == nparts - 1:
                _dsp.partition16_recover_dev(self.eq, self.Nbps, self.ph, self.out)
            return
        if self.Bbps is not None:
            # two stages: there is no part-wise form - whatever the number of parts, the last one is the one launch of the whole search
            if part == nparts - 1:
                _dsp.bps_twostage_recover_dev(self.eq, self.Mtestangles, self.Bbps, self.alphabet, self.Nbps, self.idx, self.idx2, self.ph, self.out,
                                              angles=self.angles)
            return
        _dsp.bps_recover_dev(self.eq, self.Mtestangles, self.alphabet, self.Nbps, self.idx, self.ph, self.out, angles=self.angles, part=part, nparts=nparts)

    # ------------------------------------------------------------------------------------------ the next capture's sequential prologue, ahead of time
    def load_next(self, E):
        """Host -> HBM copy of the capture that follows the one in ``self.E`` (second input buffer): ``run(prefetch=True)`` processes ``E``, prepares
        this one beside it and swaps the two buffers when it is done with ``E`` - so the call sequence of a streaming receiver is ``load(c0)``,
        ``load_next(c1)``, ``run()``, ``load_next(c2)``, ``run()``, ..."""
        E = np.ascontiguousarray(np.asarray(E), dtype=self.ct)
        assert E.shape == (self.nmodes, self.L)
        if self.E_next is None:
            self.E_next = DeviceArray((self.nmodes, self.L), self.ct)
        self._capture_to_write(next_capture=True).set(E)        # (the buffer may be the capture a filter on stream 2 is still reading)
        self._next_loaded = True

    def input_free(self):
        """run(overlap=True) leaves the filter of the last capture on stream 2: stream 0 waits for it before an input buffer is written.  The
        receiver's own loading and conditioning methods do that themselves; a caller needs it after ``run(overlap=True)`` before writing
        ``rx.E`` or ``rx.E_next`` any other way (``rx.E.copy_from(...)``, a kernel of its own on stream 0)."""
        if self._filter_pending:
            _lib.call("qh_stream_wait_event", self._ev_ready.ptr)
            self._filter_pending = False

    def release_thread_state(self):
        """The receiver's worker thread is gone (ReceiverGroup.close) and with it that thread's library streams and scratch buffers: give up what
        pointed into them - the Gram table, the overlap events and flags - and the binding to the thread."""
        self._gram = self._ev_ready = self._ev_post = self._ev_trained = None
        self._filter_pending = self._post_pending = self._post_running = False
        self._owner_thread = None

    def invalidate(self):
        """Forget what was prepared ahead (after the capture in ``self.E`` / ``self.E_next`` was changed by hand)."""
        self._prep_ready = [False, False]

    def _prepare_next(self):
        """Tier b, cold first stage: the acquisition and the eigenbasis of the NEXT capture - both depend on the capture only, not on anything this
        capture's training produces - are enqueued on library stream 1 now, so that they run beside this capture's cold stage (whose passes leave
        32 compute units free for exactly that, csrc/train_pit.h) instead of in front of the next capture's passes (qh_pit_prepare_*_dev).  The next
        capture is ``E_next`` (``load_next``), or - a receiver fed the same resident capture again and again, as bench.py does - ``E`` itself."""
        o = self.pit[0]
        if self.tier != "b" or not o.get("acquire") or self.adaptive[0] or self.ct != np.complex64 or not self._basis:
            return
        if not (o.get("acq_chunk") and o.get("mu_hint") and o.get("segments", 0) > 1):
            return
        self._prep_init()
        slot = 1 - self._prep_cur
        amax = 2 * ((int(o["acq_chunk"]) + 63) // 64 * 64) if not o.get("acq_max") else int(o["acq_max"])
        need = _k.pit_prepare_bytes(self.nmodes, self.Ntaps, amax, self.ct)
        if self._prep[slot] is None or self._prep[slot].nbytes < need:
            self._prep[slot] = DeviceArray((need,), np.uint8)
        nxt = self.E_next if self._next_loaded else self.E
        with _lib.on_stream(1):                   # (_ev_main: recorded by run() on stream 0 when the next capture was in place)
            _lib.call("qh_stream_wait_event", self._ev_main.ptr)
            if self._post_running:
                _lib.call("qh_stream_wait_event", self._ev_post.ptr)        # (the previous capture's phase search: see run)
            # (NOT behind the first trainer launch like the parts of the phase search: its chip-wide kernels - setup, Gram terms, covariance - then share
            # the ~70 us of analysis behind passes 0 and 1 with the control path, which is the critical path: gaps of 130 / 123 instead of 90 us,
            # 1120-1124 against 1135-1144 MSym/s; beside pass 0 they cost that pass 2 %)
            ok = _k.pit_prepare_dev(nxt, self.TrSyms[0], self.os, self.mu_init[0], self.wxy0, self.modes, self.symbols[0], self.methods[0],
                                    {k: v for k, v in o.items() if not k.startswith("_") and k not in ("basis", "prepared")}, self._prep[slot])
            if ok:
                self._basis_alt = _k.pit_basis_dev(nxt, self.os, self.Ntaps, self.TrSyms[0], self._basis_alt, overlap=False)
                self._ev_prep[slot].record()
        self._prep_ready[slot] = bool(ok)

    def _prep_init(self):
        if self._prep is None:
            self._prep, self._prep_ready, self._prep_cur = [None, None], [False, False], 0
            self._basis_alt, self._ev_main, self._ev_prep = None, _lib.Event(), [_lib.Event(), _lib.Event()]

    def _adopt_prepared(self):
        """Start of a run: if the previous run prepared this capture, its eigenbasis and its acquisition are there already."""
        self._use_prep = None
        if self._prep is None:
            return False
        slot = 1 - self._prep_cur
        if not self._prep_ready[slot]:
            return False
        self._prep_ready[slot] = False
        self._prep_cur = slot
        self._basis, self._basis_alt = self._basis_alt, self._basis
        _lib.call("qh_stream_wait_event", self._ev_prep[slot].ptr)
        for o in self.pit:
            o["basis"] = self._basis.ptr
        self._use_prep = self._prep[slot]
        return True

    def run(self, overlap=False, mark=None, prefetch=False):
        """One pass of the hot path over the resident capture; returns without synchronising.

        ``overlap=True`` (a receiver that is handed capture after capture): the phase search of this pass is left PENDING and goes
        onto the library's stream 2 when the next ``run`` has enqueued its covariance kernel (the one chip-wide streaming kernel of
        a tier-b pass, which would otherwise queue up behind the phase search and hold back the eigen-solver), so that it runs
        beside the training of the next pass on stream 0 - the trainers are latency-bound chains of one wave per SIMD that leave
        half of the register file and most issue slots free, the phase search is a chip-wide streaming kernel of 64 registers a
        wave that fits into them (csrc/train_seg.h; stream 2 stays off 32 of the 256 compute units, csrc/api.hip).  The results of
        a pass are complete after ``wait_post()`` (enqueues what is pending; stream 0 waits for it) or ``fetch()`` (the host waits
        too).  Bit-identical to ``overlap=False``: the same kernels on the same data, in another order.  The two-stage search (``Bbps``) has
        no part-wise form: where the pending search would go beside the passes in parts (tier b, ``post_parts``), it goes as one launch
        (``nparts = 1``) with the last of them.  Tier b leaves the capture's filter on stream 2 too, still reading the input buffer when this
        call returns: before writing ``rx.E`` or ``rx.E_next`` other than through the receiver's own loading and conditioning methods, call
        ``input_free()``.

        ``prefetch=True`` (tier b, consecutive captures): the acquisition and the eigenbasis of the NEXT capture are enqueued on stream 1 at the
        start of this run and adopted by the next one (``_prepare_next``); results bit-identical to ``prefetch=False``.

        ``mark(name)`` (bench.py): called on the stream the stage was enqueued on after "start", "gram", "train<s>", "apply", "bps",
        and around the overlapped phase search ("post_begin", "post_end")."""
        m = mark or (lambda name: None)
        self.reset()
        m("start")
        adopted = self._adopt_prepared() if prefetch else False
        if not adopted:
            self._use_prep = None
            self.build_gram()
        m("gram")
        # The pending phase search IN PARTS (tier b): one part beside each relaxation pass of this capture's training (pass_hook below).  A pass keeps
        # the chip's SIMDs busy with one latency-bound wave each, and the whole search beside it - as many single-wave workgroups per SIMD as the LDS
        # allows - costs it a third of its speed (0.36 instead of 0.27 ms per pass).  A part of an eighth of the search is ONE wave per SIMD: gated by an
        # event in front of a pass's trainer launch it starts with the trainer, lives on the issue slots the trainer's lone waves leave (0-3 % of the
        # pass) and the events space the parts one pass apart.  (Gated BEHIND the trainer launch the parts start in the ~70 us of analysis between two
        # passes and share the chip with the control path, which is the critical path: 1137-1146 against 1163-1167 MSym/s at C3.)  Number of parts: the
        # trainer launches of the previous capture less two (one may have been enqueued in vain ahead of the decision that ended a sweep; the last part
        # also unwraps and de-rotates and should not hold up this capture's filter, which overwrites what it reads); what is left when the training is
        # over is enqueued then.  Bit-identical to one launch.
        parts_mode = self.tier == "b" and int(self.post_parts) != 1
        self._hook_calls = 0
        if parts_mode and self._post_pending:
            fixed = int(self.post_parts)
            self._post_n = fixed if fixed > 1 else max(1, min(16, (self._hook_calls_prev or 10) - 2))
            self._post_next, self._post_mark = 0, m
        if self._ev_pass is None:
            self._ev_pass = _lib.Event()

        def on_pass(sweep, p):
            self._hook_calls += 1
            if parts_mode and self._post_pending:     # (else nothing to gate: no packet on stream 0 either)
                self._ev_pass.record()                # stream 0: in front of the trainer launch of this pass
                self._post_part(gated=True)

        def side_work():
            if not parts_mode:
                self._enqueue_post(m)             # phase search of the previous overlapped pass, beside the stages below
            if prefetch:
                # ... and BEHIND that phase search: started together with it, the next capture's covariance kernel (chip-wide, streaming), eigen-solver
                # and acquisition crowd the first pass of this capture - 454 instead of 290 us, the model kernels 319 instead of 47
                # (profiles/r05_timeline_prefetch_v1.txt); the phase search is through ~1 ms into the capture, the preparation then has the rest of
                # the cold stage (whose passes leave 32 CUs free)
                self._prepare_next()
        # With prefetch the ~25 launches of that side work are made from INSIDE the first stage's call, right after its first pass is enqueued
        # (qh_pit_opts.on_pass0): in front of it they cost ~0.2 ms of host time during which stream 0 had nothing to run.
        defer = bool(prefetch and self.tier == "b" and adopted)
        if prefetch and self.tier == "b":
            self._prep_init()
            self._ev_main.record()                # stream 0 up to here: the capture the preparation reads is in place
        if not defer:
            side_work()
        for s in range(self.nstage):
            self.train(s, hook=side_work if (defer and s == 0) else None, pass_hook=on_pass if parts_mode else None)
            m("train%d" % s)
        if parts_mode:
            self._hook_calls_prev = self._hook_calls or self._hook_calls_prev or 9
            self._enqueue_post(m)                 # parts the passes did not take
        # The filter of this capture.  One capture at a time it follows the training on stream 0.  Consecutive captures (tier b, overlap): it goes onto
        # stream 2 - IN FRONT of this capture's phase search, which reads its output, and behind the previous capture's search, which read the buffer it
        # overwrites: the stream's own order is all the ordering those need - with a private copy of the taps (the next run's reset() restores the start
        # taps), so that stream 0 goes straight on to the next capture: the filter (87 us chip-wide at C3) and its launch gaps were ~0.1 ms of the ~0.2 ms
        # between the last pass of a capture and the first pass of the next one (round 6; profiles/r06_c3_timeline.txt).  Bit-identical.
        aside = bool(overlap and self.Mtestangles and self.tier == "b" and self.filter_aside)
        if aside:
            if self._wxy_f is None:
                self._wxy_f = DeviceArray(self.wxy.shape, self.ct)
            if self._ev_trained is None:
                self._ev_trained = _lib.Event()
            if self._ev_post is None:
                self._ev_ready, self._ev_post = _lib.Event(), _lib.Event()
            self.input_free()                      # the previous capture's filter, a whole training ago, read the taps copy
            self._wxy_f.copy_from(self.wxy)
            self._ev_trained.record()
            with _lib.on_stream(2):
                _lib.call("qh_stream_wait_event", self._ev_trained.ptr)
                _k.apply_filter_to_signal_dev(self.E, self.os, self._wxy_f, self.modes, self.eq)
                m("apply")
                self._ev_ready.record()            # stream 2: the filter has read the capture and written its output (input_free waits for it)
            self._post_running = False             # (the previous search is in front of this filter on stream 2; wait_post() waits for the NEW search's event)
            self._filter_pending = True
        else:
            if self._post_running:
                _lib.call("qh_stream_wait_event", self._ev_post.ptr)        # the filter output of the previous pass has been consumed
                self._post_running = False
            self._apply()
            m("apply")
        if prefetch and self._next_loaded:
            # the capture load_next() brought - prepared above, where that was possible - is the next one to be processed; the old one's buffer takes
            # the next load_next()
            self.E, self.E_next = self.E_next, self.E
            self._next_loaded = False
        if not self.Mtestangles:
            return
        if not overlap:
            self._recover()
            m("bps")
            return
        if self._ev_post is None:
            self._ev_ready, self._ev_post = _lib.Event(), _lib.Event()
        if not aside:
            self._ev_ready.record()               # stream 0 up to here: the filter output the pending phase search reads
        self._post_pending = True
        self._post_n = self._post_next = 0        # (not started: the next run decides whether it goes in parts)

    def _post_part(self, gated):
        """The next part of the pending phase search onto stream 2; ``gated``: behind ``_ev_pass`` (recorded in front of the trainer launch that is
        about to go onto stream 0)."""
        i, n, mark = self._post_next, self._post_n, self._post_mark
        with _lib.on_stream(2):
            if gated:
                _lib.call("qh_stream_wait_event", self._ev_pass.ptr)
            if i == 0:
                _lib.call("qh_stream_wait_event", self._ev_ready.ptr)      # the filter output the search reads
                if mark:
                    mark("post_begin")
            self._recover(part=i, nparts=n)
            if i == n - 1:
                if mark:
                    mark("post_end")
                self._ev_post.record()
        self._post_next = i + 1
        if i == n - 1:
            self._post_pending, self._post_running = False, True

    def _enqueue_post(self, mark=None):
        if not self._post_pending:
            return
        if self._post_n and self._post_next > 0:      # a search already under way in parts: the rest of them, now
            while self._post_pending:
                self._post_part(gated=False)
            self._post_n = 0
            return
        self._post_n = 0
        with _lib.on_stream(2):                   # (_ev_ready: recorded behind the filter of the pass whose phase search is pending)
            _lib.call("qh_stream_wait_event", self._ev_ready.ptr)
            if mark:
                mark("post_begin")
            self._recover()
            if mark:
                mark("post_end")
            self._ev_post.record()
        self._post_pending, self._post_running = False, True

    def wait_post(self, mark=None):
        """After ``run(overlap=True)``: enqueue the pending phase search; work enqueued from here on (stream 0) sees its results (and the filter's)."""
        self._enqueue_post(mark)
        self.input_free()
        if self._post_running:
            _lib.call("qh_stream_wait_event", self._ev_post.ptr)
            self._post_running = False

    # ------------------------------------------------------------------------------------------ results
    def fetch(self):
        """Synchronise and copy the results to the host as a dict of ndarrays."""
        self.wait_post()
        _lib.sync()
        res = dict(wxy=self.wxy.to_host(), err=tuple(e.to_host() for e in self.err), eq=self.eq.to_host(),
                   mu=tuple(m.to_host()[0] for m in self.mu))
        if self.Mtestangles:
            res.update(out=self.out.to_host(), ph=self.ph.to_host())
            if self.carrier == "bps":
                res.update(idx=self.idx.to_host())
            if self.Bbps is not None:
                res.update(idx2=self.idx2.to_host())
        return res

    def ser(self, symbols_tx, maxlag=256, window=4096, trim=0, sync="window"):
        """Symbol error rate of the recovered (else equalised) rows against the transmitted symbols, computed in HBM
        (``qampy_amd.core.ber_functions.cal_ser_dev``); needs the alphabet.  ``sync``: ``"window"`` - bounded search on decisions -
        or ``"full"`` - the full cross-correlation, any delay, the pattern continued periodically.  Returns one dict per row."""
        from .core import ber_functions as _ber
        self._prepare_tx(symbols_tx)
        return _ber.cal_ser_dev(self.out if self.Mtestangles else self.eq, self._idx_tx, self.alphabet, maxlag, window, trim, sync=sync,
                                sync_ws=self._sync_ws)

    def metrics(self, symbols_tx, snr_db=None, maxlag=256, window=4096, trim=0, llr_minmax=False, sync="window"):
        """Signal-quality metrics (SER, BER, EVM, SNR estimate, GMI, MI) of the recovered (else equalised) rows against the
        transmitted symbols, computed in HBM (``qampy_amd.core.ber_functions.cal_metrics_dev``); aligned as :meth:`ser`
        aligns them (``sync`` as there).  ``snr_db``: the SNR the GMI / MI are evaluated at (None: estimated per row).  One dict per row."""
        from .core import ber_functions as _ber
        self._prepare_tx(symbols_tx)
        return _ber.cal_metrics_dev(self.out if self.Mtestangles else self.eq, self._idx_tx, self.alphabet, snr_db, maxlag, window, trim,
                                    llr_minmax, sync=sync, sync_ws=self._sync_ws)

    def blind_metrics(self, block=None):
        """Signal quality of the recovered (else equalised) rows WITHOUT the transmitted symbols, computed in HBM (csrc/blind.hip) after the
        pending post-processing: one dict per row with ``snr`` (linear, the second / fourth-moment estimate ``cal_snr_qam``), ``snr_db``, ``s0``
        (``cal_s0``), ``evm_blind`` (``cal_evm`` on the S0-normalised row) and, for ``M == 4``, ``snr_qpsk_db`` (``cal_snr_blind_qpsk``).
        ``block``: additionally ``snr_trace`` and ``s0_trace`` ``(N // block,)``, the estimator on every whole block of ``block`` symbols.
        Only these scalars and traces cross to the host."""
        self.wait_post()
        return _blind_metrics(self.out if self.Mtestangles else self.eq, self.M, block, self._blind_ws)

    def _sync_workspace(self):
        return self._sync_ws

    def _prepare_tx(self, symbols_tx):
        """Alphabet and transmitted indices in HBM (cached per ``symbols_tx`` object), after the pending post-processing."""
        from .core import ber_functions as _ber
        if self.alphabet_host is None:
            raise ValueError("ser() and the metrics need the alphabet")
        if self.alphabet is None:
            self.alphabet = DeviceArray.from_host(self.alphabet_host)
        self.wait_post()
        if self._idx_tx is None or self._idx_tx_src is not symbols_tx:
            self._idx_tx = _ber.tx_indices_dev(np.ascontiguousarray(symbols_tx, dtype=self.ct), self.alphabet)
            self._idx_tx_src = symbols_tx

    def bytes_per_symbol(self):
        """Algorithmic HBM bytes per symbol period of one run() (general formula)."""
        cs = np.dtype(self.ct).itemsize
        nsel = self.modes.size
        train = sum(self.Niter[s] * cs * (self.nmodes * self.os + nsel) for s in range(self.nstage))
        apply_ = cs * (self.nmodes * self.os + nsel)
        bps = nsel * (cs + cs + cs // 2) if self.Mtestangles else 0
        if self.Mtestangles and self.carrier != "bps":
            # the field in twice and out once, the trace; V&V: one double angle per sample out and in (the partition keeps one per block)
            bps = nsel * (3 * cs + cs // 2 + (16 if self.carrier == "vv" else 0))
        if self.Mtestangles and self.Bbps is not None:
            bps += nsel * (cs + 4 + 4 + 4 + 4)     # fine stage: E and the coarse index in, the fine index out; the unwrap reads both indices
        return dict(train=train, apply=apply_, bps=bps, total=train + apply_ + bps)


class ReceiverGroup:
    """
    ``n`` captures IN FLIGHT on one GPU: ``n`` :class:`ResidentReceiver` objects of identical shape, each driven by its own host thread.
    The library keeps streams, scratch buffers and the tier-b solver's events per host thread (csrc/api.hip), so the receivers share
    nothing but the chip: what one capture leaves idle (between the relaxation passes of its trainer, during acquisition and the
    eigen-solver) the others use.  Every capture gets exactly the result of a receiver that runs alone (same kernels, same data); what
    changes is when the work is scheduled.  Measured at C3 (profiles/r04_in_flight.txt): 2 receivers 1.1x the throughput of one; two
    receiver PROCESSES on the GPU reach 1.2x (their streams do not share hardware queues).

        group = ReceiverGroup(2, nmodes, L, os, M, Ntaps, mu, tier="b", ...)      # the arguments of ResidentReceiver
        group.load(E)                          # the same capture into every receiver (or group.rx[i].load(E_i))
        group.run(steps)                       # `steps` passes in total, dealt round robin; returns when all of them are complete
        group.rx[i].fetch()                    # results of the last pass of receiver i
    """

    def __init__(self, n, *args, factory=None, sync=None, release=None, **kw):
        """``factory`` / ``sync`` / ``release`` (tests): what builds a receiver, waits for the calling thread's streams and releases them -
        ResidentReceiver, the library's qh_sync and qh_thread_release by default."""
        import queue
        import threading
        if n < 1:
            raise ValueError("at least one receiver")
        self._sync = sync if sync is not None else _lib.sync
        self._release = release if release is not None else (lambda: _lib.call("qh_thread_release"))
        self.rx = [(factory or ResidentReceiver)(*args, **kw) for _ in range(int(n))]
        if len(self.rx) > 1:
            # several captures in flight fill one another's gaps; a phase search held back for the gaps of ONE of them only waits (C3, three receivers:
            # 1175 MSym/s with the search in one launch, 993 in parts)
            for r in self.rx:
                if hasattr(r, "post_parts") and "QAMPY_POST_PARTS" not in _os.environ:
                    r.post_parts = 1
        self._sync()
        self._jobs = [queue.SimpleQueue() for _ in self.rx]
        self._done = queue.SimpleQueue()
        self._threads = [threading.Thread(target=self._work, args=(i,), daemon=True, name="qampy-receiver-%d" % i) for i in range(len(self.rx))]
        for t in self._threads:
            t.start()

    def _work(self, i):
        import threading
        if hasattr(self.rx[i], "_owner_thread"):
            self.rx[i]._owner_thread = threading.get_ident()
        while True:
            job = self._jobs[i].get()
            if job is None:
                self._release()                    # this thread's streams and scratch buffers
                return
            try:
                self._done.put((i, job(self.rx[i]), None))
            except BaseException as e:             # handed to the caller of run() / map()
                self._done.put((i, None, e))

    def map(self, fn, which=None):
        """``fn(receiver)`` on the thread of every receiver (or of those in ``which``) at the same time; the list of results."""
        which = range(len(self.rx)) if which is None else list(which)
        for i in which:
            self._jobs[i].put(fn)
        res, err = {}, None
        for _ in which:
            i, r, e = self._done.get()
            res[i], err = r, (e if e is not None else err)
        if err is not None:
            raise err
        return [res[i] for i in which]

    def load(self, E):
        for r in self.rx:
            r.load(E)
        self._sync()

    def run(self, steps, overlap=True, mark=None, prefetch=False, feed=None):
        """``steps`` passes of the hot path in total, receiver ``i`` taking passes i, i + n, ...; returns when all are complete on the
        device.  ``overlap``: as ResidentReceiver.run.  ``mark(i, k)``: a mark callback for pass k of receiver i (bench.py).
        ``feed(i, k, rx)``: called on receiver ``i``'s thread before its ``k``-th pass - where a caller hands it the capture that follows
        (``rx.load_next(...)``, or a resident array as ``rx.E_next`` with ``rx._next_loaded = True``)."""
        n = len(self.rx)
        share = [len(range(i, int(steps), n)) for i in range(n)]

        def job(i):
            def go(rx):
                for k in range(share[i]):
                    if feed is not None:
                        feed(i, k, rx)
                    rx.run(overlap=overlap, mark=mark(i, k) if mark else None, **({"prefetch": True} if prefetch else {}))
                rx.wait_post(mark(i, share[i]) if mark else None)
                self._sync()                   # this thread's streams
            return go
        for i in range(n):
            self._jobs[i].put(job(i))
        err = None
        for _ in range(n):
            _, _, e = self._done.get()
            err = e if e is not None else err
        if err is not None:
            raise err

    def pit_reports(self):
        return [r.pit_reports() for r in self.rx]

    def close(self):
        for q_ in self._jobs:
            q_.put(None)
        for t in self._threads:
            t.join(timeout=10.)
        self._threads = []
        for r in self.rx:
            if hasattr(r, "release_thread_state"):
                r.release_thread_state()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ChannelBank:
    """
    ``nch`` independent captures of identical shape (WDM channels) resident on ONE GPU and processed
    together.  One exact training chain occupies one workgroup, i.e. 1/256 of the chip, so the natural way to fill an
    MI355X with the exact recurrence is many channels side by side: the trainers take the channel as ``blockIdx.y``
    (one launch per stage for the whole bank), the Gram tables, the filter and the phase search - already chip-wide per
    capture - run channel after channel on the same stream.  Per channel the results are bit-identical to a
    :class:`ResidentReceiver` of that capture.

    HBM per channel (complex64, 2 modes, 2 samples/symbol, N symbols): capture 32 N, Gram table 1024 N, error traces 16 N per
    stage, outputs 40 N bytes - about 1.1 kB per symbol, so 288 GB hold e.g. 64 channels of 2^22 symbols.
    """

    def __init__(self, nch, nmodes, L, os, M, Ntaps, mu, trainer="auto", **kw):
        self.nch = int(nch)
        # trainer: "auto" = per-method choice of the single-capture path (look-ahead for cma-type stages: lowest latency, but
        # its Gram table is 1 KiB per step); "iterative" = block-iterative form for every stage: 10-25 % longer stages,
        # a quarter of the Gram table (256 B per step, built 2.8x faster) - more channels fit and aggregate throughput is higher
        self.trainer = {"auto": 0, "direct": 1, "lookahead": 2, "iterative": 3}[trainer]
        # one receiver object provides the shared constants and the per-channel views; its own big buffers are replaced
        self.rx = ResidentReceiver(nmodes, 8 * Ntaps * os, os, M, Ntaps, mu, **kw)       # tiny dummy capture
        r = self.rx
        if r.tier != "a":
            raise ValueError("a channel bank runs the exact recurrence (tier A)")
        if r.carrier != "bps":
            raise ValueError("a channel bank recovers the carrier by blind phase search (carrier='bps')")
        self.nmodes, self.L, self.os, self.Ntaps, self.ct, self.rt = int(nmodes), int(L), int(os), int(Ntaps), r.ct, r.rt
        TrSyms = kw.get("TrSyms", (None,) * r.nstage)
        self.TrSyms = tuple(_host._cal_training_symbol_len(os, Ntaps, L) if t is None else int(t) for t in TrSyms[:r.nstage])
        self.N = (self.L - self.Ntaps + 1) // self.os
        nsel = r.modes.size
        self.E = DeviceArray((self.nch, nmodes, L), self.ct)
        self.wxy = DeviceArray((self.nch, nmodes, nmodes, Ntaps), self.ct)
        self.wxy0 = DeviceArray.from_host(np.tile(_host._init_taps(Ntaps, nmodes, nmodes, self.ct), (self.nch, 1, 1, 1)))
        self.mu = [DeviceArray((self.nch,), self.rt) for _ in range(r.nstage)]
        self.mu_init = [DeviceArray.from_host(np.full(self.nch, m, dtype=self.rt)) for m in r.mu0]
        self.err = [DeviceArray((self.nch, nmodes, self.TrSyms[s] * r.Niter[s]), self.ct, zero=True) for s in range(r.nstage)]
        self.eq = DeviceArray((self.nch, nsel, self.N), self.ct)
        if r.Mtestangles:
            self.idx = DeviceArray((self.nch, nsel, self.N), np.int32)
            if r.Bbps is not None:
                self.idx2 = DeviceArray((self.nch, nsel, self.N), np.int32)
            self.ph = DeviceArray((self.nch, nsel, self.N), self.rt)
            self.out = DeviceArray((self.nch, nsel, self.N), self.ct)
        self._gram = None
        self._taps_b = self._ev_trained = self._ev_post = None      # run_pipelined: two copies of the taps and their events, made on first use
        _lib.sync()

    def load(self, ch, E):
        E = np.ascontiguousarray(np.asarray(E), dtype=self.ct)
        assert E.shape == (self.nmodes, self.L)
        self.E.row(ch).set(E)

    def run(self):
        """One pass of the hot path over all channels; enqueue only."""
        r = self.rx
        self.wxy.copy_from(self.wxy0)
        for m, m0 in zip(self.mu, self.mu_init):
            m.copy_from(m0)
        _lib.call("qh_set_trainer", self.trainer)
        try:
            self._run_stages(r)
        finally:
            _lib.call("qh_set_trainer", 0)

    def run_pipelined(self, steps):
        """
        ``steps`` passes over the bank, software-pipelined over the library's two streams: the trainers (and Gram tables) of
        pass k+1 run on stream 0 while filter + phase search of pass k run on stream 1 with a copy of that pass's taps.  The
        trainers keep every CU busy with one or two workgroups of 8 wavefronts - issue-limited, not throughput-limited - so
        chip-wide per-channel kernels can run beside them as far as registers and LDS allow: measured at 128 channels, 8 passes,
        987 instead of 1131 ms per pass with a 512-thread phase search, nothing with the (faster) 1024-thread one that is
        built in, whose workgroups claim every vector register of a SIMD.  Same results as :meth:`run`; enqueue only
        (``_lib.sync()`` to wait).
        """
        r = self.rx
        if self._taps_b is None:
            self._taps_b = [DeviceArray(self.wxy.shape, self.ct) for _ in range(2)]
            self._ev_trained, self._ev_post = [_lib.Event(), _lib.Event()], [_lib.Event(), _lib.Event()]
        try:
            for k in range(steps):
                p = k & 1
                if k >= 2:
                    _lib.call("qh_stream_wait_event", self._ev_post[p].ptr)        # the taps copy of pass k-2 has been consumed
                self.wxy.copy_from(self.wxy0)
                for m, m0 in zip(self.mu, self.mu_init):
                    m.copy_from(m0)
                _lib.call("qh_set_trainer", self.trainer)
                self._train_stages(r)
                _lib.call("qh_set_trainer", 0)
                self._taps_b[p].copy_from(self.wxy)
                self._ev_trained[p].record()
                with _lib.on_stream(1):
                    _lib.call("qh_stream_wait_event", self._ev_trained[p].ptr)
                    self._post_stages(r, self._taps_b[p])
                    self._ev_post[p].record()
        finally:
            _lib.call("qh_set_trainer", 0)

    def _run_stages(self, r):
        self._train_stages(r)
        self._post_stages(r, self.wxy)

    def _train_stages(self, r):
        # one Gram table per channel shared by the stages when the bank's tables fit the library's scratch budget; otherwise
        # the trainers build them per time chunk themselves (csrc/train_impl.h: gram_budget)
        budget = _lib.gram_budget_gb() * 2 ** 30
        per_step = (256 if self.trainer == 3 else 1024) * (np.dtype(self.ct).itemsize // 8)
        fits = self.nch * self.TrSyms[0] * per_step <= budget
        self._gram = _k.gram_build_batch_dev(self.E, self.os, self.Ntaps, self.TrSyms[0]) if (len(set(self.TrSyms)) == 1 and fits) else None
        for s in range(r.nstage):
            _k.train_equaliser_batch_dev(self.E, self.TrSyms[s], r.Niter[s], self.os, self.mu[s], self.wxy, r.modes, r.adaptive[s],
                                         r.symbols[s], r.methods[s], self.err[s], gram=self._gram)

    def _post_stages(self, r, wxy):
        for c in range(self.nch):
            _k.apply_filter_to_signal_dev(self.E.row(c), self.os, wxy.row(c), r.modes, self.eq.row(c))
            if r.Mtestangles and r.Bbps is not None:
                _dsp.bps_twostage_recover_dev(self.eq.row(c), r.Mtestangles, r.Bbps, r.alphabet, r.Nbps, self.idx.row(c), self.idx2.row(c), self.ph.row(c),
                                              self.out.row(c), angles=r.angles)
            elif r.Mtestangles:
                _dsp.bps_recover_dev(self.eq.row(c), r.Mtestangles, r.alphabet, r.Nbps, self.idx.row(c), self.ph.row(c), self.out.row(c), angles=r.angles)

    def ser(self, ch, symbols_tx, maxlag=256, window=4096, trim=0, sync="window"):
        """Per-row symbol errors of channel ``ch`` (device harness, see :meth:`ResidentReceiver.ser`)."""
        from .core import ber_functions as _ber
        r = self.rx
        if r.alphabet is None:
            r.alphabet = DeviceArray.from_host(r.alphabet_host)
        idx_tx = _ber.tx_indices_dev(np.ascontiguousarray(symbols_tx, dtype=self.ct), r.alphabet)
        return _ber.cal_ser_dev((self.out if r.Mtestangles else self.eq).row(ch), idx_tx, r.alphabet, maxlag, window, trim, sync=sync,
                                sync_ws=r._sync_ws)

    def metrics(self, ch, symbols_tx, snr_db=None, maxlag=256, window=4096, trim=0, llr_minmax=False, sync="window"):
        """Per-row signal-quality metrics of channel ``ch`` (device pass, see :meth:`ResidentReceiver.metrics`)."""
        from .core import ber_functions as _ber
        r = self.rx
        if r.alphabet is None:
            r.alphabet = DeviceArray.from_host(r.alphabet_host)
        idx_tx = _ber.tx_indices_dev(np.ascontiguousarray(symbols_tx, dtype=self.ct), r.alphabet)
        return _ber.cal_metrics_dev((self.out if r.Mtestangles else self.eq).row(ch), idx_tx, r.alphabet, snr_db, maxlag, window, trim, llr_minmax, sync=sync,
                                    sync_ws=r._sync_ws)

    def blind_metrics(self, ch, block=None):
        """Per-row blind signal quality of channel ``ch`` (see :meth:`ResidentReceiver.blind_metrics`)."""
        r = self.rx
        return _blind_metrics((self.out if r.Mtestangles else self.eq).row(ch), r.M, block, r._blind_ws)

    def fetch(self, ch):
        _lib.sync()
        res = dict(wxy=self.wxy.row(ch).to_host(), err=tuple(e.row(ch).to_host() for e in self.err), eq=self.eq.row(ch).to_host(),
                   mu=tuple(m.to_host()[ch] for m in self.mu))
        if self.rx.Mtestangles:
            res.update(out=self.out.row(ch).to_host(), ph=self.ph.row(ch).to_host(), idx=self.idx.row(ch).to_host())
            if self.rx.Bbps is not None:
                res.update(idx2=self.idx2.row(ch).to_host())
        return res
