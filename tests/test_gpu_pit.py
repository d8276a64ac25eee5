"""
Parallel-in-time training (tier b; qh_train_equaliser_*_pit_dev) on a real MI355X.

What is asserted:
  * the relaxation's fixed point IS the sequential recurrence: S passes over S segments reproduce the exact trainer (and
    the oracle) to rounding, for every kernel form that can take the segments;
  * with the linearised coarse correction the boundary defect falls several times per pass and a tight
    tolerance reproduces the exact taps / error trace to ~1e-3 in a handful of passes;
  * at scale (64-QAM, 41 taps, 2^20 symbol periods, CMA -> MRDE + 64-angle BPS) the default settings (tol = 1e-3: estimated rms
    deviation of the output from the sequential recurrence; segment 0 starts from the caller's taps) certify themselves and the
    MEASURED deviation from the exact cold-start path is inside that tolerance: output, taps and both error traces; symbol errors
    per mode within +-3 of the exact path AND of the CPU oracle on the same capture;
  * the entry point refuses what it cannot do, and tiny sweeps fall through to the exact path bit for bit.
"""
import warnings

import numpy as np
import pytest

from oracle import oracle
from qampy_amd import synth, _lib
from qampy_amd._lib import DeviceArray
from qampy_amd.core.equalisation import hip_equalisation as hk
from qampy_amd.core.equalisation import equalisation as core_eq
from qampy_amd.pipeline import ResidentReceiver

pytestmark = pytest.mark.gpu


def _setup(method, M, nsym=2 ** 14, ntaps=15, dtype=np.complex64, seed=41):
    sig = synth.make_capture(M, nsym, nmodes=2, snr_db=28, theta=np.pi / 5.6, dgd=30e-12, seed=seed, dtype=dtype)
    E = np.ascontiguousarray(np.asarray(sig))
    rt = np.float32 if dtype == np.complex64 else np.float64
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]) - 7          # not a multiple of 64: ragged last segment
    w0 = core_eq._init_taps(ntaps, 2, 2, dtype)
    if method in ("mrde", "sbd", "dd"):                                       # phase-sensitive functions start from converged taps
        _, w0, _ = hk.train_equaliser(E, tr, 2, 2, rt(2e-3), w0, None, False, core_eq._reshape_symbols(None, "mcma", M, dtype, 2), "mcma")
    sy = core_eq._reshape_symbols(sig.coded_symbols if method in core_eq.DECISION_BASED else None, method, M, dtype, 2)
    return sig, E, tr, w0, np.ascontiguousarray(sy), rt


# table size of the segment kernel's instantiation (qh_pit_last_launch): partitions of mrde at 64-QAM, slicer thresholds of sbd at 16-QAM
_NPART = {"mcma": 0, "cma": 0, "mrde": 3, "sbd": 3}


def _run_pit(E, tr, niter, mu, w0, sy, method, pit, rt):
    dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([mu], rt))
    dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((2, tr * niter), E.dtype, zero=True)
    rep = hk.PitReportBuffer()
    hk.train_equaliser_dev(dE, tr, niter, 2, dmu, dw, None, False, dsy, method, derr, pit=pit, report=rep)
    return dw.to_host(), derr.to_host(), rep.read()


@pytest.mark.parametrize("form", ["auto", "direct", "segment16", "segment8"])
@pytest.mark.parametrize("method,M", [("mcma", 16), ("cma", 16), ("mrde", 64), ("sbd", 16)])
def test_relaxation_fixed_point_is_the_sequential_recurrence(method, M, form, forms):
    if form.startswith("segment"):              # the throughput form (train_seg.h) with 16 / 8 lanes per chain, forced at this small size
        forms.set("pit_form", "segment")
        forms.set("seg_lanes", form[7:])
    elif form != "auto":
        forms.set("trainer", form)
    sig, E, tr, w0, sy, rt = _setup(method, M)
    eo, wo, _ = hk.train_equaliser(E, tr, 2, 2, rt(5e-4), w0.copy(), None, False, sy, method)
    S = 4
    # plain relaxation, no seeds, no acquisition, a tolerance that is never met: after S passes the triangular map has
    # propagated the true start taps through every segment
    w, e, rep = _run_pit(E, tr, 2, 5e-4, w0, sy, method, dict(segments=S, max_passes=S, tol=1e-12, correction=0, phase_seed=0, acquire=0, exact_redo_off=1), rt)
    assert rep["segments"] == S and rep["passes"] == S and len(rep["defect"]) == S
    if form.startswith("segment"):              # 2 x 15 taps: 2 taps per lane + 1 padding tap on 16 lanes, 6 + 3 on 8 lanes - and it was that kernel that ran
        lay = dict(lanes=16, tpl=2, rag=1) if form == "segment16" else dict(lanes=8, tpl=6, rag=3)
        assert _lib.pit_last_launch() == dict(form=1, npart=_NPART[method], adaptive=0, **lay)
    elif form == "direct":
        assert _lib.pit_last_launch()["form"] == 4
    np.testing.assert_allclose(w, wo, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(e, eo, rtol=2e-4, atol=1e-4)
    assert rep["defect"][-1] < 1e-4 and rep["defect"][-1] <= rep["defect"][0]


@pytest.mark.parametrize("analysis", ["eigen", "probe"])
@pytest.mark.parametrize("lanes", ["16", "8"])
@pytest.mark.parametrize("method,M", [("mcma", 16), ("cma", 64), ("mrde", 64)])
def test_coarse_correction_converges_to_the_exact_trajectory(method, M, lanes, analysis, forms):
    forms.set("pit_form", "segment")
    forms.set("seg_lanes", lanes)
    # analysis of a pass: in the eigenbasis of the input covariance (complex64 default) or with the round-2 probe of the capture
    forms.set("pit_probe", "1" if analysis == "probe" else "0")
    """16 segments, tight tolerance: the defect falls fast with the correction and the result agrees with the exact
    trainer far below the gradient noise; plain relaxation needs (many) more passes for the same defect."""
    sig, E, tr, w0, sy, rt = _setup(method, M, nsym=2 ** 16, ntaps=21)
    eo, wo, _ = hk.train_equaliser(E, tr, 1, 2, rt(1e-3), w0.copy(), None, False, sy, method)
    kw = dict(segments=16, max_passes=10, tol=2e-4, phase_seed=0, acquire=0, exact_redo_off=1)       # (the iteration itself: no exact-form way out)
    w, e, rep = _run_pit(E, tr, 1, 1e-3, w0, sy, method, dict(kw, correction=1), rt)
    lay = dict(lanes=16, tpl=4, rag=3) if lanes == "16" else dict(lanes=8, tpl=6, rag=3)          # 2 x 21 taps
    assert _lib.pit_last_launch() == dict(form=1, npart=_NPART[method], adaptive=0, **lay)
    w2, e2, rep2 = _run_pit(E, tr, 1, 1e-3, w0, sy, method, dict(kw, correction=0), rt)
    assert rep["converged"] and rep["correction"] and rep["passes"] <= 8, rep
    assert rep2["passes"] >= rep["passes"], (rep, rep2)
    g = np.exp(1j * np.angle(np.vdot(w.ravel(), wo.ravel()))) if method == "cma" else 1.0     # cma: common phase is free
    assert np.linalg.norm(wo - g * w) / np.linalg.norm(wo) < 5e-3
    nlast = e.shape[1] // 2
    assert abs(np.mean(np.abs(e[:, nlast:]) ** 2) / np.mean(np.abs(eo[:, nlast:]) ** 2) - 1) < 2e-2


@pytest.mark.parametrize("form", ["auto", "segment"])
def test_complex128_and_oracle(form, forms):
    if form == "segment":                       # the throughput form in double precision (16 lanes per chain; 8 lanes are single precision only)
        forms.set("pit_form", "segment")
    sig, E, tr, w0, sy, rt = _setup("mcma", 16, dtype=np.complex128)
    eo, wo, _ = oracle.train_equaliser(E, tr, 1, 2, 5e-4, w0.copy(), None, False, sy, "mcma")
    w, e, rep = _run_pit(E, tr, 1, 5e-4, w0, sy, "mcma", dict(segments=4, max_passes=4, tol=1e-14, correction=0, phase_seed=0, acquire=0, exact_redo_off=1), rt)
    if form == "segment":
        assert _lib.pit_last_launch() == dict(form=1, lanes=16, tpl=2, rag=1, npart=0, adaptive=0)
    np.testing.assert_allclose(w, wo, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(e, eo, rtol=1e-8, atol=1e-9)


def test_small_sweeps_fall_through_and_bad_calls_raise():
    sig, E, tr, w0, sy, rt = _setup("mcma", 16, nsym=2 ** 10)
    eo, wo, _ = hk.train_equaliser(E, tr, 1, 2, rt(1e-3), w0.copy(), None, False, sy, "mcma")
    w, e, rep = _run_pit(E, tr, 1, 1e-3, w0, sy, "mcma", {}, rt)        # automatic segment count: too short to cut -> exact path
    assert rep["segments"] == 1 and rep["converged"] and rep["exact_form"]
    assert np.array_equal(w, wo) and np.array_equal(e, eo)
    dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([1e-3], rt))
    dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((2, tr), E.dtype, zero=True)
    with pytest.raises(ValueError):
        hk.train_equaliser_dev(dE, tr, 1, 2, dmu, dw, None, False, dsy, "mcma", derr, pit=dict(nonsense=1))


def _exact_and_tier_b(E, tr, niter, mu, w0, sy, method, adaptive, pit, rt):
    """One training call through the exact entry point and through the parallel-in-time one: (taps, err, mu) of both + the report."""
    out = []
    for p in (None, pit):
        dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([mu], rt))
        dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((E.shape[0], tr * niter), E.dtype, zero=True)
        rep = hk.PitReportBuffer() if p is not None else None
        hk.train_equaliser_dev(dE, tr, niter, 2, dmu, dw, None, adaptive, dsy, method, derr, pit=p, report=rep)
        out.append((dw.to_host(), derr.to_host(), dmu.to_host()[0]))
    return out[0], out[1], rep.read()


@pytest.mark.parametrize("method,adaptive,dtype", [("sbd_data", False, np.complex64), ("sbd_data", True, np.complex64), ("mcma", "per-mode", np.complex64),
                                                   ("cma2", True, np.complex64), ("mrde", True, np.complex64), ("mcma", True, np.complex128)])
def test_tier_b_is_total_calls_without_a_parallel_solver_take_the_exact_form(method, adaptive, dtype):
    """Tier b returns the reference's result for EVERY call: where no parallel-in-time solver exists (data-aided training, one step size
    per mode, the adaptive step with an error function / precision the segment kernels do not carry) the library runs the exact form
    inside the call - bit-identical to the exact entry point - and reports it (``exact_form``)."""
    M = 64 if method == "mrde" else 16
    sig, E, tr, w0, sy, rt = _setup("mcma" if method == "sbd_data" else method, M, nsym=2 ** 13, dtype=dtype)
    if method == "sbd_data":
        Er = np.roll(E, 15 // 2, axis=1)                              # symbol i at the centre tap of window i (test/test_equalisation.py:109-110)
        sy = np.ascontiguousarray(np.asarray(sig.symbols)[:, :tr + 8].astype(dtype))
        E = np.ascontiguousarray(Er)
    (wa, ea, ma), (wb, eb, mb), rep = _exact_and_tier_b(E, tr, 1, 1e-3, w0, sy, method, adaptive, {}, rt)
    assert rep["exact_form"] and rep["converged"], rep
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb) and ma == mb


@pytest.mark.parametrize("method,M,niter", [("cma", 16, 1), ("cma", 16, 2), ("mcma", 16, 2), ("mrde", 64, 1), ("sbd", 16, 1)])
def test_uncertified_sweep_is_redone_in_the_exact_form(method, M, niter, forms):
    """A sweep the passes do not certify - here: one pass against a tolerance it cannot meet - is redone in the exact form from the taps the
    call started with, inside the call: taps AND error trace are the exact entry point's bit for bit (for cma this includes NOT turning
    the exact trace by the gauge phases of the failed pass), the report says ``exact_form``; with ``exact_redo_off`` the same call
    hands back the uncertified result and says ``converged`` False."""
    forms.set("pit_form", "segment")
    sig, E, tr, w0, sy, rt = _setup(method, M, nsym=2 ** 15, ntaps=21)
    pit = dict(segments=16, max_passes=1, tol=1e-9, acquire=0)
    (wa, ea, _), (wb, eb, _), rep = _exact_and_tier_b(E, tr, niter, 1e-3, w0, sy, method, False, pit, rt)
    assert rep["exact_form"] and rep["converged"] and rep["segments"] == 16, rep
    # (the pass that was not certified ran on the segment kernel: the record of the passes survives the exact redo)
    assert _lib.pit_last_launch() == dict(form=1, lanes=16, tpl=4, rag=3, npart=_NPART[method], adaptive=0)
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    (_, _, _), (wc, ec, _), rep2 = _exact_and_tier_b(E, tr, niter, 1e-3, w0, sy, method, False, dict(pit, exact_redo_off=1), rt)
    assert not rep2["converged"] and not rep2["exact_form"], rep2
    assert not np.array_equal(wa, wc)


@pytest.mark.parametrize("method", ["cma", "mcma"])
def test_adaptive_sweep_that_falls_back_returns_the_exact_error_trace(method):
    """The adaptive solver's way out (a sweep not certified within the passes) writes the error trace in the exact form; it must come back
    as it is - for cma (continuous symmetry) NOT turned by the gauge phases of the failed passes - and every mode's report must
    survive (``per_mode``)."""
    sig = synth.make_capture(16, 2 ** 17, nmodes=2, snr_db=25, theta=np.pi / 3, dgd=30e-12, linewidth=0., seed=1000, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    kw = dict(Ntaps=13, method=method, adaptive_stepsize=True)
    wa, ea = core_eq.equalise_signal(E, 2, 1.9e-3, 16, **kw)
    wb, eb = core_eq.equalise_signal(E, 2, 1.9e-3, 16, tier="b", pit=dict(max_passes=1, tol=1e-9), **kw)
    rep = core_eq.last_pit_reports()[0]
    assert rep["exact_form"] and rep["converged"] and len(rep["per_mode"]) == 2 and all(r["exact_form"] for r in rep["per_mode"]), rep
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)


def test_real_valued_methods_through_tier_b_take_the_exact_form():
    sig = synth.make_capture(16, 2 ** 13, nmodes=2, snr_db=25, theta=np.pi / 5.6, dgd=30e-12, seed=5, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    wa, ea = core_eq.equalise_signal(E, 2, 1e-3, 16, Ntaps=15, method="cma_real")
    wb, eb = core_eq.equalise_signal(E, 2, 1e-3, 16, Ntaps=15, method="cma_real", tier="b")
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    assert core_eq.last_pit_reports()[0]["exact_form"]


def test_ser_equivalence_at_scale():
    """BASELINE config 3 shape at 2^20 symbol periods: default tier-b settings against the exact path and the CPU oracle."""
    nsym, M, ntaps, mu = 2 ** 20, 64, 41, (2e-4, 2e-4)
    d = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=d["alphabet_host"])
    res = {}
    for name, tier, pit in (("a", "a", None), ("b", "b", None), ("b_loose", "b", dict(tol=1e-2))):
        rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier=tier, pit=pit, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        r = rx.fetch()
        from qampy_amd.core import ber_functions as ber
        r["ser"] = ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, 256, 8192, 2000)
        r["rep"] = rx.pit_reports()
        res[name] = r
        del rx
    errs = {k: [s["errors"] for s in v["ser"]] for k, v in res.items()}
    for k in ("b", "b_loose"):
        assert all(st["converged"] for st in res[k]["rep"]), res[k]["rep"]
        assert all(st["segments"] >= 64 for st in res[k]["rep"])
        assert all(abs(a - b) <= 3 for a, b in zip(errs["a"], errs[k])), errs
        # the device's certificate: the last pass's estimated rms deviation is below the tolerance it was held to
        assert all(st["deviation_rms"][-1] < st["tol"] and st["deviation"][-1] < 3 * st["tol"] for st in res[k]["rep"]), res[k]["rep"]
    assert all(st["passes"] <= 10 for st in res["b"]["rep"]) and all(st["passes"] <= 6 for st in res["b_loose"]["rep"]), (res["b"]["rep"], res["b_loose"]["rep"])
    assert res["b"]["rep"][-1]["tol"] == 1e-3 and res["b"]["rep"][0]["tol"] == ResidentReceiver.NONFINAL_TOL_FACTOR * 1e-3     # (non-final stage: error trace and taps, 3 tol)
    # measured deviation from the exact path, which starts from the same taps (modulo a common quarter turn per mode): relative tap
    # deviation, rms deviation of the equalised signal, rms deviation of the error traces (in units of the signal rms; an error
    # function multiplies an output deviation by its slope, up to ~2 for cma)
    def dev(r):
        out = []
        for m in range(2):
            g = 1j ** int(np.rint(np.angle(np.vdot(r["wxy"][m].ravel(), res["a"]["wxy"][m].ravel())) / (np.pi / 2)))
            et = [np.sqrt(np.mean(np.abs(ea[m] - g * eb[m]) ** 2)) for ea, eb in zip(res["a"]["err"], r["err"])]      # absolute: the signal has unit power
            out.append((np.linalg.norm(res["a"]["wxy"][m] - g * r["wxy"][m]) / np.linalg.norm(res["a"]["wxy"][m]),
                        np.sqrt(np.mean(np.abs(res["a"]["eq"][m] - g * r["eq"][m]) ** 2)), max(et)))
        return np.array(out)
    d_b, d_l = dev(res["b"]), dev(res["b_loose"])
    assert d_b[:, 1].max() < 1e-3 and d_b[:, 0].max() < 3e-3 and d_b[:, 2].max() < 3e-3, (d_b.tolist(), [r["rep"] for r in res.values()])
    assert d_l[:, 1].max() < 1e-2 and d_l[:, 0].max() < 3e-2 and d_l[:, 2].max() < 3e-2, (d_l.tolist(), [r["rep"] for r in res.values()])
    # the CPU oracle (reference-flag build) on the same capture
    E = d["E"].to_host()
    w = core_eq._init_taps(ntaps, 2, 2, np.complex64)
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1])
    for m, mu_s in zip(("cma", "mrde"), mu):
        _, w, _ = oracle.train_equaliser(E, tr, 1, 2, np.float32(mu_s), w, None, False, core_eq._reshape_symbols(None, m, M, np.complex64, 2), m, fast=True)
    eq = oracle.apply_filter_to_signal(E, 2, w, fast=True)
    dq = DeviceArray.from_host(eq)
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
    rx.eq.copy_from(dq)
    rx.recover()                                     # carrier recovery of the CPU-equalised signal on the device: same BPS for both
    from qampy_amd.core import ber_functions as ber
    e_cpu = [s["errors"] for s in ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, 256, 8192, 2000)]
    assert all(abs(a - b) <= 3 for a, b in zip(e_cpu, errs["b"])), (e_cpu, errs)


def test_ser_equivalence_with_symbol_errors():
    """24 dB SNR: ~1.2e-3 symbol error rate, where an output deviation of 1 % rms from the sequential result would already cost
    15 % more errors (the error rate moves with (d/sigma)^2 ~ 10 times the relative change of sigma).  Default tolerance (1e-3):
    error counts within 3 standard deviations of the exact path's (the residual difference flips borderline decisions both ways)."""
    nsym, M, ntaps, mu = 2 ** 21, 64, 41, (2e-4, 2e-4)
    d = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=24, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1001)
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=d["alphabet_host"])
    from qampy_amd.core import ber_functions as ber
    errs, reps = {}, {}
    for tier in ("a", "b"):
        rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier=tier, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        errs[tier] = [s["errors"] for s in ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, 256, 8192, 2000)]
        reps[tier] = rx.pit_reports()
        del rx
    assert all(st["converged"] for st in reps["b"]), reps["b"]
    assert min(errs["a"]) > 500, errs                                   # the capture does have symbol errors
    for a, b in zip(errs["a"], errs["b"]):
        assert abs(a - b) <= 3 * np.sqrt(a), (errs, reps["b"])


def test_tier_b_through_the_mirrored_api():
    """`tier="b"` on QAMpy's own call surface (equalise_signal / dual_mode_equalisation): same return values, device reports through
    last_pit_reports(); against the default exact path on the same signal object."""
    import qampy_amd
    sig = synth.make_capture(64, 2 ** 18, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=5, dtype=np.complex64)
    ea, wa, (e1a, e2a) = qampy_amd.equalisation.dual_mode_equalisation(sig, (2e-4, 2e-4), 41, methods=("cma", "mrde"))
    assert core_eq.last_pit_reports() == []
    eb, wb, (e1b, e2b) = qampy_amd.equalisation.dual_mode_equalisation(sig, (2e-4, 2e-4), 41, methods=("cma", "mrde"), tier="b")
    reps = core_eq.last_pit_reports()
    assert len(reps) == 2 and all(r["converged"] for r in reps) and reps[0]["acquisition"]["steps"] > 0 and reps[1]["acquisition"]["steps"] == 0
    assert type(eb) is type(ea) and eb.shape == ea.shape and e1b.shape == e1a.shape and wb.shape == wa.shape
    for m in range(2):
        g = 1j ** int(np.rint(np.angle(np.vdot(wb[m].ravel(), wa[m].ravel())) / (np.pi / 2)))
        assert np.sqrt(np.mean(np.abs(np.asarray(ea)[m] - g * np.asarray(eb)[m]) ** 2)) < 1e-2
    ra, _ = qampy_amd.phaserec.bps(ea, 64, 20)
    rb, _ = qampy_amd.phaserec.bps(eb, 64, 20)
    for m in range(2):
        na = synth.count_symbol_errors(np.asarray(ra)[m], sig.symbols, sig.coded_symbols, trim=2000)[0]
        nb = synth.count_symbol_errors(np.asarray(rb)[m], sig.symbols, sig.coded_symbols, trim=2000)[0]
        assert abs(na - nb) <= 3, (na, nb)
    # one stage, warm start from given taps: no acquisition; bad option -> ValueError
    w2, err = qampy_amd.equalisation.equalise_signal(sig, 2e-4, wxy=wa.copy(), method="mrde", tier="b")
    r = core_eq.last_pit_reports()
    assert len(r) == 1 and r[0]["acquisition"]["steps"] == 0 and r[0]["converged"]
    with pytest.raises(ValueError):
        qampy_amd.equalisation.equalise_signal(sig, 2e-4, Ntaps=41, method="cma", tier="c")
    # one step size per mode: no parallel-in-time solver - tier b takes the exact form and says so, results identical to tier a
    wpa, epa = qampy_amd.equalisation.equalise_signal(sig, 2e-4, Ntaps=41, method="cma", adaptive_stepsize="per-mode")
    wpb, epb = qampy_amd.equalisation.equalise_signal(sig, 2e-4, Ntaps=41, method="cma", tier="b", adaptive_stepsize="per-mode")
    assert core_eq.last_pit_reports()[0]["exact_form"] and np.array_equal(wpa, wpb) and np.array_equal(epa, epb)


@pytest.mark.parametrize("os_", [1, 3])
def test_segment_form_at_other_sampling_rates(os_, forms):
    """The throughput form shares one sample window per PAIR of steps at 2 samples per symbol; every other rate takes its plain
    step-by-step loop: S passes of plain relaxation over S segments are the sequential recurrence there too.  At 3 samples per symbol
    a chunk of 64 steps does not fit an LDS row: a latency form takes the passes (and the launch record says so) - same result."""
    forms.set("pit_form", "segment")
    sig = synth.make_capture(16, 2 ** 13, nmodes=2, os=os_, snr_db=28, theta=np.pi / 5.6, dgd=30e-12, seed=43, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    ntaps = 9
    tr = (E.shape[1] - ntaps + 1) // os_ - 5
    w0 = core_eq._init_taps(ntaps, 2, 2, np.complex64)
    sy = np.ascontiguousarray(core_eq._reshape_symbols(None, "mcma", 16, np.complex64, 2))
    dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([5e-4], np.float32))
    eo, wo, _ = hk.train_equaliser(E, tr, 1, os_, np.float32(5e-4), w0.copy(), None, False, sy, "mcma")
    dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((2, tr), np.complex64, zero=True)
    rep = hk.PitReportBuffer()
    hk.train_equaliser_dev(dE, tr, 1, os_, dmu, dw, None, False, dsy, "mcma", derr,
                           pit=dict(segments=4, max_passes=4, tol=1e-12, correction=0, phase_seed=0, acquire=0, exact_redo_off=1), report=rep)
    r = rep.read()
    assert r["segments"] == 4 and r["passes"] == 4
    if os_ == 1:
        assert _lib.pit_last_launch() == dict(form=1, lanes=16, tpl=2, rag=1, npart=0, adaptive=0)      # 2 x 9 taps: 5 lanes of 2 taps per mode
    else:
        assert _lib.pit_last_launch()["form"] in (2, 3, 4)
    np.testing.assert_allclose(dw.to_host(), wo, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(derr.to_host(), eo, rtol=2e-4, atol=1e-4)


def test_no_certificate_without_the_estimate():
    """SURVEY 8d's own step sizes (1e-3, 5e-4) on a 2^15-symbol 64-QAM capture: round 2's stop rule (boundary defects only, after the
    correction had been switched off) called the mrde stage converged with taps 1e-2 off.  Whatever the device certifies must hold when
    measured against the exact path; what it cannot certify it must report as not converged."""
    nsym = 2 ** 15
    d = synth.make_capture_dev(64, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=0., seed=42)
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=d["alphabet_host"])
    res = {}
    for tier in ("a", "b"):
        rx = ResidentReceiver(2, 2 * nsym, 2, 64, 41, (1e-3, 5e-4), tier=tier, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        res[tier] = rx.fetch()
        res[tier]["rep"] = rx.pit_reports()
        del rx
    for st in res["b"]["rep"]:
        assert (not st["converged"]) or (st["deviation_rms"] and 0 <= st["deviation_rms"][-1] < st["tol"]), st
    if all(st["converged"] for st in res["b"]["rep"]):
        for m in range(2):
            g = 1j ** int(np.rint(np.angle(np.vdot(res["b"]["wxy"][m].ravel(), res["a"]["wxy"][m].ravel())) / (np.pi / 2)))
            assert np.sqrt(np.mean(np.abs(res["a"]["eq"][m] - g * res["b"]["eq"][m]) ** 2)) < 1e-3
            assert np.linalg.norm(res["a"]["wxy"][m] - g * res["b"]["wxy"][m]) / np.linalg.norm(res["a"]["wxy"][m]) < 3e-3


def test_phase_blind_stage_ends_in_the_frame_of_the_start_taps():
    """cma leaves the common phase of an output mode free; the segments of a pass sit in their own frames.  The result - taps and error
    trace - is taken into the frame of segment 0, i.e. of the caller's start taps: against the exact path the taps agree without any
    fitted rotation beyond the milliradians the gauge estimates leave, and so does the error trace along the whole sweep."""
    nsym = 2 ** 20
    d = synth.make_capture_dev(64, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    kw = dict(methods=("cma",), Niter=(1,), Mtestangles=None, alphabet=d["alphabet_host"])
    res = {}
    for tier in ("a", "b"):
        rx = ResidentReceiver(2, 2 * nsym, 2, 64, 41, (2e-4,), tier=tier, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        res[tier] = rx.fetch()
        res[tier]["rep"] = rx.pit_reports()
        del rx
    assert res["b"]["rep"][0]["converged"], res["b"]["rep"]
    for m in range(2):
        wa, wb = res["a"]["wxy"][m].ravel(), res["b"]["wxy"][m].ravel()
        assert abs(np.angle(np.vdot(wb, wa))) < 5e-3                                   # no free rotation left
        assert np.linalg.norm(wa - wb) / np.linalg.norm(wa) < 6e-3
        ea, eb = res["a"]["err"][0][m], res["b"]["err"][0][m]
        n4 = ea.size // 4
        for q in range(4):                                                               # every quarter of the sweep, not only its end
            assert np.sqrt(np.mean(np.abs(ea[q * n4:(q + 1) * n4] - eb[q * n4:(q + 1) * n4]) ** 2)) < 6e-3


def test_coarse_correction_above_96_taps():
    """2 x 61 taps = 122 tap directions per output mode (round 2 dropped to plain relaxation above 96 and could certify nothing about
    the weakly excited directions): eigen-solver with logged rotations (A alone fills the LDS), basis products on four waves of MFMA
    rows; the passes run in a latency form (the throughput form holds up to 48 taps at 2 samples per symbol).  Certified, and the
    certificate holds against the exact path."""
    nsym = 2 ** 17
    d = synth.make_capture_dev(16, nsym, nmodes=2, snr_db=25, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=7)
    kw = dict(methods=("mcma",), Niter=(1,), Mtestangles=None, alphabet=d["alphabet_host"])
    res = {}
    for tier in ("a", "b"):
        rx = ResidentReceiver(2, 2 * nsym, 2, 16, 61, (3e-4,), tier=tier, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        res[tier] = rx.fetch()
        res[tier]["rep"] = rx.pit_reports()
        del rx
    st = res["b"]["rep"][0]
    assert st["correction"] and st["segments"] >= 16 and st["deviation_rms"] and st["deviation_rms"][-1] >= 0, st
    assert st["converged"], st
    for m in range(2):
        g = 1j ** int(np.rint(np.angle(np.vdot(res["b"]["wxy"][m].ravel(), res["a"]["wxy"][m].ravel())) / (np.pi / 2)))
        assert np.sqrt(np.mean(np.abs(res["a"]["eq"][m] - g * res["b"]["eq"][m]) ** 2)) < 1e-3
        assert np.linalg.norm(res["a"]["wxy"][m] - g * res["b"]["wxy"][m]) / np.linalg.norm(res["a"]["wxy"][m]) < 3e-3


@pytest.mark.parametrize("log2n", [17, 20])
def test_adaptive_step_recipe_through_tier_b(log2n):
    """The reference script's recipe (Scripts/64_qam_equalisation.py:26-32: 64-QAM, 13 taps, mu = 1.9e-3, mcma -> mddma,
    adaptive_stepsize=(True, True), the reference's shared step size carried from mode to mode) through tier='b' against the exact
    path on the same capture.  A mode the passes can agree on is certified by the device (r = 1/mu and the previous error are boundary
    states next to the taps); one they cannot - the blind stage's modes, which start from centre-spike taps with a decaying / tiny
    step - is redone in the exact form (report: converged = 2), so EVERY result has to hold against the exact path: taps, final
    step size, error traces (the decision-directed stage's traces differ where a decision fell the other way)."""
    nsym = 2 ** log2n
    sig = synth.make_capture(64, nsym, nmodes=2, snr_db=25, theta=np.pi / 3, dgd=30e-12, linewidth=0., seed=1000, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    kw = dict(Ntaps=13, methods=("mcma", "mddma"), adaptive_stepsize=(True, True), symbols=sig.coded_symbols, apply=False)
    wa, (e1a, e2a) = core_eq.dual_mode_equalisation(E, 2, (1.9e-3, 1.9e-3), 64, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # nothing uncertified may come back
        wb, (e1b, e2b) = core_eq.dual_mode_equalisation(E, 2, (1.9e-3, 1.9e-3), 64, tier="b", **kw)
    reps = core_eq.last_pit_reports()
    assert len(reps) == 2 and all(r["converged"] for r in reps)
    assert not reps[1]["exact_form"] and reps[1]["segments"] > 16, reps[1]          # the decision-directed stage (last mode) ran in parallel in time
    for m in range(2):
        assert np.linalg.norm(wa[m] - wb[m]) / np.linalg.norm(wa[m]) < 3e-3
        assert np.sqrt(np.mean(np.abs(e1a[m] - e1b[m]) ** 2)) < 3e-3
        assert np.sqrt(np.mean(np.abs(e2a[m] - e2b[m]) ** 2)) < 5e-3
    assert not reps[0]["exact_form"], reps[0]                                         # ... and so did the blind stage's last mode
    # the resident chain (arrays stay in HBM) takes the same path
    if log2n == 17:
        res = {}
        for tier in ("a", "b"):
            rx = ResidentReceiver(2, E.shape[1], 2, 64, 13, (1.9e-3, 1.9e-3), methods=("mcma", "mddma"), Niter=(1, 1), adaptive_stepsize=(True, True),
                                  Mtestangles=None, alphabet=sig.coded_symbols, tier=tier)
            rx.load(E)
            rx.run()
            res[tier] = rx.fetch()
            del rx
        for m in range(2):
            assert np.linalg.norm(res["a"]["wxy"][m] - res["b"]["wxy"][m]) / np.linalg.norm(res["a"]["wxy"][m]) < 3e-3
            assert np.sqrt(np.mean(np.abs(res["a"]["eq"][m] - res["b"]["eq"][m]) ** 2)) < 1e-3
    # the oracle (CPU restatement of the reference's loop) on the short capture, first stage: float32 rounding moves the sign tests of
    # adapt_step, so the bar is the loose one of a chaotic recurrence - the tight comparison above is with the exact HIP path, which the
    # golden vectors pin to the reference (tests/test_gpu_parity.py)
    if log2n == 17:
        w1, err1 = core_eq.equalise_signal(E, 2, 1.9e-3, 64, Ntaps=13, method="mcma", adaptive_stepsize=True, tier="b")
        sy = core_eq._reshape_symbols(None, "mcma", 64, np.complex64, 2)
        tr = core_eq._cal_training_symbol_len(2, 13, E.shape[1])
        eo, wo, _ = oracle.train_equaliser(E, tr, 1, 2, np.float32(1.9e-3), core_eq._init_taps(13, 2, 2, np.complex64), None, True, sy, "mcma")
        wo = np.asarray(wo)
        assert np.linalg.norm(wo - w1) / np.linalg.norm(wo) < 5e-2
        assert abs(np.mean(np.abs(eo[:, -4096:]) ** 2) / np.mean(np.abs(err1[:, -4096:]) ** 2) - 1) < 5e-2


@pytest.mark.parametrize("M,ntaps,mu,snr", [(64, 41, (3e-4, 1e-4), 28), (16, 21, (1e-3, 2e-4), 22)])
def test_default_recipe_mcma_sbd_certifies(M, ntaps, mu, snr):
    """The API's own default pair (qampy/equalisation.py:194-195: methods=("mcma", "sbd")) through tier b at 2^20 symbols, 16- and 64-QAM: both
    stages certified by the device WITHOUT the exact-form way out, and the result holds against the exact path (equaliser output <= tol,
    taps <= 3 tol, symbol errors +-3) and - decisions - against the CPU oracle.  The sbd stage starts from taps that are locked to the
    carrier phase at the END of the capture and pulls in over its first segments: a non-linear transient that the passes can only follow
    one segment at a time; the solver notices that its estimate sits in the head of the sweep only and repeats the stage with that
    stretch as an exact head (qh_pit_opts.head_steps / head_auto_off) - sequential there, parallel in time after it."""
    nsym = 2 ** 20
    d = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=snr, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    kw = dict(methods=("mcma", "sbd"), Niter=(1, 1), Mtestangles=64 if M == 64 else 32, Nbps=20, alphabet=d["alphabet_host"])
    res = {}
    from qampy_amd.core import ber_functions as ber
    for tier in ("a", "b"):
        rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier=tier, **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        res[tier] = rx.fetch()
        res[tier]["rep"] = rx.pit_reports()
        res[tier]["ser"] = [r["errors"] for r in ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, 256, 8192, 2000)]
        del rx
    reps = res["b"]["rep"]
    assert all(r["converged"] and not r["exact_form"] for r in reps), reps
    assert all(r["deviation_rms"][-1] < r["tol"] for r in reps), reps
    # Error traces: the mcma stage's over the whole sweep.  The sbd stage's is held to the tolerance from the second quarter of the sweep on;
    # in its pull-in (the first ~10^5 steps: the exact trace's power is 5-10 x its steady state there, decisions are wrong by the thousand) the
    # recurrence AMPLIFIES whatever its start taps differ by - the 1e-3 by which tier b's mcma result differs from the exact path's comes
    # out as ~5e-3 in the trace there and re-merges afterwards (measured: 0.5e-4 for the rest of the sweep) - so that stretch is bounded loosely.
    dev = []
    for m in range(2):
        g = 1j ** int(np.rint(np.angle(np.vdot(res["b"]["wxy"][m].ravel(), res["a"]["wxy"][m].ravel())) / (np.pi / 2)))
        ed = [res["a"]["err"][s_][m] - res["b"]["err"][s_][m] for s_ in range(2)]
        q = ed[1].size // 4
        dev.append(dict(g=g, eq=float(np.sqrt(np.mean(np.abs(res["a"]["eq"][m] - res["b"]["eq"][m]) ** 2) / np.mean(np.abs(res["a"]["eq"][m]) ** 2))),
                        taps=float(np.linalg.norm(res["a"]["wxy"][m] - res["b"]["wxy"][m]) / np.linalg.norm(res["a"]["wxy"][m])),
                        err1=float(np.sqrt(np.mean(np.abs(ed[0]) ** 2))), err2_pull_in=float(np.sqrt(np.mean(np.abs(ed[1][:q]) ** 2))),
                        err2_rest=float(np.sqrt(np.mean(np.abs(ed[1][q:]) ** 2)))))
    for m, d_ in enumerate(dev):
        assert d_["g"] == 1 and d_["eq"] < 1e-3 and d_["taps"] < 3e-3, dev
        assert d_["err1"] < 3e-3 and d_["err2_rest"] < 3e-3 and d_["err2_pull_in"] < 3e-2, dev
        assert abs(res["a"]["ser"][m] - res["b"]["ser"][m]) <= 3, (res["a"]["ser"], res["b"]["ser"])


def test_exact_head_option():
    """qh_pit_opts.head_steps: the first head_steps steps of the sweep in the exact form (bit for bit the exact trainer's error trace there),
    the segments after it; the result is the sequential recurrence's within the tolerance like any tier-b call."""
    sig, E, tr, w0, sy, rt = _setup("mrde", 64, nsym=2 ** 17, ntaps=21)
    (wa, ea, _), (wb, eb, _), rep = _exact_and_tier_b(E, tr, 1, 5e-4, w0, sy, "mrde", False, dict(acquire=0, head_steps=8192, head_auto_off=1), rt)
    assert rep["converged"] and not rep["exact_form"] and rep["segments"] >= 8, rep
    assert np.array_equal(ea[:, :8192], eb[:, :8192])
    for m in range(2):
        assert np.linalg.norm(wa[m] - wb[m]) / np.linalg.norm(wa[m]) < 3e-3
        assert np.sqrt(np.mean(np.abs(ea[m] - eb[m]) ** 2)) < 3e-3


@pytest.mark.parametrize("tier", ["a", "b"])
def test_overlapped_passes_give_the_results_of_one_capture_at_a_time(tier):
    """ResidentReceiver.run(overlap=True): the phase search of pass k is enqueued on stream 2 behind the covariance kernel of pass k + 1 and
    runs beside its training.  Two DIFFERENT captures handed over one after the other: what fetch() returns after each is bit for bit what the
    same receiver returns one capture at a time - also for the capture whose phase search was still pending when the next one was loaded
    into the input buffer (the search reads the filter output, not the capture)."""
    nsym, M, ntaps, mu = 2 ** 17, 64, 41, (1e-3, 5e-4)
    caps = [synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=sd) for sd in (1000, 1003)]
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=caps[0]["alphabet_host"])
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier=tier, **kw)
    serial = []
    for c in caps:
        rx.E.copy_from(c["E"])
        rx.run()
        serial.append(rx.fetch())
    # overlapped: capture 0, then capture 1 while the search of capture 0 is pending; the recovered signal of capture 0 is read in between
    rx.E.copy_from(caps[0]["E"])
    rx.run(overlap=True)
    rx.input_free()                             # (tier b: the filter of capture 0 reads rx.E on stream 2)
    rx.E.copy_from(caps[1]["E"])
    rx.run(overlap=True)                        # enqueues the search of capture 0 beside this training
    _lib.sync()
    out0 = {k: getattr(rx, k).to_host() for k in ("out", "ph", "idx")}
    for k in out0:
        assert np.array_equal(out0[k], serial[0][k]), (tier, k, "capture 0, search overlapped with the training of capture 1")
    res1 = rx.fetch()                           # flushes the pending search of capture 1
    for k in ("wxy", "eq", "out", "ph", "idx"):
        assert np.array_equal(res1[k], serial[1][k]), (tier, k, "capture 1")
    # and a plain run after overlapped ones is unaffected
    rx.E.copy_from(caps[0]["E"])
    rx.run()
    res0 = rx.fetch()
    for k in ("wxy", "eq", "out", "ph", "idx"):
        assert np.array_equal(res0[k], serial[0][k]), (tier, k, "plain run after overlapped ones")


@pytest.mark.parametrize("parts", [1, 3, 8, 16])
def test_phase_search_in_parts_between_the_passes_is_bit_identical(parts):
    """run(overlap=True), tier b: the pending phase search goes onto stream 2 in `post_parts` parts, one beside each trainer launch of the next capture
    (qh_pit_opts.on_pass, qh_bps_recover_part_c64_dev); more parts than passes: the rest when the training is over.  Three captures handed over one
    after the other: every result bit for bit that of one capture at a time."""
    nsym, M, ntaps, mu = 2 ** 17, 64, 41, (1e-3, 5e-4)
    caps = [synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=sd) for sd in (1000, 1003, 1001)]
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=caps[0]["alphabet_host"])
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier="b", **kw)
    serial = []
    for c in caps:
        rx.E.copy_from(c["E"])
        rx.run()
        serial.append(rx.fetch())
    rx.post_parts = parts
    got = []
    for i, c in enumerate(caps):
        rx.input_free()                         # (the filter of capture i - 1 reads rx.E on stream 2)
        rx.E.copy_from(c["E"])
        rx.run(overlap=True)                    # the search of capture i - 1 in parts between this capture's passes
        if i > 0:
            _lib.sync()
            got.append({k: getattr(rx, k).to_host() for k in ("out", "ph", "idx")})
    got.append(rx.fetch())                      # the search of the last capture: pending until here
    for i in range(len(caps)):
        for k in ("out", "ph", "idx"):
            assert np.array_equal(got[i][k], serial[i][k]), (parts, i, k)
    for k in ("wxy", "eq"):
        assert np.array_equal(got[-1][k], serial[-1][k]), (parts, k)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_bps_recover_in_parts_equals_one_call(dtype):
    """qh_bps_recover_part_*_dev: nparts calls give what one call gives (streaming kernel: a run of chunks per part; the other kernels: the last part
    does it all)."""
    from qampy_amd.core import hip_dsp
    from qampy_amd import theory
    rng = np.random.default_rng(5)
    M, L, A, N = 16, 70001, 32, 12
    sy = theory.cal_symbols_qam(M).astype(dtype)
    sy /= np.sqrt(np.mean(np.abs(sy) ** 2))
    ph = np.cumsum(rng.normal(0, 2e-2, (2, L)), axis=1)
    E = (sy[rng.integers(0, M, (2, L))] * np.exp(1j * ph) + 0.05 * (rng.normal(size=(2, L)) + 1j * rng.normal(size=(2, L)))).astype(dtype)
    D = _lib.DeviceArray
    rt = np.float32 if dtype == np.complex64 else np.float64
    dE, dsy, dang = D.from_host(E), D.from_host(sy), D.from_host(hip_dsp.test_angle_grid(A, rt))
    res = []
    for nparts in (1, 2, 7):
        idx, pho, out = D((2, L), np.int32), D((2, L), rt), D((2, L), dtype)
        for part in range(nparts):
            hip_dsp.bps_recover_dev(dE, A, dsy, N, idx, pho, out, angles=dang, part=part, nparts=nparts)
        _lib.sync()
        res.append((idx.to_host(), pho.to_host(), out.to_host()))
    for r in res[1:]:
        for a, b in zip(r, res[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("tier", ["a", "b"])
def test_receiver_group_gives_every_capture_the_single_receiver_result(tier):
    """pipeline.ReceiverGroup: two captures in flight, one host thread and one set of library streams / scratch buffers each (csrc/api.hip keeps
    them per thread).  Different captures in the two receivers, several passes each: bit for bit the results of a receiver that runs alone."""
    from qampy_amd.pipeline import ReceiverGroup
    nsym, M, ntaps, mu = 2 ** 17, 64, 41, (1e-3, 5e-4)
    caps = [synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=sd) for sd in (1000, 1003)]
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=caps[0]["alphabet_host"])
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, tier=tier, **kw)
    alone = []
    for c in caps:
        rx.E.copy_from(c["E"])
        rx.run()
        alone.append(rx.fetch())
    g = ReceiverGroup(2, 2, 2 * nsym, 2, M, ntaps, mu, tier=tier, **kw)
    try:
        for r, c in zip(g.rx, caps):
            r.E.copy_from(c["E"])
        _lib.sync()
        g.run(6)                                 # three passes per receiver, at the same time
        for i, r in enumerate(g.rx):
            res = r.fetch()
            for k in ("wxy", "eq", "out", "ph", "idx"):
                assert np.array_equal(res[k], alone[i][k]), (tier, i, k)
            assert all(np.array_equal(a, b) for a, b in zip(res["err"], alone[i]["err"])), (tier, i, "error traces")
        if tier == "b":
            assert all(st["converged"] for rp in g.pit_reports() for st in rp)
        # an exception on a worker thread reaches the caller
        with pytest.raises(ZeroDivisionError):
            g.map(lambda r: 1 // 0)
    finally:
        g.close()


def test_result_of_a_capture_does_not_depend_on_what_the_receiver_saw_before():
    """A resident tier-b receiver hands the acquisition chunk length of its FIRST capture back to the library for the later ones (so that a call
    need not wait for the device to derive it from the signal power, qh_pit_opts.acq_chunk).  The chunk is 2 / mu_acq rounded to a power of two:
    a second capture with 6 % more power gets bit for bit the result a fresh receiver gives it."""
    nsym, M, ntaps, mu = 2 ** 20, 64, 41, (2e-4, 2e-4)
    a = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    b = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1003)
    Eb = DeviceArray.from_host(np.ascontiguousarray(b["E"].to_host() * np.complex64(1.03)))
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=a["alphabet_host"], tier="b")
    fresh = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
    fresh.E.copy_from(Eb)
    fresh.run()
    want = fresh.fetch()
    seen = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
    seen.E.copy_from(a["E"])
    seen.run()                                   # from here on the receiver passes acq_chunk
    assert seen.pit[0].get("acq_chunk", 0) > 0 and fresh.pit[0]["acq_chunk"] == seen.pit[0]["acq_chunk"]
    seen.E.copy_from(Eb)
    seen.run()
    got = seen.fetch()
    assert all(r["converged"] and not r["exact_form"] for r in seen.pit_reports())
    for k in ("wxy", "eq", "out", "ph", "idx"):
        assert np.array_equal(got[k], want[k]), k


def test_prefetched_prologue_is_bit_identical_and_follows_the_capture():
    """ResidentReceiver.run(prefetch=True): the acquisition and the eigenbasis of the NEXT capture are prepared on another stream beside the current
    capture's cold stage (qh_pit_prepare_c64_dev / qh_pit_opts.prepared) - the same kernels on the same data as inside the training call, so every capture's
    results are bit for bit those of a receiver that prepares nothing ahead; with two input buffers (load_next) each capture gets ITS preparation."""
    nsym, M, ntaps, mu = 2 ** 20, 64, 41, (2e-4, 2e-4)          # (long enough for the throughput form of the passes: only then is there something to prepare)
    caps = [synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000 + i) for i in range(3)]
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=caps[0]["alphabet_host"], tier="b", pit=dict(tol=1e-4))
    keys = ("wxy", "eq", "out", "idx")
    ref = []
    for c in caps:
        rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
        rx.load(c["E"].to_host())
        rx.run()
        ref.append(rx.fetch())
        assert all(r["converged"] and not r["exact_form"] for r in rx.pit_reports())
        del rx
    # (a) the same resident capture again and again (what bench.py times): the second and third run adopt what the run before prepared
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
    rx.load(caps[0]["E"].to_host())
    for k in range(3):
        rx.run(overlap=True, prefetch=True)
        got = rx.fetch()
        assert all(np.array_equal(got[q], ref[0][q]) for q in keys), k
        assert all(np.array_equal(a, b) for a, b in zip(got["err"], ref[0]["err"])), k
        assert (k == 0) or rx.pit_reports()[0]["acquisition"]["steps"] == rx_steps, "the adopted acquisition is the one the report shows"
        rx_steps = rx.pit_reports()[0]["acquisition"]["steps"]
    assert rx._prep is not None and rx._prep_cur == 0 and rx_steps > 0, "three runs: the second and the third adopted a prepared acquisition (slots 1, 0)"
    del rx
    # (b) a stream of different captures through two input buffers
    rx = ResidentReceiver(2, 2 * nsym, 2, M, ntaps, mu, **kw)
    rx.load(caps[0]["E"].to_host())
    for k in range(3):
        if k + 1 < 3:
            rx.load_next(caps[k + 1]["E"].to_host())
        rx.run(overlap=True, prefetch=True)
        got = rx.fetch()
        assert all(np.array_equal(got[q], ref[k][q]) for q in keys), (k, {q: float(np.max(np.abs(got[q].astype(np.complex128) - ref[k][q]))) for q in keys},
                                                                      [(r["passes"], r["acquisition"]["steps"]) for r in rx.pit_reports()])
    assert rx._prep is not None and rx._prep_cur == 0
