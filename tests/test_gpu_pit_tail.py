"""
The tail of a tier-b relaxation pass in one launch (pit_tail_kernel): estimate, decision and the back product for the next
pass share a launch, the segment trainer reads its start taps from X and writes its end taps to Y.  ``qh_set_form("pit_tail", "split")``
keeps the two launches and the in-place trainer.  Both forms run the same operations on the same values, so every comparison here is
``np.array_equal``: taps, error traces, and from the reports passes, converged, the deviation arrays and the per-pass defects - in one
process, on the same capture.  All cases are complex64 at 2 samples per symbol; the throughput form of the passes (the only one that takes
the fused tail) is forced, since these captures are far below the size at which it is the automatic choice.
"""
import numpy as np
import pytest

from qampy_amd import synth, _lib
from qampy_amd._lib import DeviceArray
from qampy_amd.core.equalisation import hip_equalisation as hk
from qampy_amd.core.equalisation import equalisation as core_eq
from qampy_amd.pipeline import ResidentReceiver

pytestmark = pytest.mark.gpu

_REPORT_KEYS = ("segments", "passes", "converged", "exact_form", "defect", "result_change", "deviation", "deviation_rms", "deviation_taps",
                "deviation_taps_worst")


def _setup(method, M, nsym, ntaps, seed=41):
    """Capture, training length (ragged last segment), start taps (converged ones for the phase-sensitive functions), alphabet."""
    dtype = np.complex64
    sig = synth.make_capture(M, nsym, nmodes=2, snr_db=28, theta=np.pi / 5.6, dgd=30e-12, seed=seed, dtype=dtype)
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]) - 7
    w0 = core_eq._init_taps(ntaps, 2, 2, dtype)
    if method == "mrde":
        _, w0, _ = hk.train_equaliser(E, tr, 2, 2, np.float32(2e-3), w0, None, False, core_eq._reshape_symbols(None, "mcma", M, dtype, 2), "mcma")
    sy = np.ascontiguousarray(core_eq._reshape_symbols(None, method, M, dtype, 2))
    return E, tr, w0, sy


def _run_pit(E, tr, niter, mu, w0, sy, method, pit, modes=None):
    dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([mu], np.float32))
    dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((2, tr * niter), E.dtype, zero=True)
    rep = hk.PitReportBuffer() if pit is not None else None          # (pit = None: the exact trainer)
    hk.train_equaliser_dev(dE, tr, niter, 2, dmu, dw, modes, False, dsy, method, derr, pit=pit, report=rep)
    return dw.to_host(), derr.to_host(), rep.read() if rep is not None else None


def _split_and_fused(forms, run, seg=True):
    """run() under the split tail, then under the automatic (fused) one; the throughput form of the passes ran both times (seg = False: a shape
    that form does not take)."""
    forms.set("pit_form", "segment")
    out = []
    for tail in ("split", "auto"):
        forms.set("pit_tail", tail)
        assert _lib.get_form("pit_tail") == (1 if tail == "split" else 0)
        out.append(run())
        assert (_lib.pit_last_launch()["form"] == 1) == seg
    return out


def _same_report(ra, rb):
    for k in _REPORT_KEYS:
        assert ra[k] == rb[k] or (k != "segments" and np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True)), (k, ra[k], rb[k])


@pytest.mark.parametrize("segments", [21, 100])
@pytest.mark.parametrize("method,M", [("cma", 64), ("mrde", 64), ("mcma", 16)])
def test_tile_edges(method, M, segments, forms):
    """2 x 21 taps = 42 eigen-directions (three MFMA row waves: the tail's block is wider than its product part).  21 segments: 42 columns -
    less than one 64-column estimate block, two full product tiles and a partial one; 100 segments: 200 columns - several blocks of both
    kinds, both with a partial last one.  cma: continuous symmetry (theta and the final rotation), mrde: phase seeds."""
    E, tr, w0, sy = _setup(method, M, 2 ** 16, 21)
    pit = dict(segments=segments, max_passes=10, tol=2e-4, acquire=0, exact_redo_off=1)
    (wa, ea, ra), (wb, eb, rb) = _split_and_fused(forms, lambda: _run_pit(E, tr, 1, 1e-3, w0, sy, method, pit))
    assert ra["segments"] == segments and ra["passes"] >= 2, ra                             # (the tail's product fed at least one pass)
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    _same_report(ra, rb)


def _receiver_results(rx):
    res = rx.fetch()
    return res, rx.pit_reports()


def _same_results(a, b, what=""):
    (ra, pa), (rb, pb) = a, b
    for k in ("wxy", "eq", "out", "ph", "idx"):
        assert np.array_equal(ra[k], rb[k]), (what, k)
    assert all(np.array_equal(x, y) for x, y in zip(ra["err"], rb["err"])), what
    assert len(pa) == len(pb)
    for x, y in zip(pa, pb):
        _same_report(x, y)


def test_both_lane_halves(forms):
    """2 x 41 taps = 82 directions: a tap set is longer than a wave, so the back product writes both lane halves of its rows.  Default
    segment grid, cma then mrde through the resident receiver."""
    nsym, M = 2 ** 17, 64
    d = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=d["alphabet_host"], tier="b")

    def run():
        rx = ResidentReceiver(2, 2 * nsym, 2, M, 41, (1e-3, 5e-4), **kw)
        rx.E.copy_from(d["E"])
        rx.run()
        return _receiver_results(rx)
    a, b = _split_and_fused(forms, run)
    assert all(r["passes"] >= 2 and not r["exact_form"] for r in a[1]), a[1]
    _same_results(a, b)


def test_one_mode(forms):
    """One selected output mode of two.  A wave of the segment trainer would then hold four segments' windows of two input modes - more rows
    than it stages -, so the passes of this shape run in a latency form, in place, with the two launches: the switch must leave them alone."""
    E, tr, w0, sy = _setup("mcma", 16, 2 ** 16, 21)
    pit = dict(segments=50, max_passes=10, tol=2e-4, acquire=0, exact_redo_off=1)
    (wa, ea, ra), (wb, eb, rb) = _split_and_fused(forms, lambda: _run_pit(E, tr, 1, 1e-3, w0, sy, "mcma", pit, modes=np.array([1])), seg=False)
    assert ra["passes"] >= 2 and not np.array_equal(wa[1], w0[1]), ra
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    _same_report(ra, rb)


@pytest.mark.parametrize("method,M", [("cma", 64), ("mrde", 64)])
def test_sweep_that_stops_uncertified(method, M, forms):
    """Two passes against a tolerance they cannot meet: the tail behind the last pass has written start taps for a pass that never runs, and
    the exact-form redo must not see them - both forms return the exact trainer's taps and error trace bit for bit."""
    E, tr, w0, sy = _setup(method, M, 2 ** 15, 21)
    wo, eo, _ = _run_pit(E, tr, 1, 1e-3, w0, sy, method, None)
    pit = dict(segments=16, max_passes=2, tol=1e-9, acquire=0)
    (wa, ea, ra), (wb, eb, rb) = _split_and_fused(forms, lambda: _run_pit(E, tr, 1, 1e-3, w0, sy, method, pit))
    assert ra["exact_form"] and ra["converged"], ra
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    assert np.array_equal(wa, wo) and np.array_equal(ea, eo)
    _same_report(ra, rb)
    # and the uncertified result itself, left in place
    (wc, ec, rc), (wd, ed, rd) = _split_and_fused(forms, lambda: _run_pit(E, tr, 1, 1e-3, w0, sy, method, dict(pit, exact_redo_off=1)))
    assert not rc["converged"] and rc["passes"] == 2, rc
    assert np.array_equal(wc, wd) and np.array_equal(ec, ed) and not np.array_equal(wc, wo)
    _same_report(rc, rd)


@pytest.mark.parametrize("method,M", [("cma", 64), ("mcma", 16)])
def test_second_sweep(method, M, forms):
    """Niter = 2: the second sweep is seeded from the taps the first one's decision left in wx - not from X, which the first sweep's last
    tail has overwritten."""
    E, tr, w0, sy = _setup(method, M, 2 ** 16, 21)
    pit = dict(segments=32, max_passes=10, tol=2e-4, acquire=0, exact_redo_off=1)
    (wa, ea, ra), (wb, eb, rb) = _split_and_fused(forms, lambda: _run_pit(E, tr, 2, 1e-3, w0, sy, method, pit))
    assert ra["passes"] >= 2 and np.any(ea[:, tr:] != 0), ra
    assert np.array_equal(wa, wb) and np.array_equal(ea, eb)
    _same_report(ra, rb)


def test_consecutive_captures(forms):
    """Two different captures through one receiver, run(overlap=True, prefetch=True), then the first one again: the scratch buffers carry
    the last tail's X from capture to capture, and nothing may read it."""
    nsym, M = 2 ** 17, 64
    caps = [synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=sd) for sd in (1000, 1003)]
    kw = dict(methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20, alphabet=caps[0]["alphabet_host"], tier="b")
    hosts = [c["E"].to_host() for c in caps]

    def run():
        rx = ResidentReceiver(2, 2 * nsym, 2, M, 41, (1e-3, 5e-4), **kw)
        out = []
        rx.load(hosts[0])
        for k in (1, 0, None):
            if k is not None:
                rx.load_next(hosts[k])
            rx.run(overlap=True, prefetch=True)
            out.append(_receiver_results(rx))
        return out
    a, b = _split_and_fused(forms, run)
    for k in range(3):
        _same_results(a[k], b[k], "capture %d" % k)
    _same_results(b[0], b[2], "the first capture again")
    assert not np.array_equal(b[0][0]["wxy"], b[1][0]["wxy"])

