"""
Parity of the HIP path (through the C ABI) with the reference on a real MI355X:
  * every golden vector captured from the reference (tests/golden/),
  * the oracle on seeded inputs at sizes it finishes in seconds,
  * the host API end to end (same checks as tests/test_host_layer.py, no monkeypatching).
Tolerances are the ones stated in conftest.TOL / DESIGN.md.
"""
import os
import numpy as np
import pytest

from conftest import CT, RT, TOL, golden_cases
from oracle import oracle
import qampy_amd
from qampy_amd import synth, theory, _lib
from qampy_amd.signals import SignalQAM
from qampy_amd.core.equalisation import hip_equalisation as hk
from qampy_amd.core.equalisation import equalisation as core_eq
from qampy_amd.core import hip_dsp, phaserecovery as core_ph

pytestmark = pytest.mark.gpu


def _close(a, b, dn, scale=1.0):
    t = TOL[dn]
    np.testing.assert_allclose(a, b, rtol=t["rtol"], atol=t["atol"] * scale)


@pytest.mark.parametrize("case", [c for c in golden_cases("train") if not c.get("real")], ids=lambda c: c["name"])
def test_train_equaliser_golden(golden, case):
    g = golden["train"]
    n, dn = case["name"], case["dtype"]
    E = golden.input(case["input"], CT[dn])
    wx = g[n + "__wx0"].copy()
    err, wx2, mu = hk.train_equaliser(E, case["TrSyms"], case["Niter"], case["os"], RT[dn](case["mu"]), wx,
                                      np.array(case["modes"]), case["adaptive"], g[n + "__symbols"], case["method"])
    assert wx2 is wx and err.dtype == CT[dn] and err.shape == g[n + "__err"].shape and type(mu) is RT[dn]
    _close(wx, g[n + "__wx"], dn)
    _close(err, g[n + "__err"], dn, scale=3)
    np.testing.assert_allclose(mu, g[n + "__mu"], rtol=1e-9 if dn == "c128" else 2e-4)
    unsel = [m for m in range(E.shape[0]) if m not in case["modes"]]
    assert np.all(err[unsel] == 0)


@pytest.mark.parametrize("form", ["auto", "direct"])
@pytest.mark.parametrize("case", golden_cases("train_cross"), ids=lambda c: c["name"])
def test_train_equaliser_cross_qam_golden(golden, case, form, forms):
    """Non-square alphabets (32- / 128-QAM) against the reference's outputs: the decision is a search over ALL symbols with the reference's
    first-minimum rule (det_symbol, pythran_equalisation.py:240-265) - in the form the library picks and in the direct form."""
    if form == "direct":
        forms.set("trainer", "direct")
    else:
        forms.reset("trainer")
    g = golden["train_cross"]
    n, dn = case["name"], case["dtype"]
    E = np.ascontiguousarray(g[case["input"] + "_E"].astype(CT[dn]))
    wx = g[n + "__wx0"].copy()
    err, wx2, mu = hk.train_equaliser(E, case["TrSyms"], case["Niter"], case["os"], RT[dn](case["mu"]), wx,
                                      np.array(case["modes"]), case["adaptive"], g[n + "__symbols"], case["method"])
    assert wx2 is wx and err.dtype == CT[dn] and err.shape == g[n + "__err"].shape
    _close(wx, g[n + "__wx"], dn)
    _close(err, g[n + "__err"], dn, scale=3)
    np.testing.assert_allclose(mu, g[n + "__mu"], rtol=1e-9 if dn == "c128" else 2e-4)


@pytest.mark.parametrize("case", [c for c in golden_cases("train") if c.get("real")], ids=lambda c: c["name"])
def test_train_equaliser_realvalued_golden(golden, case):
    g = golden["train"]
    n, dn = case["name"], case["dtype"]
    Ec = golden.input(case["input"], CT[dn])
    E = np.ascontiguousarray(np.vstack([Ec.real, Ec.imag]))
    wx = g[n + "__wx0"].copy()
    err, wx, mu = hk.train_equaliser_realvalued(E, case["TrSyms"], case["Niter"], 2, RT[dn](case["mu"]), wx,
                                                np.array(case["modes"]), case["adaptive"], g[n + "__symbols"],
                                                case["method"][:-5])
    _close(wx, g[n + "__wx"], dn)
    _close(err, g[n + "__err"], dn, scale=3)
    np.testing.assert_allclose(mu, g[n + "__mu"], rtol=1e-9 if dn == "c128" else 2e-4)


@pytest.mark.parametrize("case", [c for c in golden_cases("apply") if not c.get("realtaps")], ids=lambda c: c["name"])
def test_apply_filter_golden(golden, case):
    g = golden["apply"]
    n, dn = case["name"], case["dtype"]
    E = golden.input(case["input"], CT[dn])
    out = hk.apply_filter_to_signal(E, case["os"], g[n + "__wx"], case["modes"])
    assert out.shape == g[n + "__out"].shape and out.dtype == CT[dn]
    np.testing.assert_allclose(out, g[n + "__out"], rtol=1e-12 if dn == "c128" else 2e-5, atol=1e-13 if dn == "c128" else 2e-6)


@pytest.mark.parametrize("case", [c for c in golden_cases("bps") if "base" in c], ids=lambda c: c["name"])
def test_bps_index_golden(golden, case):
    g = golden["bps"]
    dn = case["dtype"]
    E = g[case["base"] + "__E"].astype(CT[dn])
    angles = np.linspace(-np.pi / 4, np.pi / 4, case["A"], endpoint=False, dtype=RT[dn]).reshape(1, -1)
    alphabet = g[case["base"] + "__alphabet"].astype(CT[dn])
    N, A = case["N"], case["A"]
    for m in range(E.shape[0]):
        idx = hip_dsp.bps(np.ascontiguousarray(E[m]), angles, alphabet, N)
        ref = g[case["name"] + "__idx"][m]
        assert idx.dtype == np.int32 and np.all(idx[:N] == 0) and np.all(idx[-N:] == 0)
        mism = np.count_nonzero(idx != ref)
        # direct 2N-term window sum vs the reference's difference of running sums: only near-ties may flip, and then to a
        # neighbouring angle (stated bar: exact for complex128, >= 99.9 % for complex64 on L <= 2^14)
        if dn == "c128":
            assert mism <= 1, mism
        else:
            assert mism <= max(1, idx.size // 1000), mism
        d = np.abs(idx.astype(int) - ref)
        assert np.all(np.minimum(d, A - d) <= 1)


def test_bps_per_symbol_grid_and_select_angles(golden):
    g = golden["bps"]
    idx = hip_dsp.bps(g["bps_grid__E"], g["bps_grid__angles"], g["bps_grid__alphabet"], 10)
    assert np.count_nonzero(idx != g["bps_grid__idx"]) <= 1
    assert np.array_equal(hip_dsp.select_angles(g["bps_grid__angles"], g["bps_grid__idx"]), g["bps_grid__sel"])
    assert np.array_equal(hip_dsp.select_angles(g["bps_grid__angles"][:1].copy(), g["bps_grid__idx"].astype(int)),
                          g["bps_grid__sel1"])


@pytest.mark.parametrize("M", [4, 16, 32, 64, 128])
@pytest.mark.parametrize("dn", ["c128", "c64"])
def test_make_decision_golden(golden, M, dn):
    g = golden["decision"]
    det, dist, idx = hk.make_decision(g["md_M%d__E" % M].astype(CT[dn]), g["md_M%d__alphabet" % M].astype(CT[dn]))
    assert det.dtype == CT[dn] and dist.dtype == RT[dn] and idx.dtype == np.int32
    assert np.array_equal(idx, g["md_M%d_%s__idx" % (M, dn)])
    assert np.array_equal(det, g["md_M%d_%s__det" % (M, dn)])
    np.testing.assert_allclose(dist, g["md_M%d_%s__dist" % (M, dn)], rtol=2e-6 if dn == "c64" else 1e-14)


# ------------------------------------------------------------------------------------------------ host API end to end
@pytest.mark.parametrize("dn", ["c128", "c64"])
def test_e2e_wrappers_match_reference_on_gpu(golden, dn):
    import test_host_layer as th
    th.test_e2e_wrappers_match_reference.__wrapped__(golden, None, dn) if hasattr(
        th.test_e2e_wrappers_match_reference, "__wrapped__") else th.test_e2e_wrappers_match_reference(golden, None, dn)


def test_real_taps_apply_on_gpu(golden):
    import test_host_layer as th
    th.test_real_taps_apply(golden, None)


@pytest.mark.parametrize("case", [c for c in golden_cases("bps") if "base" in c and c["dtype"] == "c128"], ids=lambda c: c["name"])
def test_bps_host_layer_on_gpu(golden, case):
    g = golden["bps"]
    E = g[case["base"] + "__E"]
    sig = SignalQAM(E, case["M"], coded_symbols=g[case["base"] + "__alphabet"])
    Eout, ph = qampy_amd.phaserec.bps(sig, case["A"], case["N"])
    assert type(Eout) is SignalQAM and ph.dtype == np.float64
    ref = g[case["name"] + "__ph"]
    # a flipped near-tie moves one sample by one angle step; everything else is bit-identical numpy on identical indices
    assert np.count_nonzero(ph != ref) <= 2
    np.testing.assert_allclose(ph, ref, atol=np.pi / 2 / case["A"] * 1.01)


@pytest.mark.parametrize("case", golden_cases("twostage"), ids=lambda c: c["name"])
def test_bps_twostage_on_gpu(golden, case):
    g = golden["twostage"]
    dn = case["dtype"]
    E = g[case["base"] + "__E"].astype(CT[dn])
    sig = SignalQAM(E, case["M"], coded_symbols=g[case["base"] + "__alphabet"].astype(CT[dn]))
    Eout, ph = qampy_amd.phaserec.bps_twostage(sig, case["A"], case["N"], B=case["B"])
    assert type(Eout) is SignalQAM and ph.dtype == RT[dn]
    ref = g[case["name"] + "__ph"]
    # a flipped near-tie in either stage moves single symbols by at most one coarse step; allow a handful
    step = np.pi / 2 / case["A"]
    bad = np.abs(ph - ref) > 1e-6
    assert bad.mean() < (2e-3 if dn == "c128" else 1e-2)
    assert np.all(np.abs(np.angle(np.exp(4j * (ph - ref))) / 4) <= 1.01 * step)


# ------------------------------------------------------------------------------------------------ vs oracle, seeded, larger
@pytest.mark.parametrize("method,M,ntaps,adaptive", [("cma", 64, 41, False), ("mrde", 64, 41, False), ("mcma", 16, 21, True),
                                                     ("sbd", 16, 21, True), ("rde", 16, 13, False), ("dd", 64, 17, False),
                                                     ("mddma", 64, 17, True)])
def test_train_vs_oracle_seeded(method, M, ntaps, adaptive):
    sig = synth.make_capture(M, 2 ** 14, nmodes=2, snr_db=30 if M == 64 else 25, theta=np.pi / 5.6, dgd=30e-12, seed=321,
                             dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1])
    w0 = core_eq._init_taps(ntaps, 2, 2, np.complex64)
    if method in core_eq.DECISION_BASED or method in ("rde", "mrde"):      # start from converged taps (oracle, then shared)
        s0 = core_eq._reshape_symbols(None, "mcma", M, np.complex64, 2)
        _, w0, _ = oracle.train_equaliser(E, tr, 2, 2, np.float32(1e-3), w0, None, False, s0, "mcma")
    sy = core_eq._reshape_symbols(sig.coded_symbols, method, M, np.complex64, 2)
    mu = np.float32(5e-4)
    eo, wo, muo = oracle.train_equaliser(E, tr, 1, 2, mu, w0.copy(), None, adaptive, sy, method)
    eg, wg, mug = hk.train_equaliser(E, tr, 1, 2, mu, w0.copy(), None, adaptive, sy, method)
    np.testing.assert_allclose(wg, wo, rtol=1e-3, atol=2e-4)
    # decision-directed errors can flip a decision on a near-tie: compare in the mean-square sense too
    assert np.mean(np.abs(eg - eo) ** 2) < 1e-6 * max(1.0, np.mean(np.abs(eo) ** 2) * 1e3)
    np.testing.assert_allclose(mug, muo, rtol=1e-3)


def test_full_chain_ser_matches_oracle():
    """C2-shaped recipe at 2^14 symbols: same SER from the HIP path and from the oracle's kernels."""
    sig = synth.make_capture(16, 2 ** 14, nmodes=2, snr_db=25, theta=np.pi / 5.6, dgd=30e-12, linewidth=50e3, seed=1000,
                             dtype=np.complex64)
    out, wxy, err = qampy_amd.equalisation.equalise_signal(sig, 1e-3, Ntaps=21, Niter=2, method="mcma", apply=True)
    rec, ph = qampy_amd.phaserec.bps(out, 32, 20)
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, 21, E.shape[1])
    sy = core_eq._reshape_symbols(None, "mcma", 16, np.complex64, 2)
    _, wo, _ = oracle.train_equaliser(E, tr, 2, 2, np.float32(1e-3), core_eq._init_taps(21, 2, 2, np.complex64), None, False, sy, "mcma")
    oout = oracle.apply_filter_to_signal(E, 2, wo)
    angles = np.linspace(-np.pi / 4, np.pi / 4, 32, endpoint=False, dtype=np.float32).reshape(1, -1)
    oph = np.array([oracle.select_angles(angles, oracle.bps(oout[m], angles, sig.coded_symbols, 20)) for m in range(2)])
    oph[:, 20:-20] = np.unwrap(oph[:, 20:-20] * 4) / 4
    orec = oout * np.exp(1j * oph)
    ser_g = synth.cal_ser(np.asarray(rec), sig.symbols, sig.coded_symbols, trim=500)
    ser_o = synth.cal_ser(orec, sig.symbols, sig.coded_symbols, trim=500)
    n = rec.shape[1] - 1000
    assert np.all(np.abs(ser_g - ser_o) * n <= 3), (ser_g, ser_o)      # within +-3 symbol errors per mode
    assert ser_g.max() < 2e-2


def test_resident_pipeline_equals_host_api():
    from qampy_amd.pipeline import ResidentReceiver
    sig = synth.make_capture(64, 2 ** 13, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=2e3, seed=5,
                             dtype=np.complex64)
    out, wxy, (e1, e2) = qampy_amd.equalisation.dual_mode_equalisation(sig, (1e-3, 5e-4), 41, Niter=(2, 2), methods=("cma", "mrde"))
    rec, ph = qampy_amd.phaserec.bps(out, 64, 20)
    rx = ResidentReceiver(2, sig.shape[1], 2, 64, 41, (1e-3, 5e-4), methods=("cma", "mrde"), Niter=(2, 2), Mtestangles=64, Nbps=20,
                          alphabet=sig.coded_symbols)
    rx.load(sig)
    rx.run()
    rx.run()                                  # a second pass must restart from the same initial state
    res = rx.fetch()
    assert np.array_equal(res["wxy"], wxy) and np.array_equal(res["err"][0], e1) and np.array_equal(res["err"][1], e2)
    assert np.array_equal(res["eq"], np.asarray(out))
    np.testing.assert_allclose(res["ph"], ph, atol=2e-6)
    np.testing.assert_allclose(res["out"], np.asarray(rec), atol=1e-5)


# ------------------------------------------------------------------------------------------------ edge cases
def test_edge_cases():
    E = np.ones((2, 10), np.complex64)
    w = core_eq._init_taps(11, 2, 2, np.complex64)
    assert hk.apply_filter_to_signal(E, 2, w).shape == (2, 0)                     # field shorter than the filter
    e, w2, mu = hk.train_equaliser(np.ones((2, 64), np.complex64), 0, 1, 2, np.float32(1e-3), w, None, False,
                                   np.ones((2, 1), np.complex64), "cma")
    assert e.shape == (2, 0)
    with pytest.raises(ValueError):                                               # training would read past the field
        hk.train_equaliser(np.ones((2, 64), np.complex64), 64, 1, 2, np.float32(1e-3), w, None, False,
                           np.ones((2, 1), np.complex64), "cma")
    with pytest.raises(ValueError):
        hk.apply_filter_to_signal(np.ones((2, 64), np.complex64), 2, w, modes=[2])
    # L < 2N: every index is forced to 0
    idx = hip_dsp.bps(np.ones(15, np.complex64), np.zeros((1, 4), np.float32), np.ones(4, np.complex64), 10)
    assert idx.shape == (15,) and np.all(idx == 0)


# ------------------------------------------------------------------------------------------------ look-ahead vs direct form
@pytest.mark.parametrize("method,M,ntaps,nmodes", [("cma", 64, 41, 2), ("mcma", 16, 21, 2), ("mrde", 64, 41, 2), ("rde", 16, 13, 2),
                                                   ("cma2", 16, 11, 2), ("sgncma", 16, 7, 1), ("mcma", 16, 9, 3),
                                                   ("mrde", 64, 61, 2), ("cma", 4, 3, 1), ("rde", 64, 17, 4),
                                                   ("sbd", 16, 21, 2), ("sbd", 64, 41, 2), ("mddma", 64, 15, 2), ("dd", 4, 9, 1),
                                                   ("dd", 256, 11, 2), ("sbd", 32, 13, 2)])
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_lookahead_trainer_equals_direct_trainer(method, M, ntaps, nmodes, dn, forms):
    """The three exact trainers (look-ahead: train_la.h, block-iterative: train_bi.h, direct: train_impl.h) and the oracle
    agree to rounding, including a partial last block, several sweeps, a mode subset and shapes only some of them take
    (122 taps: no look-ahead kernel, the forced form then falls through to the next one).  Decision-directed functions run
    block-iterative: per-axis slicer tables on square alphabets, a scan of the alphabet on the others (32-QAM cross)."""
    nsym = 5000 + 37
    sig = synth.make_capture(M, nsym, nmodes=nmodes, snr_db=28, theta=np.pi / 5.6 if nmodes == 2 else None, dgd=30e-12,
                             seed=99, dtype=CT[dn])
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]) - 5            # not a multiple of 64
    if method == "cma2":
        tr = 333               # cma2 is not phase blind and only stays bounded for a short run from converged taps
    w0 = core_eq._init_taps(ntaps, nmodes, nmodes, CT[dn])
    if method in ("rde", "mrde", "cma2", "sbd", "mddma", "dd"):
        s0 = core_eq._reshape_symbols(None, "mcma", M, CT[dn], nmodes)
        _, w0, _ = oracle.train_equaliser(E, tr, 3, 2, RT[dn](2e-3), w0, None, False, s0, "mcma")
    sy = core_eq._reshape_symbols(None, method, M, CT[dn], nmodes)
    mu = RT[dn](3e-4 if method != "cma2" else 1e-4)
    modes = None if nmodes < 3 else np.array([2, 0])
    eo, wo, _ = oracle.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, False, sy, method)
    forms.set("trainer", "direct")
    ed, wd, _ = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, False, sy, method)
    forms.set("trainer", "lookahead")
    el, wl, _ = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, False, sy, method)
    forms.set("trainer", "iterative")     # block-iterative form (train_bi.h): fixed-point sweeps per 64-step block
    ei, wi, _ = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, False, sy, method)
    ei2, wi2, _ = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, False, sy, method)
    assert np.array_equal(wi, wi2) and np.array_equal(ei, ei2)          # fixed reduction order: bit-reproducible
    t = dict(rtol=1e-9, atol=1e-11) if dn == "c128" else dict(rtol=2e-4, atol=2e-5)
    for w, e in ((wd, ed), (wl, el), (wi, ei)):
        np.testing.assert_allclose(w, wo, **t)
        np.testing.assert_allclose(e, eo, rtol=t["rtol"], atol=t["atol"] * 5)
    # the three forms really are different computations (different summation orders): their error traces agree to the
    # tolerance above but not bit for bit
    if dn == "c64" and ntaps <= 41 and method in ("cma", "mcma", "mrde"):      # shapes every form takes (others may fall through to the direct form)
        assert not (np.array_equal(el, ed) and np.array_equal(ei, ed))


@pytest.mark.parametrize("method,M,ntaps,nmodes", [("cma", 4, 17, 2), ("mcma", 16, 21, 2), ("mrde", 64, 41, 2), ("sbd", 16, 21, 2),
                                                   ("mddma", 64, 13, 2), ("dd", 16, 9, 3), ("rde", 16, 15, 1)])
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_adaptive_step_forms_agree(method, M, ntaps, nmodes, dn, forms):
    """adapt_step (pythran_equalisation.py:12-16, :171-172) in the block-iterative form (1/mu as a prefix sum inside the
    sweeps) and in the look-ahead form (1/mu carried by the chain wave, all sweeps in one launch) against the direct form and the
    oracle: taps, errors and the final mu, which is carried over sweeps and modes."""
    nsym = 3000 + 11
    sig = synth.make_capture(M, nsym, nmodes=nmodes, snr_db=26, theta=np.pi / 5.6 if nmodes == 2 else None, dgd=30e-12,
                             seed=123, dtype=CT[dn])
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]) - 9
    w0 = core_eq._init_taps(ntaps, nmodes, nmodes, CT[dn])
    if method in ("rde", "mrde", "sbd", "mddma", "dd"):
        s0 = core_eq._reshape_symbols(None, "mcma", M, CT[dn], nmodes)
        _, w0, _ = oracle.train_equaliser(E, tr, 3, 2, RT[dn](2e-3), w0, None, False, s0, "mcma")
    sy = core_eq._reshape_symbols(None, method, M, CT[dn], nmodes)
    mu = RT[dn](5e-3)
    modes = None if nmodes < 3 else np.array([2, 0])
    eo, wo, muo = oracle.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, True, sy, method)
    forms.set("trainer", "direct")
    ed, wd, mud = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, True, sy, method)
    forms.set("trainer", "iterative")
    ei, wi, mui = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, True, sy, method)
    forms.set("trainer", "lookahead")     # round 5: the adaptive step on the look-ahead chain (blind methods; others fall through)
    el, wl, mul = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, True, sy, method)
    forms.reset("trainer")                  # and whatever the library picks by itself
    ea, wa, mua = hk.train_equaliser(E, tr, 2, 2, mu, w0.copy(), modes, True, sy, method)
    assert muo < 0.95 * mu                                   # the step size really moved
    t = dict(rtol=1e-9, atol=1e-11) if dn == "c128" else dict(rtol=3e-4, atol=3e-5)
    for w, e, m in ((wd, ed, mud), (wi, ei, mui), (wl, el, mul), (wa, ea, mua)):
        np.testing.assert_allclose(w, wo, **t)
        np.testing.assert_allclose(e, eo, rtol=t["rtol"], atol=t["atol"] * 5)
        np.testing.assert_allclose(m, muo, rtol=1e-9 if dn == "c128" else 3e-4)


@pytest.mark.parametrize("nmodes,ntaps,os_,tr", [(1, 1, 1, 128), (1, 5, 1, 129), (2, 7, 3, 191), (2, 64, 2, 192), (4, 31, 2, 200), (8, 16, 2, 130),
                                                (8, 3, 1, 257), (2, 33, 4, 128), (3, 42, 2, 321)])
@pytest.mark.parametrize("method", ["mcma", "mrde", "sbd"])
def test_exact_trainer_forms_on_boundary_shapes(nmodes, ntaps, os_, tr, method, forms):
    """Smallest captures the block forms take (128 steps), partial / full last blocks, 1 to 8 modes, 1 to 128 taps per output
    mode, oversampling 1 to 4, adaptive and fixed step: every form the shape admits equals the oracle."""
    rng = np.random.default_rng(nmodes * 1000 + ntaps * 10 + os_)
    M = 16
    L = (tr - 1) * os_ + ntaps + 5
    alphabet = core_eq._reshape_symbols(None, "sbd", M, np.complex128, 1)[0]
    tx = alphabet[rng.integers(0, M, (nmodes, L))]
    E = (tx + 0.05 * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex128)
    w0 = core_eq._init_taps(ntaps, nmodes, nmodes, np.complex128)
    w0 += 0.01 * (rng.normal(size=w0.shape) + 1j * rng.normal(size=w0.shape))
    sy = core_eq._reshape_symbols(None, method, M, np.complex128, nmodes)
    modes = np.arange(nmodes)[::-1].copy() if nmodes > 2 else None
    for adaptive in (False, True):
        eo, wo, muo = oracle.train_equaliser(E, tr, 2, os_, np.float64(1e-3), w0.copy(), modes, adaptive, sy, method)
        for form in ("direct", "lookahead", "iterative"):
            forms.set("trainer", form)
            e, w, mu = hk.train_equaliser(E, tr, 2, os_, np.float64(1e-3), w0.copy(), modes, adaptive, sy, method)
            np.testing.assert_allclose(w, wo, rtol=1e-9, atol=1e-11, err_msg="%s adaptive=%s" % (form, adaptive))
            np.testing.assert_allclose(e, eo, rtol=1e-9, atol=1e-10, err_msg="%s adaptive=%s" % (form, adaptive))
            np.testing.assert_allclose(mu, muo, rtol=1e-9)


@pytest.mark.parametrize("method,M", [("cma", 16), ("mcma", 16), ("mrde", 64), ("sbd", 16)])
def test_time_chunked_training_equals_unchunked(method, M):
    """When the Gram tables of a call exceed the scratch budget the sweep runs chunk after chunk (taps handed on through HBM):
    same results - bit for bit in the block-iterative form (it restarts every block from the taps anyway), to rounding in the
    look-ahead form - for any capture length."""
    sig = synth.make_capture(M, 24000, nmodes=2, snr_db=28, theta=np.pi / 5.6, dgd=30e-12, seed=31, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    ntaps = 21
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]) - 3
    w0 = core_eq._init_taps(ntaps, 2, 2, np.complex64)
    if method in ("mrde", "sbd"):
        _, w0, _ = hk.train_equaliser(E, tr, 2, 2, np.float32(2e-3), w0, None, False, core_eq._reshape_symbols(None, "mcma", M, np.complex64, 2), "mcma")
    sy = core_eq._reshape_symbols(None, method, M, np.complex64, 2)
    e1, w1, _ = hk.train_equaliser(E, tr, 2, 2, np.float32(3e-4), w0.copy(), None, False, sy, method)
    budget = _lib.gram_budget_gb()
    _lib.call("qh_set_gram_budget_gb", 0.004)                        # 4 MiB: chunks of 4096 steps (the minimum)
    try:
        e2, w2, _ = hk.train_equaliser(E, tr, 2, 2, np.float32(3e-4), w0.copy(), None, False, sy, method)
    finally:
        _lib.call("qh_set_gram_budget_gb", budget)
    assert np.all(np.isfinite(w2)) and np.abs(e2[:, -1]).min() > 0
    if method in ("mrde", "sbd"):
        assert np.array_equal(w1, w2) and np.array_equal(e1, e2)
    else:
        np.testing.assert_allclose(w2, w1, rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(e2, e1, rtol=2e-4, atol=1e-4)
    eo, wo, _ = oracle.train_equaliser(E, tr, 2, 2, np.float32(3e-4), w0.copy(), None, False, sy, method)
    np.testing.assert_allclose(w2, wo, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("method,M,ntaps,nmodes", [("mcma", 16, 19, 2), ("sbd", 16, 19, 4), ("cma", 4, 7, 3), ("mrde", 64, 161, 2)])
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_per_mode_adaptive_step_equals_one_call_per_mode(method, M, ntaps, nmodes, dn):
    """adaptive='per-mode' (C flag 2): every mode adapts its own step size from mu and the modes train concurrently - by
    definition the result of one reference call per mode from the initial mu (161 taps: no block form, per-mode loop)."""
    sig = synth.make_capture(M, 6000, nmodes=nmodes, snr_db=26, seed=5, dtype=CT[dn])
    E = np.ascontiguousarray(np.asarray(sig))
    tr = core_eq._cal_training_symbol_len(2, ntaps, E.shape[1])
    w0 = core_eq._init_taps(ntaps, nmodes, nmodes, CT[dn])
    if method in ("sbd", "mrde"):
        _, w0, _ = oracle.train_equaliser(E, tr, 2, 2, RT[dn](2e-3), w0, None, False, core_eq._reshape_symbols(None, "mcma", M, CT[dn], nmodes), "mcma")
    sy = core_eq._reshape_symbols(None, method, M, CT[dn], nmodes)
    modes = np.arange(nmodes)[::-1].copy()
    mu0 = RT[dn](4e-3)
    wo, eo, muo = w0.copy(), np.zeros((nmodes, tr * 2), CT[dn]), None
    for m in modes:                                   # the definition: one sequential-semantics call per mode
        e1, wo, muo = oracle.train_equaliser(E, tr, 2, 2, mu0, wo, np.array([m]), True, sy, method)
        eo[m] = e1[m]
    e, w, mu = hk.train_equaliser(E, tr, 2, 2, mu0, w0.copy(), modes, "per-mode", sy, method)
    t = dict(rtol=1e-9, atol=1e-11) if dn == "c128" else dict(rtol=3e-4, atol=3e-5)
    np.testing.assert_allclose(w, wo, **t)
    np.testing.assert_allclose(e, eo, rtol=t["rtol"], atol=t["atol"] * 5)
    np.testing.assert_allclose(mu, muo, rtol=1e-9 if dn == "c128" else 3e-4)
    # and it differs from the sequential semantics, where later modes inherit an already reduced step
    e2, w2, mu2 = hk.train_equaliser(E, tr, 2, 2, mu0, w0.copy(), modes, True, sy, method)
    assert not np.allclose(w2[modes[-1]], w[modes[-1]], rtol=1e-3, atol=1e-4)
    with pytest.raises(ValueError):
        hk.train_equaliser(E, tr, 1, 2, mu0, w0.copy(), modes, "sometimes", sy, method)


def test_trainer_fuzz_against_oracle():
    """Randomised differential test (scripts/fuzz_trainer.py: random shapes, methods, step-size modes, sweeps, mode subsets,
    forced kernel forms; complex128, rtol 1e-8 against the oracle) - 8 500 cases were run clean when this was written."""
    import subprocess, sys
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_trainer.py"),
                          "250", "11"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "250 cases, 0 failures" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_dsp_fuzz_against_oracle():
    """scripts/fuzz_dsp.py: random shapes / dtypes / alphabets for the filter (complex and real taps, up to 4 modes x os 3 x 69
    taps), blind phase search (one and per-symbol grids), angle selection and decisions against the oracle."""
    import subprocess, sys
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_dsp.py"),
                          "300", "7"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "300 cases, 0 failures" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ phase search: streaming vs tile kernel
def _alphabets():
    q16, q64 = theory.coded_symbols_qam(16, dtype=np.complex64), theory.coded_symbols_qam(64, dtype=np.complex64)
    jit = np.random.default_rng(5).normal(size=(16, 2)) * 0.04                                # 16 points off the grid: not a product of levels
    irregular = (q16 + jit[:, 0] + 1j * jit[:, 1]).astype(np.complex64)
    return {"qam4": theory.coded_symbols_qam(4, dtype=np.complex64), "qam16": q16, "qam64": q64, "qam256": theory.coded_symbols_qam(256, dtype=np.complex64),
            "qam1024": theory.coded_symbols_qam(1024, dtype=np.complex64),
            "qam16_shifted": (q16 + np.complex64(0.11 - 0.07j)).astype(np.complex64),            # a product of levels, not mirror symmetric
            "qam32_cross": theory.coded_symbols_qam(32, dtype=np.complex64), "irregular16": irregular,   # not products
            "qam64_rect": (q64.real * 1.0 + 1j * q64.imag * 0.5).astype(np.complex64)}         # symmetric product with different levels per axis


@pytest.mark.parametrize("name", ["qam4", "qam16", "qam64", "qam64_rect", "qam256", "qam16_shifted", "irregular16"])
@pytest.mark.parametrize("L", [1024 + 39, 2 * 1024 + 20, 5 * 1024 + 20, 5 * 1024 + 21, 40 * 1024 + 777, 1 << 20])
def test_bps_register_ring_kernel_is_bit_identical_to_the_lds_ring_kernel(name, L, forms):
    """Round 6: A = 64, N = 20 - the chunks whose rows all lie inside the capture go to bps_stream40_kernel (window in registers, symbols through the
    scalar cache) when the alphabet is a mirror-symmetric product with at most four positive levels per axis; the others, and every other alphabet, stay
    with bps_stream_kernel (both kernels read the device-side descriptor, exactly one works on a chunk).  Same operations in the same order: the indices
    are IDENTICAL to the LDS-ring kernel's on every symbol - for alphabets the register kernel takes, for those it declines, at every chunk count
    (none / one / several interior chunks; a last chunk that just is / just is not interior)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((name, L)).encode()))
    alphabet = _alphabets()[name]
    scale = np.sqrt(np.mean(np.abs(alphabet) ** 2))
    sig = (alphabet[rng.integers(0, alphabet.size, L)] * np.exp(1j * (0.2 + 0.002 * np.cumsum(rng.normal(size=L)))) +
           0.04 * scale * (rng.normal(size=L) + 1j * rng.normal(size=L))).astype(np.complex64)
    ang = np.linspace(-np.pi / 4, np.pi / 4, 64, endpoint=False, dtype=np.float32).reshape(1, -1)
    forms.set("bps", "lds")
    i_lds = hip_dsp.bps(sig, ang, alphabet, 20)
    forms.reset("bps")
    i_reg = hip_dsp.bps(sig, ang, alphabet, 20)
    assert np.array_equal(i_reg, i_lds), (name, L, int(np.count_nonzero(i_reg != i_lds)))
    # two rows at once (the receiver's call: both modes in one launch) and in parts
    from qampy_amd._lib import DeviceArray
    two = np.ascontiguousarray(np.stack([sig, sig[::-1]]))
    dE, dsy, dang = DeviceArray.from_host(two), DeviceArray.from_host(alphabet), DeviceArray.from_host(ang.ravel())
    res = []
    for form, nparts in (("lds", 1), (None, 1), (None, 3)):
        forms.set("bps", form)
        idx, ph, out = DeviceArray((2, L), np.int32, zero=True), DeviceArray((2, L), np.float32), DeviceArray((2, L), np.complex64)
        for part in range(nparts):
            hip_dsp.bps_recover_dev(dE, 64, dsy, 20, idx, ph, out, angles=dang, part=part, nparts=nparts)
        _lib.sync()
        res.append((idx.to_host(), ph.to_host(), out.to_host()))
    forms.reset("bps")
    for r in res[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, res[0]))
    # (the one-row call above may cut the capture into chunks of another length - the library sizes them for the number of waves - and then re-sums its
    # windows at other rows: not compared bit for bit with the two-row call)
    assert np.mean(res[0][0][0] != i_lds) < 2e-3


@pytest.mark.parametrize("name", ["qam4", "qam16", "qam64", "qam256", "qam1024", "qam16_shifted", "qam32_cross", "irregular16", "qam64_rect"])
@pytest.mark.parametrize("L,A,N", [(1, 64, 3), (39, 64, 20), (40, 64, 20), (41, 33, 20), (1000, 64, 20), (3 * 1024 + 17, 64, 20), (5000, 5, 1), (4097, 64, 96),
                                   (2500, 17, 33)])
def test_bps_stream_kernel_equals_tile_kernel_and_double_oracle(name, L, A, N, forms):
    """complex64, one grid of <= 64 angles: the streaming kernel (lane <-> angle, LDS ring, every alphabet kind handled in the
    kernel) against the tile kernel on the same data and against the oracle run in double precision on the same values (the
    'true' arg-min: no running-sum drift).  Edges: capture shorter than / equal to / one longer than the window, ragged chunks,
    the longest ring, grids that leave lanes without an angle."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((name, L, A, N)).encode()))
    alphabet = _alphabets()[name]
    scale = np.sqrt(np.mean(np.abs(alphabet) ** 2))
    sig = (alphabet[rng.integers(0, alphabet.size, L)] * np.exp(1j * (0.2 + 0.002 * np.cumsum(rng.normal(size=L)))) +
           0.04 * scale * (rng.normal(size=L) + 1j * rng.normal(size=L))).astype(np.complex64)
    ang = np.linspace(-np.pi / 4, np.pi / 4, A, endpoint=False, dtype=np.float32).reshape(1, -1)
    forms.reset("bps")
    i_s = hip_dsp.bps(sig, ang, alphabet, N)
    forms.set("bps", "tile")
    i_t = hip_dsp.bps(sig, ang, alphabet, N)
    forms.reset("bps")
    i_o = oracle.bps(sig.astype(np.complex128), ang.astype(np.float64), alphabet.astype(np.complex128), N)
    assert i_s.shape == i_t.shape == (L,) and i_s.dtype == np.int32
    assert np.all(i_s[:N] == 0) and np.all(i_s[max(L - N, 0):] == 0)
    for other, bar in ((i_t, 2e-3), (i_o, 5e-3)):
        mism = np.nonzero(i_s != other)[0]
        assert mism.size <= max(1, int(bar * L)), (mism.size, L)
        if mism.size:                                  # a flipped near-tie goes to a neighbouring angle
            d = np.abs(i_s[mism].astype(int) - other[mism])
            assert np.all(np.minimum(d, A - d) <= 1)


# ------------------------------------------------------------------------------------------------ window batch
@pytest.mark.parametrize("nwin,hop,method,adaptive", [(6, 700, "cma", False), (5, 512, "cma", True), (4, 900, "mrde", False), (7, None, "cma", False),
                                                      (48, 128, "mcma", False)])
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_window_batch_equals_one_call_per_window(nwin, hop, method, adaptive, dn):
    """qh_train_equaliser_windows_*: a few equally spaced windows run as strided channels of the latency forms, many windows or
    irregular starts (hop None) in the direct form - every window must be what a call on that slice returns (oracle), and the
    search form must pick the window with the smallest error variance."""
    M = 64 if method == "mrde" else 16
    sig = synth.make_capture(M, 6000, nmodes=2, snr_db=27, theta=np.pi / 5.6, dgd=30e-12, seed=77, dtype=CT[dn])
    E = np.ascontiguousarray(np.asarray(sig))
    ntaps, win_len, Niter = 13, 2048, 2
    starts = (np.arange(nwin) * hop if hop else np.array([0, 300, 1111, 1500, 2900, 4000, 5100][:nwin])).astype(np.int64)
    tr = core_eq._cal_training_symbol_len(2, ntaps, win_len)
    w0 = core_eq._init_taps(ntaps, 2, 2, CT[dn])
    if method == "mrde":
        _, w0, _ = oracle.train_equaliser(E, core_eq._cal_training_symbol_len(2, ntaps, E.shape[1]), 2, 2, RT[dn](2e-3), w0, None, False,
                                          core_eq._reshape_symbols(None, "mcma", M, CT[dn], 2), "mcma")
    sy = core_eq._reshape_symbols(None, method, M, CT[dn], 2)
    mu = RT[dn](1e-3)
    err, wx, mus = hk.train_equaliser_windows(E, starts, win_len, tr, Niter, 2, mu, w0, None, adaptive, sy, method)
    t = dict(rtol=1e-9, atol=1e-11) if dn == "c128" else dict(rtol=3e-4, atol=3e-5)
    for v, s0 in enumerate(starts):
        eo, wo, mo = oracle.train_equaliser(np.ascontiguousarray(E[:, s0:s0 + win_len]), tr, Niter, 2, mu, w0.copy(), None, adaptive, sy, method)
        np.testing.assert_allclose(wx[v], wo, **t)
        np.testing.assert_allclose(err[v], eo, rtol=t["rtol"], atol=t["atol"] * 5)
        np.testing.assert_allclose(mus[v], mo, rtol=1e-9 if dn == "c128" else 2e-4)
    var, best, wbest = hk.train_equaliser_windows_search(E, starts, win_len, tr, Niter, 2, mu, w0, None, adaptive, sy, method)
    ref_var = np.var(err, axis=-1).T
    np.testing.assert_allclose(var, ref_var, rtol=1e-6 if dn == "c128" else 2e-3)
    assert np.array_equal(best, np.argmin(ref_var, axis=-1)) or np.allclose(np.sort(ref_var, axis=-1)[:, 0], np.sort(ref_var, axis=-1)[:, 1], rtol=1e-3)
    for m in range(2):
        np.testing.assert_allclose(wbest[m], wx[best[m]], **t)


def _unwrap_quarter_turns(angles, idx, N):
    """Host restatement of the unwrap in qh_bps_recover_*_dev (include/qampy_hip.h): np.unwrap of 4 * angles[idx] over the interior [N, L - N),
    its jump decisions made with numpy's own operations in the precision of the grid, half-range case included.  Returns the running
    correction of every interior symbol as an integer number of whole turns of 4 * ph, i.e. of quarter turns of ph."""
    rt = angles.dtype.type
    pi, twopi = rt(np.pi), rt(2 * np.pi)
    p4 = rt(4) * angles[idx[N:idx.size - N]]
    dd = np.diff(p4)
    ddmod = np.mod(dd + pi, twopi) - pi
    ddmod[(ddmod == -pi) & (dd > 0)] = pi
    corr = np.where(np.abs(dd) < pi, 0, np.rint((ddmod - dd).astype(np.float64) / (2 * np.pi))).astype(np.int64)
    return np.concatenate([[0], np.cumsum(corr)])


def test_bps_recover_unwrap_and_derotation_equal_host_restatement():
    """The search followed by the unwrap and de-rotation launches of qh_bps_recover_*_dev, against a host restatement built from the indices
    the same call returns, on a capture with real phase wander (the unwrapped phase leaves the grid's range many times) and at a length that is
    not a multiple of the chunk: every interior symbol carries exactly the restated number of quarter turns, the edges the raw grid value, and
    the output is the capture de-rotated by the returned phase.  (The search itself: the register-ring and tile kernel tests above.)"""
    from qampy_amd._lib import DeviceArray
    L, N = 2 ** 17 + 333, 20
    sig = synth.make_capture(16, L, nmodes=2, os=1, snr_db=22, linewidth=2e6, seed=11, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    grid = hip_dsp.test_angle_grid(32, np.float32).ravel()
    dE, alpha = DeviceArray.from_host(E), DeviceArray.from_host(np.ascontiguousarray(sig.coded_symbols, dtype=np.complex64))
    idx, ph, out = DeviceArray(E.shape, np.int32), DeviceArray(E.shape, np.float32), DeviceArray(E.shape, np.complex64)
    hip_dsp.bps_recover_dev(dE, 32, alpha, 20, idx, ph, out, angles=DeviceArray.from_host(grid))
    idx, ph, out = idx.to_host(), ph.to_host(), out.to_host()
    assert np.abs(ph).max() > np.pi                              # the phase did wander: the unwrap correction is exercised
    for m in range(E.shape[0]):
        raw = grid[idx[m]]
        turns = np.rint((ph[m, N:L - N].astype(np.float64) - raw[N:L - N]) / (np.pi / 2)).astype(np.int64)
        np.testing.assert_array_equal(turns, _unwrap_quarter_turns(grid, idx[m], N))
        np.testing.assert_array_equal(ph[m, :N], raw[:N])
        np.testing.assert_array_equal(ph[m, L - N:], raw[L - N:])
    _close(out, E.astype(np.complex128) * np.exp(1j * ph.astype(np.float64)), "c64")


@pytest.mark.parametrize("key,value", [("bps", "fused"), ("bps", "plain"), ("pit_xaside", "1"), ("la_profile", "1")])
def test_set_form_rejects_retired_forms(key, value, forms):
    """Forms that measurements rejected are gone from the table: qh_set_form answers QH_ERR_ARG and leaves the phase search automatic."""
    with pytest.raises(ValueError):
        forms.set(key, value)
    assert _lib.get_form("bps") == 0
