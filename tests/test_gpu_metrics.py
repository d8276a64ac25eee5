"""Signal-quality metrics on the MI355X against the reference (tests/golden/metrics.npz, gen_golden_metrics.py): SignalQAM's
metric methods, the pythran_dsp drop-ins, the pilot-frame forms and the device-resident pass of ResidentReceiver.metrics."""
import numpy as np
import pytest

from qampy_amd import synth, theory
from qampy_amd.core import hip_dsp, signal_quality
from qampy_amd.signals import PilotSignal, SignalQAM

pytestmark = pytest.mark.gpu

MS = (4, 16, 32, 64, 128, 256)
CT = {"c64": np.complex64, "c128": np.complex128}
RTOL = {"c64": 1e-5, "c128": 1e-12}         # evm / snr / s0 / n0
GABS = {"c64": 1e-5, "c128": 1e-10}         # gmi, gmi per bit, mi


@pytest.fixture(scope="module")
def fx(golden):
    return golden["metrics"]


def _cx(q, fx):
    """Complex samples from the fixture's int16 (re, im) * rx_scale."""
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(fx["rx_scale"])


def _rx(fx, M, j):
    """Received rows of case (M, j): the stored offsets from the rounded transmitted points, put back together."""
    base = np.round(fx["M%d_c128_coded" % M][fx["M%d_s%d_tx_label" % (M, j)]] * float(fx["rx_scale"]))
    return _cx(fx["M%d_s%d_rxd" % (M, j)] + np.stack([base.real, base.imag], axis=-1), fx)


def _signal(fx, rx, label, M, dn):
    coded = fx["M%d_%s_coded" % (M, dn)]
    return SignalQAM(rx.astype(CT[dn]), M, symbols=coded[label], coded_symbols=coded)


def _close_where_finite(got, ref, atol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(got[fin])), (what, got, ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=0, atol=atol, err_msg=what)


def _check_metrics(sig, fx, pre, dn):
    np.testing.assert_array_equal(sig.cal_ser(), fx[pre + "ser"])
    np.testing.assert_array_equal(sig.cal_ber(), fx[pre + "ber"])
    snr, s0, n0 = sig.est_snr(verbose=True)
    for name, v in (("snr", snr), ("s0", s0), ("n0", n0)):
        np.testing.assert_allclose(v, fx[pre + name], rtol=RTOL[dn], err_msg=name)
    np.testing.assert_allclose(sig.cal_evm(), fx[pre + "evm"], rtol=RTOL[dn])
    np.testing.assert_allclose(sig.cal_evm(blind=True), fx[pre + "evm_blind"], rtol=RTOL[dn])
    for suf, minmax in (("", False), ("_minmax", True)):
        gmi, per_bit = sig.cal_gmi(llr_minmax=minmax)
        _close_where_finite(gmi, fx[pre + "gmi" + suf], GABS[dn], pre + "gmi" + suf)
        _close_where_finite(per_bit, fx[pre + "gmi_per_bit" + suf], GABS[dn], pre + "gmi_per_bit" + suf)
    _close_where_finite(sig.cal_mi(), fx[pre + "mi"], GABS[dn], pre + "mi")


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_signal_metrics_match_the_reference(fx, M, j, dn):
    pre = "M%d_s%d_%s_" % (M, j, dn)
    sig = _signal(fx, _rx(fx, M, j), fx["M%d_s%d_tx_label" % (M, j)], M, dn)
    _check_metrics(sig, fx, pre, dn)
    if j == 0:       # the Monte-Carlo MI over every transmitted point, on the reference's slice and N0
        n = int(fx["M%d_mi_slow_n" % M])
        rx, tx = np.asarray(sig), sig.symbols
        got = [signal_quality.cal_mi(np.ascontiguousarray(rx[m, :n]), np.ascontiguousarray(tx[m, :n]), sig.coded_symbols,
                                     1 / fx[pre + "snr"][m], fast=False) for m in range(2)]
        _close_where_finite(got, fx[pre + "mi_slow"], GABS[dn], pre + "mi_slow")


def _normal_sums(r0, coded, snr, nb):
    """(N, nb) mask: both of the reference's unshifted double sums sum_{bit_k = b} exp(-snr |s - r|^2) are normal numbers.  Below
    2.2e-308 they are subnormal and carry only a few significant bits, so the reference's LLR itself is off there (by up to ~0.3)."""
    d = np.abs(r0.astype(np.complex128)[:, None] - np.asarray(coded, dtype=np.complex128)[None, :]) ** 2
    e = np.exp(-snr * d)
    bits = (np.arange(coded.size)[None, :] >> np.arange(nb - 1, -1, -1)[:, None]) & 1
    tiny = np.finfo(np.float64).tiny
    return np.stack([np.minimum(e[:, b == 0].sum(1), e[:, b == 1].sum(1)) >= tiny for b in bits], axis=1)


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_demappers_match_the_reference(fx, M, j, dn):
    pre = "M%d_s%d_%s_" % (M, j, dn)
    nllr = int(fx["nllr"])
    r0 = np.ascontiguousarray(_rx(fx, M, j)[0, :nllr].astype(CT[dn]))
    bitmap, nb = fx["M%d_%s_bitmap_sig" % (M, dn)], int(np.log2(M))
    snr = fx[pre + "snr"][0]
    tol = dict(rtol=1e-5, atol=1e-4) if dn == "c64" else dict(rtol=1e-9, atol=1e-8)
    for suf, fn in (("llr", hip_dsp.soft_l_value_demapper), ("llr_minmax", hip_dsp.soft_l_value_demapper_minmax)):
        got, ref = fn(r0, nb, snr, bitmap), fx[pre + suf]
        assert got.shape == ref.shape == (nllr, nb) and got.dtype == np.float64
        fin = np.isfinite(ref)
        assert np.all(np.isfinite(got[fin])), suf
        cmp = fin & (_normal_sums(r0, fx["M%d_%s_coded" % (M, dn)], snr, nb) if suf == "llr" else True)
        np.testing.assert_allclose(got[cmp], ref[cmp], err_msg=suf, **tol)


@pytest.mark.parametrize("dn", CT)
def test_high_snr_llrs_stay_finite(fx, dn):
    """64-QAM at 25 dB: the exact LLRs of the MSBs are far beyond fp32's exp range (|L| > 88); the reference's double sums
    are still finite there, and so must the complex64 kernel be."""
    M, nb = int(fx["hisnr_M"]), 6
    r0 = np.ascontiguousarray(_cx(fx["hisnr_rxq"], fx).astype(CT[dn]))
    bitmap, snr = fx["M%d_%s_bitmap_sig" % (M, dn)], 10 ** (float(fx["hisnr_snr_db"]) / 10)
    # the reference's double sums on this input: finite and normal everywhere (its complex64 run, evaluated in float32, is not)
    ref = fx["hisnr_c128_llr"]
    assert ref.dtype == np.float64 and np.all(np.isfinite(ref)) and np.abs(ref).max() > 88 and np.all(_normal_sums(r0, fx["M%d_%s_coded" % (M, dn)], snr, nb))
    got = hip_dsp.soft_l_value_demapper(r0, nb, snr, bitmap)
    assert np.all(np.isfinite(got))
    tol = dict(rtol=1e-5, atol=1e-4) if dn == "c64" else dict(rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(got, ref, **tol)
    np.testing.assert_allclose(hip_dsp.soft_l_value_demapper_minmax(r0, nb, snr, bitmap), fx["hisnr_%s_llr_minmax" % dn], **tol)


@pytest.mark.parametrize("dn", CT)
def test_unsynchronised_signal_metrics(fx, dn):
    """Quarter turn, cyclic shift and swapped modes, synced=False: aligned on the host like the reference, then measured."""
    M = int(fx["sync_M"])
    sig = _signal(fx, _cx(fx["sync_rxq"], fx), fx["sync_%s_tx_label" % dn], M, dn)
    _check_metrics(sig, fx, "sync_%s_" % dn, dn)


def test_estimate_snr_and_mi_drop_ins():
    """The host-array drop-ins on one row: estimate_snr against an independent numpy restatement, an empty class is NaN,
    cal_mi_mc_fast equals cal_mi_mc's order of magnitude at moderate SNR."""
    rng = np.random.default_rng(5)
    al = theory.coded_symbols_qam(16)
    tx = al[rng.integers(0, 16, 8192)]
    rx = tx + 0.1 * (rng.standard_normal(tx.size) + 1j * rng.standard_normal(tx.size))
    snr, s0, n0 = hip_dsp.estimate_snr(rx, tx, al)
    mu = np.array([rx[tx == a].mean() for a in al])
    var = np.array([np.mean(np.abs(rx[tx == a] - m) ** 2) for a, m in zip(al, mu)])
    px = np.array([np.count_nonzero(tx == a) for a in al]) / tx.size
    np.testing.assert_allclose([s0, n0], [np.sum(np.abs(mu) ** 2 * px), np.sum(var * px)], rtol=1e-12)
    assert np.isnan(hip_dsp.estimate_snr(rx, np.where(tx == al[3], al[4], tx), al)[0])
    fast = hip_dsp.cal_mi_mc_fast(rx, tx, al, n0)
    slow = hip_dsp.cal_mi_mc(rx[:256] - tx[:256], al, n0)
    assert 3.5 < fast <= 4 and abs(fast - slow) < 0.1


@pytest.mark.parametrize("snr_db", [5., 10., 15.])
def test_qpsk_gmi_equals_mi(snr_db):
    """For Gray-labelled QPSK the GMI equals the MI (the reference's own check, test_signal_quality_calc.py:180-196)."""
    tx = np.asarray(synth.make_capture(4, 2 ** 14, nmodes=2, os=1, seed=31, dtype=np.complex128).symbols)
    rng = np.random.default_rng(32)
    rx = tx + 10 ** (-snr_db / 20) * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape)) / np.sqrt(2)
    sig = SignalQAM(rx, 4, symbols=tx)
    gmi, _ = sig.cal_gmi()
    np.testing.assert_allclose(gmi, sig.cal_mi(), rtol=0.05)


def test_pilot_signal_metrics_equal_the_payload_metrics():
    M, frame_len, seq_len, ins_rat, nframes = 16, 2 ** 12, 128, 32, 2
    rng = np.random.default_rng(77)
    _, idx_dat, idx_pil = PilotSignal._cal_pilot_idx(frame_len, seq_len, ins_rat)
    al, alp = theory.coded_symbols_qam(M), theory.coded_symbols_qam(4)
    payload = al[rng.integers(0, M, (2, np.count_nonzero(idx_dat)))]
    pilots = alp[rng.integers(0, 4, (2, np.count_nonzero(idx_pil)))]
    frame = np.zeros((2, frame_len), np.complex128)
    frame[:, idx_dat], frame[:, idx_pil] = payload, pilots
    data = np.tile(frame, nframes)
    data = data + 0.08 * (rng.standard_normal(data.shape) + 1j * rng.standard_normal(data.shape))
    p = PilotSignal(data, M, 1., 1., frame_len, seq_len, ins_rat, pilots, symbols=payload)
    ref = SignalQAM(p.get_data(), M, symbols=np.tile(payload, nframes), coded_symbols=p.coded_symbols)
    np.testing.assert_array_equal(p.cal_ber(), ref.cal_ber(synced=True))
    np.testing.assert_array_equal(p.cal_evm(), ref.cal_evm(synced=True))
    np.testing.assert_array_equal(p.est_snr(), ref.est_snr(synced=True))
    np.testing.assert_array_equal(p.cal_gmi()[1], ref.cal_gmi(synced=True)[1])
    psnr = p.est_snr(use_pilots=True)
    assert np.all(np.abs(10 * np.log10(psnr / p.est_snr())) < 1.5)             # pilots see the same noise
    np.testing.assert_array_equal(p.cal_gmi(use_pilot_snr=True)[0], ref.cal_gmi(synced=True, snr=10 * np.log10(psnr))[0])


def test_resident_receiver_metrics_at_c3_shape():
    """C3 shape (64-QAM, 2 x 2^22 symbols, cma + mrde, 64 test angles), synthesised on the device: the fused pass counts the same
    errors as .ser(), and every other field equals the host methods on the fetched rows aligned explicitly; repeat calls are
    bit-identical."""
    from qampy_amd.pipeline import ResidentReceiver
    M, nsym, trim = 64, 2 ** 22, 2000
    d = synth.make_capture_dev(M, nsym, nmodes=2, snr_db=30, theta=np.pi / 5.6, dgd=30e-12, linewidth=100., seed=1000)
    rx = ResidentReceiver(2, 2 * nsym, 2, M, 41, (2e-4, 2e-4), methods=("cma", "mrde"), Niter=(1, 1), Mtestangles=64, Nbps=20,
                          alphabet=d["alphabet_host"])
    rx.E.copy_from(d["E"])
    rx.run()
    tx = d["symbols"].to_host()
    ser = rx.ser(tx, maxlag=256, trim=trim)
    met = rx.metrics(tx, maxlag=256, trim=trim)
    again = rx.metrics(tx, maxlag=256, trim=trim)
    out = rx.fetch()["out"]
    for r in range(2):
        m, s = met[r], ser[r]
        assert (m["errors"], m["compared"], m["tx_mode"], m["rotation"], m["lag"]) == (s["errors"], s["compared"], s["tx_mode"], s["rotation"], s["lag"])
        assert m["ser"] == s["ser"]
        for k in ("gmi", "mi", "ber", "evm", "snr", "s0", "n0"):
            assert again[r][k] == m[k], k
        np.testing.assert_array_equal(again[r]["gmi_per_bit"], m["gmi_per_bit"])
        i = np.arange(trim, out.shape[1] - trim)
        i = i[(i - m["lag"] >= 0) & (i - m["lag"] < tx.shape[1])]
        host = SignalQAM((out[r, i] * 1j ** m["rotation"])[None], M, symbols=tx[m["tx_mode"], i - m["lag"]][None], coded_symbols=d["alphabet_host"])
        assert m["compared"] == i.size
        assert m["ber"] == host.cal_ber(synced=True)[0]
        snr, s0, n0 = host.est_snr(synced=True, verbose=True)
        np.testing.assert_allclose([m["snr"], m["s0"], m["n0"], m["evm"]], [snr[0], s0[0], n0[0], host.cal_evm(synced=True)[0]], rtol=1e-5)
        gmi, per_bit = host.cal_gmi(synced=True)
        np.testing.assert_allclose(m["gmi"], gmi[0], rtol=0, atol=1e-5)
        np.testing.assert_allclose(m["gmi_per_bit"], per_bit[0], rtol=0, atol=1e-5)
        np.testing.assert_allclose(m["mi"], host.cal_mi(synced=True)[0], rtol=0, atol=1e-5)
        assert m["ber"] < 1e-3 and 5.5 < m["gmi"] <= 6 + 1e-6 and 5.5 < m["mi"] <= 6 + 1e-6       # estimates: log2(M) up to rounding
