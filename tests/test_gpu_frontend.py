"""Whole-row transforms (csrc/fft.hip) and the analog front end (csrc/iq.hip) on the GPU: the transforms against ``np.fft`` in double, the
spectral multiplies and the IQ maps against the float64 restatement (tests/frontend_ref.py), the drop-ins and signal wrappers against the
reference's outputs (tests/golden/frontend.npz), and ``ResidentReceiver.frontend`` in front of the receiver.

Bars are max-abs errors over the row relative to the rms of the expected output, the project's own for transforms (tests/test_gpu_cd.py):
1e-5 for complex64 and 1e-11 for complex128."""
import json

import numpy as np
import pytest

import frontend_ref as fr
import qampy_amd
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import analog_frontend as caf
from qampy_amd.core import filter as cfilter
from qampy_amd.core import hip_dsp

pytestmark = pytest.mark.gpu

BAR = {np.dtype(np.complex64): 1e-5, np.dtype(np.complex128): 1e-11}
SR = 50e9
SAMPLE = SR / 2                    # one sample of delay on the reference's grid fftfreq(L, sampling_rate / 2)


def rel_max(got, want):
    """worst row: max-abs error over the row relative to the rms of the expected row"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2, axis=-1))
    return float((np.abs(got - want).max(axis=-1) / np.where(rms > 0, rms, 1.0)).max())


def check(got, want, dtype, what=None):
    e = rel_max(got, want)
    print("%s %s: %.3g (bar %g)" % (what, np.dtype(dtype).name, e, BAR[np.dtype(dtype)]))
    assert np.all(np.isfinite(got))
    assert e <= BAR[np.dtype(dtype)], (what, e)


def field(rows, L, dtype, seed=0):
    rng = np.random.default_rng(1000 * seed + L % 9973)
    rt = np.float32 if dtype == np.complex64 else np.float64
    x = np.empty((rows, L), dtype)
    x.real = rng.standard_normal((rows, L), dtype=rt)
    x.imag = rng.standard_normal((rows, L), dtype=rt)
    return x


def run(f, x, *a, inplace=False, **k):
    E = DeviceArray.from_host(x)
    out = E if inplace else DeviceArray(x.shape, x.dtype)
    f(E, out, *a, **k)
    return out.to_host()


# ------------------------------------------------------------------------------------------------ transforms
POW2 = [(lg, np.complex64) for lg in range(8, 25)] + [(lg, np.complex128) for lg in range(8, 21)]
BLUE = [2, 3, 255, 257, 1000, 4095, 4097, 12289, 100003]


@pytest.mark.parametrize("lg,dtype", POW2)
def test_fft_power_of_two(lg, dtype):
    rows = 2 if lg in (8, 13, 14, 15) else 1
    x = field(rows, 2 ** lg, dtype, lg)
    x128 = x.astype(np.complex128)
    check(run(hip_dsp.fft_dev, x), np.fft.fft(x128, axis=1), dtype, "fft 2^%d" % lg)
    check(run(hip_dsp.ifft_dev, x), np.fft.ifft(x128, axis=1), dtype, "ifft 2^%d" % lg)


@pytest.mark.parametrize("L", BLUE)
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_fft_bluestein(L, dtype):
    x = field(2, L, dtype, 3)
    x128 = x.astype(np.complex128)
    check(run(hip_dsp.fft_dev, x), np.fft.fft(x128, axis=1), dtype, "fft %d" % L)
    check(run(hip_dsp.ifft_dev, x), np.fft.ifft(x128, axis=1), dtype, "ifft %d" % L)


@pytest.mark.parametrize("L", [256, 8192, 2 ** 14, 2 ** 17, 3, 1000, 4097, 100003])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_round_trip_repeat_and_in_place(L, dtype):
    x = field(2, L, dtype, 7)
    E = DeviceArray.from_host(x)
    X, X2, y = DeviceArray(x.shape, dtype), DeviceArray(x.shape, dtype), DeviceArray(x.shape, dtype)
    hip_dsp.fft_dev(E, X)
    hip_dsp.ifft_dev(X, y)
    check(y.to_host(), x, dtype, "ifft(fft) %d" % L)
    hip_dsp.fft_dev(E, X2)                                                 # a repeated call is bit-identical
    a, b = X.to_host(), X2.to_host()
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    hip_dsp.fft_dev(E, E)                                                  # out may be E itself
    assert np.array_equal(E.to_host().view(np.uint8), a.view(np.uint8))
    hip_dsp.ifft_dev(X2, X2)
    assert np.array_equal(X2.to_host().view(np.uint8), y.to_host().view(np.uint8))


def test_lengths_out_of_range_are_argument_errors_in_the_library_too():
    import ctypes as C
    lib = _lib.load()
    x = DeviceArray((1, 256), np.complex64)
    for L in (0, 1, 2 ** 24 + 2, 2 ** 25, 2 ** 23 + 1):
        assert lib.qh_fft_c64_dev(C.c_void_p(x.ptr), 1, L, 0, C.c_void_p(x.ptr)) == _lib.QH_ERR_ARG
        assert lib.qh_spectral_filter_c64_dev(C.c_void_p(x.ptr), 1, L, 1, 0., 0., 0., 0, 0, None, C.c_void_p(x.ptr)) == _lib.QH_ERR_ARG
    assert lib.qh_spectral_filter_c64_dev(C.c_void_p(x.ptr), 1, 256, 0, 0., 0., 0., 0, 0, None, C.c_void_p(x.ptr)) == _lib.QH_ERR_ARG
    assert lib.qh_spectral_filter_c64_dev(C.c_void_p(x.ptr), 1, 256, 5, 0., 0., 0., 0, 0, None, C.c_void_p(x.ptr)) == _lib.QH_ERR_ARG


# ------------------------------------------------------------------------------------------------ spectral multiplies
FILTER_L = [1024, 2 ** 14, 1001, 1000, 4097]          # even and one workgroup; four-step; odd (Bluestein); even Bluestein; Bluestein on a four-step M


def ref_delay(v, t, L):
    """comp_rf_delay of qampy/core/analog_frontend.py:54-88 on real rows"""
    return np.fft.ifft(np.exp(-1j * 2 * np.pi * t * np.fft.fftfreq(L, SR / 2)) * np.fft.fft(v, axis=1)).real


@pytest.mark.parametrize("L", FILTER_L)
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_spectral_kinds_match_restatement(L, dtype):
    x = field(2, L, dtype, 11)
    for bw in (8, 16, 3.7):
        check(run(hip_dsp.pre_filter_dev, x, bw), fr.spectral(x, fr.H_brick(L, bw)), dtype, "brick %g L=%d" % (bw, L))
    assert not np.any(run(hip_dsp.pre_filter_dev, x, 0.01))                # the reference's own test case: an empty slice, all zeros
    for os_, bw, cf in ((2, 0.8, 0.25), (2, 1.0, 0.0), (4, 0.5, -1.1)):
        check(run(hip_dsp.pre_filter_wdm_dev, x, bw, os_, cf), fr.spectral(x, fr.H_band(L, bw, os_, cf)), dtype, "band L=%d" % L)
    for ti, tq in ((0.3 * SAMPLE, -2.6 * SAMPLE), (0.0, 5.25 * SAMPLE)):
        got = run(hip_dsp.skew_dev, x, ti, tq, SR)
        check(got, fr.skew(x, ti, tq, SR), dtype, "two rails L=%d" % L)
        x128 = x.astype(np.complex128)
        check(got, ref_delay(x128.real, ti, L) + 1j * ref_delay(x128.imag, tq, L), dtype, "two separate delays L=%d" % L)
    check(run(hip_dsp.delay_dev, x, 1.7 * SAMPLE, SR), fr.spectral(x, fr.H_ramp(L, 1.7 * SAMPLE, SR)), dtype, "ramp L=%d" % L)
    rng = np.random.default_rng(L)
    rt = np.float32 if dtype == np.complex64 else np.float64
    Hr = rng.standard_normal(L).astype(rt)
    Hc = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(dtype)
    check(run(hip_dsp.spectral_filter_dev, x, DeviceArray.from_host(Hr)), fr.spectral(x, Hr.astype(np.float64)), dtype, "real table L=%d" % L)
    check(run(hip_dsp.spectral_filter_dev, x, DeviceArray.from_host(Hc)), fr.spectral(x, Hc.astype(np.complex128)), dtype, "complex table L=%d" % L)
    a = run(hip_dsp.skew_dev, x, 0.3 * SAMPLE, -2.6 * SAMPLE, SR)
    b = run(hip_dsp.skew_dev, x, 0.3 * SAMPLE, -2.6 * SAMPLE, SR, inplace=True)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ IQ conditioning
T = hip_dsp.IQ_TILE


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_moments_at_the_edges(dtype):
    for L in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        for os_ in (1, 2, 3):
            x = field(2, L, dtype, L + os_) + dtype(0.3 - 0.2j)
            E = DeviceArray.from_host(x)
            got = hip_dsp.iq_moments_dev(E, os_).to_host()
            want = fr.moments(x, os_)
            assert got.shape == (2, 10)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (L, os_)
            assert np.array_equal(got, hip_dsp.iq_moments_dev(E, os_).to_host())           # bit-reproducible


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_orthonormalize_and_imbalance_match_restatement(dtype):
    for L, os_ in ((1000, 1), (1001, 2), (T + 1, 3), (3 * T + 5, 2)):
        x = field(2, L, dtype, 5)
        x = (x.real + 1j * (1.2 * (x.imag * np.cos(0.3) + x.real * np.sin(0.3))) + (0.2 - 0.1j)).astype(dtype)
        check(run(hip_dsp.orthonormalize_dev, x, os_), fr.orthonormalize(x, os_), dtype, "orthonormalize L=%d os=%d" % (L, os_))
        check(run(hip_dsp.orthonormalize_dev, x, os_, inplace=True), fr.orthonormalize(x, os_), dtype, "orthonormalize in place")
        E = DeviceArray.from_host(x)
        out = DeviceArray(x.shape, dtype)
        hip_dsp.comp_iq_imbalance_dev(E, out)
        check(out.to_host(), fr.comp_iq_imbalance(x), dtype, "imbalance L=%d" % L)
        check(E.to_host(), x.astype(np.complex128) - x.astype(np.complex128).mean(), dtype, "centred in place")


# ------------------------------------------------------------------------------------------------ drop-ins against the reference's outputs
@pytest.fixture(scope="module")
def gold(golden):
    g = golden["frontend"]
    return g, json.loads(str(g["cases"]))


def sig_of(x, fb, fs):
    from qampy_amd.signals import SignalQAM
    return SignalQAM(np.array(x), 16, fb=fb, fs=fs)


def test_pre_filter_matches_fixture(gold):
    g, cases = gold
    for c, bws in cases["pre"]:
        x = g["pre_x_" + c]
        for i, bw in enumerate(bws):
            want = g["pre_y_%s_%d" % (c, i)]
            got = cfilter.pre_filter(x, bw)
            assert got.shape == want.shape and got.dtype == want.dtype
            check(got, want, x.dtype, "pre_filter %s bw=%g" % (c, bw))
            assert (bw == 0.01) == (not np.any(got))
            if x.ndim == 2:
                s = qampy_amd.filtering.pre_filter(sig_of(x, 1.0, 2.0), bw)
                assert type(s).__name__ == "SignalQAM" and s.fs == 2.0 and np.array_equal(np.asarray(s), got)


def test_pre_filter_wdm_is_the_restated_reference():
    import scipy.fft as sf
    for L in (1000, 1001):
        x = field(1, L, np.complex128, 2)[0]
        h = np.zeros(L)
        h[np.where(abs(sf.fftfreq(L, 1 / 2) - 0.25) < 0.8 / 2)] = 1
        got = cfilter.pre_filter_wdm(x, 0.8, 2, 0.25)
        assert got.shape == x.shape and got.dtype == x.dtype
        check(got, sf.ifft(sf.fft(x) * h), np.complex128, "pre_filter_wdm L=%d" % L)
    assert cfilter.pre_filter_wdm(field(2, 1000, np.complex64, 2), 0.8, 2).dtype == np.complex64


def test_comp_rf_delay_matches_fixture(gold):
    g, cases = gold
    for c, delays, sr in cases["delay"]:
        x = g["delay_x_" + c]
        for i, d in enumerate(delays):
            want = g["delay_y_%s_%d" % (c, i)]
            got = caf.comp_rf_delay(x, d, sr)
            assert got.shape == want.shape and got.dtype == np.float64
            check(got, want, np.complex128, "comp_rf_delay %s %g" % (c, d))
            if np.iscomplexobj(x):
                s = qampy_amd.analog_frontend.comp_rf_delay(sig_of(x, sr / 2, sr), d)
                assert type(s).__name__ == "SignalQAM" and np.array_equal(np.asarray(s), np.atleast_2d(got))
    assert caf.comp_rf_delay(g["delay_x_e1"].astype(np.float32), delays[0], sr).dtype == np.float64


def test_orthonormalize_signal_matches_fixture(gold):
    g, cases = gold
    for c, os_ in cases["orth"]:
        x, want = g["orth_x_" + c], g["orth_y_" + c]
        got = caf.orthonormalize_signal(x, os_)
        assert got.shape == want.shape and got.ndim == 2 and got.dtype == want.dtype
        check(got, want, x.dtype, "orthonormalize_signal %s" % c)
        s = qampy_amd.analog_frontend.orthonormalize_signal(sig_of(x, 1.0, float(os_)))
        assert np.array_equal(np.asarray(s), got)


def test_comp_iq_inbalance_matches_fixture(gold):
    g, cases = gold
    for c in cases["iq"]:
        x, want, centred = np.array(g["iq_x_" + c]), g["iq_y_" + c], g["iq_c_" + c]
        got = caf.comp_IQ_inbalance(x)
        assert got.shape == want.shape and got.dtype == want.dtype
        check(got, want, x.dtype, "comp_IQ_inbalance %s" % c)
        check(x, centred, x.dtype, "comp_IQ_inbalance %s: the argument, centred in place" % c)


# ------------------------------------------------------------------------------------------------ resident path
NSYM, TRIM = 2 ** 14, 4000
SNR_DB = 30                 # 16-QAM, no channel: the clean receiver makes no symbol error here (and none on the CPU restatement of this test)
PHI, GAIN, DC, TAU_Q, TONE, BW = np.deg2rad(15.0), 1.15, 0.15 - 0.1j, 0.4 * SAMPLE, (0.4, 0.5), 10


def hybrid_impair(E):
    """quadrature error, Q gain and offsets of the hybrid, a longer cable on the Q rail, and a tone outside the signal band"""
    E = np.asarray(E).astype(np.complex128)
    L = E.shape[1]
    y = E.real + 1j * GAIN * (E.imag * np.cos(PHI) + E.real * np.sin(PHI)) + DC
    y = fr.skew(y, 0.0, TAU_Q, SR)
    return y + TONE[1] * np.exp(2j * np.pi * TONE[0] * np.arange(L))


def receive(E, sig, frontend, tier):
    from qampy_amd.pipeline import ResidentReceiver
    rx = ResidentReceiver(2, E.shape[1], 2, 16, 21, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(2, 1), Mtestangles=32, Nbps=20,
                          alphabet=sig.coded_symbols, tier=tier)
    rx.load(E)
    if frontend:
        rx.frontend(**frontend)
    cond = rx.E.to_host()
    rx.run()
    out = rx.fetch()["out"]
    nerr = [synth.count_symbol_errors(r, sig.symbols, sig.coded_symbols, max_lag=256, trim=TRIM)[0] for r in out]
    return cond, nerr, rx


@pytest.mark.parametrize("tier", ["a", "b"])
def test_resident_frontend(tier):
    sig = synth.make_capture(16, NSYM, nmodes=2, snr_db=SNR_DB, seed=21, dtype=np.complex64)
    clean = np.ascontiguousarray(np.asarray(sig))
    bad = hybrid_impair(clean).astype(np.complex64)
    _, nerr_clean, _ = receive(clean, sig, None, tier)
    assert nerr_clean == [0, 0], nerr_clean
    cond, nerr, rx = receive(bad, sig, dict(orthonormalize=True, skew=(0.0, -TAU_Q), sampling_rate=SR, pre_filter_bw=BW), tier)
    # the conditioned buffer is the host drop-ins in the same order
    want = caf.comp_rf_delay(np.ascontiguousarray(bad.real), 0.0, SR) + 1j * caf.comp_rf_delay(np.ascontiguousarray(bad.imag), -TAU_Q, SR)
    want = caf.orthonormalize_signal(cfilter.pre_filter(want, BW), 2)
    check(cond, want, np.complex64, "resident frontend, tier %s" % tier)
    assert nerr == nerr_clean, (nerr, nerr_clean)
    if tier == "b":
        assert abs(rx._load_power - np.mean(np.abs(cond[:, :4096].astype(np.complex128)) ** 2)) < 1e-6
        assert 0.5 < rx._load_power < 2.0
    # the impairment is not harmless: untreated, the receiver fails
    if tier == "a":
        _, nerr_raw, _ = receive(bad, sig, None, tier)
        assert min(nerr_raw) > 100, nerr_raw
