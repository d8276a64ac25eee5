"""The float64 restatement of the whole-row transforms and the analog front end (tests/frontend_ref.py) against ``np.fft`` and against
fixtures recorded from the reference (tests/golden/frontend.npz).  No GPU."""
import json

import numpy as np
import pytest

import frontend_ref as fr

# double arithmetic throughout: the restatement differs from np.fft and from the reference by roundings of a log-depth transform
BAR = 1e-11


def err(got, want):
    want = np.asarray(want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    return np.abs(np.asarray(got) - want).max() / (rms if rms > 0 else 1.0)


def rows(L, n=2, seed=5):
    rng = np.random.default_rng(seed + L)
    return rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))


@pytest.fixture(scope="module")
def gold(golden):
    g = golden["frontend"]
    return g, json.loads(str(g["cases"]))


def test_plan():
    assert fr.plan(256) == (256, 1, 256, False) and fr.plan(8192) == (8192, 1, 8192, False)
    assert fr.plan(2 ** 14) == (2 ** 14, 128, 128, False) and fr.plan(2 ** 15) == (2 ** 15, 128, 256, False)
    assert fr.plan(2 ** 24) == (2 ** 24, 4096, 4096, False)
    assert fr.plan(2) == (256, 1, 256, True) and fr.plan(128) == (256, 1, 256, True) and fr.plan(129) == (512, 1, 512, True)
    assert fr.plan(4095)[0] == 8192 and fr.plan(4097) == (16384, 128, 128, True) and fr.plan(2 ** 23 - 1)[0] == 2 ** 24
    assert fr.plan(2 ** 23)[3] is False
    for bad in (0, 1, 2 ** 24 + 1, 2 ** 25, 2 ** 23 + 1):
        with pytest.raises(ValueError):
            fr.plan(bad)


@pytest.mark.parametrize("L", [2 ** 14, 2 ** 15, 2 ** 17])
def test_four_step_is_the_dft(L):
    x = rows(L, 1)
    _, N1, N2, _ = fr.plan(L)
    assert err(fr.four_step(x, N1, N2), np.fft.fft(x, axis=1)) < BAR
    assert err(fr.fft(x, inverse=True), np.fft.ifft(x, axis=1)) < BAR


@pytest.mark.parametrize("L", [2, 3, 255, 257, 1000, 4095, 4097, 12289])
def test_bluestein_is_the_dft(L):
    x = rows(L)
    assert err(fr.bluestein(x), np.fft.fft(x, axis=1)) < BAR
    assert err(fr.bluestein(x, inverse=True), np.fft.ifft(x, axis=1)) < BAR


def test_integer_chirp():
    L = 100003
    n = np.arange(L)
    exact = np.exp(-1j * np.pi * np.array([(int(v) * int(v)) % (2 * L) for v in n[-50:]], dtype=np.float64) / L)
    assert np.abs(fr.chirp(L)[-50:] - exact).max() < 1e-15


@pytest.mark.parametrize("L", [3, 1000, 4097, 30011])
def test_single_precision_bluestein_leaves_a_margin(L):
    """the chirp cast from double, the transforms in single: well inside the complex64 bar of 1e-5"""
    x = rows(L).astype(np.complex64)
    want = np.fft.fft(x.astype(np.complex128), axis=1)
    assert err(fr.bluestein(x, dtype=np.complex64), want) < 3e-6


@pytest.mark.parametrize("L", [8, 9, 600, 601])
def test_brick_wall_is_the_reference_mask(L):
    for bw in (8, 16, 0.01, 3.7, 2 * L + 1.0, 1e9):
        c = int(L / (bw / 2))
        h = np.zeros((1, L))
        h[:, c:-c] = 1
        assert np.array_equal(fr.H_brick(L, bw), np.fft.ifftshift(h[0])), (L, bw)


def test_band_and_ramp_grids():
    import scipy.fft as sf
    for L in (16, 17):
        f = sf.fftfreq(L, 1 / 2)
        assert np.array_equal(fr.H_band(L, 0.8, 2, 0.25), (np.abs(f - 0.25) < 0.4).astype(float))
        fv = np.fft.fftfreq(L, 50e9 / 2)
        assert np.array_equal(fr.signed_bins(L) * (1.0 / (L * (50e9 / 2))), fv)
        assert np.abs(fr.H_ramp(L, 0.3 * 25e9, 50e9) - np.exp(-1j * 2 * np.pi * 0.3 * 25e9 * fv)).max() < 1e-15


def test_two_rail_is_two_separate_delays():
    for L in (64, 65, 1000):
        x = rows(L)
        sr, ti, tq = 50e9, 0.3 * 25e9, -2.6 * 25e9

        def delay(v, t):
            return np.fft.ifft(np.exp(-1j * 2 * np.pi * t * np.fft.fftfreq(L, sr / 2)) * np.fft.fft(v, axis=1)).real
        want = delay(x.real, ti) + 1j * delay(x.imag, tq)
        assert err(fr.skew(x, ti, tq, sr), want) < BAR


def test_fixtures_pre_filter(gold):
    g, cases = gold
    for c, bws in cases["pre"]:
        x = g["pre_x_" + c]
        for i, bw in enumerate(bws):
            want = g["pre_y_%s_%d" % (c, i)]
            got = fr.spectral(x, fr.H_brick(x.shape[-1], bw)).reshape(want.shape)
            bar = 1e-5 if x.dtype == np.complex64 else BAR            # the reference's scipy.fft keeps complex64
            assert err(got, want) < bar, (c, bw)
            assert (bw == 0.01) == (not np.any(got))


def test_fixtures_comp_rf_delay(gold):
    g, cases = gold
    for c, delays, sr in cases["delay"]:
        x = g["delay_x_" + c]
        for i, d in enumerate(delays):
            want = g["delay_y_%s_%d" % (c, i)]
            if np.iscomplexobj(x):
                got = fr.spectral(x, fr.H_ramp(x.shape[-1], d, sr)).real
            else:
                got = fr.skew(x, d, 0.0, sr)
                assert np.abs(got.imag).max() < 1e-13                  # rail Q of a real input: roundings of X[k] - conj X[-k]
                got = got.real
            assert err(got.reshape(want.shape), want) < BAR, (c, d)


def test_fixtures_orthonormalize(gold):
    g, cases = gold
    for c, os_ in cases["orth"]:
        x, want = g["orth_x_" + c], g["orth_y_" + c]
        bar = 1e-5 if x.dtype == np.complex64 else BAR                # the reference computes a complex64 input in float32
        assert err(fr.orthonormalize(x, os_), want) < bar, c
        if x.dtype == np.complex128:
            y = fr.orthonormalize(x, os_)[:, ::os_]
            assert np.abs(np.mean(np.abs(y) ** 2, axis=1) - 1).max() < 1e-12 and np.abs(y.mean(axis=1)).max() < 1e-12


def test_fixtures_comp_iq_imbalance(gold):
    g, cases = gold
    for c in cases["iq"]:
        x, want, centred = g["iq_x_" + c], g["iq_y_" + c], g["iq_c_" + c]
        bar = 1e-5 if x.dtype == np.complex64 else BAR
        assert err(fr.comp_iq_imbalance(x).reshape(want.shape), want) < bar, c
        xx = np.atleast_2d(x)
        got_c = fr.affine(xx, fr.coeffs_imbalance(fr.moments(xx), xx.shape[1], centre_only=True))
        assert err(got_c.reshape(centred.shape), centred) < bar, c
