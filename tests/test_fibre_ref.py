"""Pins the numpy restatement of the fibre model (tests/fibre_ref.py) to physics, so that the GPU tests compare against something that is itself
checked: a fundamental soliton, the two limits with a closed form, and the inverse.  No GPU."""
import numpy as np
import pytest

import fibre_ref as fr

FS, D, GAMMA = 64e9, 17e-6, 1.3e-3
SPAN = 80e3


def field(rows, L, seed=0):
    """Gaussian, band-limited to half the band, unit power per row"""
    rng = np.random.default_rng(100 * seed + rows + L)
    x = rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))
    S = np.fft.fft(x, axis=-1)
    S[:, np.abs(np.fft.fftfreq(L)) > 0.25] = 0
    x = np.fft.ifft(S, axis=-1)
    return x / np.sqrt(np.mean(np.abs(x) ** 2, axis=-1, keepdims=True))


def soliton_error(steps, sign=1.0):
    """A fundamental soliton, gamma P0 T0^2 = |beta2|, over two dispersion lengths: the error against A exp(0.5j gamma P0 z), max-abs over the
    row relative to the row's rms (the pulse fills a fortieth of the window: its peak is 20 rms)"""
    L, fs, T0 = 4096, 256e9, 20e-12
    b2 = fr.beta2(D)                                                      # the project's sign: positive for D > 0, the anomalous regime
    P0 = abs(b2) / (GAMMA * T0 ** 2)
    z = 2 * T0 ** 2 / abs(b2)
    t = (np.arange(L) - L // 2) / fs
    A = np.sqrt(P0) / np.cosh(t / T0)
    out = fr.ssfm(A, fs, sign * D, z, 1, GAMMA, 0.0, steps, 1.0)[0]
    return fr.rel_max(out, A * np.exp(0.5j * GAMMA * P0 * z))


def test_soliton_keeps_its_shape_to_second_order():
    e = [soliton_error(n) for n in (20, 40, 80)]
    print("soliton error at 20 / 40 / 80 steps: %.3g %.3g %.3g" % tuple(e))
    for a, b in zip(e, e[1:]):
        assert 3.5 <= a / b <= 4.5, e
    assert e[2] <= 4e-3, e


def test_soliton_needs_the_sign_of_beta2():
    e = soliton_error(80, sign=-1.0)
    print("soliton with -beta2: %.3g" % e)
    assert e > 1, e


@pytest.mark.parametrize("rows", [1, 2])
def test_gamma_zero_is_one_dispersion_filter(rows):
    x = field(rows, 4096, 1)
    nspans = 2
    out = fr.ssfm(x, FS, D, SPAN, nspans, 0.0, fr.alpha_per_m(0.2), 8, 1e-3)
    w = 2 * np.pi * np.fft.fftfreq(4096, 1 / FS)
    want = np.fft.ifft(np.exp(-0.5j * w ** 2 * fr.beta2(D) * nspans * SPAN) * np.fft.fft(x, axis=-1), axis=-1)
    e = fr.rel_max(out, want)
    print("gamma = 0 against one filter: %.3g" % e)
    assert e <= 1e-12


@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("amplify", [True, False])
def test_no_dispersion_one_step_is_the_closed_form(rows, amplify):
    x = field(rows, 4096, 2)
    alpha, pscale = fr.alpha_per_m(0.2), 2e-3 / rows
    out = fr.ssfm(x, FS, 0.0, SPAN, 1, GAMMA, alpha, 1, pscale, amplify=amplify)
    heff = (1 - np.exp(-alpha * SPAN)) / alpha
    kappa = 8 / 9 if rows == 2 else 1.0
    want = x * np.exp(1j * kappa * GAMMA * pscale * heff * np.sum(np.abs(x) ** 2, axis=0)) * (1.0 if amplify else np.exp(-alpha * SPAN / 2))
    e = fr.rel_max(out, want)
    print("D = 0 against the closed form: %.3g" % e)
    assert e <= 1e-12


@pytest.mark.parametrize("steps", [8, [10e3, 30e3, 40e3]], ids=["equal", "list"])
@pytest.mark.parametrize("nspans", [1, 3])
@pytest.mark.parametrize("alpha_db_km", [0.0, 0.2])
@pytest.mark.parametrize("amplify", [True, False])
def test_backward_inverts_forward(steps, nspans, alpha_db_km, amplify):
    x = field(2, 1000, 3)
    alpha, pscale = fr.alpha_per_m(alpha_db_km), fr.pscale_of(x, 3.0)
    fw = fr.ssfm(x, FS, D, SPAN, nspans, GAMMA, alpha, steps, pscale, amplify=amplify)
    assert fr.rel_max(fw, x) > 0.1                                        # the link does something
    bk = fr.ssfm(fw, FS, D, SPAN, nspans, GAMMA, alpha, steps, pscale, backward=True, amplify=amplify)
    e = fr.rel_max(bk, x)
    print("backward after forward: %.3g" % e)
    assert e <= 1e-12
