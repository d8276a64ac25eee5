"""Nonlinear fibre on the GPU (csrc/fibre.hip): split-step propagation and back-propagation against the float64 restatement
(tests/fibre_ref.py, itself pinned in tests/test_fibre_ref.py), the two limits with a closed form, the amplifier noise against the draws of the
point-wise impairment pass, and ``ResidentReceiver.backpropagate`` in front of the receiver.

The error is the project's own for whole-row work (``rel_max`` of tests/test_gpu_frontend.py): max-abs over a row relative to the rms of the
expected row.  The bar of a call is derived from what it launches (``hip_dsp.fibre_plan``): every spectral filter may add the transforms' bar,
1e-5 (complex64) / 1e-11 (complex128), every nonlinear launch 4 eps of the real type (its rotator is good to 4 ulp).  Every case prints what it
measured beside its bar."""
import numpy as np
import pytest

import fibre_ref as fr
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import fibre as cfibre
from qampy_amd.core import hip_dsp
from qampy_amd.core import impairments as cimp

pytestmark = pytest.mark.gpu

BAR = {np.dtype(np.complex64): 1e-5, np.dtype(np.complex128): 1e-11}
FS, D, GAMMA, SPAN, DBM = 64e9, 17e-6, 1.3e-3, 80e3, 3.0
LIST = [10e3, 30e3, 40e3]
SHAPES = [(rows, L) for L in (1000, 4096, 16384) for rows in (1, 2)]
DTYPES = [np.complex64, np.complex128]


def eps(dtype):
    return float(np.finfo(np.float32 if np.dtype(dtype) == np.complex64 else np.float64).eps)


def bar(dtype, L, steps, nspans, scale=1.0):
    p = hip_dsp.fibre_plan(L, steps, nspans, SPAN)
    return scale * (p["filters"] * BAR[np.dtype(dtype)] + p["nonlinear"] * 4 * eps(dtype))


def check(got, want, b, what):
    e = fr.rel_max(got, want)
    print("%s: %.3g (bar %.3g)" % (what, e, b))
    assert np.all(np.isfinite(got))
    assert e <= b, (what, e, b)
    return e


_FIELDS = {}


def field(rows, L, dtype, seed=0):
    """Gaussian, band-limited to half the band, unit power per row; made once per shape, never written"""
    key = (rows, L, np.dtype(dtype), seed)
    if key not in _FIELDS:
        rng = np.random.default_rng(1000 * seed + 10 * L + rows)
        x = rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))
        S = np.fft.fft(x, axis=-1)
        S[:, np.abs(np.fft.fftfreq(L)) > 0.25] = 0
        x = np.fft.ifft(S, axis=-1)
        x = (x / np.sqrt(np.mean(np.abs(x) ** 2, axis=-1, keepdims=True))).astype(dtype)
        x.setflags(write=False)
        _FIELDS[key] = x
    return _FIELDS[key]


def run(f, x, inplace=False, **k):
    E = DeviceArray.from_host(np.ascontiguousarray(x))
    out = E if inplace else DeviceArray(x.shape, x.dtype)
    f(E, out, FS, D, SPAN, **k)
    return out.to_host()


# An orthogonal array of strength two over the seven two-valued factors of a call: every pair of settings meets in two of the eight rows.
# (backward, list of steps, three spans, no loss, no amplifier, in place, pscale instead of power_dbm)
CONFIGS = [tuple(bool(v) for v in (a, b, c, a ^ b, a ^ c, b ^ c, a ^ b ^ c)) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,L", SHAPES)
def test_parity_with_the_restatement(rows, L, dtype):
    """A forward case launches the unit-power field at 3 dBm.  A backward case is given what the same link delivers - the restatement's forward
    output, rounded to the dtype - at the same watts per unit of |E|^2, so it undoes a link that exists: without the amplifier that field is
    16 dB per span below the launch, and back-propagating the unit-power field itself would mean a launch of 19 dBm and more, Kerr phases of
    tens of radians, and an error of the filters in front of them multiplied by as much, which the bar's sum of launches does not describe
    (measured that way on one row of 16384 samples, the three-step list, no amplifier: the kernels 4.2e-5 from the restatement, the same
    steps in numpy's complex64 6.6e-5, the bar 4.1e-5)."""
    x0 = field(rows, L, dtype)
    ps = fr.pscale_of(x0, DBM)
    for backward, lst, three, lossless, bare, inplace, by_pscale in CONFIGS:
        steps, nspans, adb = LIST if lst else 8, 3 if three else 1, 0.0 if lossless else 0.2
        x, dbm = x0, DBM
        if backward:
            x = fr.ssfm(x0, FS, D, SPAN, nspans, GAMMA, fr.alpha_per_m(adb), steps, ps, amplify=not bare).astype(dtype)
            dbm = 10 * np.log10(ps * np.sum(np.mean(np.abs(x.astype(np.complex128)) ** 2, axis=-1)) / 1e-3)      # the same pscale, said as a power
        want = fr.ssfm(x, FS, D, SPAN, nspans, GAMMA, fr.alpha_per_m(adb), steps, ps, backward=backward, amplify=not bare)
        got = run(hip_dsp.dbp_dev if backward else hip_dsp.ssfm_dev, x, inplace=inplace, nspans=nspans, gamma=GAMMA, alpha_db_km=adb, steps=steps,
                  amplify=not bare, **(dict(pscale=ps) if by_pscale else dict(power_dbm=dbm)))
        assert got.dtype == np.dtype(dtype) and got.shape == x.shape
        check(got, want, bar(dtype, L, steps, nspans),
              "%s %dx%d %s steps=%s spans=%d alpha=%g amplify=%d inplace=%d %s" % ("dbp" if backward else "ssfm", rows, L, np.dtype(dtype).name,
                                                                                  "list" if lst else "8", nspans, adb, not bare, inplace,
                                                                                  "pscale" if by_pscale else "power_dbm"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,L", SHAPES)
def test_power_dbm_and_pscale_agree(rows, L, dtype):
    x = field(rows, L, dtype)
    for backward in (False, True):
        f = hip_dsp.dbp_dev if backward else hip_dsp.ssfm_dev
        a = run(f, x, nspans=3, gamma=GAMMA, steps=LIST, power_dbm=DBM)
        b = run(f, x, nspans=3, gamma=GAMMA, steps=LIST, pscale=fr.pscale_of(x, DBM))
        check(a, b, bar(dtype, L, LIST, 3, scale=2.0), "power_dbm against pscale, backward=%d %dx%d %s" % (backward, rows, L, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,L", SHAPES)
def test_round_trip(rows, L, dtype):
    x = field(rows, L, dtype)
    for steps, nspans, adb in ((8, 3, 0.2), (LIST, 1, 0.2), (LIST, 3, 0.0)):
        k = dict(nspans=nspans, gamma=GAMMA, alpha_db_km=adb, steps=steps, power_dbm=DBM)
        E = DeviceArray.from_host(np.ascontiguousarray(x))
        mid = DeviceArray(x.shape, x.dtype)
        hip_dsp.ssfm_dev(E, mid, FS, D, SPAN, **k)
        moved = fr.rel_max(mid.to_host(), x)
        hip_dsp.dbp_dev(mid, mid, FS, D, SPAN, **k)
        assert moved > 0.1, moved                                            # the link is not the identity
        check(mid.to_host(), x, bar(dtype, L, steps, nspans, scale=2.0),
              "round trip %dx%d %s steps=%s spans=%d alpha=%g (the link moved the field by %.2g)" % (rows, L, np.dtype(dtype).name,
                                                                                                      "list" if steps is LIST else "8", nspans, adb, moved))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 2])
def test_gamma_zero_is_add_dispersion(rows, dtype):
    L, nspans = 4096, 3
    x = field(rows, L, dtype)
    got = run(hip_dsp.ssfm_dev, x, nspans=nspans, gamma=0.0, steps=8, power_dbm=DBM)
    want = cimp.add_dispersion(np.array(x), FS, D, nspans * SPAN)
    check(got, want, (hip_dsp.fibre_plan(L, 8, nspans)["filters"] + 1) * BAR[np.dtype(dtype)], "gamma = 0 against add_dispersion %dx%d %s" % (rows, L, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,L", SHAPES)
def test_no_dispersion_one_step_is_the_closed_form(rows, L, dtype):
    x = field(rows, L, dtype)
    ps, alpha = fr.pscale_of(x, DBM), fr.alpha_per_m(0.2)
    E = DeviceArray.from_host(np.ascontiguousarray(x))
    out = DeviceArray(x.shape, x.dtype)
    hip_dsp.ssfm_dev(E, out, FS, 0.0, SPAN, gamma=GAMMA, steps=1, pscale=ps)
    got = out.to_host()
    x128 = x.astype(np.complex128)
    heff = (1 - np.exp(-alpha * SPAN)) / alpha
    want = x128 * np.exp(1j * (8 / 9 if rows == 2 else 1.0) * GAMMA * ps * heff * np.sum(np.abs(x128) ** 2, axis=0))
    check(got, want, BAR[np.dtype(dtype)] + 4 * eps(dtype), "D = 0, one step, against the closed form %dx%d %s" % (rows, L, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_call_is_bit_identical(dtype):
    for rows, L in ((2, 1000), (2, 16384)):
        x = field(rows, L, dtype)
        k = dict(nspans=2, gamma=GAMMA, steps=LIST, power_dbm=DBM, nf_db=5.0, seed=11)
        a, b = run(hip_dsp.ssfm_dev, x, **k), run(hip_dsp.ssfm_dev, x, inplace=True, **k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        k = dict(nspans=2, gamma=GAMMA, steps=LIST, power_dbm=DBM)
        a, b = run(hip_dsp.dbp_dev, x, **k), run(hip_dsp.dbp_dev, x, **k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def one(v):
    return DeviceArray.from_host(np.array([v], dtype=np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("L", [1, 2, 1001, 2048, 2050, 5001])
def test_nonlinear_step_alone(L, rows, dtype):
    """the launch at lengths around its tile (2048 samples in complex64, 1024 in complex128), odd ones (complex64 then moves 8 bytes per lane:
    the second row does not start on 16), in place.  The field is scaled so that the largest phase is pi.  Bar, relative to the largest sample:
    the power is a sum of up to four products (1.5 eps), the coefficient and its product with the power are rounded once each (1 eps), so the
    phase is off by 2.5 eps pi at most; the rotator 4 eps; a times the rotator and the complex product 1.5 eps: 13.4 eps, taken as 14."""
    rng = np.random.default_rng(L + rows)
    x = rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))
    a, coef, ps = 0.75, 0.4, 1.7
    x = (x * np.sqrt(np.pi / (coef * ps * np.sum(np.abs(x) ** 2, axis=0).max()))).astype(dtype)
    E = DeviceArray.from_host(x)
    got = hip_dsp.fibre_nl_dev(E, E, a, coef, one(ps)).to_host()
    x128 = x.astype(np.complex128)
    want = a * np.exp(1j * coef * ps * np.sum(np.abs(x128) ** 2, axis=0)) * x128
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print("nonlinear step %dx%d %s: %.2f eps of the largest sample (bar 14)" % (rows, L, np.dtype(dtype).name, e / eps(dtype)))
    assert e <= 14 * eps(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rotator_is_good_to_four_ulp(dtype):
    """one real row x: the power fl(x^2) and the phase fl(1 * P) are exact roundings, so the output is x times the rotator of a phase the test
    knows exactly; phases over [-pi, pi] (a negative coefficient gives the lower half)"""
    rt = np.float32 if dtype == np.complex64 else np.float64
    P = np.linspace(0, np.pi, 40001).astype(rt)
    x = np.sqrt(P.astype(np.float64)).astype(rt)
    P = (x * x).astype(rt)                                                   # what the kernel forms
    for sign in (1.0, -1.0):
        E = DeviceArray.from_host(np.ascontiguousarray(x.astype(dtype).reshape(1, -1)))
        got = hip_dsp.fibre_nl_dev(E, E, 1.0, sign, one(1.0)).to_host()[0].astype(np.complex128)
        nz = x > 0
        r = got[nz] / (x[nz].astype(np.float64) * np.exp(1j * sign * P[nz].astype(np.float64)))
        mod, ph = float(np.abs(np.abs(r) - 1).max()), float(np.abs(np.angle(r)).max())
        print("rotator %s sign %+d: modulus off by %.2f eps, phase by %.2f eps (bar 4)" % (np.dtype(dtype).name, sign, mod / eps(dtype), ph / eps(dtype)))
        assert mod <= 4 * eps(dtype) and ph <= 4 * eps(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_row_length(dtype):
    """1001 samples: Bluestein in the filters, and in complex64 the 8-byte form of the nonlinear step"""
    x = field(2, 1001, dtype)
    ps = fr.pscale_of(x, DBM)
    want = fr.ssfm(x, FS, D, SPAN, 2, GAMMA, fr.alpha_per_m(0.2), LIST, ps)
    got = run(hip_dsp.ssfm_dev, x, nspans=2, gamma=GAMMA, steps=LIST, power_dbm=DBM)
    check(got, want, bar(dtype, 1001, LIST, 2), "ssfm 2x1001 %s" % np.dtype(dtype).name)
    check(run(hip_dsp.dbp_dev, got, inplace=True, nspans=2, gamma=GAMMA, steps=LIST, power_dbm=DBM), x, bar(dtype, 1001, LIST, 2, scale=2.0),
          "round trip 2x1001 %s" % np.dtype(dtype).name)


def test_c_entry_refuses_before_any_launch():
    """QH_ERR_ARG (ValueError) from the library itself, past the Python checks, and nothing written: the output keeps its fill"""
    import ctypes as C
    x = field(2, 1000, np.complex64)
    E = DeviceArray.from_host(np.ascontiguousarray(x))
    out = DeviceArray.from_host(np.full(x.shape, 7 + 7j, np.complex64))
    good = dict(nmodes=2, L=1000, fs=FS, beta2=fr.beta2(D), gamma=GAMMA, alpha=fr.alpha_per_m(0.2), dz=[40e3, 40e3], nspans=1, backward=0, amplify=1,
                power_mode=1, power=2e-3, ase_w=0.0, seed=0)

    def call(**kw):
        a = dict(good, **kw)
        dz = (C.c_double * len(a["dz"]))(*a["dz"])
        _lib.call("qh_fibre_ssfm_c64_dev", E.ptr, a["nmodes"], a["L"], a["fs"], a["beta2"], a["gamma"], a["alpha"], dz, a.get("nsteps", len(a["dz"])), a["nspans"],
                  a["backward"], a["amplify"], a["power_mode"], a["power"], a["ase_w"], a["seed"], out.ptr)

    for bad in (dict(nmodes=3), dict(nmodes=0), dict(L=1), dict(L=2 ** 24 - 1), dict(nsteps=0), dict(nspans=0), dict(nspans=4097), dict(dz=[40e3, 0.0]),
                dict(dz=[40e3, -1.0]), dict(dz=[np.inf, 1.0]), dict(dz=[np.nan, 1.0]), dict(fs=0.0), dict(fs=np.nan), dict(beta2=np.inf), dict(gamma=np.nan),
                dict(alpha=np.inf), dict(ase_w=1e-7, backward=1), dict(ase_w=-1e-7), dict(ase_w=np.nan), dict(power=0.0), dict(power=-1.0),
                dict(power=np.nan), dict(power_mode=2)):
        with pytest.raises(ValueError):
            call(**bad)
    _lib.sync()
    assert np.all(out.to_host() == 7 + 7j)
    call()                                                                  # and the arguments they were varied from are accepted
    assert fr.rel_max(out.to_host(), x) > 0.1


def unit_draws(rows, L, dtype, seed, nspans):
    """w of span s: what impair_pointwise_dev adds to a zero field with sigma = 1 under the seed ``seed + s``"""
    w = np.empty((nspans, rows, L), dtype)
    for s in range(nspans):
        Z = DeviceArray((rows, L), dtype, zero=True)
        hip_dsp.impair_pointwise_dev(Z, Z, sigma=1.0, seed=(seed + s) % 2 ** 64)
        w[s] = Z.to_host()
    return w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,L,seed", [(2, 1000, 5), (1, 4096, 2 ** 64 - 1), (2, 16384, 2 ** 40 + 3)])
def test_amplifier_noise_is_the_restatements(rows, L, seed, dtype):
    x = field(rows, L, dtype)
    nspans, ps, alpha = 2, fr.pscale_of(x, DBM), fr.alpha_per_m(0.2)
    w = unit_draws(rows, L, dtype, seed, nspans)
    assert 0.9 < np.mean(np.abs(w) ** 2) < 1.1 and not np.array_equal(w[0], w[1])
    sigma = np.sqrt(hip_dsp.ase_power(5.0, alpha, SPAN, FS) / ps)
    want = fr.ssfm(x, FS, D, SPAN, nspans, GAMMA, alpha, 8, ps, sigma=sigma, w=w.astype(np.complex128))
    clean = fr.ssfm(x, FS, D, SPAN, nspans, GAMMA, alpha, 8, ps)
    assert fr.rel_max(want, clean) > 100 * bar(dtype, L, 8, nspans)         # the noise is far above the bar: the test sees it
    got = run(hip_dsp.ssfm_dev, x, nspans=nspans, gamma=GAMMA, steps=8, power_dbm=DBM, nf_db=5.0, seed=seed)
    check(got, want, bar(dtype, L, 8, nspans), "noise %dx%d %s seed=%d" % (rows, L, np.dtype(dtype).name, seed))


@pytest.mark.parametrize("dtype", DTYPES)
def test_amplifier_noise_power(dtype):
    """gamma = 0 and D = 0: the link is the identity plus the noise of its two amplifiers, 2 sigma^2 per mode.  65536 x 2 complex samples: the
    standard error of the mean power is sigma^2 sqrt(2) / sqrt(131072) = 0.4 % of sigma^2, 0.2 % of the total - 2 % is ten of them wide, and draws
    used twice would give 4 sigma^2."""
    rows, L = 2, 65536
    x = field(rows, L, dtype)
    ps = fr.pscale_of(x, DBM)
    E = DeviceArray.from_host(np.ascontiguousarray(x))
    out = DeviceArray(x.shape, x.dtype)
    hip_dsp.ssfm_dev(E, out, FS, 0.0, SPAN, nspans=2, gamma=0.0, steps=2, pscale=ps, nf_db=5.0, seed=77)
    added = float(np.mean(np.abs(out.to_host().astype(np.complex128) - x) ** 2))
    want = 2 * hip_dsp.ase_power(5.0, fr.alpha_per_m(0.2), SPAN, FS) / ps
    print("added noise power %s: %.6g, 2 sigma^2 = %.6g, ratio %.4f" % (np.dtype(dtype).name, added, want, added / want))
    assert abs(added / want - 1) <= 0.02


def test_host_layer_keeps_shape_and_dtype():
    x = field(2, 1000, np.complex64)
    k = dict(nspans=2, gamma=GAMMA, steps=8, power_dbm=DBM)
    want = run(hip_dsp.ssfm_dev, x, **k)
    got = cfibre.ssfm(np.array(x), FS, D, SPAN, **k)
    assert got.dtype == np.complex64 and np.array_equal(got, want)
    one = cfibre.ssfm(np.array(x[0]), FS, D, SPAN, **k)
    assert one.shape == (1000,) and one.dtype == np.complex64
    back = cfibre.dbp(one, FS, D, SPAN, **k)
    check(back, x[0], bar(np.complex64, 1000, 8, 2, scale=2.0), "core.fibre round trip on a 1-d row")
    assert cfibre.ssfm(np.array(x[0]).astype(np.complex128).real, FS, D, SPAN, **k).dtype == np.complex128
    np.random.seed(3)
    a = cfibre.ssfm(np.array(x), FS, D, SPAN, nf_db=5.0, **k)
    np.random.seed(3)
    b = cfibre.ssfm(np.array(x), FS, D, SPAN, nf_db=5.0, **k)
    assert np.array_equal(a, b) and not np.array_equal(a, got)


def test_resident_receiver_backpropagates():
    """16-QAM, two modes, 2^15 samples through two spans at 6 dBm: back-propagation in the receiver returns the launched field, dispersion
    compensation alone does not come near it"""
    from qampy_amd.pipeline import ResidentReceiver
    M, L, nspans, dbm = 16, 2 ** 15, 2, 6.0
    sig = synth.make_capture(M, L // 2, nmodes=2, seed=5, dtype=np.complex64)
    x = np.ascontiguousarray(np.asarray(sig), dtype=np.complex64)
    assert x.shape == (2, L)
    link = dict(nspans=nspans, gamma=GAMMA, alpha_db_km=0.2, steps=8, power_dbm=dbm)
    y = run(hip_dsp.ssfm_dev, x, **link)
    b = bar(np.complex64, L, 8, nspans, scale=2.0)
    rx = ResidentReceiver(2, L, 2, M, 21, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(2, 1), Mtestangles=32, Nbps=20, alphabet=sig.coded_symbols)
    rx.load(y)
    rx.backpropagate(FS, D, SPAN, nspans, GAMMA, 0.2, 8, dbm)
    check(rx.E.to_host(), x, b, "ResidentReceiver.backpropagate against the launched field")
    rx.load(y)
    rx.compensate_cd(FS, D, nspans * SPAN)
    e = fr.rel_max(rx.E.to_host(), x)
    print("compensate_cd alone: %.3g (%.0f bars)" % (e, e / (b / 2)))
    assert e > 100 * (b / 2)
    rx.run()                                                                # the receiver still runs behind the new stage
    _lib.sync()
