"""Transmitter response on the GPU (csrc/txresp.hip) against the reference's outputs (tests/golden/txresp.npz), scipy.signal.sosfilt and
the float64 restatement (tests/txresp_ref.py).

Inputs lie on a dyadic grid, so complex64 and complex128 hold the same values.  The bar is the project's: max-abs error over the signal
rms, 1e-5 (complex64) and 1e-11 (complex128).  The signal is the expected output, except for the sections filter, where it is the input
(unit rms): a narrow low-pass leaves little of it, and the filter's error - roundings of the state - scales with what goes in."""
import os

import numpy as np
import pytest
import scipy.signal as scisig

import impair_ref as ir
import txresp_ref as tr
import qampy_amd
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import filter as cfilter
from qampy_amd.core import hip_dsp
from qampy_amd.core import impairments as cimp
from qampy_amd.core import resample as crs
from qampy_amd.pipeline import ResidentReceiver

pytestmark = pytest.mark.gpu

DT = [np.complex64, np.complex128]
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txresp.npz")
FS = 40e9
C, T = hip_dsp.SOS_CHUNK, hip_dsp.SOS_TILE
IIR_LS = [1, 2, C - 1, C, C + 1, T - 1, T, T + 1, 3 * T + 5, 70 * T + 3]
FILTERS = {"bessel2": (18e9, "bessel", 2), "bessel4": (50e6, "bessel", 4), "butter6": (100e6, "butter", 6)}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def x_of(g, L):
    q = g["x_%d" % L]
    return (q[..., 0] + 1j * q[..., 1]) / g["scale"]


def kept(g, a, L):
    return a if L == 2048 else a[:, g["cols"]]


def relerr(a, b, rms=None):
    b = np.asarray(b, np.complex128)
    rms = np.sqrt(np.mean(np.abs(b) ** 2)) if rms is None else rms
    return np.abs(np.asarray(a, np.complex128) - b).max() / rms


def mod_prms(g):
    return dict(dcbias=complex(g["mod_dcbias"]), gfactr=complex(g["mod_gfactr"]), cfactr=complex(g["mod_cfactr"]), dcbias_out=float(g["mod_dcbias_out"]),
                gfactr_out=float(g["mod_gfactr_out"]))


def dev(fn, x, dtype, inplace=False):
    E = DeviceArray.from_host(np.ascontiguousarray(np.asarray(x).astype(dtype)))
    out = E if inplace else DeviceArray(E.shape, dtype)
    fn(E, out)
    _lib.sync()
    return out.to_host()


# ------------------------------------------------------------------------------------------------ extrema
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("L", [1, 63, 64, 65, T + 1])
def test_row_extrema_equal_numpys(L, dtype):
    """the maximum at the first, the last and an interior position, of either sign, in re or in im"""
    rng = np.random.default_rng(L)
    x = (rng.uniform(-1, 1, (4, L)) + 1j * rng.uniform(-1, 1, (4, L))).astype(dtype)
    x[0, 0] = 3 - 0.5j
    x[1, L - 1] = 0.25 - 3j
    x[2, L // 2] = -3.5 + 3.25j
    x[3, L // 3] = -0.5 + 2.5j
    x[3, (2 * L) // 3] += -2.75
    ext = hip_dsp.row_extrema_dev(DeviceArray.from_host(x))
    _lib.sync()
    got = ext.to_host()
    assert got.dtype == np.float64 and got.shape == (4, 2)
    assert np.array_equal(got, tr.row_extrema(x))
    again = hip_dsp.row_extrema_dev(DeviceArray.from_host(x), ext=DeviceArray((4, 2), np.float64)).to_host()
    assert again.tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ clip and quantiser
def level_index(y, nbits, swing):
    """level indices (re, im) of a quantiser's output scaled by ``swing``"""
    d = 2.0 / 2 ** nbits
    k = (np.stack([y.real, y.imag]).astype(np.float64) / swing + 1 - d / 2) / d
    assert np.abs(k - np.round(k)).max() < 1e-3
    return np.round(k).astype(np.int64)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("clip_rat", [1, 0.8])
@pytest.mark.parametrize("nbits", [1, 4, 8])
def test_quantiser_and_clip_on_the_exact_fixtures(gold, nbits, clip_rat, dtype):
    """Row maxima of exactly 2 and samples exactly on thresholds: the golden values at the bar, the level indices equal everywhere."""
    for L in (2048, 12388):
        xq = tr.exact_quant_field(x_of(gold, L))
        assert np.array_equal(xq.astype(dtype).astype(np.complex128), xq)
        want = gold[("q%d_%d" if clip_rat == 1 else "cq%d_%d") % (nbits, L)]
        qin = xq if clip_rat == 1 else tr.clip(xq, clip_rat)
        _, ir_, ii_, u = tr.quantise(qin, nbits)
        assert tr.on_threshold(u, nbits) >= 1
        got = dev(lambda E, out: hip_dsp.dac_pointwise_dev(E, out, clip_rat=clip_rat, quant_bits=nbits), xq, dtype)
        assert got.dtype == dtype
        e = relerr(kept(gold, got, L), want)
        print("L %d: %.3e of the rms" % (L, e))
        assert e <= BAR[dtype]
        swing = 2.0 if clip_rat == 1 else 1.0
        assert np.array_equal(level_index(got, nbits, swing), np.stack([ir_, ii_]))
        if clip_rat != 1:
            c = dev(lambda E, out: hip_dsp.dac_pointwise_dev(E, out, clip_rat=clip_rat), xq, dtype)
            assert relerr(kept(gold, c, L), gold["clip_%d" % L]) <= BAR[dtype]


@pytest.mark.parametrize("dtype", DT)
def test_quantiser_on_a_general_field(dtype):
    """Two rows of 2^16 Gaussian samples, 6 bits, against the restatement on the same (cast) values.  Samples whose scaled value lies within
    1e-4 of a level of a threshold are left out - at most 0.2 % of them; every other sample matches at the bar."""
    nbits = 6
    x = (np.random.default_rng(8).standard_normal((2, 2 ** 16, 2)) @ np.array([1, 1j])).astype(dtype)
    want, _, _, u = tr.quantise(x.astype(np.complex128), nbits)
    got = dev(lambda E, out: hip_dsp.dac_pointwise_dev(E, out, quant_bits=nbits), x, dtype, inplace=True)
    near = tr.threshold_distance(u, nbits) < 1e-4
    share = near.mean()
    print("share left out %.2e" % share)
    assert share <= 2e-3
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    err = np.abs(np.stack([got.real - want.real, got.imag - want.imag]))
    assert err[~near].max() / rms <= BAR[dtype]


# ------------------------------------------------------------------------------------------------ sections filter
@pytest.fixture(scope="module")
def iir_ref():
    """Two rows of Gaussian samples on a 2^-10 grid and, per filter, scipy's result and the restatement's on the longest row: the filter is
    causal, so a shorter row's result is a prefix."""
    Lmax = max(IIR_LS)
    x = np.round(np.random.default_rng(12).standard_normal((2, Lmax, 2)) * 1024) / 1024 @ np.array([1, 1j])
    out = {"x": x}
    for name, (cutoff, ftype, order) in FILTERS.items():
        sos = tr.design(FS, cutoff, ftype, order)
        y = scisig.sosfilt(sos, x, axis=-1)
        loop = tr.sosfilt_loop(sos, x)
        assert relerr(loop, y, 1.0) <= 1e-12
        out[name] = (sos, y, loop)
    return out


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", list(FILTERS))
def test_sections_filter_is_sosfilt(iir_ref, name, dtype, inplace):
    sos, y, loop = iir_ref[name]
    x = iir_ref["x"]
    rms = np.sqrt(np.mean(np.abs(x) ** 2))
    if name != "bessel2":
        r = tr.pole_radius(sos)
        assert r ** C > 1e3 * BAR[np.complex64], "the chunks must still ring at their ends: a wrong or missing carry cannot pass"
    for L in IIR_LS:
        got = dev(lambda E, out: hip_dsp.sosfilt_dev(E, out, sos), x[:, :L], dtype, inplace=inplace)
        e1, e2 = relerr(got, y[:, :L], rms), relerr(got, loop[:, :L], rms)
        print("L %d: %.3e (scipy) %.3e (restatement) of the input rms" % (L, e1, e2))
        assert e1 <= BAR[dtype] and e2 <= BAR[dtype], L


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("ftype,order,cutoff", [("bessel", 3, 2e9), ("butter", 8, 1e9), ("butter", 1, 5e9)])
def test_sections_filter_other_orders(iir_ref, ftype, order, cutoff, dtype):
    """order 3 (an odd order is padded with zeros), order 8 (four sections) and order 1, through filter_signal_dev"""
    L = 3 * T + 5
    x = iir_ref["x"][:, :L]
    y = scisig.sosfilt(tr.design(FS, cutoff, ftype, order), x, axis=-1)
    got = dev(lambda E, out: hip_dsp.filter_signal_dev(E, out, FS, cutoff, ftype, order), x, dtype)
    assert relerr(got, y, np.sqrt(np.mean(np.abs(x) ** 2))) <= BAR[dtype]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("pos", [C - 1, T - 1])
def test_an_impulse_rings_across_the_boundary(pos, dtype):
    """an impulse in the last sample of a chunk, and of a tile: the filter's impulse response on the other side"""
    sos = tr.design(FS, 100e6, "butter", 6)
    L = T + 2 * C
    x = np.zeros((2, L), np.complex128)
    x[0, pos], x[1, pos] = 1.0, -2j
    h = scisig.sosfilt(sos, np.r_[1.0, np.zeros(L - 1)])
    got = dev(lambda E, out: hip_dsp.sosfilt_dev(E, out, sos), x, dtype)
    assert np.all(got[:, :pos] == 0)
    peak = np.abs(h).max()
    assert np.abs(got[0, pos:] - h[:L - pos]).max() <= BAR[dtype] * peak
    assert np.abs(got[1, pos:] + 2j * h[:L - pos]).max() <= 2 * BAR[dtype] * peak
    assert np.abs(h[1:C]).max() > 0.1 * peak                                     # it does ring on the other side


# ------------------------------------------------------------------------------------------------ modulator
@pytest.mark.parametrize("dtype", DT)
def test_modulator_against_the_reference(gold, dtype):
    s = np.ascontiguousarray(x_of(gold, 2048)[:, :512])
    ideal = dev(lambda E, out: hip_dsp.modulator_response_dev(E, out), s, dtype)
    real = dev(lambda E, out: hip_dsp.modulator_response_dev(E, out, **mod_prms(gold)), s, dtype, inplace=True)
    amp = dev(lambda E, out: hip_dsp.modulator_response_dev(E, out, tgt_v=0.7), s, dtype)
    for got, key, rest in ((ideal, "mod_ideal", tr.modulator(s)), (real, "mod_real", tr.modulator(s, **mod_prms(gold))),
                           (amp, "mod_amp", tr.modulator(tr.amplifier(s, 0.7)))):
        print(key, relerr(got, gold[key]))
        assert relerr(got, gold[key]) <= BAR[dtype] and relerr(got, rest) <= BAR[dtype], key


def test_modulator_complex64_up_to_four_volts():
    """|volt| <= 4: the angles are reduced in double before the single-precision sine and cosine"""
    v = np.linspace(-3, 3, 4097)
    s = (v[None, :] + 1j * v[None, ::-1]).astype(np.complex64)
    got = dev(lambda E, out: hip_dsp.modulator_response_dev(E, out, dcbias=1 - 1j, cfactr=0.3), s, np.complex64)
    assert relerr(got, tr.modulator(s.astype(np.complex128), dcbias=1 - 1j, cfactr=0.3)) <= BAR[np.complex64]


# ------------------------------------------------------------------------------------------------ the chain
CHAINS = {"a": dict(enob=0, tgt_v=0.7, clip_rat=0.8, quant_bits=5), "b": dict(enob=0, tgt_v=0.5, quant_bits=4, dac_params={})}


def chain_kw(gold, which):
    kw = dict(CHAINS[which])
    if which == "b":
        kw.update(mod_prms(gold))
    return kw


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("L", [2048, 12388])
@pytest.mark.parametrize("which", ["a", "b"])
def test_the_chain_against_the_reference(gold, which, L, dtype):
    xq = tr.exact_quant_field(x_of(gold, L))
    kw = chain_kw(gold, which)
    got = dev(lambda E, out: hip_dsp.sim_tx_response_dev(E, out, FS, **kw), xq, dtype)
    rest = tr.sim_tx(xq, FS, **{k: v for k, v in kw.items() if k != "enob"})
    e1, e2 = relerr(kept(gold, got, L), gold["chain_%s_%d" % (which, L)]), relerr(got, rest)
    print("%.3e (reference) %.3e (restatement) of the rms" % (e1, e2))
    assert e1 <= BAR[dtype] and e2 <= BAR[dtype]
    same = dev(lambda E, out: hip_dsp.sim_tx_response_dev(E, out, FS, **kw), xq, dtype, inplace=True)
    assert same.tobytes() == got.tobytes()
    arr = cimp.sim_tx_response(xq.astype(dtype), FS, **kw)
    assert type(arr) is np.ndarray and arr.dtype == dtype and arr.shape == xq.shape and arr.tobytes() == got.tobytes()
    one = cimp.sim_tx_response(xq[0].astype(dtype), FS, **kw)
    assert one.shape == (L,) and one.dtype == dtype
    sig = qampy_amd.signals.SignalQAM(xq.astype(dtype), 16, fb=FS / 2, fs=FS)
    obj = qampy_amd.impairments.sim_tx_response(sig, **kw)
    assert type(obj) is type(sig) and obj.fs == FS and obj.dtype == dtype and obj.shape == xq.shape and np.asarray(obj).tobytes() == got.tobytes()


@pytest.mark.parametrize("dtype", DT)
def test_the_layers_of_the_single_stages(gold, dtype):
    """sim_DAC_response, sim_mod_response, filter_signal and quantize_signal_New on ndarrays and signal objects: the bytes of the _dev forms"""
    xq = tr.exact_quant_field(x_of(gold, 2048)).astype(dtype)
    sig = qampy_amd.signals.SignalQAM(xq, 16, fb=FS / 2, fs=FS)
    dac = dev(lambda E, out: hip_dsp.sim_dac_response_dev(E, out, FS, enob=0, clip_rat=0.8, quant_bits=4, cutoff=18e9), xq, dtype)
    a = cimp.sim_DAC_response(xq, FS, enob=0, clip_rat=0.8, quant_bits=4, cutoff=18e9)
    b = qampy_amd.impairments.sim_DAC_response(sig, enob=0, clip_rat=0.8, quant_bits=4, cutoff=18e9)
    assert a.tobytes() == dac.tobytes() == np.asarray(b).tobytes() and type(b) is type(sig) and a.dtype == dtype
    want = tr.sosfilt_loop(tr.design(FS, 18e9), tr.dac_pointwise(xq.astype(np.complex128), 0.8, 4))
    assert relerr(dac, want) <= BAR[dtype]
    mod = dev(lambda E, out: hip_dsp.modulator_response_dev(E, out, **mod_prms(gold)), xq, dtype)
    assert cimp.modulator_response(xq, **mod_prms(gold)).tobytes() == mod.tobytes()
    m = qampy_amd.impairments.sim_mod_response(sig, **mod_prms(gold))
    assert np.asarray(m).tobytes() == mod.tobytes() and type(m) is type(sig)
    flt = dev(lambda E, out: hip_dsp.filter_signal_dev(E, out, FS, 1e9, "butter", 4), xq, dtype)
    assert cfilter.filter_signal(xq, FS, 1e9, "butter", 4).tobytes() == flt.tobytes()
    f = qampy_amd.filtering.filter_signal(sig, 1e9, "butter", 4)
    assert np.asarray(f).tobytes() == flt.tobytes() and type(f) is type(sig) and f.dtype == dtype
    assert cfilter.filter_signal(xq[1], FS, 1e9, "butter", 4).tobytes() == flt[1].tobytes()
    assert cimp.apply_DAC_filter(xq, FS).tobytes() == cfilter.filter_signal(xq, FS, 18e9).tobytes()
    q = cimp.quantize_signal_New(sig, 4)
    assert type(q) is type(sig) and relerr(np.asarray(q), gold["q4_2048"]) <= BAR[dtype]
    assert type(cimp.quantize_signal_New(xq, 4)) is np.ndarray
    shaped = qampy_amd.filtering.rrcos_pulseshaping(sig, 0.1)
    assert type(shaped) is type(sig) and shaped.shape == sig.shape
    assert np.asarray(shaped).tobytes() == cfilter.rrcos_pulseshaping(xq, FS, 2 / FS, 0.1).tobytes()


# ------------------------------------------------------------------------------------------------ ENOB noise
@pytest.mark.parametrize("dtype", DT)
def test_enob_noise(gold, dtype):
    """apply_enob_as_awgn is impair_pointwise_dev at the restatement's sigma; its power is 2 delta^2 / 12; repeatable, and a function of the seed"""
    n = 2 ** 16
    x = ir.qam_field(16, 2, n // 2, 2, 0.1, 77).astype(dtype)
    sigma = tr.enob_sigma(x.astype(np.complex128), 6)
    got = cimp.apply_enob_as_awgn(x, 6, seed=5)
    want = dev(lambda E, out: hip_dsp.impair_pointwise_dev(E, out, sigma=sigma, seed=5), x, dtype)
    assert got.dtype == dtype and relerr(got, want) <= BAR[dtype]
    delta = tr.row_max(x).max() / 2 ** 5
    p = np.mean(np.abs(got.astype(np.complex128) - x) ** 2, axis=-1)
    print("noise power over 2 delta^2 / 12:", p / (2 * delta ** 2 / 12))
    assert np.all(np.abs(p / (2 * delta ** 2 / 12) - 1) <= 5 / np.sqrt(n))
    assert cimp.apply_enob_as_awgn(x, 6, seed=5).tobytes() == got.tobytes()
    assert cimp.apply_enob_as_awgn(x, 6, seed=6).tobytes() != got.tobytes()
    out, snr = cimp.apply_enob_as_awgn(x, 6, verbose=True, seed=5)
    assert out.tobytes() == got.tobytes() and abs(snr - 10 * np.log10(np.mean(np.abs(x) ** 2) / 2 / (delta ** 2 / 12))) < 1e-4


# ------------------------------------------------------------------------------------------------ nothing to do, argument errors
@pytest.mark.parametrize("dtype", DT)
def test_nothing_to_do_returns_the_bytes(dtype):
    x = (np.random.default_rng(2).standard_normal((2, 1000, 2)) @ np.array([1, 1j])).astype(dtype)
    x[0, :4] = [0.0, -0.0, complex(0.0, -0.0), complex(-0.0, 0.0)]
    for inplace in (False, True):
        assert dev(lambda E, out: hip_dsp.dac_pointwise_dev(E, out, clip_rat=1, quant_bits=0, enob=0), x, dtype, inplace).tobytes() == x.tobytes()
        assert dev(lambda E, out: hip_dsp.sim_dac_response_dev(E, out, FS, enob=0), x, dtype, inplace).tobytes() == x.tobytes()
    assert cimp.sim_DAC_response(x, FS, enob=0, clip_rat=1, quant_bits=0).tobytes() == x.tobytes()


def test_argument_errors_leave_the_device_alone():
    E = DeviceArray.from_host(np.ones((2, 64), np.complex64))
    for kw in (dict(clip_rat=0), dict(quant_bits=2.5), dict(quant_bits=17), dict(enob=-1), dict(dcbias=np.nan), dict(dac_params={"cutoff": 21e9})):
        with pytest.raises(ValueError):
            hip_dsp.sim_tx_response_dev(E, E, FS, **kw)
    with pytest.raises(ValueError):
        hip_dsp.filter_signal_dev(E, E, FS, 18e9, order=9)
    with pytest.raises(TypeError):
        hip_dsp.sosfilt_dev(DeviceArray((2, 64), np.float32), E, tr.design(FS, 18e9))
    with pytest.raises(NotImplementedError):
        cfilter.filter_signal(np.ones(8, np.complex64), FS, 18e9, ftype="gauss")
    _lib.sync()
    assert np.array_equal(E.to_host(), np.ones((2, 64), np.complex64))


# ------------------------------------------------------------------------------------------------ the resident receiver
def test_resident_receiver_applies_the_transmitter_first():
    clean = synth.make_capture(16, 2 ** 14, nmodes=2, snr_db=None, theta=None, dgd=None, linewidth=0., seed=5, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(clean))
    fs = clean.fs
    rx = ResidentReceiver(2, E.shape[1], 2, 16, 9, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(2, 1), Mtestangles=32, Nbps=20,
                          alphabet=clean.coded_symbols)
    tx = dict(enob=5, quant_bits=6, tgt_v=0.4, seed=3)
    kw = dict(snr=20.0, lwdth=100e3, seed=11)
    src = DeviceArray.from_host(E)
    rx.load(np.zeros_like(E))
    rx.impair(fs, tx=tx, source=src, **kw)
    _lib.sync()
    got = rx.E.to_host()
    assert np.array_equal(src.to_host(), E)
    hand = DeviceArray(E.shape, E.dtype)
    hip_dsp.sim_tx_response_dev(src, hand, fs, **tx)
    crs.center_scale_dev(hand, crs.row_moments_dev(hand), power=1.0)
    rx.load(hand.to_host())
    rx.impair(fs, **kw)
    _lib.sync()
    assert rx.E.to_host().tobytes() == got.tobytes()
    assert np.allclose(np.mean(np.abs(hand.to_host()) ** 2, axis=-1), 1.0, atol=1e-4)
    rx.load(E)
    rx.impair(fs, tx=tx, **kw)                         # in place
    _lib.sync()
    assert rx.E.to_host().tobytes() == got.tobytes()
    rx.load(E)
    rx.impair(fs, tx=None, **kw)
    _lib.sync()
    a = rx.E.to_host()
    rx.load(E)
    rx.impair(fs, **kw)
    _lib.sync()
    assert rx.E.to_host().tobytes() == a.tobytes() and a.tobytes() != got.tobytes()
    with pytest.raises(ValueError):
        rx.impair(fs, tx=dict(quant_bits=2.5), **kw)
    rx.load(got)
    rx.run()
    ser = synth.cal_ser(rx.fetch()["out"], clean.symbols, clean.coded_symbols, trim=200)
    assert ser.max() < 5e-2, ser


# ------------------------------------------------------------------------------------------------ link level
LINK_SNR = 15.0


def test_ser_behind_the_transmitter_matches_the_host_restatement():
    """16-QAM, 2^15 symbols through sim_tx_response(enob=5, quant_bits=6, DAC cutoff 18 GHz, tgt_v=0.4) on the device against the same symbols
    through the restatement on the host with numpy noise of the same sigma; both renormalised, then change_snr at LINK_SNR dB,
    dual_mode_equalisation and bps.  The two symbol error rates lie within five binomial standard errors of the pooled count, which
    exceeds 100 errors.  LINK_SNR = 15 dB, chosen on an MI355X run: 2.671e-2 behind the device's transmitter, 2.571e-2 behind the host's,
    five standard errors 4.7e-3, 3015 errors pooled."""
    clean = synth.make_capture(16, 2 ** 15, nmodes=2, snr_db=None, theta=None, dgd=None, linewidth=0., seed=21, dtype=np.complex64)
    fs = clean.fs
    tx = dict(enob=5, quant_bits=6, dac_params={"cutoff": 18e9}, tgt_v=0.4)
    devsig = qampy_amd.impairments.sim_tx_response(clean, seed=4, **tx)
    x = np.asarray(clean).astype(np.complex128)
    rng = np.random.default_rng(9)
    w = (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * np.sqrt(0.5)
    host = tr.sim_tx(x, fs, tgt_v=0.4, quant_bits=6, dac_params={"cutoff": 18e9}, noise=(w, 5))
    assert devsig.dtype == np.complex64 and type(devsig) is type(clean)

    def renorm(a):
        a = np.asarray(a, np.complex128)
        a = a - a.mean(axis=-1, keepdims=True)
        return clean.recreate_from_np_array((a / np.sqrt(np.mean(np.abs(a) ** 2, axis=-1, keepdims=True))).astype(np.complex64))

    def errors(sig, seed):
        sig = qampy_amd.impairments.change_snr(sig, LINK_SNR, seed=seed)
        out, _, _ = qampy_amd.equalisation.dual_mode_equalisation(sig, (2e-3, 5e-4), 21, Niter=(2, 1), methods=("mcma", "sbd"))
        rec, _ = qampy_amd.phaserec.bps(out, 32, 20)
        trim = 2000
        ser = synth.cal_ser(np.asarray(rec), sig.symbols, sig.coded_symbols, trim=trim)
        n = 2 * (np.asarray(rec).shape[1] - 2 * trim)
        return float(np.mean(ser)), n
    p1, n1 = errors(renorm(devsig), 31)
    p2, n2 = errors(renorm(host), 32)
    pooled = (p1 * n1 + p2 * n2) / (n1 + n2)
    se = np.sqrt(pooled * (1 - pooled) * (1 / n1 + 1 / n2))
    print("SER device transmitter %.3e, host transmitter %.3e, five standard errors %.3e, pooled count %.0f" % (p1, p2, 5 * se, pooled * (n1 + n2)))
    assert pooled * (n1 + n2) > 100
    assert abs(p1 - p2) <= 5 * se
