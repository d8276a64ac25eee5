"""CPU checks of the theory layer: the closed-form curves against the reference's values (tests/golden/theory.npz; both sides perform the same
scipy operations, rtol 1e-12), the hybrid formula's limits, the shaping probabilities, the place of the new entry points in the C ABI (additive:
the version stays 11) and the argument checks, which fire before the library is touched."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from qampy_amd import _lib, helpers, synth, theory
from qampy_amd.core import hip_dsp, special_fcts

G = np.load(os.path.join(GOLDEN, "theory.npz"))
NEW = ["qh_awgn_mc_noise_c64_dev", "qh_awgn_mc_noise_c128_dev", "qh_awgn_mc_c64_dev", "qh_awgn_mc_c128_dev", "qh_ps_symbols_c64_dev",
       "qh_ps_symbols_c128_dev"]
RTOL = 1e-12
c64, c128 = np.complex64, np.complex128


class _Stub:
    """A stand-in with a DeviceArray's attributes: the checks must fire before any library call."""
    def __init__(self, shape, dtype, ptr=1):
        self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), ptr


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "DeviceArray", refuse)


# ------------------------------------------------------------------------------------------------ closed forms
def test_closed_form_curves_against_the_reference():
    snr, evm = G["snr_lin"], G["evm_db"]
    np.testing.assert_allclose(helpers.dB2lin(G["snr_db"]), snr, rtol=RTOL)
    np.testing.assert_allclose(helpers.dB2lin(evm), G["db2lin"], rtol=RTOL)
    np.testing.assert_allclose(helpers.lin2dB(snr), G["lin2db"], rtol=RTOL, atol=1e-13)
    np.testing.assert_allclose(special_fcts.q_function(G["q_x"]), G["q_function"], rtol=RTOL)
    for M in (4, 16, 64, 256):
        np.testing.assert_allclose(theory.ser_vs_es_over_n0_qam(snr, M), G["ser_qam_%d" % M], rtol=RTOL)
        np.testing.assert_allclose(theory.ber_vs_es_over_n0_qam(snr, M), G["ber_qam_%d" % M], rtol=RTOL)
        np.testing.assert_allclose(theory.ber_vs_evm_qam(evm, M), G["ber_evm_%d" % M], rtol=RTOL)
    for M in (4, 8):
        np.testing.assert_allclose(theory.ser_vs_es_over_n0_psk(snr, M), G["ser_psk_%d" % M], rtol=RTOL)
    np.testing.assert_allclose(theory.ser_vs_es_over_n0_4pam(snr), G["ser_4pam"], rtol=RTOL)


def test_helpers():
    x = np.array([1 + 2j, -3j, 0.5])
    assert np.array_equal(helpers.cabssquared(x), x.real ** 2 + x.imag ** 2)
    assert helpers.normalise_and_center is synth.normalise_and_center
    np.testing.assert_allclose(helpers.lin2dB(helpers.dB2lin(np.array([-3., 0., 17.]))), [-3., 0., 17.], atol=1e-13)


def test_symbol_tables():
    for M in (2, 4, 8, 16):
        np.testing.assert_allclose(theory.cal_symbols_psk(M), G["psk_%d" % M], rtol=RTOL, atol=1e-15)
    for M in (4, 16, 64, 256):
        assert np.array_equal(theory.cal_symbols_square_qam(M), theory.cal_symbols_qam(M))
    for M in (8, 32, 128):
        assert np.array_equal(theory.cal_symbols_cross_qam(M), theory.cal_symbols_qam(M))


def test_hybrid_formula_limits():
    snr_db = np.array([3., 9.5, 14., 21.])
    lin = 10 ** (snr_db / 10)
    for M1, M2 in ((4, 16), (16, 64)):
        np.testing.assert_allclose(theory.hybrid_qam_ber_vs_esn0(snr_db, 0.7, 0, M1, M2), theory.ber_vs_es_over_n0_qam(lin, M1), rtol=1e-14)
    for fr in (0.0, 0.25, 1.0):
        np.testing.assert_allclose(theory.hybrid_qam_ber_vs_esn0(snr_db, 1, fr, 16, 16), theory.ber_vs_es_over_n0_qam(lin, 16), rtol=1e-14)
    assert np.ndim(theory.hybrid_qam_ber_vs_esn0(12., 0.5, 0.5, 4, 16)) == 0


def test_shaping_probabilities_against_the_reference():
    for M in (16, 64):
        for j, nu in enumerate(G["ps_nu"]):
            lev, px = theory.cal_ps_probablts(theory.coded_symbols_qam(M), nu)
            np.testing.assert_allclose(lev, G["ps_%d_%d_levels" % (M, j)], rtol=RTOL)
            np.testing.assert_allclose(px, G["ps_%d_%d_px" % (M, j)], rtol=RTOL)
            assert abs(px.sum() - 1) < 1e-15


def test_generate_ps_symbols_numpy_path():
    lev, px = theory.cal_ps_probablts(theory.coded_symbols_qam(16), 1.0)
    a = theory.generate_ps_symbols(4096, lev, px, normalize=False, seed=7)
    b = theory.generate_ps_symbols(4096, lev, px, normalize=False, seed=7)
    rng = np.random.default_rng(7)
    want = rng.choice(lev, 4096, p=px) + 1j * rng.choice(lev, 4096, p=px)
    assert a.shape == (4096,) and np.array_equal(a, b) and np.array_equal(a, want)
    n = theory.generate_ps_symbols((2, 4096), lev, px, seed=7)               # the reference raises NameError here
    assert n.shape == (2, 4096)
    np.testing.assert_allclose(n.mean(axis=-1), 0, atol=1e-15)
    np.testing.assert_allclose(np.mean(np.abs(n) ** 2, axis=-1), 1, rtol=1e-14)
    with pytest.raises(ValueError):
        theory.generate_ps_symbols(16, lev, px, method="cuda")
    with pytest.raises(ValueError):
        theory.generate_ps_symbols(16, lev, px[:-1])
    with pytest.raises(ValueError):
        theory.generate_ps_symbols(0, lev, px)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", plain))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
        params = re.search(r"\bint %s\((.*?)\);" % n, plain, flags=re.S).group(1).split(",")
        assert len(_lib.SIGNATURES[n]) == len(params), n
    for stem in ("qh_awgn_mc_noise", "qh_awgn_mc", "qh_ps_symbols"):
        assert _lib.SIGNATURES[stem + "_c64_dev"] == _lib.SIGNATURES[stem + "_c128_dev"]
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    src = open(os.path.join(ROOT, "qampy_amd", "csrc", "philox.h")).read()
    assert re.search(r"IMP_STREAM_MC = 3u", src) and re.search(r"IMP_STREAM_SHAPE = 4u", src)


def test_library_refuses_bad_sizes_without_a_device():
    """The size checks of the C entry points come before the device is initialised: QH_ERR_ARG on a box with or without a GPU."""
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    cdf, short, falling = np.array([0.5, 1.0]), np.array([0.5, 0.9]), np.array([0.7, 0.5, 1.0])
    bad = [lib.qh_awgn_mc_noise_c64_dev(p, p, 0, 4, 1), lib.qh_awgn_mc_noise_c128_dev(p, p, 1, 0, 1), lib.qh_awgn_mc_noise_c64_dev(None, p, 1, 4, 1),
           lib.qh_awgn_mc_c64_dev(p, 12, p, 1, p, 4, p), lib.qh_awgn_mc_c128_dev(p, 2048, p, 1, p, 4, p), lib.qh_awgn_mc_c64_dev(p, 16, p, 70000, p, 4, p),
           lib.qh_awgn_mc_c64_dev(p, 16, p, 1, p, 4, None),
           lib.qh_ps_symbols_c64_dev(p, 1, 4, p, p, 65, 1, None, None), lib.qh_ps_symbols_c128_dev(p, 0, 4, p, cdf.ctypes.data, 2, 1, None, None),
           lib.qh_ps_symbols_c64_dev(p, 1, 4, p, cdf.ctypes.data, 2, 1, p, None),
           lib.qh_ps_symbols_c64_dev(p, 1, 4, p, short.ctypes.data, 2, 1, None, None),
           lib.qh_ps_symbols_c64_dev(p, 1, 4, p, falling.ctypes.data, 3, 1, None, None),
           lib.qh_ps_symbols_c64_dev(p, 1, 2 ** 31 + 1, p, cdf.ctypes.data, 2, 1, None, None)]
    assert bad == [_lib.QH_ERR_ARG] * len(bad)
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ argument checks
def test_monte_carlo_arguments_are_checked_before_the_library(no_library):
    al16, bm = theory.coded_symbols_qam(16), G["bitmap_16"]
    for kw, exc in ((dict(symbols=al16.real.copy()), TypeError), (dict(symbols=al16[:8]), ValueError), (dict(snr=-1.0), ValueError),
                    (dict(snr=np.nan), ValueError), (dict(snr=[1.0, 2.0]), ValueError), (dict(ns=0), ValueError), (dict(ns=2.5), ValueError),
                    (dict(noise=np.zeros(3, c128)), ValueError), (dict(bit_map=bm[:, :4]), ValueError), (dict(seed=1.5), ValueError)):
        args = dict(symbols=al16, snr=10.0, ns=8, bit_map=bm)
        args.update(kw)
        with pytest.raises(exc):
            hip_dsp.cal_gmi_mc(**args)
    with pytest.raises(ValueError):
        hip_dsp.awgn_mc(np.ones(12, c128), 10.0, 8)
    with pytest.raises(ValueError):
        hip_dsp.awgn_mc(np.ones(2048, c64), 10.0, 8)
    with pytest.raises(ValueError):
        hip_dsp.awgn_mc(al16, [10.0, 0.0], 8)
    A, S, out = _Stub((16,), c64), _Stub((2,), np.float64), _Stub((2, 6), np.float64)
    for a, s, z, o, exc in ((A, S, _Stub((2, 8), c128), out, TypeError), (A, S, _Stub((3, 8), c64), out, ValueError), (A, S, _Stub((2, 8), c64), _Stub((2, 5), np.float64), ValueError),
                            (_Stub((12,), c64), S, _Stub((2, 8), c64), out, ValueError), (A, _Stub((2,), np.float32), _Stub((2, 8), c64), out, TypeError),
                            (A, [1.0, -2.0], _Stub((2, 8), c64), out, ValueError), (_Stub((16,), np.float32), S, _Stub((2, 8), c64), out, TypeError)):
        with pytest.raises(exc):
            hip_dsp.awgn_mc_dev(a, s, z, o)
    for z, s, seed, exc in ((_Stub((2, 8), np.float64), S, 1, TypeError), (_Stub((8,), c64), S, 1, ValueError), (_Stub((2, 8), c64), S, 0.5, ValueError),
                            (_Stub((2, 8), c64), [1.0, np.inf], 1, ValueError)):
        with pytest.raises(exc):
            hip_dsp.awgn_mc_noise_dev(z, s, seed)
    with pytest.raises(ValueError):
        theory.cal_gmi(16, [10.0, np.nan], N=8)
    with pytest.raises(ValueError):
        theory.cal_gmi(16, 10.0, N=0)
    with pytest.raises(TypeError):
        theory.sim_mi_mc(np.ones((2, 4), np.complex128), 10.0, 8)


def test_shaped_source_arguments_are_checked_before_the_library(no_library):
    lev, px = np.array([-1., 1.]), np.array([0.5, 0.5])
    out = _Stub((2, 100), c64)
    for o, l, p, kw, exc in ((_Stub((2, 100), np.float32), lev, px, {}, TypeError), (_Stub((2, 0), c64), lev, px, {}, ValueError), (_Stub((2 ** 31 + 1,), c64), lev, px, {}, ValueError),
                             (out, lev, [0.5, -0.5], {}, ValueError),
                             (out, lev, [0., 0.], {}, ValueError), (out, lev[:1], px, {}, ValueError), (out, np.arange(65.), np.ones(65), {}, ValueError),
                             (out, [np.nan, 1.], px, {}, ValueError), (out, lev, px, dict(labels=_Stub((2, 100), np.int32)), ValueError),
                             (out, lev, px, dict(labels=_Stub((2, 100), np.int64), label_table=np.zeros((2, 2), np.int32)), ValueError),
                             (out, lev, px, dict(labels=_Stub((2, 100), np.int32), label_table=np.zeros((3, 3), np.int32)), ValueError)):
        with pytest.raises(exc):
            hip_dsp.ps_symbols_dev(o, l, p, 1, **kw)
    with pytest.raises(ValueError):
        hip_dsp.ps_symbols_dev(out, lev, px, 1.5)
    for kw in (dict(M=32), dict(M=2), dict(nsym=0), dict(nmodes=0), dict(nu=np.inf)):
        args = dict(M=16, nu=0.1, nsym=8)
        args.update(kw)
        with pytest.raises(ValueError):
            synth.make_ps_symbols_dev(**args)
    with pytest.raises(ValueError):
        theory.generate_ps_symbols(16, lev, [0.5, -0.5], method="hip")


def test_sim_mi_mc_leaves_its_argument_untouched(monkeypatch):
    """The reference divides the caller's alphabet in place; here a copy is normalised and the copy is what reaches the kernel."""
    seen = {}

    def fake(alphabet, snr, ns, noise=None, seed=None, return_noise=False):
        seen.update(alphabet=np.array(alphabet), snr=np.array(snr), ns=ns, seed=seed)
        return np.tile(np.arange(2.0 + 4), (np.size(snr), 1))
    monkeypatch.setattr(hip_dsp, "awgn_mc", fake)
    al = 3 * theory.coded_symbols_qam(16)
    keep = al.copy()
    mi = theory.sim_mi_mc(al, 10.0, 32, seed=9)
    assert np.array_equal(al, keep) and isinstance(mi, float) and mi == 1.0
    np.testing.assert_allclose(np.mean(np.abs(seen["alphabet"]) ** 2), 1, rtol=1e-14)
    np.testing.assert_allclose(seen["snr"], [10.0])
    assert seen["ns"] == 32 and seen["seed"] == 9
    pam = np.array([-3., -1., 1., 3.])                       # a real alphabet, as the reference takes it
    assert theory.sim_mi_mc(pam, 10.0, 32, seed=9) == 1.0 and seen["alphabet"].dtype == c128 and pam[0] == -3.
    np.testing.assert_allclose(seen["alphabet"], pam / np.sqrt(5), rtol=1e-15)
    mi = theory.sim_mi_mc(al, [10.0, 20.0], 32, seed=9)
    assert np.array_equal(al, keep) and mi.shape == (2,)
    np.testing.assert_allclose(seen["snr"], [10.0, 100.0])


def test_cal_gmi_shapes(monkeypatch):
    def fake(alphabet, snr, ns, noise=None, seed=None, return_noise=False):
        assert np.array_equal(alphabet, theory.coded_symbols_qam(16, dtype=c64)) and alphabet.dtype == c64 and ns == 64 and seed == 5
        return np.arange(np.size(snr) * 6.0).reshape(np.size(snr), 6)
    monkeypatch.setattr(hip_dsp, "awgn_mc", fake)
    g = theory.cal_gmi(16, 8.0, N=64, seed=5, dtype=c64)
    assert g.shape == (1,) and g[0] == 0
    g, pb = theory.cal_gmi(16, [8.0, 12.0], N=64, seed=5, dtype=c64, per_bit=True)
    assert np.array_equal(g, [0, 6]) and pb.shape == (2, 4) and np.array_equal(pb[1], [8, 9, 10, 11])


def test_fresh_seeds_differ():
    a, b = hip_dsp.fresh_seed(), hip_dsp.fresh_seed()
    assert a != b and 0 <= a < 2 ** 64
