"""CPU checks of the blind signal-quality layer: ``method="pyt"`` of core.signal_quality against the reference's values (tests/golden/blind.npz:
both sides evaluate the same numpy expressions on the same samples, rtol 1e-12), ``_cal_gamma``, the float64 restatement tests/blind_ref.py
against the complex128 fixture values within the fixture's measured tolerance, the argument checks - which fire before the library is touched -
and the place of the new entry points in the C ABI (additive: the version stays 11)."""
import os
import re

import numpy as np
import pytest

import blind_ref
from conftest import GOLDEN, ROOT
from qampy_amd import _lib, helpers, pipeline, theory
from qampy_amd.core import hip_dsp, signal_quality as sq

G = np.load(os.path.join(GOLDEN, "blind.npz"))
CASES = [(int(M), float(db)) for M, db in G["cases"]]
NO_SNR = set(int(M) for M in G["no_snr_M"])
BLOCK = int(G["block"])
NEW = ["qh_blind_moments_c64_dev", "qh_blind_moments_c128_dev", "qh_blind_finish_dev", "qh_scale_by_stat_c64_dev", "qh_scale_by_stat_c128_dev",
       "qh_blind_evm_c64_dev", "qh_blind_evm_c128_dev", "qh_qpsk_blind_c64_dev", "qh_qpsk_blind_c128_dev"]
RTOL = 1e-12
CT = {"c64": np.complex64, "c128": np.complex128}


def rows_of(c, dtype):
    """``(received, known)`` of fixture case c in ``dtype``: the same values in either precision."""
    M = CASES[c][0]
    q = G["c%d_rx" % c].astype(np.float64) / float(G["rx_scale"])
    k = np.rint(G["alphabet_%d" % M][G["c%d_idx" % c]].view(np.float64).reshape(-1, 2) * float(G["rx_scale"])) / float(G["rx_scale"])
    return (q[:, 0] + 1j * q[:, 1]).astype(dtype), (k[:, 0] + 1j * k[:, 1]).astype(dtype)


class _Stub:
    """A stand-in with a DeviceArray's attributes: the checks must fire before any library call."""
    def __init__(self, shape, dtype, ptr=1):
        self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), ptr


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


# ------------------------------------------------------------------------------------------------ the host path against the reference
@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("c", range(len(CASES)))
def test_pyt_equals_the_reference(c, dt, no_library):
    M = CASES[c][0]
    E, K = rows_of(c, CT[dt])
    pre = "c%d_%s_" % (c, dt)
    assert sq.cal_evm(E, M) == pytest.approx(float(G[pre + "evm"]), rel=RTOL)
    if M in NO_SNR:
        return
    assert sq.cal_snr_qam(E, M) == pytest.approx(float(G[pre + "snr"]), rel=RTOL)
    assert sq.cal_s0(E, M) == pytest.approx(float(G[pre + "s0"]), rel=RTOL)
    assert sq.cal_evm(E, M, known=K) == pytest.approx(float(G[pre + "evmk"]), rel=RTOL)
    np.testing.assert_allclose(sq.norm_to_s0(E, M), E / np.sqrt(G[pre + "s0"]), rtol=RTOL)
    if M == 4:
        assert sq.cal_snr_blind_qpsk(E) == pytest.approx(float(G[pre + "qpsk"]), rel=RTOL)


def test_pyt_takes_rows_and_returns_one_value_each(no_library):
    (a, ka), (b, kb) = rows_of(1, np.complex128), rows_of(0, np.complex128)
    E = np.stack([a, b])
    np.testing.assert_allclose(sq.cal_snr_qam(E, 4), [G["c1_c128_snr"], G["c0_c128_snr"]], rtol=RTOL)
    np.testing.assert_allclose(sq.cal_s0(E, 4), [G["c1_c128_s0"], G["c0_c128_s0"]], rtol=RTOL)
    np.testing.assert_allclose(sq.cal_evm(E, 4), [G["c1_c128_evm"], G["c0_c128_evm"]], rtol=RTOL)
    np.testing.assert_allclose(sq.cal_evm(E, 4, known=np.stack([ka, kb])), [G["c1_c128_evmk"], G["c0_c128_evmk"]], rtol=RTOL)
    np.testing.assert_allclose(sq.cal_snr_blind_qpsk(E), [G["c1_c128_qpsk"], G["c0_c128_qpsk"]], rtol=RTOL)
    assert sq.norm_to_s0(E, 4).shape == E.shape and np.ndim(sq.cal_snr_qam(a, 4)) == 0


@pytest.mark.parametrize("c", [int(c) for c in G["block_cases"]])
def test_pyt_per_block_values(c, no_library):
    M = CASES[c][0]
    E = rows_of(c, np.complex128)[0].reshape(-1, BLOCK)
    np.testing.assert_allclose(sq.cal_snr_qam(E, M), G["c%d_c128_bsnr" % c], rtol=RTOL)
    np.testing.assert_allclose(sq.cal_s0(E, M), G["c%d_c128_bs0" % c], rtol=RTOL)


def test_gamma(no_library):
    for M, g in zip(G["gamma_M"], G["gamma"]):
        assert sq._cal_gamma(int(M)) == pytest.approx(float(g), rel=RTOL)
        assert blind_ref.gamma_of(theory.cal_symbols_qam(int(M))) == pytest.approx(float(g), rel=RTOL)
    assert sq._cal_gamma(4) == pytest.approx(1.0, rel=RTOL)


@pytest.mark.parametrize("c", range(len(CASES)))
def test_the_restatement_meets_the_fixture_within_its_tolerance(c):
    """tests/blind_ref.py (numpy's own summation order here) against the reference's complex128 values, within the tolerance the generator
    measured between two summation orders: the yardstick the device values are held to."""
    M = CASES[c][0]
    E, K = rows_of(c, np.complex128)
    gamma, ideal, tol = float(G["gamma"][list(G["gamma_M"]).index(M)]), theory.cal_symbols_qam(M).ravel(), float(G["tol_c128"])
    pre = "c%d_c128_" % c
    st = blind_ref.row_stats(E, gamma)
    np.testing.assert_allclose(st[:2], G[pre + "mom"], rtol=1e-12)
    np.testing.assert_allclose(st[2:4], G[pre + "S"], rtol=1e-12)
    assert blind_ref.evm(E, ideal, gamma) == pytest.approx(float(G[pre + "evm"]), rel=tol)
    if M in NO_SNR:
        return
    assert st[4] == pytest.approx(float(G[pre + "snr"]), rel=tol) and st[5] == pytest.approx(float(G[pre + "s0"]), rel=tol)
    assert blind_ref.evm(E, ideal, gamma, known=K) == pytest.approx(float(G[pre + "evmk"]), rel=tol)
    if M == 4:
        assert blind_ref.qpsk_snr(E)[2] == pytest.approx(float(G[pre + "qpsk"]), rel=tol)


def test_fixture_tolerances_are_what_the_generator_measured():
    t = G["tol_table"]
    assert float(G["tol_c128"]) == pytest.approx(10 * np.nanmax(t[:, 3::2]), rel=1e-12)
    for j, q in enumerate(("snr", "s0", "evm", "evmk", "qpsk")):
        assert float(G["tol_c64_" + q]) == pytest.approx(2 * np.nanmax(t[:, 4 + 2 * j]), rel=1e-12)
    assert float(G["tol_c128"]) < 1e-11 and float(G["tol_c64_snr"]) < 1e-4 and float(G["tol_c64_evm"]) < 1e-6


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_errors_come_before_the_library(no_library):
    E = _Stub((2, 4096), np.complex64)
    with pytest.raises(ValueError):
        hip_dsp.blind_moments_dev(E, block=4097)
    with pytest.raises(ValueError):
        hip_dsp.blind_stats_dev(E, 16, block=5000)
    with pytest.raises(ValueError):
        hip_dsp.qpsk_blind_snr_dev(E, block=-1)
    with pytest.raises(ValueError):
        hip_dsp.blind_stats_dev(E, 2048)
    with pytest.raises(ValueError):
        hip_dsp.blind_evm_dev(E, 4096)
    with pytest.raises(ValueError):
        hip_dsp.norm_to_s0_dev(E, 16, _Stub((2, 4095), np.complex64))
    with pytest.raises(ValueError):
        hip_dsp.blind_evm_dev(E, 16, known=_Stub((2, 4095), np.complex64))
    with pytest.raises(TypeError):
        hip_dsp.blind_moments_dev(_Stub((2, 4096), np.float32))
    with pytest.raises(ValueError):
        hip_dsp.blind_moments_dev(E, mom=_Stub((2, 3), np.float64))
    with pytest.raises(ValueError):
        pipeline._blind_metrics(E, 16, 4097, {})
    real = np.ones(64)
    for f in (lambda m: sq.cal_snr_qam(real, 4, method=m), lambda m: sq.cal_s0(real, 4, method=m), lambda m: sq.cal_evm(real, 4, method=m),
              lambda m: sq.norm_to_s0(real, 4, method=m), lambda m: sq.cal_snr_blind_qpsk(real, method=m)):
        for m in ("pyt", "hip"):
            with pytest.raises(TypeError):
                f(m)
    z = np.ones(64, dtype=np.complex128)
    for f in (lambda: sq.cal_snr_qam(z, 4, method="af"), lambda: sq.cal_s0(z, 4, method="cpu"), lambda: sq.cal_evm(z, 4, method=None),
              lambda: sq.norm_to_s0(z, 4, method="pyx"), lambda: sq.cal_snr_blind_qpsk(z, method="HIP")):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        sq.cal_evm(z, 2048, method="hip")
    with pytest.raises(ValueError):
        sq.cal_evm(z, 4, known=z[:-1])


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
    for stem in ("qh_blind_moments", "qh_scale_by_stat", "qh_blind_evm", "qh_qpsk_blind"):
        assert _lib.SIGNATURES[stem + "_c64_dev"] == _lib.SIGNATURES[stem + "_c128_dev"]
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read()).group(1).split()
    assert "blind" in units


# ------------------------------------------------------------------------------------------------ normalisation
def test_host_normalise_and_center(no_library):
    """helpers.normalise_and_center, the yardstick of SignalQAM.normalize_and_center (whose plain branch runs on the device and is compared
    with it in tests/test_gpu_blind.py): zero mean and unit power per row, the reference's expression row by row."""
    rng = np.random.default_rng(5)
    E = (rng.standard_normal((2, 1000)) + 1j * rng.standard_normal((2, 1000))) * np.array([[0.3], [4.]]) + (0.2 - 0.7j)
    out = helpers.normalise_and_center(E)
    np.testing.assert_allclose(out.mean(axis=-1), 0, atol=1e-15)
    np.testing.assert_allclose(np.mean(abs(out) ** 2, axis=-1), 1, rtol=1e-14)
    for r, o in zip(E, out):
        c = r - r.mean()
        np.testing.assert_allclose(o, c / np.sqrt(np.mean(c.real ** 2 + c.imag ** 2)), rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(helpers.normalise_and_center(E[0]), out[:1], rtol=1e-14, atol=1e-16)
