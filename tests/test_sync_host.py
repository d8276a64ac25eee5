"""CPU checks of the device synchronisation's Python layers and of its float64 restatement (tests/sync_ref.py): the restatement equals the
host ``sync_and_adjust`` on the whole grid and the reference's recorded results (tests/golden/sync.npz); the keywords refuse unknown
values; the argument checks run before the library is touched; the entry points have their place in the C ABI."""
import os
import re

import numpy as np
import pytest

import sync_ref
from conftest import ROOT
from qampy_amd import _lib, pipeline
from qampy_amd.core import ber_functions, hip_dsp
from qampy_amd.signals import SignalQAM

NEW = ["qh_xcorr_c64_dev", "qh_xcorr_c128_dev", "qh_xcorr_peak_c64_dev", "qh_xcorr_peak_c128_dev", "qh_cyclic_gather_c64_dev",
       "qh_cyclic_gather_c128_dev", "qh_cyclic_gather_i32_dev", "qh_labels_to_symbols_c64_dev", "qh_labels_to_symbols_c128_dev"]


class _Stub:
    """A stand-in with a DeviceArray's attributes: the checks must fire before any library call."""
    def __init__(self, shape, dtype, ptr=1):
        self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), ptr

    def row(self, i):
        return _Stub(self.shape[1:], self.dtype, self.ptr + 1 + i)


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


@pytest.fixture(scope="module")
def fx(golden):
    return golden["sync"]


def _cx(q, fx):
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(fx["scale"])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("adjust", ["tx", "rx"])
@pytest.mark.parametrize("ntx,nrx", sync_ref.LENGTHS)
def test_restatement_equals_the_host_form(ntx, nrx, adjust):
    """Roll, roll-and-cut and periodic extension are one gather formula: exact equality with the host form, five shifts, four turns."""
    for shift in sync_ref.shifts(ntx):
        for turns in range(4):
            tx, rx = sync_ref.case(ntx, nrx, shift, turns)
            (htx, hrx), hpeak = ber_functions.sync_and_adjust(tx, rx, adjust)
            (rtx, rrx), rpeak = sync_ref.sync_and_adjust(tx, rx, adjust)
            assert htx.shape == rtx.shape and hrx.shape == rrx.shape, (shift, turns)
            assert np.array_equal(htx, rtx) and np.array_equal(hrx, rrx), (shift, turns)
            assert abs(hpeak - rpeak) <= 1e-11 * abs(hpeak), (shift, turns)


def test_gather_formula_with_negative_offsets_and_whole_periods():
    src = np.arange(7) + 1j * np.arange(7)[::-1]
    for offset in (-15, -7, -1, 0, 3, 7, 14, 22):
        for nout in (3, 7, 20):
            want = np.array([src[(i - offset) % 7] for i in range(nout)])
            for turns in range(4):
                assert np.array_equal(sync_ref.gather(src, offset, turns, nout), want * 1j ** turns)
    assert np.array_equal(sync_ref.gather(np.arange(5), 2, 0, 5), np.roll(np.arange(5), 2))


def test_restatement_correlation_is_fftconvolve():
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(3)
    x, y = (rng.standard_normal(n) + 1j * rng.standard_normal(n) for n in (300, 77))
    np.testing.assert_allclose(sync_ref.xcorr(x, y), fftconvolve(x, y.conj()[::-1], "full"), rtol=0, atol=1e-11)
    res = sync_ref.peak(np.array([1, -5j, 3, 5, -2], dtype=np.complex128))
    assert list(res) == [1, 5, 0, 2, 5, 5]


def test_golden_cases_hold_for_the_host_form_and_the_restatement(fx):
    for k, (ntx, nrx, shift, turns) in enumerate(fx["cases"]):
        tx, rx = _cx(fx["c%d_txq" % k], fx), _cx(fx["c%d_rxq" % k], fx)
        assert tx.shape == (ntx,) and rx.shape == (nrx,)
        for adjust in ("tx", "rx"):
            p = "c%d_%s_" % (k, adjust)
            for f in (ber_functions.sync_and_adjust, sync_ref.sync_and_adjust):
                (atx, arx), peak = f(tx, rx, adjust)
                assert np.array_equal(atx, _cx(fx[p + "txq"], fx)) and np.array_equal(arx, _cx(fx[p + "rxq"], fx)), (k, adjust, f.__module__)
                np.testing.assert_allclose(peak, fx[p + "peak"], rtol=1e-11)
            x, y = (rx, tx) if adjust == "tx" else (tx, rx)
            offset, _, nturns, _ = ber_functions.find_sequence_offset_complex(x, y)
            if fx[p + "runner_up"] < 0.9:
                assert (offset, nturns) == (fx[p + "offset"], fx[p + "turns"])


# ------------------------------------------------------------------------------------------------ keywords
def test_unknown_keyword_values_are_refused(no_library):
    x = np.ones(16, np.complex128)
    for bad in ("gpu", "", None, "HIP"):
        with pytest.raises(ValueError):
            ber_functions.find_sequence_offset(x, x, method=bad)
        with pytest.raises(ValueError):
            ber_functions.find_sequence_offset_complex(x, x, method=bad)
        with pytest.raises(ValueError):
            ber_functions.sync_and_adjust(x, x, method=bad)
    out, idx, al = _Stub((2, 100), np.complex64), _Stub((2, 100), np.int32), _Stub((16,), np.complex64)
    for bad in ("fft", "", None, "Full"):
        with pytest.raises(ValueError):
            ber_functions.cal_ser_dev(out, idx, al, sync=bad)
        with pytest.raises(ValueError):
            ber_functions.cal_metrics_dev(out, idx, al, sync=bad)
    sig = SignalQAM(np.ones((1, 16), np.complex128), 4, symbols=np.ones((1, 16), np.complex128))
    for name in ("cal_ser", "cal_ber", "cal_evm", "est_snr", "cal_gmi", "cal_mi"):
        with pytest.raises(ValueError):
            getattr(sig, name)(sync_method="gpu")


def test_defaults_are_the_host_and_the_window_forms(no_library):
    import inspect
    for f in (ber_functions.find_sequence_offset, ber_functions.find_sequence_offset_complex, ber_functions.sync_and_adjust):
        assert inspect.signature(f).parameters["method"].default == "pyt"
    for f in (ber_functions.cal_ser_dev, ber_functions.cal_metrics_dev, pipeline.ResidentReceiver.ser, pipeline.ResidentReceiver.metrics,
              pipeline.ChannelBank.ser, pipeline.ChannelBank.metrics):
        assert inspect.signature(f).parameters["sync"].default == "window"
    for name in ("_sync_and_adjust", "cal_ser", "cal_ber", "cal_evm", "est_snr", "cal_gmi", "cal_mi"):
        assert inspect.signature(getattr(SignalQAM, name)).parameters["sync_method"].default == "pyt"
    tx, rx = sync_ref.case(100, 257, 37, 1)           # the host form runs with the library out of reach
    (atx, arx), peak = ber_functions.sync_and_adjust(tx, rx)
    assert atx.shape == arx.shape == (257,) and peak > 0


def test_signal_methods_hand_the_method_down(monkeypatch):
    seen = []

    def fake(tx, rx, adjust="tx", method="pyt"):
        seen.append(method)
        return (tx, rx), 1.
    monkeypatch.setattr(ber_functions, "sync_and_adjust", fake)
    x = np.ones((1, 16), np.complex128)
    sig = SignalQAM(x, 4, symbols=x)
    sig._sync_and_adjust(x, x, sync_method="hip")
    sig._sync_and_adjust(x, x)
    assert seen == ["hip", "pyt"]


def test_receiver_and_bank_pass_sync_through(monkeypatch):
    seen = []
    monkeypatch.setattr(ber_functions, "cal_ser_dev", lambda *a, **k: seen.append(("ser", k.get("sync"))))
    monkeypatch.setattr(ber_functions, "cal_metrics_dev", lambda *a, **k: seen.append(("metrics", k.get("sync"))))
    monkeypatch.setattr(ber_functions, "tx_indices_dev", lambda *a, **k: "idx")
    rx = object.__new__(pipeline.ResidentReceiver)
    rx.alphabet_host, rx.alphabet, rx.Mtestangles, rx.out, rx.eq, rx.ct = np.ones(4), "alphabet", 0, None, _Stub((2, 8), np.complex64), np.complex64
    rx.wait_post, rx._sync_ws, rx._idx_tx = lambda *a: None, {}, None
    rx._prepare_tx = lambda s: setattr(rx, "_idx_tx", "idx")
    tx = np.ones((2, 8), np.complex64)
    rx.ser(tx, sync="full"); rx.metrics(tx, sync="full"); rx.ser(tx); rx.metrics(tx)
    bank = object.__new__(pipeline.ChannelBank)
    bank.rx, bank.ct, bank.eq, bank.out = rx, np.complex64, _Stub((1, 2, 8), np.complex64), None
    bank.ser(0, tx, sync="full"); bank.metrics(0, tx, sync="full"); bank.metrics(0, tx)
    assert seen == [("ser", "full"), ("metrics", "full"), ("ser", "window"), ("metrics", "window"), ("ser", "full"), ("metrics", "full"),
                    ("metrics", "window")]


# ------------------------------------------------------------------------------------------------ argument checks
def test_xcorr_checks_its_arguments(no_library):
    c64, c128 = np.complex64, np.complex128
    x, y = _Stub((2, 100), c64), _Stub((50,), c64)
    for xx, yy, out, exc in ((x, y, _Stub((2, 150), c64), ValueError),                  # nx + ny - 1 = 149
                             (x, y, _Stub((149,), c64), ValueError),
                             (x, _Stub((1, 50), c64), _Stub((2, 149), c64), ValueError),      # y is one row
                             (x, _Stub((50,), c128), _Stub((2, 149), c64), TypeError),
                             (x, y, _Stub((2, 149), c128), TypeError),
                             (_Stub((2, 100), np.float32), y, _Stub((2, 149), c64), TypeError),
                             (_Stub((2, 2 ** 23 + 1), c64), _Stub((2 ** 23 + 1,), c64), _Stub((2, 2 ** 24 + 1), c64), ValueError),
                             (_Stub((2, 3, 100), c64), y, _Stub((2, 3, 149), c64), ValueError),
                             (_Stub((0,), c64), y, _Stub((49,), c64), ValueError)):
        with pytest.raises(exc):
            hip_dsp.xcorr_dev(xx, yy, out)
    with pytest.raises(ValueError):
        ber_functions.find_sequence_offset(np.ones(2 ** 23 + 1, np.complex64), np.ones(2 ** 23 + 1, np.complex64), method="hip")
    with pytest.raises(ValueError):
        ber_functions.sync_and_adjust(np.ones((2, 8), c128), np.ones(8, c128), method="hip")


def test_peak_and_gather_check_their_arguments(no_library):
    c64 = np.complex64
    cc = _Stub((2, 149), c64)
    for c, n, res, exc in ((cc, 149, _Stub((2, 5), np.float64), ValueError), (cc, 149, _Stub((2, 6), np.float32), ValueError),
                           (cc, 100, _Stub((2, 6), np.float64), ValueError),               # a stack is searched whole
                           (_Stub((149,), c64), 150, _Stub((6,), np.float64), ValueError), (_Stub((149,), c64), 0, _Stub((6,), np.float64), ValueError),
                           (_Stub((149,), np.float64), 149, _Stub((6,), np.float64), TypeError)):
        with pytest.raises(exc):
            hip_dsp.xcorr_peak_dev(c, n, res)
    src, out = _Stub((100,), c64, 10), _Stub((257,), c64, 20)
    for s, off, t, o, exc in ((src, 1.5, 0, out, ValueError), (src, 0, 0.5, out, ValueError), (src, 0, 0, _Stub((257,), np.complex128, 20), TypeError),
                              (src, 0, 0, _Stub((100,), c64, 10), ValueError),              # out is src
                              (_Stub((2, 100), c64, 10), 0, 0, out, ValueError), (src, 2 ** 31 + 1, 0, out, ValueError),
                              (_Stub((100,), np.int32, 10), 0, 1, _Stub((100,), np.int32, 20), ValueError),
                              (_Stub((100,), np.float32, 10), 0, 0, _Stub((100,), np.float32, 20), TypeError)):
        with pytest.raises(exc):
            hip_dsp.cyclic_gather_dev(s, off, t, o)
    idx, al = _Stub((2, 100), np.int32), _Stub((16,), c64)
    for i, a, o, exc in ((_Stub((2, 100), np.int64), al, _Stub((2, 100), c64), TypeError), (idx, al, _Stub((2, 99), c64), ValueError),
                         (idx, al, _Stub((2, 100), np.complex128), ValueError), (idx, _Stub((16,), np.float32), _Stub((2, 100), c64), TypeError)):
        with pytest.raises(exc):
            hip_dsp.labels_to_symbols_dev(i, a, o)
    with pytest.raises(ValueError):
        hip_dsp.sync_and_adjust_dev(src, out, adjust="both")
    with pytest.raises(ValueError):
        hip_dsp.sync_and_adjust_dev(src, out, out=_Stub((100,), c64))                     # adjust="tx": out has rx's length
    with pytest.raises(TypeError):
        hip_dsp.find_sequence_offset_complex_dev(src, _Stub((257,), np.complex128))


def test_full_alignment_checks_before_the_library(no_library):
    al = _Stub((16,), np.complex64)
    with pytest.raises(ValueError, match="modes"):
        ber_functions.cal_metrics_dev(_Stub((3, 100), np.complex64), _Stub((2, 100), np.int32), al, sync="full")
    with pytest.raises(ValueError, match="modes"):
        ber_functions.cal_ser_dev(_Stub((3, 100), np.complex64), _Stub((2, 100), np.int32), al, sync="full")
    with pytest.raises(ValueError):
        ber_functions.cal_ser_dev(_Stub((1, 2 ** 23 + 1), np.complex64), _Stub((1, 2 ** 23 + 1), np.int32), al, sync="full")
    with pytest.raises(TypeError):
        ber_functions.cal_ser_dev(_Stub((1, 100), np.complex64), _Stub((1, 100), np.int32), _Stub((16,), np.complex128), sync="full")


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    c64, c128 = np.complex64, np.complex128
    hip_dsp.xcorr_dev(_Stub((2, 100), c64, 10), _Stub((50,), c64, 20), _Stub((2, 149), c64, 30))
    hip_dsp.xcorr_dev(_Stub((100,), c128, 10), _Stub((1,), c128, 20), _Stub((100,), c128, 30))
    hip_dsp.xcorr_peak_dev(_Stub((2, 149), c64, 30), 149, _Stub((2, 6), np.float64, 40))
    hip_dsp.xcorr_peak_dev(_Stub((256,), c128, 30), 149, _Stub((6,), np.float64, 40))
    hip_dsp.cyclic_gather_dev(_Stub((100,), c64, 10), -3, 5, _Stub((257,), c64, 20))
    hip_dsp.cyclic_gather_dev(_Stub((100,), np.int32, 10), 7, 0, _Stub((40,), np.int32, 20))
    hip_dsp.labels_to_symbols_dev(_Stub((2, 100), np.int32, 10), _Stub((16,), c128, 20), _Stub((2, 100), c128, 30))
    assert seen == [("qh_xcorr_c64_dev", 10, 2, 100, 20, 50, 30), ("qh_xcorr_c128_dev", 10, 1, 100, 20, 1, 30),
                    ("qh_xcorr_peak_c64_dev", 30, 2, 149, 40), ("qh_xcorr_peak_c128_dev", 30, 1, 149, 40),
                    ("qh_cyclic_gather_c64_dev", 10, 100, -3, 1, 257, 20), ("qh_cyclic_gather_i32_dev", 10, 100, 7, 40, 20),
                    ("qh_labels_to_symbols_c128_dev", 10, 200, 20, 16, 30)]


def test_peak_decision_rule():
    assert hip_dsp.peak_decision(np.array([120., 1., 7., 3., 2., 7.]), 100) == (21, 1, 7.)
    assert hip_dsp.peak_decision(np.array([120., 4., 4., 3., 2., 4.]), 100) == (21, 0, 4.)          # the first of equal hypotheses
    assert hip_dsp.peak_decision(np.array([5., 0., 0., 0., 0., 0.]), 3) == (0, 0, 0.)
    assert hip_dsp.peak_decision(np.array([5., np.nan, np.nan, np.nan, np.nan, np.nan]), 3) == (0, 0, 0.)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["qh_xcorr_c64_dev"]) == 6 and len(_lib.SIGNATURES["qh_xcorr_peak_c128_dev"]) == 4
    assert len(_lib.SIGNATURES["qh_cyclic_gather_c64_dev"]) == 6 and len(_lib.SIGNATURES["qh_cyclic_gather_i32_dev"]) == 5
    assert len(_lib.SIGNATURES["qh_labels_to_symbols_c64_dev"]) == 5
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "sync" in units
