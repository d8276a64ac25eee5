"""CPU checks of the impairment layers' argument, dtype and shape rules and of the ``seed=None`` behaviour, with the library call stubbed:
the checks fire before the library is touched, and what reaches it is recorded."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import qampy_amd
from qampy_amd import _lib
from qampy_amd.core import hip_dsp
from qampy_amd.core import impairments as core_imp

NEW = ["qh_impair_pointwise_c64", "qh_impair_pointwise_c128", "qh_impair_pointwise_c64_dev", "qh_impair_pointwise_c128_dev",
       "qh_phase_noise_c64_dev", "qh_phase_noise_c128_dev", "qh_rotate_field_c64_dev", "qh_rotate_field_c128_dev",
       "qh_apply_pmd_c64", "qh_apply_pmd_c128", "qh_apply_pmd_c64_dev", "qh_apply_pmd_c128_dev", "qh_modal_delay_c64_dev", "qh_modal_delay_c128_dev"]
FS = 40e9


class _Stub:
    """A stand-in with a DeviceArray's attributes: the checks must fire before any library call."""
    def __init__(self, shape, dtype, ptr=1):
        self.shape, self.dtype, self.ptr = tuple(shape), np.dtype(dtype), ptr


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


@pytest.fixture
def recorded(monkeypatch):
    """The library replaced by a recorder: DeviceArrays are host arrays, every call is noted and leaves its buffers as they are."""
    calls = []

    class FakeArray:
        _n = 0

        def __init__(self, shape, dtype, zero=False):
            self.shape, self.dtype = tuple(int(s) for s in np.atleast_1d(shape)), np.dtype(dtype)
            self.a = np.zeros(self.shape, self.dtype)
            FakeArray._n += 1
            self.ptr = FakeArray._n

        @classmethod
        def from_host(cls, arr):
            out = cls(arr.shape, arr.dtype)
            out.a = np.array(arr)
            return out

        def to_host(self):
            return self.a.copy()
    monkeypatch.setattr(_lib, "DeviceArray", FakeArray)
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name,) + args))
    return calls


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11


def test_the_reference_names_exist():
    for n in ("rotate_field", "apply_PMD_to_field", "phase_noise", "apply_phase_noise", "add_awgn", "change_snr", "add_carrier_offset", "add_modal_delay",
              "simulate_transmission", "add_dispersion"):
        assert callable(getattr(core_imp, n)), n
    for n in ("apply_PMD", "apply_phase_noise", "change_snr", "add_carrier_offset", "simulate_transmission", "add_dispersion"):
        assert callable(getattr(qampy_amd.impairments, n)), n
    from qampy_amd.pipeline import ResidentReceiver
    assert callable(ResidentReceiver.impair)


def test_device_wrappers_check_their_arguments(no_library):
    E, E128 = _Stub((2, 4096), np.complex64), _Stub((2, 4096), np.complex128, ptr=2)
    out = _Stub((2, 4096), np.complex64, ptr=3)
    with pytest.raises(TypeError):
        hip_dsp.impair_pointwise_dev(_Stub((2, 4096), np.float32), out, sigma=0.1)
    with pytest.raises(TypeError):
        hip_dsp.impair_pointwise_dev(_Stub((4096,), np.complex64), out, sigma=0.1)
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, E128, sigma=0.1)
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, _Stub((2, 4000), np.complex64), sigma=0.1)
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, sigma=0.1, snr=(10, 2))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            hip_dsp.impair_pointwise_dev(E, out, sigma=bad)
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, snr=(10, 0))
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, phase=(-1e5, FS))
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, freq=(np.inf, FS))
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, sigma=0.1, seed=1.5)
    with pytest.raises(ValueError):                                      # a trace without phase noise
        hip_dsp.impair_pointwise_dev(E, out, sigma=0.1, trace=_Stub((2, 4096), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.impair_pointwise_dev(E, out, phase=(1e5, FS), trace=_Stub((2, 4096), np.float32))
    with pytest.raises(TypeError):
        hip_dsp.phase_noise_dev(_Stub((2, 4096), np.float32), 1e5, FS, 0)
    with pytest.raises(TypeError):
        hip_dsp.phase_noise_dev(_Stub((2, 4096), np.float64), 1e5, FS, 0, draws=np.float16)
    with pytest.raises(ValueError):
        hip_dsp.phase_noise_dev(_Stub((2, 4096), np.float64), -1e5, FS, 0)
    three, three_out = _Stub((3, 4096), np.complex64), _Stub((3, 4096), np.complex64, ptr=4)
    for fn in (lambda a, b: hip_dsp.apply_pmd_dev(a, b, 0.3, 30e-12, FS), lambda a, b: hip_dsp.rotate_field_dev(a, b, 0.3),
               lambda a, b: hip_dsp.simulate_transmission_dev(a, b, FS / 2, FS, dgd=30e-12)):
        with pytest.raises(ValueError, match="two modes"):
            fn(three, three_out)
    with pytest.raises(ValueError, match="out of place"):
        hip_dsp.apply_pmd_dev(E, E, 0.3, 30e-12, FS)
    with pytest.raises(ValueError, match="out of place"):
        hip_dsp.modal_delay_dev(E, E, [1, 2])
    for bad in ([1], [1, 2, 3], [[1, 2]], [1.5, 2]):
        with pytest.raises(ValueError):
            hip_dsp.modal_delay_dev(E, out, bad)
    with pytest.raises(ValueError):
        hip_dsp.apply_pmd_dev(E, out, 0.3, np.nan, FS)


def test_ndarray_layer_checks_its_arguments(no_library):
    x = np.zeros((2, 512), np.complex64)
    with pytest.raises(ValueError):
        core_imp.rotate_field(np.zeros((3, 512), np.complex64), 0.1)
    with pytest.raises(ValueError):
        core_imp.rotate_field(np.zeros(512, np.complex64), 0.1)
    with pytest.raises(ValueError):
        core_imp.apply_PMD_to_field(np.zeros((1, 512), np.complex128), 0.1, 30e-12, FS)
    with pytest.raises(ValueError):
        core_imp.add_modal_delay(x, [1, 2, 3])
    with pytest.raises(ValueError):
        core_imp.add_modal_delay(np.zeros(512, np.complex64), [1])
    with pytest.raises(ValueError):
        core_imp.add_awgn(np.zeros((2, 2, 8), np.complex64), 0.1)
    with pytest.raises(ValueError):
        core_imp.add_awgn(x, 0.1, seed=0.5)
    with pytest.raises(ValueError):
        core_imp.simulate_transmission(np.zeros(512, np.complex64), FS / 2, FS, dgd=30e-12)
    with pytest.raises(ValueError):
        core_imp.phase_noise((2, 3, 4), 1e5, FS)
    # nothing to impair: no library call at all
    assert core_imp.add_awgn(np.zeros((2, 0), np.complex64), 0.1, seed=1).shape == (2, 0)
    assert core_imp.phase_noise((2, 0), 1e5, FS, seed=1).shape == (2, 0)


@pytest.mark.parametrize("dtype,want", [(np.complex64, np.complex64), (np.complex128, np.complex128), (np.float32, np.complex128), (np.int16, np.complex128)])
def test_dtype_and_shape_are_kept(recorded, dtype, want):
    for shape in ((2, 300), (300,)):
        x = np.ones(shape, dtype)
        for out in (core_imp.add_awgn(x, 0.1, seed=1), core_imp.change_snr(x, 10, FS / 2, FS, seed=1), core_imp.apply_phase_noise(x, 1e5, FS, seed=1),
                    core_imp.add_carrier_offset(x, 1e6, FS), core_imp.simulate_transmission(x, FS / 2, FS, snr=10, lwdth=1e5, freq_off=1e6, seed=2)):
            assert out.shape == shape and out.dtype == want
    x = np.ones((2, 300), dtype)
    for out in (core_imp.rotate_field(x, 0.2), core_imp.apply_PMD_to_field(x, 0.2, 30e-12, FS), core_imp.add_modal_delay(x, [1, -1]),
                core_imp.simulate_transmission(x, FS / 2, FS, dgd=30e-12, modal_delay=[1, 2])):
        assert out.shape == (2, 300) and out.dtype == want
    suffix = "c64" if want == np.complex64 else "c128"
    assert recorded and all(c[0].startswith("qh_") and suffix + "_dev" in c[0] for c in recorded), [c[0] for c in recorded]
    assert core_imp.phase_noise(300, 1e5, FS, seed=1).shape == (300,) and core_imp.phase_noise((2, 300), 1e5, FS, seed=1).dtype == np.float64


def test_what_reaches_the_library(recorded):
    x = np.ones((2, 300), np.complex64)
    core_imp.simulate_transmission(x, 10e9, 20e9, snr=20, lwdth=1e5, freq_off=1e6, dgd=30e-12, theta=0.5, modal_delay=[3, -5], seed=7)
    names = [c[0] for c in recorded]
    assert names == ["qh_impair_pointwise_c64_dev", "qh_modal_delay_c64_dev", "qh_apply_pmd_c64_dev"]          # the reference's order
    _, E, nm, L, mode, noise, have_phase, var, have_freq, freq, seed, trace, out = recorded[0]
    assert (nm, L, mode, have_phase, have_freq, seed, trace) == (2, 300, 2, 1, 1, 7, None)
    assert noise == pytest.approx(0.1 * np.sqrt(2)) and var == pytest.approx(2 * np.pi * 1e5 / 20e9) and freq == pytest.approx(1e6 / 20e9)
    assert recorded[2][4] == 0.5 and recorded[2][5] == pytest.approx(30e-12 * 20e9)
    assert recorded[2][-1] != recorded[2][1] and recorded[1][-1] != recorded[1][1]                           # out of place
    del recorded[:]
    core_imp.add_awgn(x, 0.25, seed=2 ** 40 + 3)
    assert recorded[0][4:6] == (1, 0.25) and recorded[0][10] == 2 ** 40 + 3
    del recorded[:]
    core_imp.simulate_transmission(x, 10e9, 20e9)
    assert recorded[0][4] == 0 and recorded[0][6] == 0 and recorded[0][8] == 0


def test_seed_none_follows_numpy_random(recorded):
    x = np.ones((1, 64), np.complex128)

    def seeds(fn):
        del recorded[:]
        fn()
        return [c[10] if c[0].startswith("qh_impair") else c[5] for c in recorded]
    for fn in (lambda: core_imp.add_awgn(x, 0.1), lambda: core_imp.change_snr(x, 10, FS / 2, FS), lambda: core_imp.apply_phase_noise(x, 1e5, FS),
               lambda: core_imp.phase_noise((1, 64), 1e5, FS), lambda: core_imp.simulate_transmission(x, FS / 2, FS, snr=10)):
        np.random.seed(123)
        a = seeds(fn)
        b = seeds(fn)                           # the generator has moved on
        np.random.seed(123)
        c = seeds(fn)
        assert len(a) == 1 and a == c and a != b, (a, b, c)
        assert 0 <= a[0] < 2 ** 64
    # an explicit seed leaves numpy's generator alone
    np.random.seed(5)
    want = np.random.randint(0, 1000)
    np.random.seed(5)
    core_imp.add_awgn(x, 0.1, seed=3)
    assert np.random.randint(0, 1000) == want


def test_signal_wrappers_pass_the_signals_own_rates(recorded):
    from qampy_amd.signals import SignalQAM
    sig = SignalQAM(np.ones((2, 256), np.complex64), 16, fb=10e9, fs=20e9, symbols=np.ones((2, 128), np.complex64),
                    coded_symbols=np.ones(16, np.complex64))
    out = qampy_amd.impairments.change_snr(sig, 20, seed=1)
    assert type(out) is type(sig) and out.fs == sig.fs and recorded[-1][5] == pytest.approx(0.1 * np.sqrt(2))
    out = qampy_amd.impairments.apply_PMD(sig, 0.3, 50e-12)
    assert type(out) is type(sig) and recorded[-1][0] == "qh_apply_pmd_c64_dev" and recorded[-1][5] == pytest.approx(1.0)
    qampy_amd.impairments.apply_phase_noise(sig, 1e5, seed=1)
    assert recorded[-1][7] == pytest.approx(2 * np.pi * 1e5 / 20e9)
    qampy_amd.impairments.add_carrier_offset(sig, 2e6)
    assert recorded[-1][9] == pytest.approx(1e-4)
    del recorded[:]
    out = qampy_amd.impairments.simulate_transmission(sig, snr=20, lwdth=1e5, dgd=30e-12, modal_delay=[1, 2], seed=3)
    assert [c[0] for c in recorded] == ["qh_impair_pointwise_c64_dev", "qh_modal_delay_c64_dev", "qh_apply_pmd_c64_dev"] and type(out) is type(sig)
