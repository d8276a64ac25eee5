"""CPU checks of the Python layers of the feed-forward carrier recovery (Viterbi-Viterbi, QPSK partition): the argument checks, which run
before the library is touched, what the signal-level wrappers hand down, the receiver's ``carrier`` option and the entry points' place in
the C ABI."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qampy_amd import _lib, phaserec, pipeline
from qampy_amd.core import hip_dsp, phaserecovery

NEW = ["qh_vv_recover_c64_dev", "qh_vv_recover_c128_dev", "qh_partition16_recover_c64_dev", "qh_partition16_recover_c128_dev"]


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


@pytest.mark.parametrize("N,L", [(1025, 4096), (0, 4096), (-3, 4096), (12, 11), (1024, 1023)])
def test_vv_window_out_of_range_is_refused(no_library, N, L):
    x = np.zeros((2, L), np.complex64)
    with pytest.raises(ValueError):
        phaserecovery.viterbiviterbi(x, N, 4)
    with pytest.raises(ValueError):
        hip_dsp.vv_recover(x, N, 4)
    with pytest.raises(ValueError):
        hip_dsp.vv_recover_dev(_Stub((2, L), np.complex64), N, 4, _Stub((2, max(L - N + 1, 1)), np.float32), _Stub((2, L), np.complex64))


@pytest.mark.parametrize("M", [1, 0, 65, 128])
def test_vv_order_out_of_range_is_refused(no_library, M):
    with pytest.raises(ValueError):
        phaserecovery.viterbiviterbi(np.zeros(100, np.complex128), 11, M)
    with pytest.raises(ValueError):
        hip_dsp.vv_recover_dev(_Stub((1, 100), np.complex128), 11, M, _Stub((1, 90), np.float64), _Stub((1, 100), np.complex128))


@pytest.mark.parametrize("Nblock", [0, -1, 4097])
def test_partition_block_out_of_range_is_refused(no_library, Nblock):
    x = np.zeros((1, 5000), np.complex64)
    with pytest.raises(ValueError):
        phaserecovery.phase_partition_16qam(x, Nblock)
    with pytest.raises(ValueError):
        hip_dsp.partition16_recover_dev(_Stub((1, 5000), np.complex64), Nblock, _Stub((1, 5000), np.float32), _Stub((1, 5000), np.complex64))


def test_device_wrappers_check_their_buffers(no_library):
    E = _Stub((2, 1000), np.complex64)
    good_t, good_o = _Stub((2, 990), np.float32), _Stub((2, 1000), np.complex64)
    for tr, out in ((_Stub((2, 1000), np.float32), good_o),             # the trace of V&V has L - N + 1 entries per row
                    (_Stub((2, 990), np.float64), good_o),              # ... in the signal's real type
                    (_Stub((1, 990), np.float32), good_o),
                    (good_t, _Stub((2, 990), np.complex64)),
                    (good_t, _Stub((2, 1000), np.complex128))):
        with pytest.raises(ValueError):
            hip_dsp.vv_recover_dev(E, 11, 4, tr, out)
    with pytest.raises(ValueError):
        hip_dsp.vv_recover_dev(_Stub((1000,), np.complex64), 11, 4, good_t, good_o)
    with pytest.raises((ValueError, TypeError)):
        hip_dsp.vv_recover_dev(_Stub((2, 1000), np.float32), 11, 4, good_t, good_o)
    full = _Stub((2, 1000), np.float32)
    for tr, out in ((good_t, good_o), (_Stub((2, 1000), np.float64), good_o), (full, _Stub((2, 999), np.complex64)), (full, _Stub((2, 1000), np.complex128))):
        with pytest.raises(ValueError):
            hip_dsp.partition16_recover_dev(E, 64, tr, out)


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    hip_dsp.vv_recover_dev(_Stub((2, 1000), np.complex64, 10), 11, 4, _Stub((2, 990), np.float32, 20), _Stub((2, 1000), np.complex64, 30))
    hip_dsp.vv_recover_dev(_Stub((1, 1024), np.complex128, 10), 1024, 8, _Stub((1, 1), np.float64, 20), _Stub((1, 1024), np.complex128, 30))
    hip_dsp.partition16_recover_dev(_Stub((3, 999), np.complex128, 10), 4096, _Stub((3, 999), np.float64, 20), _Stub((3, 999), np.complex128, 30))
    assert seen == [("qh_vv_recover_c64_dev", 10, 2, 1000, 11, 4, 20, 30), ("qh_vv_recover_c128_dev", 10, 1, 1024, 1024, 8, 20, 30),
                    ("qh_partition16_recover_c128_dev", 10, 3, 999, 4096, 20, 30)]


class _Sig(np.ndarray):
    M = 8

    def recreate_from_np_array(self, arr):
        out = np.asarray(arr).view(_Sig)
        out.tag = "recreated"
        return out


def test_phaserec_wrappers_pass_the_order_and_keep_the_class(monkeypatch):
    seen = []

    def vv(E, N, M, all_modes=False):
        seen.append(("vv", type(E), N, M))
        return np.zeros_like(E), np.zeros(E.shape[1] - N + 1)

    def p16(E, Nblock):
        seen.append(("p16", type(E), Nblock))
        return np.zeros_like(E), np.zeros(E.shape, E.real.dtype)
    monkeypatch.setattr(phaserecovery, "viterbiviterbi", vv)
    monkeypatch.setattr(phaserecovery, "phase_partition_16qam", p16)
    sig = np.ones((2, 50), np.complex64).view(_Sig)
    out, ph = phaserec.viterbiviterbi(sig, 11)
    assert seen[-1] == ("vv", np.ndarray, 11, 8) and type(out) is _Sig and out.tag == "recreated" and ph.shape == (40,)
    out, ph = phaserec.phase_partition_16qam(sig, 16)
    assert seen[-1] == ("p16", np.ndarray, 16) and type(out) is _Sig and out.tag == "recreated" and ph.shape == (2, 50)


def test_core_return_shapes(monkeypatch):
    """1-d in: flat out; 2-d in: every field, and the last mode's V&V trace unless all are asked for."""
    monkeypatch.setattr(hip_dsp, "vv_recover", lambda E, N, M: (np.zeros_like(E), np.arange(E.shape[0])[:, None] * np.ones((1, E.shape[1] - N + 1))))
    monkeypatch.setattr(hip_dsp, "partition16_recover", lambda E, Nb: (np.zeros_like(E), np.zeros(E.shape)))
    out, ph = phaserecovery.viterbiviterbi(np.zeros(100, np.complex128), 11, 4)
    assert out.shape == (100,) and ph.shape == (90,)
    out, ph = phaserecovery.viterbiviterbi(np.zeros((3, 100), np.complex128), 11, 4)
    assert out.shape == (3, 100) and ph.shape == (90,) and np.all(ph == 2)
    out, ph = phaserecovery.viterbiviterbi(np.zeros((3, 100), np.complex128), 11, 4, all_modes=True)
    assert ph.shape == (3, 90)
    out, ph = phaserecovery.phase_partition_16qam(np.zeros(100, np.complex128), 32)
    assert out.shape == ph.shape == (100,)
    out, ph = phaserecovery.phase_partition_16qam(np.zeros((2, 100), np.complex128), 32)
    assert out.shape == ph.shape == (2, 100)


@pytest.mark.parametrize("kw", [dict(M=16, carrier="vv"), dict(M=4, carrier="partition"), dict(M=64, carrier="partition"), dict(M=4, carrier="cma"),
                                dict(M=4, carrier="vv", Bbps=4)])
def test_receiver_refuses_a_wrong_carrier(no_library, kw):
    kw = dict(kw)
    M = kw.pop("M")
    with pytest.raises(ValueError):
        pipeline.ResidentReceiver(2, 4096, 2, M, 17, (1e-3,), methods=("cma",), Nbps=11, **kw)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["qh_vv_recover_c64_dev"]) == 7 and len(_lib.SIGNATURES["qh_partition16_recover_c128_dev"]) == 6
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version()      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "cpr" in units
