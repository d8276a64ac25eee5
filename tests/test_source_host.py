"""CPU checks of the bit source's Python layers: argument and range errors are raised before the library is touched, valid calls reach it
with the ABI's arguments, the entry points have their place in the C ABI (additive: the version stays 11), ``RandomBits`` draws the
reference's values and ``PRBSBits`` warns about a short ``order``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qampy_amd import _lib, signals, synth
from qampy_amd.core import hip_dsp, prbs

NEW = ["qh_prbs_bits_dev", "qh_bits_to_labels_dev", "qh_labels_to_bits_dev", "qh_modulate_bits_c64_dev", "qh_modulate_bits_c128_dev",
       "qh_prbs_symbols_c64_dev", "qh_prbs_symbols_c128_dev"]
c64, c128, u8, i32 = np.complex64, np.complex128, np.uint8, np.int32


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
    monkeypatch.setattr(_lib, "DeviceArray", refuse)


def test_prbs_arguments_are_checked_before_the_library(no_library):
    out = _Stub((100,), u8)
    for kw, exc in ((dict(order=9), ValueError), (dict(order=15, seed=2 ** 15), ValueError), (dict(order=15, seed=-1), ValueError),
                    (dict(order=7, seed=np.ones(8, bool)), ValueError), (dict(order=15, seed=1.5), ValueError), (dict(order=15, kind="fib"), ValueError),
                    (dict(order=15, start=-1), ValueError), (dict(order=15, start=2 ** 62 + 1), ValueError), (dict(order=15, start=0.5), ValueError)):
        with pytest.raises(exc):
            hip_dsp.prbs_bits_dev(out, **kw)
    for bad, exc in ((_Stub((100,), np.int8), TypeError), (_Stub((2, 100), u8), ValueError), (_Stub((0,), u8), ValueError),
                     (_Stub((2 ** 31 + 1,), u8), ValueError)):
        with pytest.raises(exc):
            hip_dsp.prbs_bits_dev(bad, 15)
    assert hip_dsp.prbs_seed(7) == 127 and hip_dsp.prbs_seed(7, [1, 0, 0, 0, 0, 0, 1]) == 65 and hip_dsp.prbs_seed(31, 2 ** 31 - 1) == 2 ** 31 - 1
    with pytest.raises(AssertionError):
        prbs.make_prbs_extXOR(9, 100)
    with pytest.raises(AssertionError):
        prbs.make_prbs_intXOR(8, 100)
    with pytest.raises(ValueError):
        prbs.make_prbs_extXOR(15, 100, seed=2 ** 15)
    with pytest.raises(ValueError):
        prbs.make_prbs_intXOR(23, 100, seed=-3)


def test_mapping_arguments_are_checked_before_the_library(no_library):
    bits, lab = _Stub((2, 600), u8), _Stub((2, 100), i32)
    for b, nb, l, exc in ((bits, 1, lab, ValueError), (bits, 11, lab, ValueError), (bits, 7, lab, ValueError), (bits, 6, _Stub((2, 99), i32), ValueError),
                          (bits, 6, _Stub((2, 100), np.int64), TypeError), (_Stub((2, 600), np.int32), 6, lab, TypeError), (bits, 6, None, ValueError)):
        with pytest.raises(exc):
            hip_dsp.bits_to_labels_dev(b, nb, l)
        with pytest.raises(exc):
            hip_dsp.labels_to_bits_dev(l, nb, b)
    al, sy = _Stub((64,), c64), _Stub((2, 100), c64)
    for b, a, s, l, exc in ((bits, al, _Stub((2, 100), c128), None, ValueError), (bits, al, _Stub((2, 99), c64), None, ValueError),
                            (bits, _Stub((48,), c64), sy, None, ValueError), (bits, _Stub((64,), np.float32), sy, None, TypeError),
                            (bits, al, sy, _Stub((2, 100), np.int16), TypeError), (_Stub((2, 601), u8), al, sy, None, ValueError),
                            (bits, _Stub((2,), c64), sy, None, ValueError), (bits, _Stub((2048,), c64), sy, None, ValueError)):
        with pytest.raises(exc):
            hip_dsp.modulate_bits_dev(b, a, s, l)
    with pytest.raises(ValueError):
        hip_dsp.modulate_bits_dev(bits, _Stub((48,), c64), sy, nb=12)
    row = _Stub((100,), c64)
    for kw, exc in ((dict(symbols=_Stub((2, 100), c64)), ValueError), (dict(symbols=_Stub((100,), c128)), ValueError), (dict(order=8), ValueError),
                    (dict(seed=2 ** 23), ValueError), (dict(kind="galois"), ValueError), (dict(labels=_Stub((99,), i32)), ValueError),
                    (dict(labels=_Stub((100,), np.int64)), ValueError), (dict(bits=_Stub((599,), u8)), ValueError), (dict(bits=_Stub((600,), i32)), TypeError),
                    (dict(alphabet=_Stub((48,), c64)), ValueError), (dict(symbols=_Stub((2 ** 31 // 6 + 1,), c64)), ValueError)):
        args = dict(symbols=row, alphabet=al, order=23)
        args.update(kw)
        with pytest.raises(exc):
            hip_dsp.prbs_symbols_dev(**args)
    E = _Stub((2, 100), c64)
    for e, a, b, l, exc in ((E, _Stub((64,), c128), bits, None, TypeError), (E, al, _Stub((2, 599), u8), None, ValueError),
                            (E, al, bits, _Stub((2, 99), i32), ValueError), (E, _Stub((48,), c64), bits, None, ValueError)):
        with pytest.raises(exc):
            hip_dsp.demodulate_dev(e, a, b, l)
    with pytest.raises(ValueError):
        synth.make_symbols_dev(16, 100, nmodes=3)
    with pytest.raises(ValueError):
        synth.make_symbols_dev(16, 0)


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    hip_dsp.prbs_bits_dev(_Stub((100,), u8, 10), 15)
    hip_dsp.prbs_bits_dev(_Stub((7,), np.bool_, 10), 31, seed=[0, 1, 1], kind="int", start=2 ** 62, invert=True)
    hip_dsp.bits_to_labels_dev(_Stub((2, 600), u8, 10), 6, _Stub((2, 100), i32, 20))
    hip_dsp.labels_to_bits_dev(_Stub((50,), i32, 20), 3, _Stub((150,), u8, 10))
    hip_dsp.modulate_bits_dev(_Stub((2, 600), u8, 10), _Stub((64,), c64, 30), _Stub((2, 100), c64, 40))
    hip_dsp.modulate_bits_dev(_Stub((400,), u8, 10), _Stub((12,), c128, 30), _Stub((100,), c128, 40), _Stub((100,), i32, 20), nb=4)
    hip_dsp.prbs_symbols_dev(_Stub((100,), c64, 40), _Stub((8,), c64, 30), 23, seed=5, start=9)
    hip_dsp.prbs_symbols_dev(_Stub((100,), c128, 40), _Stub((8,), c128, 30), 7, kind="int", labels=_Stub((100,), i32, 20), bits=_Stub((300,), u8, 10))
    assert seen == [("qh_prbs_bits_dev", 15, 0, 2 ** 15 - 1, 0, 0, 100, 10), ("qh_prbs_bits_dev", 31, 1, 6, 2 ** 62, 1, 7, 10),
                    ("qh_bits_to_labels_dev", 10, 200, 6, 20), ("qh_labels_to_bits_dev", 20, 50, 3, 10),
                    ("qh_modulate_bits_c64_dev", 10, 200, 6, 30, 64, 40, None), ("qh_modulate_bits_c128_dev", 10, 100, 4, 30, 12, 40, 20),
                    ("qh_prbs_symbols_c64_dev", 23, 0, 5, 9, 100, 3, 30, 8, 40, None, None),
                    ("qh_prbs_symbols_c128_dev", 7, 1, 127, 0, 100, 3, 30, 8, 40, 20, 10)]


def test_the_library_refuses_bad_arguments_before_any_launch():
    """QH_ERR_ARG from the C entry points themselves, on a machine without a device: the checks come before the device is initialised."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    bad = [lib.qh_prbs_bits_dev(9, 0, 1, 0, 0, 8, p), lib.qh_prbs_bits_dev(15, 2, 1, 0, 0, 8, p), lib.qh_prbs_bits_dev(15, 0, 2 ** 15, 0, 0, 8, p),
           lib.qh_prbs_bits_dev(15, 0, -1, 0, 0, 8, p), lib.qh_prbs_bits_dev(15, 0, 1, -1, 0, 8, p), lib.qh_prbs_bits_dev(15, 0, 1, 2 ** 62 + 1, 0, 8, p),
           lib.qh_prbs_bits_dev(15, 0, 1, 0, 0, 0, p), lib.qh_prbs_bits_dev(15, 0, 1, 0, 0, 2 ** 31 + 1, p), lib.qh_prbs_bits_dev(15, 0, 1, 0, 0, 8, None),
           lib.qh_bits_to_labels_dev(p, 4, 1, p), lib.qh_bits_to_labels_dev(p, 4, 11, p), lib.qh_bits_to_labels_dev(p, 0, 4, p),
           lib.qh_bits_to_labels_dev(None, 4, 4, p), lib.qh_bits_to_labels_dev(p, 4, 4, None), lib.qh_labels_to_bits_dev(None, 4, 4, p),
           lib.qh_labels_to_bits_dev(p, 4, 4, None), lib.qh_labels_to_bits_dev(p, 4, 12, p), lib.qh_modulate_bits_c64_dev(p, 4, 4, None, 16, p, None),
           lib.qh_modulate_bits_c128_dev(p, 4, 4, p, 16, None, None), lib.qh_modulate_bits_c64_dev(p, 4, 4, p, 0, p, None),
           lib.qh_prbs_symbols_c64_dev(15, 0, 1, 0, 4, 4, p, 16, None, None, None), lib.qh_prbs_symbols_c64_dev(15, 0, 1, 0, 4, 4, None, 16, p, None, None),
           lib.qh_prbs_symbols_c128_dev(15, 0, 1, 0, 4, 4, p, 8, p, None, None), lib.qh_prbs_symbols_c128_dev(15, 0, 1, 0, 2 ** 29, 8, p, 256, p, None, None),
           lib.qh_prbs_symbols_c64_dev(16, 0, 1, 0, 4, 4, p, 16, p, None, None), lib.qh_prbs_symbols_c64_dev(15, 0, 1, 0, 0, 4, p, 16, p, None, None)]
    assert bad == [_lib.QH_ERR_ARG] * len(bad)
    assert not buf.any()


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["qh_prbs_bits_dev"]) == 7 and len(_lib.SIGNATURES["qh_prbs_symbols_c64_dev"]) == 11
    assert _lib.SIGNATURES["qh_prbs_bits_dev"][3] is C.c_int64                                   # start: 64 bits
    assert len(_lib.SIGNATURES["qh_modulate_bits_c128_dev"]) == 7 and len(_lib.SIGNATURES["qh_labels_to_bits_dev"]) == 4
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "source" in units
    src = open(os.path.join(ROOT, "qampy_amd", "csrc", "source.hip")).read()
    assert int(re.search(r"SRC_WPT_BITS = (\d+)", src).group(1)) * 256 * 32 == hip_dsp.PRBS_W
    assert int(re.search(r"SRC_SPT = (\d+)", src).group(1)) * 256 == hip_dsp.SOURCE_SYMS


def test_random_bits_are_the_references(golden):
    g = golden["source"]
    n, nmodes, seed = (int(v) for v in g["rb_args"])
    rb = signals.RandomBits(n, nmodes=nmodes, seed=seed)
    assert isinstance(rb, signals.RandomBits) and rb.dtype == bool and rb.shape == (nmodes, n)
    assert np.array_equal(np.asarray(rb), np.unpackbits(g["rb_bits"], axis=-1)[:, :n].astype(bool))
    assert rb[:, 3:9]._seed == seed


def test_prbsbits_warns_about_a_short_order(monkeypatch):
    calls = []

    class _Dev(_Stub):
        def __init__(self, shape, dtype):
            super().__init__(tuple(shape), dtype)

        def to_host(self):
            return np.zeros(self.shape, self.dtype)

    monkeypatch.setattr(_lib, "DeviceArray", _Dev)
    monkeypatch.setattr(hip_dsp, "prbs_bits_dev", lambda out, order, seed=None, **kw: calls.append((order, seed, kw)))
    with pytest.warns(UserWarning, match="PRBSorder is not given for all dimensions"):
        b = signals.PRBSBits(40, nmodes=3, seed=[None, 5], order=[15, 23])
    assert b.shape == (3, 40) and b.dtype == bool
    assert calls[0][:2] == (15, None) and calls[1][:2] == (23, 5) and calls[2][0] in (15, 23) and 0 <= calls[2][1] < 2 ** calls[2][0]
    assert all(c[2] == dict(kind="ext") for c in calls) and b._order[:2] == [15, 23]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        signals.PRBSBits(40, nmodes=2)
    assert [c[:2] for c in calls[3:]] == [(15, None), (23, None)]


def test_the_module_docstring_no_longer_calls_the_signal_classes_out_of_scope():
    assert "SignalQAMGrayCoded" in signals.__doc__ and "PRBSBits" in signals.__doc__
    assert issubclass(signals.SignalQAMGrayCoded, signals.SignalQAM)
