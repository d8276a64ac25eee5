"""CPU checks of the Python layers of PSK, resampled and time-domain hybrid QAM signals (csrc/hybrid.hip): the entry points' place in the C ABI,
the argument checks - which run before the device is touched -, the classes' attributes, and the host ("pyt") paths against the reference's
arrays (tests/golden/hybrid.npz).  No GPU: where a constructor would make its parts on the device, the golden parts stand in for them."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import hybrid_ref as ref
import resample_ref
from conftest import ROOT
from qampy_amd import _lib, signals, synth
from qampy_amd.core import hip_dsp

NEW = ["qh_tdh_assemble_c64_dev", "qh_tdh_assemble_c128_dev", "qh_tdh_class_sums_c64_dev", "qh_tdh_class_sums_c128_dev", "qh_tdh_align_dev",
       "qh_tdh_split_c64_dev", "qh_tdh_split_c128_dev", "qh_tdh_metrics_c64_dev", "qh_tdh_metrics_c128_dev"]
PREFIXES = ["t%d_n%d_" % (k, nm) for k in range(4) for nm in (1, 2)] + ["tfs_", "tpsk_"]
DTS = sorted(ref.DT)


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


def part_objects(s):
    """The golden parts as signal objects made on the host (the generating classes map their bits on the device)."""
    return [signals.SignalQAM(s[p].copy(), M, coded_symbols=s[c], symbols=s[p].copy()) for p, c, M in (("part1", "coded1", s["M"][0]), ("part2", "coded2", s["M"][1]))]


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["qh_tdh_assemble_c64_dev"]) == 11 and len(_lib.SIGNATURES["qh_tdh_class_sums_c128_dev"]) == 5
    assert len(_lib.SIGNATURES["qh_tdh_align_dev"]) == 6 and len(_lib.SIGNATURES["qh_tdh_split_c64_dev"]) == 10
    assert len(_lib.SIGNATURES["qh_tdh_metrics_c128_dev"]) == 14
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "hybrid" in units


def test_signatures_of_the_public_forms():
    p = inspect.signature(signals.TDHQAMSymbols.__new__).parameters
    assert [(k, v.default) for k, v in p.items() if k not in ("cls", "kwargs")] == [
        ("M", inspect.Parameter.empty), ("N", inspect.Parameter.empty), ("fr", 0.5), ("power_method", "dist"), ("M1class", signals.SignalQAMGrayCoded),
        ("M2class", signals.SignalQAMGrayCoded)]
    p = inspect.signature(signals.ResampledQAM.__new__).parameters
    assert [(k, v.default) for k, v in p.items() if k not in ("cls", "kwargs")] == [
        ("M", inspect.Parameter.empty), ("N", inspect.Parameter.empty), ("fb", 1), ("fs", 1), ("resamplekwargs", {"beta": 0.1})]
    for fn in (signals.TDHQAMSymbols.cal_ser, signals.TDHQAMSymbols.cal_ber, signals.TDHQAMSymbols.cal_evm):
        q = inspect.signature(fn).parameters
        assert [(k, v.default) for k, v in q.items() if k != "self"] == [("signal_rx", None), ("synced", True), ("method", "pyt")]
    assert inspect.signature(signals.TDHQAMSymbols.divide).parameters["method"].default == "pyt"
    assert inspect.signature(signals.TDHQAMSymbols.cal_gmi).parameters["snr"].default is None
    assert inspect.signature(hip_dsp.tdh_divide).parameters["method"].default == "pyt"
    p = inspect.signature(synth.make_tdh_symbols_dev).parameters
    assert [(k, v.default) for k, v in p.items()] == [("M", inspect.Parameter.empty), ("nsym", inspect.Parameter.empty), ("fr", inspect.Parameter.empty),
                                                      ("nmodes", 2), ("order", (15, 23)), ("seed", (None, None)), ("kind", "ext"), ("dtype", np.complex64)]
    assert issubclass(signals.SignalPSKGrayCoded, signals.SignalQAMGrayCoded) and issubclass(signals.ResampledQAM, signals.SignalQAMGrayCoded)


def test_geometry_and_power_ratio():
    g = ref.gold()
    for k, fr in enumerate(g["tdh_fr"]):
        want = tuple(int(v) for v in g["t%d_n1_geometry" % k])
        assert hip_dsp.tdh_geometry(fr) == want == signals.TDHQAMSymbols._cal_fractions(fr)
    assert hip_dsp.tdh_geometry(1 / 257) == (257, 256, 1)                    # the geometry itself has no limit: the device forms have
    for prefix in PREFIXES:
        for dt in DTS:
            s = ref.golden_signal(prefix, dt)
            assert hip_dsp.tdh_power_ratio(s["coded1"], s["coded2"]) == s["powratio"] == signals.TDHQAMSymbols.calculate_power_ratio(s["coded1"], s["coded2"])
    with pytest.raises(NotImplementedError):
        hip_dsp.tdh_power_ratio(np.ones(4), np.ones(4), "power")


def test_a_frame_the_device_forms_cannot_take_is_refused(no_library):
    c = np.complex64
    fM, fM1, _ = hip_dsp.tdh_geometry(1 / 257)
    E, S, I = _Stub((2, 257 * 4), c), _Stub((2, 257), np.float64), _Stub((2, 257 * 4), np.int32)
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_class_sums_dev(E, fM)
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_align_dev(S, fM1, (16, 4))
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_split_dev(E, fM, fM1, 5.0, _Stub((2, 1024), c, 2), _Stub((2, 4), c, 3))
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_assemble_dev(_Stub((2, 1024), c, 2), _Stub((2, 4), c, 3), fM, fM1, 5.0, E)
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_metrics_dev(E, I, fM, fM1, 5.0, _Stub((16,), c), _Stub((4,), c))
    with pytest.raises(ValueError, match="256"):
        synth.make_tdh_symbols_dev((16, 4), 1028, 1 / 257)
    with pytest.raises(ValueError, match="256"):
        hip_dsp.tdh_divide(np.ones((1, 257), c), 1 / 257, (16, 4), 5.0, method="hip")
    for fM in (1, 2.5, 0, -4):                                             # no frame at all
        with pytest.raises(ValueError):
            hip_dsp.tdh_class_sums_dev(_Stub((2, 40), c), fM)
    for fM1 in (0, 4, 5, 1.5):                                             # one of the formats without a place in it
        with pytest.raises(ValueError):
            hip_dsp.tdh_split_dev(_Stub((2, 40), c), 4, fM1, 5.0, _Stub((2, 30), c, 2), _Stub((2, 10), c, 3))


def test_rows_of_broken_frames_are_refused(no_library):
    c = np.complex128
    E = _Stub((2, 41), c)
    with pytest.raises(ValueError, match="whole frames"):
        hip_dsp.tdh_class_sums_dev(E, 4)
    with pytest.raises(ValueError, match="whole frames"):
        hip_dsp.tdh_split_dev(E, 4, 3, 5.0, _Stub((2, 30), c, 2), _Stub((2, 10), c, 3))
    with pytest.raises(ValueError, match="whole frames"):
        hip_dsp.tdh_metrics_dev(E, _Stub((2, 41), np.int32), 4, 3, 5.0, _Stub((16,), c), _Stub((4,), c))
    for method in ("pyt", "hip"):
        with pytest.raises(ValueError, match="whole frames"):
            hip_dsp.tdh_divide(np.ones((2, 41), c), 0.25, (16, 4), 5.0, method=method)
    with pytest.raises(ValueError, match="method"):
        hip_dsp.tdh_divide(np.ones((2, 40), c), 0.25, (16, 4), 5.0, method="cuda")


def test_mismatched_modes_dtypes_and_buffers_are_refused(no_library):
    c, d = np.complex64, np.complex128
    E = _Stub((2, 40), c)
    p1, p2 = _Stub((2, 30), c, 2), _Stub((2, 10), c, 3)
    l1, l2, I = _Stub((2, 30), np.int32), _Stub((2, 10), np.int32), _Stub((2, 40), np.int32)
    a1, a2 = _Stub((16,), c), _Stub((4,), c)
    for kw in (dict(part1=_Stub((1, 30), c)), dict(part2=_Stub((3, 10), c)), dict(part1=_Stub((2, 30), d)), dict(part2=_Stub((2, 10), d)),
               dict(part1=_Stub((2, 31), c)), dict(labels1=l1), dict(labels1=l1, labels2=l2),
               dict(labels1=l1, labels2=l2, idx_out=_Stub((2, 40), np.int64)), dict(labels1=_Stub((2, 10), np.int32), labels2=l2, idx_out=I),
               dict(powratio=0.0), dict(powratio=float("nan")), dict(powratio=-1.0)):
        a = dict(part1=p1, part2=p2, out=E, powratio=5.0)
        a.update(kw)
        with pytest.raises(ValueError):
            hip_dsp.tdh_assemble_dev(a.pop("part1"), a.pop("part2"), 4, 3, a.pop("powratio"), a.pop("out"), **a)
    for kw in (dict(part1=_Stub((1, 30), c, 2)), dict(part2=_Stub((2, 10), d, 3)), dict(part1=_Stub((2, 30), c, 1)), dict(shift=_Stub((3,), np.int32)),
               dict(shift=_Stub((2,), np.int64)), dict(shift=0.5), dict(shift=[1, 2]), dict(powratio=0.0)):
        a = dict(part1=p1, part2=p2, powratio=5.0, shift=0)
        a.update(kw)
        with pytest.raises(ValueError):
            hip_dsp.tdh_split_dev(E, 4, 3, a["powratio"], a["part1"], a["part2"], a["shift"])
    for kw in (dict(idx_tx=_Stub((1, 40), np.int32)), dict(idx_tx=_Stub((2, 40), np.int64)), dict(alphabet1=_Stub((16,), d)), dict(alphabet2=_Stub((2048,), c)),
               dict(alphabet1=_Stub((4, 4), c)), dict(sums=_Stub((2, 4), np.float64)), dict(sums=_Stub((2, 8), np.float32)), dict(shift=_Stub((1,), np.int32))):
        a = dict(idx_tx=I, alphabet1=a1, alphabet2=a2, shift=0, sums=None)
        a.update(kw)
        with pytest.raises(ValueError):
            hip_dsp.tdh_metrics_dev(E, a["idx_tx"], 4, 3, 5.0, a["alphabet1"], a["alphabet2"], a["shift"], a["sums"])
    for real in (np.float32, np.float64):                                   # not a complex field at all: a TypeError, as everywhere in hip_dsp
        with pytest.raises(TypeError):
            hip_dsp.tdh_class_sums_dev(_Stub((2, 40), real), 4)
        with pytest.raises(TypeError):
            hip_dsp.tdh_assemble_dev(p1, p2, 4, 3, 5.0, _Stub((2, 40), real))
    with pytest.raises(ValueError):
        hip_dsp.tdh_class_sums_dev(E, 4, _Stub((2, 5), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.tdh_align_dev(_Stub((2, 4), np.float32), 3, (16, 4))
    with pytest.raises(ValueError):
        hip_dsp.tdh_align_dev(_Stub((2, 4), np.float64), 4, (16, 4))


def test_the_library_checks_its_arguments_before_the_device():
    """QH_REQUIRE: a bad geometry handed straight to the C entry points is an argument error - a ValueError - with or without a device."""
    with pytest.raises(ValueError, match="whole frames"):
        _lib.call("qh_tdh_class_sums_c64_dev", 1, 1, 41, 4, 1)
    with pytest.raises(ValueError, match="2 .. 256"):
        _lib.call("qh_tdh_class_sums_c128_dev", 1, 1, 257 * 2, 257, 1)
    with pytest.raises(ValueError, match="fM1"):
        _lib.call("qh_tdh_split_c64_dev", 1, 1, 40, 4, 4, 5.0, None, 0, 2, 3)
    with pytest.raises(ValueError, match="must not be E"):
        _lib.call("qh_tdh_split_c64_dev", 1, 1, 40, 4, 3, 5.0, None, 0, 1, 3)
    with pytest.raises(ValueError, match="powratio"):
        _lib.call("qh_tdh_metrics_c64_dev", 1, 1, 40, 4, 3, 0.0, None, 0, 2, 3, 16, 4, 4, 5)
    with pytest.raises(ValueError, match="1024"):
        _lib.call("qh_tdh_metrics_c128_dev", 1, 1, 40, 4, 3, 5.0, None, 0, 2, 3, 2048, 4, 4, 5)
    with pytest.raises(ValueError, match="come together"):
        _lib.call("qh_tdh_assemble_c64_dev", 1, 2, 3, None, 1, 10, 4, 3, 5.0, 4, None)
    with pytest.raises(ValueError, match="nmodes"):
        _lib.call("qh_tdh_align_dev", 1, 0, 4, 3, 1, 2)


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    c = np.complex64
    hip_dsp.tdh_assemble_dev(_Stub((2, 30), c, 10), _Stub((2, 10), c, 20), 4, 3, 5.0, _Stub((2, 40), c, 30), _Stub((2, 30), np.int32, 40),
                             _Stub((2, 10), np.int32, 50), _Stub((2, 40), np.int32, 60))
    hip_dsp.tdh_class_sums_dev(_Stub((3, 40), np.complex128, 10), 10, _Stub((3, 10), np.float64, 20))
    hip_dsp.tdh_align_dev(_Stub((3, 10), np.float64, 20), 7, (16, 4), _Stub((3,), np.int32, 30))
    hip_dsp.tdh_align_dev(_Stub((3, 10), np.float64, 20), 7, (16, 16), _Stub((3,), np.int32, 30))            # M1 == M2: format 2 is the reference's branch
    hip_dsp.tdh_split_dev(_Stub((2, 40), c, 10), 4, 1, 0.2, _Stub((2, 10), c, 20), _Stub((2, 30), c, 30), _Stub((2,), np.int32, 40))
    hip_dsp.tdh_split_dev(_Stub((2, 40), c, 10), 4, 1, 0.2, _Stub((2, 10), c, 20), _Stub((2, 30), c, 30), 3)
    hip_dsp.tdh_metrics_dev(_Stub((2, 40), c, 10), _Stub((2, 40), np.int32, 20), 4, 3, 5.0, _Stub((16,), c, 30), _Stub((4,), c, 40), _Stub((2,), np.int32, 50),
                            _Stub((2, 8), np.float64, 60))
    assert seen == [("qh_tdh_assemble_c64_dev", 10, 20, 40, 50, 2, 10, 4, 3, 5.0, 30, 60),
                    ("qh_tdh_class_sums_c128_dev", 10, 3, 40, 10, 20),
                    ("qh_tdh_align_dev", 20, 3, 10, 7, 1, 30),
                    ("qh_tdh_align_dev", 20, 3, 10, 7, 0, 30),
                    ("qh_tdh_split_c64_dev", 10, 2, 40, 4, 1, 0.2, 40, 0, 20, 30),
                    ("qh_tdh_split_c64_dev", 10, 2, 40, 4, 1, 0.2, None, 3, 20, 30),
                    ("qh_tdh_metrics_c64_dev", 10, 2, 40, 4, 3, 5.0, 50, 0, 20, 30, 16, 40, 4, 60)]


# ---- TDHQAMSymbols on the host
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("prefix", PREFIXES)
def test_from_symbol_arrays_gives_the_reference_array(prefix, dt):
    s = ref.golden_signal(prefix, dt)
    p1, p2 = part_objects(s)
    sig = signals.TDHQAMSymbols.from_symbol_arrays(p1, p2, s["fM2"] / s["fM"])
    assert isinstance(sig, signals.TDHQAMSymbols) and sig.dtype == ref.DT[dt]
    assert np.array_equal(np.asarray(sig), s["row"]) and sig.powratio == s["powratio"]
    assert np.array_equal(np.asarray(sig.symbols_M1), s["part1"]) and np.array_equal(np.asarray(sig.symbols_M2), s["part2_scaled"])
    assert np.array_equal(np.asarray(p2), s["part2"])                        # the caller's part is left as it was
    assert (sig.f_M, sig.f_M1, sig.f_M2) == (s["fM"], s["fM1"], s["fM2"]) and sig.M == s["M"] and sig.fb == sig.fs == 1 and sig.fr == s["fM2"] / s["fM"]


@pytest.mark.parametrize("dt", DTS)
def test_the_constructor_gives_the_reference_array(dt):
    """``TDHQAMSymbols(M, N, fr, ...)`` with part classes that hand out the golden parts (on a GPU the Gray-coded classes make them)."""
    g = ref.gold()
    for k in range(4):
        s = ref.golden_signal("t%d_n2_" % k, dt)
        parts = dict(zip(s["M"], part_objects(s))) if s["M"][0] != s["M"][1] else None
        made = []

        def part_class(M, N, **kwargs):
            made.append((M, N, kwargs))
            return parts[M]
        N = int(g["tdh_cases"][k][2])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            sig = signals.TDHQAMSymbols(s["M"], N, fr=float(g["tdh_fr"][k]), M1class=part_class, M2class=part_class, nmodes=2, seed=5)
        assert made == [(s["M"][0], N // s["fM"] * s["fM1"], dict(nmodes=2, seed=5)), (s["M"][1], N // s["fM"] * s["fM2"], dict(nmodes=2, seed=5))]
        assert np.array_equal(np.asarray(sig), s["row"]) and sig.powratio == s["powratio"] and sig.shape == (2, N)


def test_truncation_warns_and_keeps_whole_frames():
    s = ref.golden_signal("t3_n1_", "c128")                                 # (16, 4), 40 symbols, frames of 3 + 1
    p1, p2 = part_objects(s)
    with pytest.warns(UserWarning, match="truncating to 40"):
        sig = signals.TDHQAMSymbols((16, 4), 43, fr=0.25, M1class=lambda M, N: p1, M2class=lambda M, N: p2)
    assert sig.shape == (1, 40) and np.array_equal(np.asarray(sig), s["row"])
    # parts that do not fill whole frames: the reference fails on a shape mismatch, here each part is cut
    p1, p2 = part_objects(s)
    short = p2.recreate_from_np_array(np.array(p2)[:, :8], symbols=np.array(p2)[:, :8])
    with pytest.warns(UserWarning, match="truncate"):
        sig = signals.TDHQAMSymbols.from_symbol_arrays(p1, short, 0.25)
    assert sig.shape == (1, 32) and np.array_equal(np.asarray(sig), s["row"][:, :32])
    assert sig.symbols_M1.shape == (1, 24) and sig.symbols_M2.shape == (1, 8) and sig.symbols_M1.symbols.shape == (1, 24)


def test_class_attributes_survive_slicing_arithmetic_and_recreation():
    s = ref.golden_signal("tfs_", "c64")
    sig = signals.TDHQAMSymbols.from_symbol_arrays(*part_objects(s), 0.3)
    for other in (sig[:, :20], sig[0], sig * 2, sig + sig, np.roll(sig, 3, axis=-1), sig.copy(), sig.recreate_from_np_array(np.zeros((2, 100), np.complex64))):
        assert isinstance(other, signals.TDHQAMSymbols)
        assert other.powratio == sig.powratio and other.fr == 0.3 and other.M == (16, 4) and (other.f_M, other.f_M1, other.f_M2) == (10, 7, 3)
        assert other.symbols_M1 is sig.symbols_M1 and other.symbols_M2 is sig.symbols_M2 and other.fb == 1 and other.fs == 1
    faster = sig.recreate_from_np_array(np.zeros((2, 100), np.complex64), fb=2)
    assert faster.fb == 2 and faster.fs == 2 and faster.powratio == sig.powratio
    with pytest.raises(NotImplementedError):
        sig._modulate()
    with pytest.raises(NotImplementedError):
        sig._demodulate()


@pytest.mark.parametrize("dt", DTS)
def test_the_host_divide_and_metrics_follow_the_restatement(dt):
    for case in ref.CASES:
        s, x, labels, shifts = ref.received(case, 2, dt)
        sig = signals.TDHQAMSymbols.from_symbol_arrays(*part_objects(s), s["fM2"] / s["fM"])
        p1, p2, got = sig.divide(x, return_shifts=True)
        w1, w2 = ref.split(x, s["fM"], s["fM1"], s["powratio"], shifts)
        assert list(got) == list(shifts) and np.array_equal(np.asarray(p1), w1.astype(x.dtype))
        assert np.abs(np.asarray(p2) - w2).max() <= np.finfo(x.dtype).eps * np.abs(w2).max()
        assert type(p1) is signals.SignalQAM and p1.M == s["M"][0] and p2.M == s["M"][1] and np.array_equal(p2.symbols, s["part2"])
        want = ref.rates(ref.metrics(x, labels, s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], shifts)[0], s["M"])
        # the same rows as they were sent are in step with the transmitted parts (synced); the rolled ones come out a frame late and are not
        _, x0, _, zero = ref.received(case, 2, dt, rolled=False)
        assert not zero.any() and list(sig.divide(x0, return_shifts=True)[2]) == [0, 0]
        for key, fn in (("ser", sig.cal_ser), ("ber", sig.cal_ber), ("evm", sig.cal_evm)):
            for rows, synced in ((x0, True), (x, False)):
                per, both = fn(rows, synced=synced)
                assert per.shape == (2, 2) and both.shape == (2,)
                if key == "evm":
                    assert np.allclose(per, want[key][0], rtol=1e-6) and np.allclose(both, want[key][1], rtol=1e-6)
                else:
                    assert np.array_equal(per, want[key][0]) and np.array_equal(both, want[key][1])
        assert sig.cal_ser(x)[1].min() > 0.5                                  # aligned to the frame, a frame late against the sequence
        dec = sig.make_decision(x)
        assert dec.shape == x.shape and np.mean(np.roll(dec[0], case["roll"] + case["shift"]) != s["row"][0]) == pytest.approx(want["ser"][1][0], abs=1e-12)
    with pytest.raises(ValueError, match="method"):
        sig.cal_ser(x, method="cuda")
    with pytest.raises(ValueError, match="whole frames"):
        sig.cal_ser(x[:, :-1])


# ---- PSK and resampled signals on the host
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [2, 4, 8, 16])
def test_psk_mapping_is_the_references(M, dt):
    g = ref.gold()
    coded = signals.SignalPSKGrayCoded._alphabet(M, ref.DT[dt])
    assert coded.dtype == ref.DT[dt] and np.array_equal(coded, g["psk%d_%s_coded" % (M, dt)])
    assert np.array_equal(signals.SignalPSKGrayCoded._alphabet(M, ref.DT[dt], power=2.0), coded)          # like the reference's mapping: the circle, whatever the power
    labels, bits = g["psk%d_labels" % M].astype(np.int64), g["psk%d_bits" % M]
    # neighbours on the circle differ in one bit
    order = np.argsort(np.angle(coded.astype(np.complex128) * np.exp(-1j * np.angle(coded[0]))) % (2 * np.pi))
    assert all(bin(int(a ^ b)).count("1") == 1 for a, b in zip(order, np.roll(order, 1)))
    # bits <-> labels, MSB first (the host half of demodulate), and BPSK's modulation, which stays on the host
    sig = signals.SignalQAM.__new__(signals.SignalPSKGrayCoded, coded[labels], M, coded_symbols=coded)
    assert np.array_equal(sig.demodulate(labels), bits)
    if M == 2:
        assert np.array_equal(signals.SignalPSKGrayCoded._modulate(bits, coded), coded[labels])
        made = signals.SignalPSKGrayCoded.from_bit_array(bits, 2, dtype=ref.DT[dt])
        assert isinstance(made, signals.SignalPSKGrayCoded) and np.array_equal(np.asarray(made), coded[labels]) and np.array_equal(made.symbols, coded[labels])
        assert np.array_equal(made.coded_symbols, coded) and made.M == 2 and made.Nbits == 1


@pytest.mark.parametrize("dt", DTS)
def test_resampled_row_is_the_plain_resampling_of_its_symbols(dt):
    """What ``ResampledQAM`` is thin over: the golden row is the root-raised-cosine resampling of the golden symbols (bars of
    tests/test_resample_host.py for the restatement in double; the complex64 row carries its storage rounding)."""
    g = ref.gold()
    fb, fs, beta, taps = g["rs_params"]
    sym = g["rs_%s_coded" % dt][g["rs_labels"]]
    want = g["rs_%s_out" % dt]
    got = np.array([resample_ref.rrcos_resample(row.astype(np.complex128), fb, fs, Ts=1 / fb, beta=beta, taps=int(taps), fftconv=True) for row in sym])
    assert got.shape == want.shape == (2, 256)
    err = np.abs(got - want).max() / np.sqrt(np.mean(np.abs(want) ** 2))
    assert err <= (1e-12 if dt == "c128" else 1e-5), err
    with pytest.raises(NotImplementedError, match="taps=None"):
        signals.SignalQAM(sym, 16, fb=fb, symbols=sym).resample(fs, beta=0.1, taps=None)
