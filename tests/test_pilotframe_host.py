"""CPU checks of the Python layers of the pilot frames (csrc/pilot.hip): the entry points' place in the C ABI, the geometry rule against
``PilotSignal._cal_pilot_idx``, the argument checks - which run before the library is touched -, what the device wrappers hand down and the
signatures of the mirrored API."""
import inspect
import os
import re
import threading

import numpy as np
import pytest

from conftest import ROOT
from qampy_amd import _lib, phaserec, signals, synth
from qampy_amd.core import hip_dsp, pilotbased_receiver

NEW = ["qh_pilot_frame_c64_dev", "qh_pilot_frame_c128_dev", "qh_pilot_split_c64_dev", "qh_pilot_split_c128_dev", "qh_pilot_phase_c64_dev",
       "qh_pilot_phase_c128_dev", "qh_pilot_knots_dev", "qh_pilot_cpe_c64_dev", "qh_pilot_cpe_c128_dev", "qh_pilot_foe_c64_dev", "qh_pilot_foe_c128_dev",
       "qh_pilot_const_phase_c64_dev", "qh_pilot_const_phase_c128_dev", "qh_rotate_rows_c64_dev", "qh_rotate_rows_c128_dev"]


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


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["qh_pilot_frame_c64_dev"]) == 12 and len(_lib.SIGNATURES["qh_pilot_split_c128_dev"]) == 10
    assert len(_lib.SIGNATURES["qh_pilot_phase_c64_dev"]) == 12 and len(_lib.SIGNATURES["qh_pilot_cpe_c128_dev"]) == 14
    assert len(_lib.SIGNATURES["qh_pilot_knots_dev"]) == 9 and len(_lib.SIGNATURES["qh_pilot_foe_c64_dev"]) == 7
    assert len(_lib.SIGNATURES["qh_pilot_const_phase_c64_dev"]) == 5 and len(_lib.SIGNATURES["qh_rotate_rows_c128_dev"]) == 5
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "pilot" in units


@pytest.mark.parametrize("fn", [pilotbased_receiver.pilot_based_cpe_new, pilotbased_receiver.pilot_based_foe, phaserec.pilot_cpe,
                                phaserec.find_pilot_const_phase, signals.PilotSignal.get_data, signals.PilotSignal.extract_pilots])
def test_the_host_path_stays_the_default(fn):
    assert inspect.signature(fn).parameters["method"].default == "pyt"


def test_signatures_of_the_generators():
    p = inspect.signature(signals.SignalWithPilots.__new__).parameters
    assert [(k, v.default) for k, v in p.items() if k not in ("cls", "kwargs")] == [
        ("M", inspect.Parameter.empty), ("frame_len", inspect.Parameter.empty), ("pilot_seq_len", inspect.Parameter.empty),
        ("pilot_ins_rat", inspect.Parameter.empty), ("nframes", 1), ("pilot_scale", 1), ("Mpilots", 4), ("dataclass", signals.SignalQAMGrayCoded),
        ("nmodes", 1), ("dtype", np.complex128), ("repeat_data", True), ("repeat_pilots", True)]
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD and issubclass(signals.SignalWithPilots, signals.PilotSignal)
    p = inspect.signature(signals.SignalWithPilots.from_symbol_array).parameters
    assert [p[k].default for k in ("pilots", "pilot_idx", "nframes", "pilot_scale", "payload_is_frame")] == [None, None, 1, 1, False]
    p = inspect.signature(synth.make_pilot_frames_dev).parameters
    assert [(k, v.default) for k, v in p.items()] == [
        ("M", inspect.Parameter.empty), ("frame_len", inspect.Parameter.empty), ("seq_len", inspect.Parameter.empty), ("ins_rat", inspect.Parameter.empty),
        ("nframes", 1), ("nmodes", 2), ("Mpilots", 4), ("order", (15, 23)), ("seed", (None, None)), ("dtype", np.complex64), ("repeat_data", True)]


GRID = [(F, S, R) for F in (1, 2, 7, 12, 96, 100) for S in (0, 1, 3, 4, 12) for R in (0, None, 2, 3, 4, 32) if S <= F and (not R or (F - S) % R == 0)]


def test_the_grid_has_the_corners():
    assert any(not R for F, S, R in GRID) and any(R == 2 for F, S, R in GRID) and any(S == 0 and R for F, S, R in GRID) and len(GRID) > 60


@pytest.mark.parametrize("F,S,R", GRID)
def test_the_rule_is_the_index_table(F, S, R):
    _, idx_dat, idx_pil = signals.PilotSignal._cal_pilot_idx(F, S, R)
    NP, ND = hip_dsp.pilot_counts(F, S, R)
    assert (NP, ND) == (np.count_nonzero(idx_pil), np.count_nonzero(idx_dat))
    pil, ordinal = hip_dsp.pilot_ordinals(F, S, R)
    assert np.array_equal(pil, idx_pil)
    assert np.array_equal(ordinal[idx_pil], np.arange(NP)) and np.array_equal(ordinal[idx_dat], np.arange(ND))
    pos_p, pos_d = hip_dsp.pilot_positions(F, S, R)
    assert np.array_equal(pos_p, np.flatnonzero(idx_pil)) and np.array_equal(pos_d, np.flatnonzero(idx_dat))


BAD_GEOMETRY = [(100, 10, 1), (100, 10, 7), (10, 11, 0), (10, -1, 3), (0, 0, 0), (16, 0, -2)]


@pytest.mark.parametrize("F,S,R", BAD_GEOMETRY)
def test_a_bad_geometry_is_refused_everywhere(no_library, F, S, R):
    c = np.complex64
    with pytest.raises(ValueError):
        hip_dsp.pilot_counts(F, S, R)
    with pytest.raises(ValueError):
        hip_dsp.pilot_frame_dev(_Stub((2, 4), c), _Stub((2, 4), c), F, S, R, 1, _Stub((2, max(F, 1)), c))
    with pytest.raises(ValueError):
        hip_dsp.pilot_split_dev(_Stub((2, 4 * max(F, 1)), c), F, S, R, None, payload=_Stub((2, 4), c))
    with pytest.raises(ValueError):
        signals.SignalWithPilots(16, F, S, R)
    with pytest.raises(ValueError):
        synth.make_pilot_frames_dev(16, F, S, R)


def test_what_the_reference_cannot_do_is_refused(no_library):
    with pytest.raises(ValueError, match="repeat_pilots"):
        signals.SignalWithPilots(16, 64, 8, 8, nframes=2, repeat_pilots=False)
    with pytest.raises(NotImplementedError, match="pilot_idx"):
        signals.SignalWithPilots.from_symbol_array(np.zeros((1, 64), np.complex128), 64, 8, 8, pilot_idx=[0, 1, 2])
    for fn, args in ((pilotbased_receiver.pilot_based_foe, (np.ones((1, 8), complex), np.ones((1, 8), complex))),
                     (phaserec.find_pilot_const_phase, (np.ones((1, 8), complex), np.ones((1, 8), complex))),
                     (pilotbased_receiver.pilot_based_cpe_new, (np.ones((1, 64), complex), np.ones((1, 8), complex), np.arange(8), 64))):
        with pytest.raises(ValueError, match="method"):
            fn(*args, method="cuda")
    sig = signals.PilotSignal(np.ones((1, 64), np.complex64), 16, 1., 1., 32, 4, 4, np.ones((1, 11), np.complex64))
    with pytest.raises(ValueError, match="method"):
        sig.get_data(method="cuda")


def test_frame_buffers_are_checked(no_library):
    c = np.complex64
    F, S, R, nfr = 32, 4, 4, 3                                   # NP = 11, ND = 21
    good = dict(pilots=_Stub((2, 11), c), payload=_Stub((2, 21), c), frame=_Stub((2, 96), c))

    def run(**kw):
        a = dict(good, **{k: v for k, v in kw.items() if k in good})
        rest = {k: v for k, v in kw.items() if k not in good}
        return hip_dsp.pilot_frame_dev(a["pilots"], a["payload"], F, S, R, nfr, a["frame"], **rest)
    for kw in (dict(pilots=_Stub((2, 12), c)), dict(pilots=_Stub((2, 11), np.complex128)), dict(payload=_Stub((2, 63), c)), dict(payload=_Stub((1, 21), c)),
               dict(frame=_Stub((2, 95), c)), dict(payload=_Stub((2, 21), c), repeat_data=False), dict(labels=_Stub((2, 21), np.int32)),
               dict(labels=_Stub((2, 21), np.int64), idx_frame=_Stub((2, 96), np.int32)), dict(labels=_Stub((2, 21), np.int32), idx_frame=_Stub((2, 21), np.int32)),
               dict(pilot_scale=float("nan"))):
        with pytest.raises((ValueError, TypeError)):
            run(**kw)
    with pytest.raises((ValueError, TypeError)):
        hip_dsp.pilot_frame_dev(good["pilots"], good["payload"], F, S, R, 0, good["frame"])
    with pytest.raises((ValueError, TypeError)):
        hip_dsp.pilot_frame_dev(_Stub((2, 11), np.float32), _Stub((2, 21), np.float32), F, S, R, nfr, _Stub((2, 96), np.float32))


@pytest.mark.parametrize("frames", [[3], [0, 3], [-1], [], [[0, 1]], [0.5]])
def test_a_frame_outside_the_signal_is_refused(no_library, frames):
    c = np.complex128
    E = _Stub((2, 3 * 32 + 20), c)                               # three whole frames and a piece
    with pytest.raises(ValueError):
        hip_dsp.pilot_split_dev(E, 32, 4, 4, frames, payload=_Stub((2, 21 * max(np.size(frames), 1)), c))


def test_split_buffers_are_checked(no_library):
    c = np.complex128
    E = _Stub((2, 96), c)
    for kw in (dict(), dict(payload=_Stub((2, 42), c)), dict(pilots=_Stub((2, 33), np.complex64)), dict(payload=_Stub((2, 63), c), pilots=_Stub((2, 32), c))):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.pilot_split_dev(E, 32, 4, 4, None, **kw)
    with pytest.raises(ValueError):
        hip_dsp.pilot_split_dev(_Stub((96,), c), 32, 4, 4, None, payload=_Stub((63,), c))


def test_estimates_check_their_arguments(no_library):
    c, F = np.complex64, 32
    E, sent, where = _Stub((2, 96), c), _Stub((2, 11), c), np.array([0, 1, 2, 3, 4, 8, 12, 16, 20, 24, 28])
    n = 33
    ok = dict(E=E, where=where, F=F, nframes=3, sent=sent, N=5, Eout=_Stub((2, 96), c), trace=_Stub((2, 96), np.float32))
    for kw in (dict(N=4), dict(N=1), dict(N=1025), dict(N=35), dict(where=where[::-1]), dict(where=np.array([0, 0, 4])), dict(where=np.array([0, 32])),
               dict(where=np.array([-1, 3])), dict(where=np.zeros(0, np.int64)), dict(where=np.array([0.5, 2.0])), dict(sent=_Stub((1, 11), c)),
               dict(sent=_Stub((2, 11), np.complex128)), dict(nframes=0), dict(F=0), dict(span=0), dict(span=97), dict(Eout=_Stub((2, 95), c)),
               dict(trace=_Stub((2, 96), np.float64)), dict(E=_Stub((96,), c)), dict(span=40, Eout=_Stub((2, 96), c))):
        a = dict(ok, **kw)
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.pilot_cpe_dev(a["E"], a["where"], a["F"], a["nframes"], a["sent"], a["N"], a["Eout"], a["trace"], span=a.get("span"))
    assert hip_dsp.pilot_used(where, F, 3, 96) == n and hip_dsp.pilot_used(where, F, 3, 64 + 9) == 22 + 6 and hip_dsp.pilot_used(where, F, 2, 96) == 22
    for ph in (_Stub((2, 32), np.float64), _Stub((2, 33), np.float32), _Stub((1, 33), np.float64)):
        with pytest.raises(ValueError):
            hip_dsp.pilot_phase_dev(E, where, F, 3, sent, ph)
    with pytest.raises(ValueError):
        hip_dsp.pilot_phase_dev(E, where[5:], F, 1, sent, _Stub((2, 1), np.float64), span=8)          # no pilot below 8
    rec, ref = _Stub((2, 40), c), _Stub((2, 40), c)
    fit, fo = _Stub((2, 2), np.float64), _Stub((2,), np.float64)
    for a in ((rec, _Stub((2, 39), c), fit, fo), (rec, _Stub((2, 40), np.complex128), fit, fo), (rec, ref, _Stub((2, 3), np.float64), fo),
              (rec, ref, fit, _Stub((3,), np.float64)), (_Stub((2, 1), c), _Stub((2, 1), c), fit, fo)):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.pilot_foe_dev(*a)
    with pytest.raises(ValueError):
        hip_dsp.pilot_const_phase_dev(rec, ref, _Stub((2,), np.float32))
    with pytest.raises(ValueError):
        hip_dsp.rotate_rows_dev(rec, _Stub((3,), np.float64), rec)
    with pytest.raises(ValueError):
        hip_dsp.rotate_rows_dev(rec, fo, _Stub((2, 41), c))
    for N in (2, 4, 1025):
        with pytest.raises(ValueError):
            hip_dsp.pilot_knots_dev(_Stub((2, 2000), np.float64), N, _Stub((2, 2001 - N), np.float64))
    # the host-array forms check before they upload
    with pytest.raises(ValueError):
        hip_dsp.pilot_cpe(np.zeros((2, 96), c), np.zeros((2, 11), c), where, F, 3, 4)
    with pytest.raises(ValueError):
        hip_dsp.pilot_cpe(np.zeros((2, 96), c), np.zeros((2, 11), c), where[::-1], F, 3, 5)
    with pytest.raises(TypeError):
        hip_dsp.pilot_cpe(np.zeros((2, 96)), np.zeros((2, 11), c), where, F, 3, 5)
    with pytest.raises(ValueError):
        hip_dsp.pilot_foe(np.zeros((2, 1), c), np.zeros((2, 1), c))
    with pytest.raises(ValueError):
        hip_dsp.pilot_foe(np.zeros((2, 9), c), np.zeros((2, 8), c))


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    monkeypatch.setattr(_lib.DeviceArray, "from_host", classmethod(lambda cls, arr: _Stub(arr.shape, arr.dtype, 77)))
    monkeypatch.setattr(hip_dsp.pilot, "_PILOT_TABLES", threading.local())          # (the stand-in tables must not outlive this test)
    c = np.complex64
    hip_dsp.pilot_frame_dev(_Stub((2, 11), c, 10), _Stub((2, 63), c, 20), 32, 4, 4, 3, _Stub((2, 96), c, 30), pilot_scale=1.5, repeat_data=False,
                            labels=_Stub((2, 63), np.int32, 40), idx_frame=_Stub((2, 96), np.int32, 50))
    assert hip_dsp.pilot_split_dev(_Stub((2, 100), np.complex128, 10), 32, 4, 4, [2, 0], pilots=_Stub((2, 22), np.complex128, 30)) == 2
    where = np.array([0, 8, 16])
    assert hip_dsp.pilot_cpe_dev(_Stub((1, 70), c, 10), where, 32, 3, _Stub((1, 5), c, 20), 7, _Stub((1, 70), c, 30), _Stub((1, 70), np.float32, 40)) == 7
    hip_dsp.pilot_foe_dev(_Stub((3, 9), c, 10), _Stub((3, 9), c, 20), _Stub((3, 2), np.float64, 30), _Stub((3,), np.float64, 40), average=True)
    hip_dsp.rotate_rows_dev(_Stub((3, 9), np.complex128, 10), _Stub((3,), np.float64, 20), _Stub((3, 9), np.complex128, 10))
    assert seen == [("qh_pilot_frame_c64_dev", 10, 20, 40, 2, 32, 4, 4, 3, 1, 1.5, 30, 50),
                    ("qh_pilot_split_c128_dev", 10, 2, 100, 32, 4, 4, 77, 2, None, 30),
                    ("qh_pilot_cpe_c64_dev", 10, 1, 70, 77, 3, 3, 32, 70, 7, 20, 5, 7, 30, 40),
                    ("qh_pilot_foe_c64_dev", 10, 20, 3, 9, 1, 30, 40),
                    ("qh_rotate_rows_c128_dev", 10, 3, 9, 20, 10)]


def test_the_mirrored_functions_hand_down_to_the_device_forms(monkeypatch):
    """method="hip": the selection of the pilots stays on the host, the estimate goes to hip_dsp in one call; shapes and dtypes are the host path's."""
    seen = {}

    def cpe(E, sent, where, F, nframes, N):
        seen["cpe"] = (E.dtype, E.shape, sent.shape, list(where), F, nframes, N)
        return np.zeros_like(E), np.zeros(E.shape, E.real.dtype)
    monkeypatch.setattr(hip_dsp, "pilot_cpe", cpe)
    monkeypatch.setattr(hip_dsp, "pilot_foe", lambda rec, ref: (np.arange(2. * rec.shape[0]).reshape(-1, 2), None))
    monkeypatch.setattr(hip_dsp, "pilot_const_phase", lambda rec, ref: np.arange(1. * rec.shape[0]))
    x, refs = np.ones((2, 100), np.complex64), np.ones((2, 11), np.complex128)
    pos = np.flatnonzero(signals.PilotSignal._cal_pilot_idx(32, 4, 4)[2])
    with pytest.warns(UserWarning):
        out, tr = pilotbased_receiver.pilot_based_cpe_new(x, refs, pos, 32, num_average=4, use_pilot_ratio=2, max_num_blocks=8, nframes=2, method="hip")
    assert seen["cpe"] == (np.complex128, (2, 64), (2, 6), list(pos[:8:2]), 32, 2, 5)
    assert out.shape == tr.shape == (2, 64) and out.dtype == tr.dtype == np.complex128
    foe, modes, icpt = pilotbased_receiver.pilot_based_foe(x[:, :11], refs, method="hip")
    assert modes.shape == icpt.shape == (2, 1) and foe == 1.0 and list(icpt[:, 0]) == [1., 3.]
    assert phaserec.find_pilot_const_phase(x[0, :11], refs[0], method="hip").shape == (1, 1)
