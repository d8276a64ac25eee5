"""CPU checks of the Python layers of the digital pre-compensation (csrc/precomp.hip): the entry points' place in the C ABI, the signatures of
the mirrored module against the reference's, the argument checks - which run before the library is touched -, the stated limits and what the
device wrappers hand down."""
import inspect
import os
import re
import threading

import numpy as np
import pytest

from conftest import ROOT
from qampy_amd import _lib
from qampy_amd.core import digital_pre_compensation as dpc
from qampy_amd.core import hip_dsp, impairments

NEW = ["qh_pattern_index_c64_dev", "qh_pattern_index_c128_dev", "qh_lut_accumulate_c64_dev", "qh_lut_accumulate_c128_dev", "qh_lut_apply_c64_dev",
       "qh_lut_apply_c128_dev", "qh_lut_predistort_c64_dev", "qh_lut_predistort_c128_dev", "qh_comp_mod_sin_c64_dev", "qh_comp_mod_sin_c128_dev",
       "qh_dac_preemphasis_table_c64_dev", "qh_dac_preemphasis_table_c128_dev"]

E = inspect.Parameter.empty


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
    monkeypatch.setattr(_lib.DeviceArray, "__init__", refuse)
    monkeypatch.setattr(_lib.DeviceArray, "from_host", classmethod(refuse))


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    sizes = {"qh_pattern_index": 12, "qh_lut_accumulate": 12, "qh_lut_apply": 9, "qh_lut_predistort": 14, "qh_comp_mod_sin": 7, "qh_dac_preemphasis_table": 8}
    for stem, n in sizes.items():
        assert len(_lib.SIGNATURES[stem + "_c64_dev"]) == len(_lib.SIGNATURES[stem + "_c128_dev"]) == n, stem
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11      # additive: unchanged
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "precomp" in units and os.path.exists(os.path.join(ROOT, "qampy_amd", "csrc", "precomp.hip"))


def test_the_mirrored_signatures_are_the_references():
    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]
    assert sig(dpc.clipper) == [("sig", E), ("clipping_level", E)] and dpc.clipper is impairments.clipper
    assert sig(dpc.comp_mod_sin) == [("sig", E), ("vpi", 1.14)]
    assert sig(dpc.comp_dac_resp) == [("dpe_fb", E), ("sim_len", E), ("rrc_beta", E), ("PAPR", 9), ("prms_dac", (16e9, 2, "sos", 6)), ("os", 2)]
    assert sig(dpc.find_sym_patterns) == [("sig", E), ("ref_sym", E), ("N", E), ("ret_ptrns", False)]
    assert sig(dpc.cal_lut) == [("tx_sig", E), ("rx_sig", E), ("ref_sym", E), ("mem_len", 3), ("idx_data", None), ("real_ptrns", True)]
    assert sig(dpc.apply_lut) == [("sig", E), ("ea", E), ("idx_I", E), ("idx_Q", E), ("gain", 1.0)]
    for name in ("pattern_index_dev", "cal_lut_dev", "lut_apply_dev", "lut_predistort_dev", "comp_mod_sin_dev", "comp_dac_resp_dev", "dac_preemphasis_dev"):
        assert callable(getattr(hip_dsp, name)), name
    from qampy_amd import core
    assert core.digital_pre_compensation is dpc


def test_the_levels_follow_cal_lut():
    qam = (np.arange(-3, 4, 2)[:, None] + 1j * np.arange(-3, 4, 2)[None, :]).ravel()[::-1]
    lv = hip_dsp.pattern_levels(qam)
    assert list(lv.lev_I) == list(lv.lev_Q) == [-3, -1, 1, 3] and lv.alphabet is None and lv.M == 4 and lv.N(3) == 64
    lv = hip_dsp.pattern_levels(qam, real_ptrns=False)
    assert np.array_equal(lv.alphabet, np.unique(qam)) and lv.alphabet.dtype == np.complex128 and lv.M == 16 and lv.N(3) == 4096
    rect = np.array([-3, -1, 1, 3])[:, None] + 1j * np.array([-1, 1])[None, :]                  # fewer quadrature levels: M from the in-phase rail
    lv = hip_dsp.pattern_levels(rect.ravel())
    assert lv.M == 4 and lv.lev_Q.size == 2 and lv.N(2) == 16


def test_the_limits(no_library):
    lv2, lv8 = hip_dsp.PatternLevels([-1, 1], [-1, 1]), hip_dsp.PatternLevels(np.arange(8.), np.arange(8.))
    assert lv2.N(15) == 2 ** 15 and lv2.N(1) == 2 and lv8.N(8) == 2 ** 24
    big = hip_dsp.PatternLevels(np.arange(4096.), np.arange(4096.))
    assert big.N(2) == 2 ** 24
    for lv, m in ((lv2, 0), (lv2, 16), (lv2, 2.5), (lv2, True), (lv8, 9), (big, 3)):
        with pytest.raises(ValueError):
            lv.N(m)
    for kw in (dict(lev_I=[1.], lev_Q=[1.]), dict(lev_I=np.arange(4097.), lev_Q=[0., 1.]), dict(lev_I=[0., 0.], lev_Q=[0., 1.]), dict(lev_I=[1., 0.], lev_Q=[0., 1.]),
               dict(lev_I=[0., np.nan], lev_Q=[0., 1.]), dict(lev_I=[0., 1.], lev_Q=[0., 1., 2.]), dict(lev_I=[[0., 1.]], lev_Q=[0., 1.]), dict(alphabet=[1 + 1j]),
               dict(alphabet=np.arange(4097) + 0j), dict(alphabet=[1, np.inf]), dict(lev_I=[0., 1.], lev_Q=[0., 1.], alphabet=[0, 1j])):
        with pytest.raises(ValueError):
            hip_dsp.PatternLevels(**kw)
    with pytest.raises(ValueError):
        hip_dsp.pattern_levels(np.zeros((2, 2), complex))
    assert hip_dsp.PRECOMP_LUT_LMAX == hip_dsp.PRECOMP_N_MAX == 2 ** 24 and hip_dsp.PRECOMP_MEM_MAX == 15 and hip_dsp.PRECOMP_M_MAX == 4096
    c = np.complex64
    L = 2 ** 24 + 1
    with pytest.raises(ValueError, match="2\\*\\*24"):
        hip_dsp.lut_accumulate_dev(_Stub((1, L), c), _Stub((1, L), c), _Stub((1, L), np.int32), _Stub((1, L), np.int32), 64)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        hip_dsp.cal_lut_dev(_Stub((1, L), c), _Stub((1, L), c), lv2)
    for N in (0, 2 ** 24 + 1, 2.5):
        with pytest.raises(ValueError):
            hip_dsp.lut_accumulate_dev(_Stub((1, 8), c), _Stub((1, 8), c), _Stub((1, 8), np.int32), _Stub((1, 8), np.int32), N)


def test_pattern_index_checks_its_arguments(no_library):
    c = np.complex64
    lv = hip_dsp.PatternLevels([-1, 1], [-1, 1])
    x, ii = _Stub((2, 9), c), _Stub((2, 9), np.int32)
    for a in ((_Stub((9,), c), lv, 3, ii, ii), (_Stub((2, 9), np.float32), lv, 3, ii, ii), (x, ([-1, 1], [-1, 1]), 3, ii, ii), (x, lv, 16, ii, ii),
              (x, lv, 3, _Stub((2, 8), np.int32), ii), (x, lv, 3, ii, _Stub((2, 9), np.int64)), (_Stub((2, 0), c), lv, 3, _Stub((2, 0), np.int32), None)):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.pattern_index_dev(*a)


def test_the_table_forms_check_their_arguments(no_library):
    c = np.complex128
    lv = hip_dsp.PatternLevels([-1, 1], [-1, 1])
    tx, ii = _Stub((2, 9), c), _Stub((2, 9), np.int32)
    ok = dict(tx=tx, rx=_Stub((2, 9), c), idx_I=ii, idx_Q=ii, N=8)
    for kw in (dict(rx=_Stub((2, 9), np.complex64)), dict(rx=_Stub((2, 8), c)), dict(idx_I=_Stub((2, 9), np.int64)), dict(idx_Q=None), dict(idx_data=_Stub((9,), np.bool_)),
               dict(idx_data=_Stub((3, 9), np.uint8)), dict(idx_data=_Stub((2, 8), np.uint8)), dict(ea=_Stub((2, 8), np.complex64)), dict(ea=_Stub((1, 8), c)),
               dict(nI=_Stub((2, 8), np.int64)), dict(nQ=_Stub((2, 7), np.int32))):
        a = dict(ok, **kw)
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.lut_accumulate_dev(a.pop("tx"), a.pop("rx"), a.pop("idx_I"), a.pop("idx_Q"), a.pop("N"), **a)
    for kw in (dict(mem_len=0), dict(ea=_Stub((2, 9), c)), dict(idx_I=_Stub((2, 8), np.int32)), dict(idx_data=_Stub((9,), np.int32)), dict(nI=_Stub((2, 8), np.uint8))):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.cal_lut_dev(tx, _Stub((2, 9), c), lv, **kw)
    with pytest.raises(TypeError):
        hip_dsp.cal_lut_dev(tx, _Stub((2, 9), c), [-1, 1])
    ea = _Stub((2, 8), c)
    for a in ((tx, _Stub((2, 8), np.complex64), ii, ii, tx), (tx, _Stub((1, 8), c), ii, ii, tx), (tx, ea, _Stub((2, 8), np.int32), ii, tx), (tx, ea, ii, ii, _Stub((2, 8), c)),
              (tx, ea, ii, ii, _Stub((2, 9), np.complex64)), (_Stub((9,), c), ea, ii, ii, tx)):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.lut_apply_dev(*a)
    for g in (np.nan, np.inf, 1j):
        with pytest.raises(ValueError):
            hip_dsp.lut_apply_dev(tx, ea, ii, ii, tx, gain=g)
    out = _Stub((2, 9), c, ptr=2)
    with pytest.raises(ValueError, match="another buffer"):
        hip_dsp.lut_predistort_dev(tx, lv, 3, ea, tx)
    with pytest.raises(ValueError, match="another buffer"):
        hip_dsp.lut_predistort_dev(tx, lv, 3, ea, _Stub((2, 9), c, ptr=1))
    for a in ((tx, lv, 2, ea, out), (tx, lv, 3, _Stub((2, 8), np.complex64), out), (tx, lv, 3, ea, _Stub((2, 8), c, ptr=2)), (tx, None, 3, ea, out)):
        with pytest.raises((ValueError, TypeError)):
            hip_dsp.lut_predistort_dev(*a)


def test_comp_mod_sin_checks_its_arguments(no_library):
    c = np.complex64
    x = _Stub((2, 9), c)
    for kw in (dict(vpi=np.nan), dict(vpi=[1.0, 2.0]), dict(vpi=complex(1, np.inf)), dict(clip=-1), dict(clip=np.nan), dict(clip=1j)):
        with pytest.raises(ValueError):
            hip_dsp.comp_mod_sin_dev(x, x, **kw)
    with pytest.raises((ValueError, TypeError)):
        hip_dsp.comp_mod_sin_dev(x, _Stub((2, 8), c))
    with pytest.raises(TypeError):
        hip_dsp.comp_mod_sin_dev(_Stub((2, 9), np.float64), _Stub((2, 9), np.float64))
    assert hip_dsp.precomp._vpi_rails(1.14) == (1.14, 1.14) and hip_dsp.precomp._vpi_rails(1.2 + 0.9j) == (1.2, 0.9) and hip_dsp.precomp._vpi_rails(1.2 + 0j) == (1.2, 0.0)
    with pytest.raises(ValueError):
        dpc.comp_mod_sin(np.zeros(4, complex), vpi=np.nan)


def test_the_dac_table_checks_its_arguments(no_library):
    for kw in (dict(prms_dac=(16e9, 2, "ba", 6)), dict(prms_dac=(16e9, 2, "zpk", 6)), dict(prms_dac=(16e9, 2, "sos")), dict(prms_dac=(16e9, 9, "sos", 6)),
               dict(prms_dac=(30e9, 2, "sos", 6)), dict(prms_dac=(16e9, 2.5, "sos", 6)), dict(sim_len=0), dict(sim_len=2 ** 24 + 1), dict(sim_len=100.5), dict(rrc_beta=-0.1),
               dict(rrc_beta=1.5), dict(dpe_fb=0), dict(os=0), dict(PAPR=np.inf), dict(PAPR=4000)):
        a = dict(dict(dpe_fb=20e9, sim_len=256, rrc_beta=0.1), **kw)
        with pytest.raises(ValueError):
            hip_dsp.comp_dac_resp_dev(**a)
        with pytest.raises(ValueError):
            dpc.comp_dac_resp(**a)
    with pytest.raises(TypeError):
        hip_dsp.comp_dac_resp_dev(20e9, 256, 0.1, dtype=np.float64)
    with pytest.raises(ValueError):
        hip_dsp.comp_dac_resp_dev(20e9, 256, 0.1, dtype=np.complex64, out=_Stub((256,), np.complex128))
    with pytest.raises(ValueError):
        hip_dsp.dac_preemphasis_dev(_Stub((2, 1), np.complex64), _Stub((2, 1), np.complex64), 20e9, 0.1)          # no transform of one sample
    with pytest.raises(ValueError):
        hip_dsp.dac_preemphasis_dev(_Stub((2, 256), np.complex64), _Stub((2, 256), np.complex64), 20e9, 0.1, table=_Stub((255,), np.complex64))
    fb, fs, beta, noise, sos = hip_dsp.precomp._dac_preemphasis_args(20e9, 256, 0.1, 9, (16e9, 2, "sos", 6), 2)
    assert (fb, fs, beta) == (20e9, 40e9, 0.1) and sos.shape == (1, 6) and noise == 10 ** 0.9 / (6 * 20e9 * 2 ** 12)


def test_the_mirrored_functions_check_before_they_upload(no_library):
    qam = (np.arange(-3, 4, 2)[:, None] + 1j * np.arange(-3, 4, 2)[None, :]).ravel()
    x = qam[np.arange(32) % 16]
    with pytest.raises(ValueError):
        dpc.cal_lut(x.reshape(2, 16), x.reshape(2, 16), qam)                     # 1-d only
    with pytest.raises(ValueError):
        dpc.cal_lut(x, x[:-1], qam)
    with pytest.raises(ValueError):
        dpc.cal_lut(x, x, qam, mem_len=16)
    with pytest.raises(ValueError):
        dpc.cal_lut(x, x, qam, mem_len=7, real_ptrns=False)                     # 16**7 entries
    with pytest.raises(ValueError):
        dpc.cal_lut(x, x, qam, idx_data=np.ones(31, bool))
    with pytest.raises(ValueError):
        dpc.find_sym_patterns(x.reshape(2, 16), qam, 3)
    with pytest.raises(ValueError):
        dpc.find_sym_patterns(x, qam, 7)
    ea, idx = np.zeros(64, complex), np.zeros(32, np.int64)
    for a in ((x, ea, idx[:-1], idx), (x, ea, idx, idx + 64), (x, ea, idx - 1, idx), (x, ea, idx.astype(float), idx), (x, np.zeros((2, 64), complex), idx, idx)):
        with pytest.raises(ValueError):
            dpc.apply_lut(*a)
    with pytest.raises(ValueError):
        dpc.apply_lut(x, ea, idx, idx, gain=np.nan)


def test_the_level_tables_live_as_long_as_their_levels(monkeypatch):
    """The launches get raw pointers of the level tables: the tables are owned by the PatternLevels object, go up once, and are still alive at
    every call - also with the small cache of the pilot tables full and turning over between the calls, and for two different rails."""
    live, freed, calls = {}, [], []

    class Table(_Stub):
        def __del__(self):
            freed.append(self.ptr)

    def from_host(cls, arr):
        t = Table(arr.shape, arr.dtype, 1000 + len(live) + len(freed))
        live[t.ptr] = arr.copy()
        return t

    def call(name, *a):
        if name.startswith(("qh_pattern_index", "qh_lut_predistort")):
            ptrs = [p for p in (a[3], a[5], a[7]) if p is not None]
            assert ptrs and not set(ptrs) & set(freed), "a level table was released before the launch"
            calls.append([live[p] for p in ptrs])
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib.DeviceArray, "from_host", classmethod(from_host))
    monkeypatch.setattr(hip_dsp.pilot, "_PILOT_TABLES", threading.local())
    c = np.complex64
    x, out, ii, ea = _Stub((1, 9), c, 10), _Stub((1, 9), c, 11), _Stub((1, 9), np.int32, 20), _Stub((1, 16), np.complex128, 30)
    square = hip_dsp.PatternLevels([-3, -1, 1, 3], [-3, -1, 1, 3])
    hip_dsp.pattern_index_dev(x, square, 2, ii, ii)
    for k in range(2 * hip_dsp.PILOT_TABLES_KEPT):                              # other tables come and go
        hip_dsp.pilot._pilot_table(np.arange(k + 2, dtype=np.int64))
    rect = hip_dsp.PatternLevels([-3, -1, 1, 3], [-1, 1])                      # the same in-phase rail, another quadrature rail
    hip_dsp.pattern_index_dev(x, rect, 2, ii, ii)
    hip_dsp.lut_predistort_dev(x, rect, 2, ea, out)
    hip_dsp.pattern_index_dev(x, square, 2, ii, ii)
    hip_dsp.pattern_index_dev(x, hip_dsp.PatternLevels(alphabet=[1, 1j, -1, -1j]), 2, ii, None)
    assert [[list(t) for t in tabs] for tabs in calls] == [[[-3, -1, 1, 3]] * 2, [[-3, -1, 1, 3], [-1, 1]], [[-3, -1, 1, 3], [-1, 1]], [[-3, -1, 1, 3]] * 2, [[1, 1j, -1, -1j]]]
    assert len(square._tables()) == 2 and square._tables() is square._tables() and len(rect._tables()) == 2
    uploads = len(live)
    hip_dsp.pattern_index_dev(x, rect, 2, ii, ii)
    assert len(live) == uploads                                                 # nothing goes up twice
    kept = [t.ptr for t in rect._tables()]
    del rect
    import gc
    gc.collect()
    assert set(kept) <= set(freed)                                              # and the tables go with their levels


def test_valid_calls_reach_the_library_with_the_abi_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name,) + a))
    monkeypatch.setattr(_lib.DeviceArray, "from_host", classmethod(lambda cls, arr: _Stub(arr.shape, arr.dtype, 70 + arr.size)))
    c = np.complex64
    rails = hip_dsp.PatternLevels([-3, -1, 1, 3], [-1, 1])
    alpha = hip_dsp.PatternLevels(alphabet=[1, 1j, -1])
    x, out = _Stub((2, 9), c, 10), _Stub((2, 9), c, 11)
    iI, iQ = _Stub((2, 9), np.int32, 20), _Stub((2, 9), np.int32, 21)
    ea, nI, nQ = _Stub((2, 64), np.complex128, 30), _Stub((2, 64), np.int32, 31), _Stub((2, 64), np.int32, 32)
    hip_dsp.pattern_index_dev(x, rails, 3, iI, iQ)
    hip_dsp.pattern_index_dev(_Stub((1, 5), np.complex128, 12), alpha, 2, _Stub((1, 5), np.int32, 22), None)
    hip_dsp.lut_accumulate_dev(x, out, iI, iQ, 64, idx_data=_Stub((2, 9), np.uint8, 40), ea=ea, nI=nI, nQ=nQ)
    hip_dsp.lut_accumulate_dev(x, out, iI, iQ, 64, idx_data=_Stub((9,), np.uint8, 41), ea=ea, nI=nI, nQ=nQ)
    hip_dsp.lut_apply_dev(x, ea, iI, iQ, x, gain=-0.5)
    hip_dsp.lut_predistort_dev(x, rails, 3, ea, out)
    hip_dsp.comp_mod_sin_dev(x, x, vpi=1.2 + 0.9j, clip=0.95)
    sos = hip_dsp.design_lowpass_sos(40e9, 16e9, "bessel", 2)
    tab = hip_dsp.comp_dac_resp_dev(20e9, 256, 0.1, dtype=c, out=_Stub((256,), c, 50))
    name, n, fb, fs, beta, noise, psos, nsec, p = seen.pop()
    assert (name, n, fb, fs, beta, nsec, p) == ("qh_dac_preemphasis_table_c64_dev", 256, 20e9, 40e9, 0.1, 1, 50) and tab.ptr == 50 and sos.shape == (1, 6)
    assert noise == 10 ** 0.9 / (6 * 20e9 * 2 ** 12) and isinstance(psos, int)
    assert seen == [("qh_pattern_index_c64_dev", 10, 2, 9, 74, 4, 72, 2, None, 0, 3, 20, 21),
                    ("qh_pattern_index_c128_dev", 12, 1, 5, None, 0, None, 0, 73, 3, 2, 22, None),
                    ("qh_lut_accumulate_c64_dev", 10, 11, 2, 9, 20, 21, 40, 2, 64, 30, 31, 32),
                    ("qh_lut_accumulate_c64_dev", 10, 11, 2, 9, 20, 21, 41, 1, 64, 30, 31, 32),
                    ("qh_lut_apply_c64_dev", 10, 2, 9, 30, 64, 20, 21, -0.5, 10),
                    ("qh_lut_predistort_c64_dev", 10, 2, 9, 74, 4, 72, 2, None, 0, 3, 30, 64, 1.0, 11),
                    ("qh_comp_mod_sin_c64_dev", 10, 2, 9, 1.2, 0.9, 0.95, 10)]
