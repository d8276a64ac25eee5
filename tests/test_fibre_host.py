"""Host side of the nonlinear fibre (core.hip_dsp ssfm_dev / dbp_dev, core.fibre, the signal wrappers, ResidentReceiver.backpropagate): every
check raises before the device is touched, the launch plan counts, the amplifier's noise power, and header / binding consistency.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import fibre_ref as fr
import qampy_amd
from qampy_amd import _lib
from qampy_amd.core import fibre as cfibre
from qampy_amd.core import hip_dsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDev:
    """Shape, dtype and pointer of a DeviceArray: enough for the checks, useless for a launch."""
    def __init__(self, shape, dtype, ptr=64):
        self.shape, self.dtype, self.ptr = tuple(shape), np.dtype(dtype), ptr


E = FakeDev((2, 1000), np.complex64)
KW = dict(fs=64e9, D=17e-6, span_length=80e3, power_dbm=3.0)


def both(**kw):
    a = dict(KW, **kw)
    return [lambda: hip_dsp.ssfm_dev(E, E, **a), lambda: hip_dsp.dbp_dev(E, E, **a)]


VALUE_ERRORS = (
    both(power_dbm=None) + both(pscale=1e-3) + both(power_dbm=None, pscale=0.0) + both(power_dbm=None, pscale=-1.0) + both(power_dbm=np.nan)
    + both(power_dbm=None, pscale=np.inf) + both(steps=0) + both(steps=4097) + both(steps=2.5) + both(steps=[]) + both(steps=[40e3, 30e3])
    + both(steps=[40e3, -40e3, 80e3]) + both(steps=[40e3, np.nan]) + both(steps=[80e3 * (1 + 1e-8)]) + both(nspans=0) + both(nspans=4097)
    + both(nspans=1.5) + both(span_length=0) + both(span_length=np.inf) + both(fs=0) + both(fs=np.nan) + both(D=np.inf) + both(gamma=np.nan)
    + both(alpha_db_km=np.inf) + both(alpha_db_km=1e6) + both(wl0=np.nan)
    + [lambda: hip_dsp.ssfm_dev(E, E, nf_db=np.nan, **KW), lambda: hip_dsp.ssfm_dev(E, E, nf_db=5, seed=1.5, **KW),
       lambda: hip_dsp.dbp_dev(E, E, nf_db=5, **KW),
       lambda: hip_dsp.ssfm_dev(FakeDev((3, 1000), np.complex64), FakeDev((3, 1000), np.complex64), **KW),
       lambda: hip_dsp.dbp_dev(FakeDev((3, 1000), np.complex64), FakeDev((3, 1000), np.complex64), **KW),
       lambda: hip_dsp.ssfm_dev(FakeDev((2, 2 ** 24 - 1), np.complex64), FakeDev((2, 2 ** 24 - 1), np.complex64), **KW),
       lambda: hip_dsp.dbp_dev(FakeDev((1, 1), np.complex128), FakeDev((1, 1), np.complex128), **KW),
       lambda: hip_dsp.ssfm_dev(E, FakeDev((2, 1001), np.complex64), **KW), lambda: hip_dsp.dbp_dev(E, FakeDev((2, 1000), np.complex128), **KW)])


@pytest.mark.parametrize("call", VALUE_ERRORS)
def test_value_errors_before_the_device(call):
    with pytest.raises(ValueError):
        call()


def test_type_errors_before_the_device():
    for f in (hip_dsp.ssfm_dev, hip_dsp.dbp_dev):
        with pytest.raises(TypeError):
            f(FakeDev((2, 1000), np.float32), E, **KW)
        with pytest.raises(TypeError):
            f(FakeDev((1000,), np.complex64), E, **KW)
    with pytest.raises(TypeError):
        hip_dsp.dbp_dev(E, E, seed=3, **KW)                                  # back-propagation draws nothing


def test_nonlinear_step_refuses_before_the_device():
    ps = FakeDev((1,), np.float64)
    for call in (lambda: hip_dsp.fibre_nl_dev(E, E, np.nan, 1.0, ps), lambda: hip_dsp.fibre_nl_dev(E, E, 1.0, np.inf, ps),
                 lambda: hip_dsp.fibre_nl_dev(E, E, 1.0, 1.0, ps, sigma_w=-1.0), lambda: hip_dsp.fibre_nl_dev(E, E, 1.0, 1.0, FakeDev((1,), np.float32)),
                 lambda: hip_dsp.fibre_nl_dev(E, E, 1.0, 1.0, FakeDev((2,), np.float64)), lambda: hip_dsp.fibre_nl_dev(E, FakeDev((2, 999), np.complex64), 1.0, 1.0, ps),
                 lambda: hip_dsp.fibre_nl_dev(FakeDev((3, 8), np.complex64), FakeDev((3, 8), np.complex64), 1.0, 1.0, ps),
                 lambda: hip_dsp.fibre_nl_dev(FakeDev((2, 0), np.complex64), FakeDev((2, 0), np.complex64), 1.0, 1.0, ps),
                 lambda: hip_dsp.fibre_nl_dev(E, E, 1.0, 1.0, ps, sigma_w=1.0, seed=0.5)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        hip_dsp.fibre_nl_dev(FakeDev((2, 8), np.float64), FakeDev((2, 8), np.float64), 1.0, 1.0, ps)
    for name in ("qh_fibre_nl_c64_dev", "qh_fibre_nl_c128_dev"):
        assert len(_lib.SIGNATURES[name]) == 9 and hasattr(_lib.load(), name)
        assert re.search(r"int %s\(const void \*E, int nmodes, int64_t L, double a, double coef, const double \*pscale, double sigma_w, uint64_t seed, void \*out\);" % name,
                         open(os.path.join(ROOT, "include", "qampy_hip.h")).read())


def test_a_valid_call_reaches_the_device():
    """the checks above refuse nothing that is valid: with every argument in range the call gets as far as the library"""
    if _lib.device_count() > 0:
        pytest.skip("only meaningful on a box without a GPU")
    for f in (hip_dsp.ssfm_dev, hip_dsp.dbp_dev):
        with pytest.raises(RuntimeError):
            f(E, E, steps=[10e3, 30e3, 40e3], nspans=3, **KW)


def test_host_layer_refuses_before_the_device():
    x = np.zeros((2, 1000), np.complex64)
    a = dict(D=17e-6, span_length=80e3)
    for f in (cfibre.ssfm, cfibre.dbp):
        with pytest.raises(ValueError):
            f(x, 64e9, **a)                                                  # neither power_dbm nor pscale
        with pytest.raises(ValueError):
            f(x, 64e9, power_dbm=3, pscale=1e-3, **a)
        with pytest.raises(ValueError):
            f(np.zeros((3, 1000), np.complex64), 64e9, power_dbm=3, **a)
        with pytest.raises(ValueError):
            f(np.zeros((2, 2, 256), np.complex64), 64e9, power_dbm=3, **a)
        with pytest.raises(ValueError):
            f(np.zeros(1, np.complex64), 64e9, power_dbm=3, **a)             # a row of one sample
        with pytest.raises(ValueError):
            f(x, 64e9, power_dbm=3, steps=[1e3], **a)
        with pytest.raises(ValueError):
            f(x, 0, power_dbm=3, **a)
    with pytest.raises(ValueError):
        cfibre.dbp(x, 64e9, power_dbm=3, nf_db=5, **a)
    with pytest.raises(ValueError):
        cfibre.ssfm(x, 64e9, power_dbm=3, seed=0.5, **a)


def plan_by_hand(steps, span, nspans, backward=False):
    """walk the spans as the model states them, with two tables of which the one used longest ago goes"""
    dz = fr.step_list(steps, span)
    if backward:
        dz = dz[::-1]
    held, age, filters, nonlinear, tables = {}, 0, 0, 0, 0
    for _ in range(nspans):
        lengths = [dz[0] / 2]
        for i in range(len(dz)):
            nonlinear += 1
            lengths.append(dz[i] / 2 + (dz[i + 1] / 2 if i + 1 < len(dz) else 0.0))
        for h in lengths:
            filters += 1
            age += 1
            if h not in held:
                tables += 1
                if len(held) == 2:
                    del held[min(held, key=held.get)]
            held[h] = age
    return dict(filters=filters, nonlinear=nonlinear, tables=tables)


def test_fibre_plan_counts():
    p = hip_dsp.fibre_plan(4096, 8, 3)
    assert p == dict(filters=27, nonlinear=24, tables=2, power=1)
    assert hip_dsp.fibre_plan(4096, 8, 3, power_dbm=3)["power"] == 2
    assert hip_dsp.fibre_plan(1000, 1, 1) == dict(filters=2, nonlinear=1, tables=1, power=1)
    # 5 km, 20 km, 35 km, 20 km: three tables in the first span; the next span finds 20 km and 35 km, forms 5 km over 35 km, keeps 20 km, forms 35 km
    assert hip_dsp.fibre_plan(1000, [10e3, 30e3, 40e3], 1, 80e3) == dict(filters=4, nonlinear=3, tables=3, power=1)
    for steps, span in ((8, 80e3), (1, 80e3), (2, 80e3), ([10e3, 30e3, 40e3], 80e3), ([40e3, 40e3], 80e3), ([1e3, 2e3, 3e3, 4e3], 10e3)):
        for nspans in (1, 2, 3):
            for backward in (False, True):
                got = hip_dsp.fibre_plan(1000, steps, nspans, span, backward=backward)
                want = plan_by_hand(steps, span, nspans, backward)
                assert {k: got[k] for k in want} == want, (steps, nspans, backward, got, want)
    with pytest.raises(ValueError):
        hip_dsp.fibre_plan(1, 8, 1)
    with pytest.raises(ValueError):
        hip_dsp.fibre_plan(4096, 0, 1)
    with pytest.raises(ValueError):
        hip_dsp.fibre_plan(4096, 8, 0)


def test_ase_power_and_alpha():
    alpha = hip_dsp.fibre_alpha(0.2)
    assert alpha == pytest.approx(0.2e-3 * np.log(10) / 10, rel=1e-15)
    assert np.exp(alpha * 80e3) == pytest.approx(10 ** 1.6, rel=1e-12)     # 16 dB of loss over 80 km
    p = hip_dsp.ase_power(5.0, alpha, 80e3, 64e9)
    want = 10 ** 0.5 / 2 * 6.62607015e-34 * (2.99792458e8 / 1550e-9) * (10 ** 1.6 - 1) * 64e9
    assert p == pytest.approx(want, rel=1e-12) and p == pytest.approx(fr.ase_power(5.0, alpha, 80e3, 64e9), rel=1e-14)
    assert 4e-7 < p < 6e-7                                                   # half a microwatt per mode in 64 GHz
    assert hip_dsp.ase_power(5.0, 0.0, 80e3, 64e9) == 0.0                    # no loss, no gain, no noise
    assert hip_dsp.ase_power(5.0, alpha, 80e3, 64e9, wl0=1300e-9) == pytest.approx(p * 1550 / 1300, rel=1e-12)


def test_header_binding_and_version_agree():
    header = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    assert re.search(r"#define\s+QH_ABI_VERSION\s+11\b", header) and _lib.ABI_VERSION == 11
    for name in ("qh_fibre_ssfm_c64_dev", "qh_fibre_ssfm_c128_dev"):
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == ["E", "nmodes", "L", "fs", "beta2", "gamma", "alpha", "dz", "nsteps", "nspans", "backward",
                                                             "amplify", "power_mode", "power", "ase_w", "seed", "out"]
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args) == 17
        C = _lib.C
        for a, t in zip(args, sig):
            want = C.c_void_p if "*" in a else {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "uint64_t": C.c_uint64}[a.split()[0]]
            assert t is want, (name, a, t)
        assert hasattr(_lib.load(), name)
    assert _lib.load().qh_abi_version() == _lib.ABI_VERSION
    units = re.search(r'^UNITS="([^"]*)"', open(os.path.join(ROOT, "qampy_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "fibre" in units and os.path.exists(os.path.join(ROOT, "qampy_amd", "csrc", "fibre.hip"))
    common = open(os.path.join(ROOT, "qampy_amd", "csrc", "common.h")).read()
    assert re.search(r"^\s*FIBRE,", common, flags=re.M)


def test_surface():
    assert hasattr(qampy_amd.core, "fibre")
    p = inspect.signature(hip_dsp.ssfm_dev).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("fs", inspect.Parameter.empty), ("D", inspect.Parameter.empty), ("span_length", inspect.Parameter.empty),
                                                         ("nspans", 1), ("gamma", 1.3e-3), ("alpha_db_km", 0.2), ("steps", 8), ("power_dbm", None),
                                                         ("pscale", None), ("amplify", True), ("nf_db", None), ("wl0", 1550e-9), ("seed", 0)]
    named = [k for k, v in inspect.signature(hip_dsp.dbp_dev).parameters.items() if v.kind is not inspect.Parameter.VAR_KEYWORD]
    assert named == [k for k in p if k not in ("nf_db", "seed")]
    assert list(inspect.signature(cfibre.ssfm).parameters)[:2] == ["sig", "fs"] and list(inspect.signature(cfibre.dbp).parameters)[:2] == ["sig", "fs"]
    assert list(inspect.signature(qampy_amd.impairments.simulate_fibre).parameters)[:3] == ["sig", "D", "span_length"]
    assert list(inspect.signature(qampy_amd.equalisation.backpropagate).parameters)[:3] == ["sig", "D", "span_length"]
    from qampy_amd.pipeline import ResidentReceiver
    q = inspect.signature(ResidentReceiver.backpropagate).parameters
    assert [(k, v.default) for k, v in q.items() if k != "self"] == [(k, inspect.Parameter.empty) for k in ("fs", "D", "span_length", "nspans", "gamma", "alpha_db_km",
                                                                                                        "steps", "power_dbm")] + [
        ("amplify", True), ("wl0", 1550e-9), ("next_capture", False)]
