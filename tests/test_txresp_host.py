"""Host side of the transmitter response: argument checks that raise before the device is touched, the chunk transition matrix against
brute-force stepping, the sections design against scipy's, and the exported geometry.  No GPU: on a machine without one any call that got
past the checks would raise RuntimeError instead."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal as scisig

import txresp_ref as tr
import qampy_amd
from qampy_amd import _lib
from qampy_amd.core import filter as cfilter
from qampy_amd.core import hip_dsp
from qampy_amd.core import impairments as cimp


class FakeDev:
    """Shape, dtype and pointer of a DeviceArray: enough for the checks, useless for a launch."""
    def __init__(self, shape, dtype, ptr=64):
        self.shape, self.dtype, self.ptr = tuple(shape), np.dtype(dtype), ptr


E = FakeDev((2, 64), np.complex64)


def test_geometry_is_the_librarys():
    c, t = C.c_int(0), C.c_int(0)
    _lib.call("qh_sos_geometry", C.byref(c), C.byref(t))
    assert (c.value, t.value) == (hip_dsp.SOS_CHUNK, hip_dsp.SOS_TILE)
    assert hip_dsp.SOS_TILE % hip_dsp.SOS_CHUNK == 0


@pytest.mark.parametrize("order,ftype,cutoff", [(2, "bessel", 18e9), (4, "bessel", 50e6), (6, "butter", 100e6), (3, "bessel", 2e9), (8, "butter", 1e9), (1, "butter", 5e9)])
def test_transition_matrix_against_stepping(order, ftype, cutoff):
    sos = hip_dsp.design_lowpass_sos(40e9, cutoff, ftype, order)
    for Cn in (0, 1, 2, 7, hip_dsp.SOS_CHUNK):
        P = hip_dsp.sos_transition(sos, Cn)
        B = tr.transition_brute(sos, Cn)
        assert P.shape == (2 * len(sos), 2 * len(sos))
        assert np.abs(P - B).max() <= 1e-15 * max(1.0, np.abs(B).max()), (Cn, np.abs(P - B).max())          # both in extended precision, rounded once


def test_transition_carries_a_chunk():
    """state after a chunk from s = P s + state after the chunk from zero: the identity the device relies on"""
    sos = hip_dsp.design_lowpass_sos(40e9, 100e6, "butter", 6)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(2 * hip_dsp.SOS_CHUNK)
    Cn = hip_dsp.SOS_CHUNK
    _, z1 = scisig.sosfilt(sos, x[:Cn], zi=np.zeros((len(sos), 2)))
    _, z2 = scisig.sosfilt(sos, x[Cn:], zi=z1)
    _, f2 = scisig.sosfilt(sos, x[Cn:], zi=np.zeros((len(sos), 2)))
    got = hip_dsp.sos_transition(sos, Cn) @ z1.ravel() + f2.ravel()
    assert np.abs(got - z2.ravel()).max() <= 1e-12 * np.abs(z2).max()


def test_design_is_scipys():
    assert np.array_equal(hip_dsp.design_lowpass_sos(40e9, 18e9), scisig.bessel(2, 18e9, "low", norm="mag", output="sos", fs=40e9))
    assert np.array_equal(hip_dsp.design_lowpass_sos(40e9, 1e8, "butter", 6), scisig.butter(6, 1e8, "low", output="sos", fs=40e9))
    assert np.array_equal(hip_dsp.design_lowpass_sos(40e9, 2e9, "bessel", 3), tr.design(40e9, 2e9, "bessel", 3))


BAD_TX = [dict(clip_rat=0), dict(clip_rat=-1), dict(clip_rat=np.nan), dict(quant_bits=2.5), dict(quant_bits=17), dict(quant_bits=-1), dict(enob=-1), dict(enob=np.inf),
          dict(dcbias=np.nan), dict(gfactr=complex(1, np.inf)), dict(cfactr=np.inf), dict(dcbias_out=np.nan), dict(gfactr_out=np.inf), dict(tgt_v=np.nan),
          dict(dac_params={"cutoff": 21e9}), dict(dac_params={"cutoff": 0}), dict(seed=1.5)]


@pytest.mark.parametrize("kw", BAD_TX)
def test_tx_response_refuses(kw):
    with pytest.raises(ValueError):
        hip_dsp.sim_tx_response_dev(E, E, 40e9, **kw)
    with pytest.raises(ValueError):
        cimp.sim_tx_response(np.zeros((2, 64), np.complex64), 40e9, **kw)


def test_tx_response_refuses_shapes_and_dtypes():
    with pytest.raises(TypeError):
        hip_dsp.sim_tx_response_dev(FakeDev((2, 64), np.float32), E, 40e9)
    with pytest.raises(TypeError):
        hip_dsp.dac_pointwise_dev(FakeDev((64,), np.complex64), E)
    with pytest.raises(ValueError):
        hip_dsp.sim_tx_response_dev(E, FakeDev((2, 65), np.complex64), 40e9)
    with pytest.raises(ValueError):
        hip_dsp.sosfilt_dev(E, FakeDev((2, 64), np.complex128), hip_dsp.design_lowpass_sos(40e9, 18e9))
    with pytest.raises(ValueError):
        hip_dsp.row_extrema_dev(E, FakeDev((2, 3), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.dac_pointwise_dev(E, E, quant_bits=4, ext=FakeDev((2, 2), np.float32))
    with pytest.raises(ValueError):
        hip_dsp.modulator_response_dev(FakeDev((2000, 4), np.complex64), FakeDev((2000, 4), np.complex64))
    with pytest.raises(NotImplementedError):
        hip_dsp.sim_tx_response_dev(E, E, 40e9, dac_params={"cutoff": 18e9, "fn": "measured.npz"})
    with pytest.raises(TypeError):
        hip_dsp.sim_dac_response_dev(E, E, 40e9, bandwidth=3)


@pytest.mark.parametrize("kw", [dict(order=0), dict(order=9), dict(order=2.5), dict(cutoff=0), dict(cutoff=20e9), dict(cutoff=-1e9), dict(cutoff=np.nan), dict(ftype="cheby")])
def test_filter_refuses(kw):
    a = dict(cutoff=18e9, ftype="bessel", order=2)
    a.update(kw)
    with pytest.raises(ValueError):
        hip_dsp.filter_signal_dev(E, E, 40e9, a["cutoff"], a["ftype"], a["order"])
    with pytest.raises(ValueError):
        cfilter.filter_signal(np.zeros(64, np.complex64), 40e9, a["cutoff"], ftype=a["ftype"], order=a["order"])


def test_sections_are_checked():
    good = hip_dsp.design_lowpass_sos(40e9, 18e9)
    for bad in (np.zeros((5, 6)), np.zeros((1, 5)), good * 2, np.full((1, 6), np.nan)):
        with pytest.raises(ValueError):
            hip_dsp.sosfilt_dev(E, E, bad)


def test_what_is_out_of_scope_says_so():
    x = np.zeros(64, np.complex64)
    for ftype in ("gauss", "exp"):
        with pytest.raises(NotImplementedError, match="frequency domain"):
            cfilter.filter_signal(x, 40e9, 18e9, ftype=ftype)
    with pytest.raises(NotImplementedError, match="lsim"):
        cfilter.filter_signal(x, 40e9, 18e9, analog=True)
    with pytest.raises(NotImplementedError, match="measured"):
        cimp.apply_DAC_filter(x, 40e9, fn="measured.npz")
    with pytest.raises(NotImplementedError):
        cimp.quantize_signal_New(x, 4, rescale_out=False)
    with pytest.raises(ValueError):
        cimp.quantize_signal_New(x, 0)
    with pytest.raises(ValueError):
        cimp.apply_enob_as_awgn(x, -2)


def test_host_helpers():
    assert cimp.er_to_g(20) == (10 ** 1.0 - 1) / (10 ** 1.0 + 1)
    x = np.array([[1.5 - 0.25j, -3 + 2j]], np.complex64)
    c = cimp.clipper(x, 1)
    assert c.dtype == np.complex64 and np.array_equal(c, [[1 - 0.25j, -1 + 1j]])
    a = cimp.ideal_amplifier_response(x, 0.6)
    assert np.allclose(a, x / 3 * 0.6)
    assert hip_dsp.enob_sigma(2.0, 6) == tr.enob_sigma(np.array([[2.0 + 1j]]), 6)
    assert hasattr(qampy_amd, "filtering") and qampy_amd.filtering.filter_signal and qampy_amd.filtering.rrcos_pulseshaping
    for name in ("sim_tx_response", "sim_DAC_response", "sim_mod_response"):
        assert hasattr(qampy_amd.impairments, name)


def test_resident_receiver_checks_tx_before_the_device():
    import inspect
    from qampy_amd.pipeline import ResidentReceiver
    assert inspect.signature(ResidentReceiver.impair).parameters["tx"].default is None
