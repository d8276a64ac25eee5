"""The float64 restatement of the transmitter response (tests/txresp_ref.py) against the reference's outputs (tests/golden/txresp.npz,
written by tests/golden/gen_golden_txresp.py).  No GPU.  The restatement follows the reference's order of operations, so it is held to
1e-13 of the signal rms: a few hundred roundings of 2^-53 along the recurrence and through the exponentials."""
import os

import numpy as np
import pytest
import scipy.signal as scisig

import txresp_ref as tr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txresp.npz")
TOL = 1e-13


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def x_of(g, L):
    q = g["x_%d" % L]
    return (q[..., 0] + 1j * q[..., 1]) / g["scale"]


def kept(g, a, L):
    return a if L == 2048 else a[:, g["cols"]]


def relerr(a, b):
    return np.abs(a - b).max() / np.sqrt(np.mean(np.abs(b) ** 2))


def mod_prms(g):
    return dict(dcbias=complex(g["mod_dcbias"]), gfactr=complex(g["mod_gfactr"]), cfactr=complex(g["mod_cfactr"]), dcbias_out=float(g["mod_dcbias_out"]),
                gfactr_out=float(g["mod_gfactr_out"]))


@pytest.mark.parametrize("L", [2048, 12388])
def test_clip_and_quantiser(gold, L):
    xq = tr.exact_quant_field(x_of(gold, L))
    assert np.array_equal(tr.row_max(xq), [2.0, 2.0])
    assert relerr(kept(gold, tr.dac_pointwise(xq, clip_rat=0.8), L), gold["clip_%d" % L]) <= TOL
    for b in (1, 4, 8):
        q, ir, ii, u = tr.quantise(xq, b)
        assert tr.on_threshold(u, b) >= 1
        assert np.array_equal(kept(gold, q, L), gold["q%d_%d" % (b, L)])
        q32, ir32, ii32, _ = tr.quantise(xq, b, np.float32)
        assert np.array_equal(ir, ir32) and np.array_equal(ii, ii32)
        assert relerr(kept(gold, tr.dac_pointwise(xq, clip_rat=0.8, quant_bits=b), L), gold["cq%d_%d" % (b, L)]) <= TOL


def test_a_value_on_a_threshold_goes_up():
    x = np.array([[-1.0, -0.5, -0.25, 0.0, 0.5 - 1e-12, 0.5, 1.0]], np.complex128)
    q, ir, _, _ = tr.quantise(x, 2)
    assert ir.tolist() == [[0, 1, 1, 2, 2, 3, 3]]
    assert np.array_equal(q.real, [[-0.75, -0.25, -0.25, 0.25, 0.25, 0.75, 0.75]])


def test_sections_loop_is_sosfilt(gold):
    x = x_of(gold, 2048)
    for name, cutoff, ftype, order in (("bessel4", 50e6, "bessel", 4), ("butter6", 100e6, "butter", 6), ("bessel3", 2e9, "bessel", 3), ("butter8", 1e9, "butter", 8)):
        sos = tr.design(float(gold["fs"]), cutoff, ftype, order)
        y = tr.sosfilt_loop(sos, x)
        assert relerr(y[:, :1024], gold["filt_" + name]) <= TOL, name
        assert relerr(y, scisig.sosfilt(sos, x, axis=-1)) <= TOL, name
    sos = tr.design(float(gold["fs"]), 2e9, "bessel", 3)
    assert sos.shape == (2, 6) and np.sum(sos[:, 5] == 0) == 1 and np.sum(sos[:, 2] == 0) == 1     # the odd order is padded with zeros


@pytest.mark.parametrize("L", [2048, 12388])
def test_default_dac_filter(gold, L):
    y = tr.sosfilt_loop(tr.design(float(gold["fs"]), 18e9), x_of(gold, L))
    assert relerr(kept(gold, y, L), gold["filt_%d" % L]) <= TOL


def test_modulator_and_amplifier(gold):
    s = np.ascontiguousarray(x_of(gold, 2048)[:, :512])
    assert relerr(tr.modulator(s), gold["mod_ideal"]) <= TOL
    assert relerr(tr.modulator(s, **mod_prms(gold)), gold["mod_real"]) <= TOL
    assert relerr(tr.modulator(tr.amplifier(s, 0.7)), gold["mod_amp"]) <= TOL


@pytest.mark.parametrize("L", [2048, 12388])
def test_chains(gold, L):
    xq = tr.exact_quant_field(x_of(gold, L))
    fs = float(gold["fs"])
    assert relerr(kept(gold, tr.sim_tx(xq, fs, tgt_v=0.7, clip_rat=0.8, quant_bits=5), L), gold["chain_a_%d" % L]) <= TOL
    assert relerr(kept(gold, tr.sim_tx(xq, fs, tgt_v=0.5, quant_bits=4, dac_params={}, **mod_prms(gold)), L), gold["chain_b_%d" % L]) <= TOL


def test_pole_radius_takes_every_section():
    sos = tr.design(40e9, 100e6, "butter", 6)
    r = tr.pole_radius(sos)
    assert r > np.abs(np.roots([1.0, sos[0, 4], sos[0, 5]])).max()
    assert abs(r - np.abs(scisig.sos2zpk(sos)[1]).max()) < 1e-12
