"""CPU checks of the impairment restatement (tests/impair_ref.py): its deterministic stages against the reference's outputs
(tests/golden/impair.npz), its Philox4x32-10 against the published known-answer vectors, and the pure power-factor function."""
import os

import numpy as np
import pytest

import impair_ref as ir
from qampy_amd.core import hip_dsp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "impair.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def x_of(g, L):
    q = g["x_%d" % L]
    return (q[..., 0] + 1j * q[..., 1]) / g["scale"]


def relerr(a, b, x):
    return np.abs(a - b).max() / np.sqrt(np.mean(np.abs(x) ** 2))


def test_philox_known_answers():
    """The known-answer vectors of Philox4x32-10 published with Random123 (kat_vectors): counter, key -> output."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in ir.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key, [hex(v) for v in got])
    # arrays go through the same rounds
    got = ir.philox4x32_10(*[np.array([c, 0]) for c in kat[2][0]], *kat[2][1])
    assert tuple(int(v[0]) for v in got) == kat[2][2]


def test_draws_depend_on_seed_mode_and_index_only():
    a = ir.gauss(5, 1, np.arange(100), ir.STREAM_NOISE, True)[0]
    b = ir.gauss(5, 1, np.arange(40, 60), ir.STREAM_NOISE, True)[0]
    assert np.array_equal(a[40:60], b)
    assert not np.array_equal(a, ir.gauss(6, 1, np.arange(100), ir.STREAM_NOISE, True)[0])
    assert not np.array_equal(a, ir.gauss(5, 0, np.arange(100), ir.STREAM_NOISE, True)[0])
    assert not np.array_equal(a, ir.gauss(5, 1, np.arange(100), ir.STREAM_PHASE, True)[0])
    n = ir.noise(3, 2, 1 << 15, False)
    assert abs(np.mean(np.abs(n) ** 2) - 1) < 5 / np.sqrt(n.size)


def test_whole_row_pmd_is_the_reference(gold):
    x = x_of(gold, 4096)
    got = ir.pmd(x, float(gold["theta"]), 30e-12 * float(gold["fs"]))
    assert relerr(got, gold["pmd_4096_30"], x) <= 1e-11


def test_overlap_save_pmd_deviates_as_stated(gold):
    """Not the reference's operation: the wrapped 1/n tail of a fractional delay.  30 ps at 40 GS/s: a few 1e-4 of the rms; 200 ps is a
    delay of whole samples and exact."""
    x = x_of(gold, 12388)
    th, fs = float(gold["theta"]), float(gold["fs"])
    d30 = relerr(ir.pmd(x, th, 30e-12 * fs), gold["pmd_12388_30"], x)
    assert 1e-5 < d30 <= 3e-4, d30
    d200 = relerr(ir.pmd(x, th, 200e-12 * fs)[:, gold["cols_200"]], gold["pmd_12388_200"], x)
    assert d200 <= 1e-11, d200
    # the full-length form of the restatement is the reference at this length too
    assert relerr(ir.pmd_whole(x, th, 30e-12 * fs), gold["pmd_12388_30"], x) <= 1e-11


def test_pointwise_stages_are_the_reference(gold):
    x = np.ascontiguousarray(x_of(gold, 4096)[:, :512])
    fs = float(gold["fs"])
    assert relerr(ir.rotate_field(x, float(gold["theta"])), gold["rot"], x) <= 1e-11
    assert relerr(ir.carrier_offset(x, gold["fo_values"][0] / fs), gold["fo_pos"], x) <= 1e-11
    assert relerr(ir.carrier_offset(x, gold["fo_values"][1] / fs), gold["fo_neg"], x) <= 1e-11
    assert np.array_equal(ir.modal_delay(x, [3, -5]), gold["delay"])


def test_order_of_simulate_transmission(gold):
    x = x_of(gold, 2048)
    fs, th = float(gold["fs"]), float(gold["theta"])
    got = ir.simulate(x, fs, freq_off=float(gold["sim_fo"]), modal=[3, -5], dgd=30e-12, theta=th)
    assert relerr(got, gold["sim"], x) <= 1e-11
    # another order is another result
    other = ir.modal_delay(ir.pmd(ir.carrier_offset(x, float(gold["sim_fo"]) / fs), th, 30e-12 * fs), [3, -5])
    assert relerr(other, gold["sim"], x) > 1e-3


def test_snr_factors():
    assert hip_dsp.snr_power_factor(10, 2) == pytest.approx(1.2, rel=1e-15)
    assert hip_dsp.snr_power_factor(0, 1) == pytest.approx(2.0, rel=1e-15)
    assert hip_dsp.snr_power_factor(300, 2) == 1.0
    assert hip_dsp.snr_noise_factor(20, 2) == pytest.approx(0.1 * np.sqrt(2), rel=1e-15)
    # the noise power the factor adds is the square of the noise strength
    for snr, os_ in ((18, 2), (7.5, 1), (25, 4)):
        assert hip_dsp.snr_power_factor(snr, os_) - 1 == pytest.approx(hip_dsp.snr_noise_factor(snr, os_) ** 2, rel=1e-12)
    with pytest.raises(ValueError):
        hip_dsp.snr_noise_factor(10, 0)
