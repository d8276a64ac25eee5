"""The float64 restatement of the theory kernels (tests/theory_ref.py) against the reference's values (tests/golden/theory.npz, made by
tests/golden/gen_golden_theory.py) and against the distribution it is meant to draw.  No GPU.

- ``gmi_mc`` on the reference's own draws: GMI and MI at atol 1e-12.  The restatement evaluates |y - s_j|^2 - |z|^2 where the reference evaluates
  |s_i - s_j|^2 + 2 Re(z (s_i - s_j)); the two agree to a few ulp of an exponent of at most ~10^2, and the means are of O(1) terms.
- the shaped draw: over N = 2^16 samples the share of every level lies within 6 sqrt(p (1 - p) / N) of its probability (a binomial share; the
  worst of the 48 seed / mode / rail / level combinations is 2.9 sigma)."""
import os

import numpy as np
import pytest

import theory_ref as tr
from conftest import GOLDEN
from qampy_amd import theory
from qampy_amd.core import hip_dsp

G = np.load(os.path.join(GOLDEN, "theory.npz"))
CASES = [(int(M), int(ns), float(db)) for M, ns, db in G["mc_cases"]]


def test_golden_cases_are_the_ones_the_kernels_are_held_to():
    assert CASES == [(4, 64, 6.), (16, 64, 12.), (64, 16, 15.), (256, 4, 22.)]


@pytest.mark.parametrize("c", range(len(CASES)))
def test_restatement_against_the_reference(c):
    M, ns, db = CASES[c]
    alphabet = hip_dsp.bits_map_labels(G["bitmap_%d" % M])
    assert np.array_equal(np.sort_complex(alphabet), np.sort_complex(G["coded_%d" % M]))
    z = G["mc%d_z" % c]
    assert z.shape == (ns,)
    gmi, per_bit, mi = tr.gmi_mc(alphabet, 10 ** (db / 10), z)
    print(M, gmi - float(G["mc%d_gmi" % c]), mi - float(G["mc%d_mi" % c]))
    np.testing.assert_allclose(gmi, float(G["mc%d_gmi" % c]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(mi, float(G["mc%d_mi" % c]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(per_bit.sum(), gmi, rtol=0, atol=1e-12)


def test_restatement_is_finite_at_any_snr_and_for_any_draw():
    al = theory.coded_symbols_qam(16)
    z = np.array([0.1 + 0.2j, 10j, -1e3, 0])
    for db in (-40, 0, 60, 120):
        gmi, per_bit, mi = tr.gmi_mc(al, 10 ** (db / 10), z)
        assert np.isfinite(gmi) and np.all(np.isfinite(per_bit)) and np.isfinite(mi)


def test_qpsk_gmi_equals_mi_per_realisation():
    al = theory.coded_symbols_qam(4)
    rng = np.random.default_rng(3)
    for db in (-5, 5, 30):
        z = 10 ** (-db / 20) * (rng.standard_normal(8) + 1j * rng.standard_normal(8)) / np.sqrt(2)
        gmi, _, mi = tr.gmi_mc(al, 10 ** (db / 10), z)
        np.testing.assert_allclose(gmi, mi, rtol=0, atol=1e-13)


def test_shaped_draw_frequencies():
    levels, px = theory.cal_ps_probablts(theory.coded_symbols_qam(64), 2.0)
    assert levels.size == 8
    N = 2 ** 16
    worst = 0.0
    for seed in (1, 2, 3):
        for mode in (0, 1):
            for idx in tr.shaped_indices(seed, mode, np.arange(N), px):
                assert idx.min() >= 0 and idx.max() < px.size
                share = np.bincount(idx, minlength=px.size) / N
                dev = np.abs(share - px) / np.sqrt(px * (1 - px) / N)
                worst = max(worst, dev.max())
                assert np.all(dev <= 6), (seed, mode, dev)
    print("worst deviation %.2f sigma" % worst)


def test_shaped_cdf_ends_at_one():
    px = np.array([0.1, 0.2, 0.3, 0.4]) * 3
    cdf = tr.shaped_cdf(px)
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0) and np.array_equal(cdf, hip_dsp.ps_cdf(px))
