"""Host side of the resampler: the float64 restatement (tests/resample_ref.py) against the reference's outputs (tests/golden/resample.npz),
and the host functions of qampy_amd.core.resample / special_fcts against both.  No GPU."""
import os

import numpy as np
import pytest

import resample_ref as ref
from qampy_amd.core import resample as rs
from qampy_amd.core.special_fcts import rrcos_time

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
CASES = [(7, 10, 1000, 401), (7, 10, 1000, 400), (7, 10, 1003, 4001), (2, 1, 1000, 401), (28, 25, 997, 255), (1, 1, 512, 101)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def deq(g, key):
    return (g[key][..., 0] + 1j * g[key][..., 1]) / g["scale"]


def rel_max(got, want):
    return np.abs(got - want).max() / np.sqrt(np.mean(np.abs(want) ** 2))


def test_fixture_is_small():
    assert os.path.getsize(GOLD) < 2 ** 20


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fftconv", [True, False])
def test_restatement_matches_reference(gold, case, fftconv):
    up, down, n, taps = case
    x = deq(gold, "x_%d" % n)
    want = gold["rrc_%d_%d_%d_%d_%s" % (up, down, n, taps, "fft" if fftconv else "poly")]
    got = ref.rrcos_resample(x, gold["fold"], gold["fold"] * up / down, Ts=gold["Ts"], beta=gold["beta"], taps=taps, fftconv=fftconv)
    assert got.shape == want.shape == (ref.n_out(n, up, down),)
    assert rel_max(got, want) <= 1e-12
    if (up, down) == (1, 1) and not fftconv:
        assert np.array_equal(want, x)                          # scipy filters nothing at a ratio of 1


def test_restatement_matches_the_other_entries(gold):
    x, fold, Ts = deq(gold, "x_1000"), gold["fold"], gold["Ts"]
    assert rel_max(ref.rrcos_resample(x, fold, fold * 0.7, Ts=Ts, beta=1, taps=401), gold["rrcb1_7_10_1000_401"]) <= 1e-12
    for up, down in ((7, 10), (2, 1)):
        assert rel_max(ref.rrcos_resample(x, fold, fold * up / down), gold["poly_%d_%d_1000" % (up, down)]) <= 1e-12
    assert rel_max(ref.rrcos_resample(x, fold, fold * 0.7, Ts=Ts, beta=0.1, taps=401, renorm=True), gold["renorm_7_10_1000_401"]) <= 1e-12
    got = ref.resample(deq(gold, "shape_in"), ref.rrcos_taps(101, 56e9, Ts, 0.1), 1, 1, 1.0)
    assert got.shape == (2, 512) and rel_max(got, gold["shape_out"]) <= 1e-12
    sig = ref.rrcos_resample(deq(gold, "sig_in"), 28e9, 56e9, Ts=1 / 28e9, beta=0.1, taps=4001, renorm=True)
    assert sig.shape == (2, 4096) and rel_max(sig, gold["sig_out"]) <= 1e-12


@pytest.mark.parametrize("fn", [rrcos_time, ref.rrcos_time])
def test_rrcos_time_matches_the_reference_taps(gold, fn):
    for key in sorted(k for k in gold if k.startswith("taps")):
        up, _, _, taps = (int(v) for v in key.split("_")[1:])
        beta = 1.0 if key.startswith("tapsb1") else float(gold["beta"])
        t = (np.arange(taps) - (taps - 1) // 2) / (up * gold["fold"])
        h = fn(t, beta, gold["Ts"])
        assert np.abs(h / h.max() - gold[key]).max() <= 1e-12, key
        assert np.abs(rs.rrcos_taps(taps, up * gold["fold"], gold["Ts"], beta) - gold[key]).max() <= 1e-12


def test_rrcos_time_singular_points():
    T = 1 / 28e9
    for beta in (0.1, 0.25, 1.0):
        t = np.array([-T / (4 * beta), 0.0, T / (4 * beta), 0.3 * T])
        h = rrcos_time(t, beta, T)
        assert np.all(np.isfinite(h)) and h[0] == h[2]
        assert h[1] == pytest.approx((1 + beta * (4 / np.pi - 1)) / T, rel=1e-15)
        d = 1e-6 * T                                             # the limits: the closed form a little to either side
        for i in (0, 1, 2):
            near = ref.rrcos_time(np.array([t[i] - d, t[i] + d]), beta, T)
            assert h[i] == pytest.approx(near.mean(), rel=1e-6)
    # the taps of the 7/10 fixture case hit |t| = T / (4 beta) on the grid: samples 200 +- 50
    h = rs.rrcos_taps(401, 7 * 80e9, T, 0.1)
    assert h[200] == 1.0 and np.all(np.isfinite(h)) and abs(h[150] - h[250]) < 1e-15
    assert rrcos_time(np.array([0.0]), 0.5, T).shape == (1,)


def test_default_window_matches_scipys(gold):
    for up, down in ((7, 10), (2, 1)):
        want = gold["win_%d_%d" % (up, down)]
        for fn in (rs.default_window, ref.default_window):
            got = fn(up, down)
            assert got.shape == want.shape == (20 * max(up, down) + 1,)
            assert np.abs(got - want).max() <= 1e-15
            assert got.sum() == pytest.approx(1.0, abs=1e-14)


@pytest.mark.parametrize("T, up", [(1, 1), (2, 3), (255, 28), (400, 7), (401, 7), (4001, 2), (8191, 64)])
def test_phase_major_table_round_trips(T, up):
    h = np.random.default_rng(T).standard_normal(T)
    tab = rs.polyphase_table(h, up)
    J = -(-T // up)
    assert tab.shape == (up, J) and tab.flags.c_contiguous
    assert np.array_equal(tab, ref.phase_major(h, up))
    back = tab.T.ravel()
    assert np.array_equal(back[:T], h) and not back[T:].any()
    for p in range(up):
        for j in (0, J - 1):
            assert tab[p, j] == (h[p + j * up] if p + j * up < T else 0.0)


def test_resampling_factors():
    for fn in (rs._resamplingfactors, ref.factors):
        assert fn(80e9, 56e9) == (7, 10)
        assert fn(50e9, 56e9) == (28, 25)
        assert fn(28e9, 56e9) == (2, 1)
        assert fn(1.0, 1.0) == (1, 1)
    assert rs.n_out(1003, 7, 10) == 703 and rs.n_out(997, 28, 25) == 1117 and rs.n_out(1000, 2, 1) == 2000


def test_argument_errors():
    x = np.zeros(64, np.complex128)
    with pytest.raises(NotImplementedError, match="taps=None"):
        rs.rrcos_resample(x, 1.0, 2.0, beta=0.1, taps=None)
    from qampy_amd.core.filter import rrcos_pulseshaping
    with pytest.raises(NotImplementedError, match="taps=None"):
        rrcos_pulseshaping(x, 2.0, 1.0, 0.1, taps=None)
    for beta in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match="beta"):
            rs.rrcos_resample(x, 1.0, 2.0, beta=beta)
    with pytest.raises(ValueError):
        rs.rrcos_resample(np.zeros((2, 2, 8), np.complex128), 1.0, 2.0, beta=0.1)
    from qampy_amd.pipeline import ResidentReceiver
    assert callable(ResidentReceiver.load_resampled)
    from qampy_amd.signals import SignalQAM
    assert callable(SignalQAM.resample)
