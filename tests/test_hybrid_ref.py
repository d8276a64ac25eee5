"""The float64 restatement of time-domain hybrid QAM (tests/hybrid_ref.py) against the reference's constructor arrays (tests/golden/hybrid.npz),
and the conditions the GPU cases of tests/test_gpu_hybrid.py rely on, asserted on the restatement alone.  No GPU."""
import os

import numpy as np
import pytest

import hybrid_ref as ref

PREFIXES = ["t%d_n%d_" % (k, nm) for k in range(4) for nm in (1, 2)] + ["tfs_", "tpsk_"]
DTS = sorted(ref.DT)


def test_fixture_is_small():
    assert os.path.getsize(ref.GOLD) < 400 * 1024


def test_geometry_and_power_ratio_are_the_references():
    g = ref.gold()
    for k, fr in enumerate(g["tdh_fr"]):
        assert ref.geometry(fr) == tuple(int(v) for v in g["t%d_n1_geometry" % k])
    assert ref.geometry(0.3) == (10, 7, 3) and ref.geometry(0.5) == (2, 1, 1) and ref.geometry(0.75) == (4, 1, 3) and ref.geometry(0.25) == (4, 3, 1)
    for prefix in PREFIXES:
        for dt in DTS:
            s = ref.golden_signal(prefix, dt)
            assert ref.power_ratio(s["coded1"], s["coded2"]) == s["powratio"]
    # the values the semantics quote
    for k, want in ((0, 5.0), (1, 4.2), (2, 0.2)):
        assert ref.golden_signal("t%d_n1_" % k, "c128")["powratio"] == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("prefix", PREFIXES)
def test_assembling_the_golden_parts_gives_the_golden_row(prefix, dt):
    s = ref.golden_signal(prefix, dt)
    row = ref.assemble(s["part1"], s["part2"], s["fM"], s["fM1"], s["powratio"])
    assert row.dtype == ref.DT[dt] and np.array_equal(row, s["row"])
    idx1, idx2 = ref.positions(row.shape[1], s["fM"], s["fM1"])
    assert np.array_equal(row[:, idx1], s["part1"]) and np.array_equal(row[:, idx2], s["part2_scaled"])
    assert np.array_equal(s["idx_tx"][:, idx1], s["labels1"]) and np.array_equal(s["idx_tx"][:, idx2], s["labels2"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("prefix", PREFIXES)
def test_split_at_shift_zero_returns_the_parts(prefix, dt):
    s = ref.golden_signal(prefix, dt)
    p1, p2 = ref.split(s["row"], s["fM"], s["fM1"], s["powratio"], 0)
    assert np.array_equal(p1, s["part1"])
    # part 2 was rounded once when it was divided and is rounded once more here
    eps = np.finfo(ref.DT[dt]).eps
    assert np.abs(p2 - s["part2"]).max() <= 4 * eps * np.abs(s["part2"]).max()
    sums, _ = ref.metrics(s["row"], s["idx_tx"], s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], 0)
    assert not sums[:, :, :2].any() and np.array_equal(sums[:, :, 2], np.tile([p1.shape[1], p2.shape[1]], (p1.shape[0], 1)))
    assert sums[:, :, 3].max() <= (8 * eps) ** 2 * row_len(s)


def row_len(s):
    return s["row"].shape[1]


def test_a_row_of_broken_frames_is_refused():
    x = np.ones((1, 41), np.complex128)
    with pytest.raises(ValueError):
        ref.split(x, 4, 3, 5.0, 0)
    with pytest.raises(ValueError):
        ref.align(x, 4, 3, (16, 4))


def test_the_clean_rows_align_at_zero_and_a_roll_is_found():
    for k in range(3):
        s = ref.golden_signal("t%d_n2_" % k, "c128")
        assert list(ref.align(s["row"], s["fM"], s["fM1"], s["M"])) == [0, 0]
        for r in range(s["fM"]):
            assert list(ref.align(np.roll(s["row"], -r, axis=1), s["fM"], s["fM1"], s["M"])) == [(s["fM"] - r) % s["fM"]] * 2
    # class sums carry the same information: the means are sums of class sums over the positions of the higher-order format
    s = ref.golden_signal("t0_n2_", "c128")
    S, m = ref.class_sums(s["row"], 10), ref.alignment_means(s["row"], 10, 7, (16, 4))
    via = np.array([[sum(S[row, (r + j) % 10] for r in range(7)) for j in range(10)] for row in range(2)]) / (7 * 413)
    assert np.allclose(via, m, rtol=1e-13, atol=0)


def test_a_tie_takes_the_first_shift():
    x = np.array([[1, -1, 1j, -1j] * 5], dtype=np.complex128)                # both formats with |x| = 1: every m_j is the same
    assert list(ref.align(x, 4, 3, (16, 4))) == [0] and list(ref.align(x, 10, 7, (4, 16))) == [0]


# ---- the conditions of the GPU cases
@pytest.mark.parametrize("nm", ref.NMODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c["name"] for c in ref.CASES])
def test_gpu_cases_keep_their_margins(case, dt, nm):
    s, x, labels, shifts = ref.received(case, nm, dt)
    assert x.dtype == ref.DT[dt] and x.shape == (nm, s["row"].shape[1]) and shifts[0] == case["shift"]
    # (a) the alignment is clear: the best m_j leads the runner-up by at least 2 %
    assert list(ref.align(x, s["fM"], s["fM1"], s["M"])) == list(shifts)
    assert ref.align_margin(x, s["fM"], s["fM1"], s["M"]) >= ref.ALIGN_MARGIN
    # (b) no sample - none is left out - sits within 1e-4 of a decision boundary, so complex64 rounding cannot flip a decision
    sums, tie = ref.metrics(x, labels, s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], shifts)
    assert tie >= ref.TIE_MARGIN
    assert sums[:, :, 2].sum() == x.size
    # the cases are worth measuring: errors in the higher-order format of every row
    high = 0 if s["M"][0] > s["M"][1] else 1
    assert np.all(sums[:, high, 0] > 0) and np.all(sums[:, :, 1] >= sums[:, :, 0])


def test_the_seeds_are_the_first_that_keep_the_margin():
    case = ref.CASES[0]
    assert ref.find_seeds(case) == ref.SEEDS[case["name"]]


def test_rates_weight_the_combined_ber_by_bits():
    sums = np.array([[[10, 12, 700, 7.0], [1, 1, 300, 1.2]]])
    r = ref.rates(sums, (16, 4))
    assert r["ser"][1][0] == 11 / 1000 and r["ber"][1][0] == 13 / (700 * 4 + 300 * 2)
    assert np.allclose(r["ber"][0], [[12 / 2800, 1 / 600]]) and np.allclose(r["evm"][0], np.sqrt([[0.01, 0.004]])) and r["evm"][1][0] == np.sqrt(8.2 / 1000)
