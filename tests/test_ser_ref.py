"""The restatement of the device SER harness (tests/ser_ref.py) pinned on the CPU: against the reference's own cal_ser error masks
(tests/golden/harness.npz), against the host counter bench.py uses (qampy_amd.synth.count_symbol_errors), on hand-made rows whose seven
numbers are written out here, and the two conditions that hold the inputs of tests/test_gpu_ser_edges.py: clear_of_ties moves at most
1e-3 of a case's samples and leaves every margin at 1e-4 or more, and every aligned noisy case counts an error share in [1e-4, 0.1]."""
import numpy as np
import pytest

import ser_ref as ref
from conftest import golden_cases
from qampy_amd import synth
from test_harness_golden import _expected


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("case", golden_cases("harness"), ids=lambda c: c["name"])
def test_restatement_matches_reference_cal_ser(golden, case):
    g = golden["harness"]
    al = g["ser_alphabet"].astype(np.complex128)
    idx_tx = np.stack([ref.decide(row, al)[0] for row in g["ser_tx"]])
    rx = g["ser_%s_rx" % case["name"]]
    for m in range(2):
        errors, compared, mode, k, lag, matches, W = ref.ser(rx[m], idx_tx, al, 256, 2048, 0)
        e_ref, n_ref, mode_ref, rot_ref, lag_ref = _expected(g, case, m)
        assert (mode, k, lag, compared) == (mode_ref, rot_ref, lag_ref, n_ref)
        assert errors == e_ref
        assert W == 2048 and matches > 0.8 * W


def test_restatement_matches_host_counter():
    """The scenario of test_gpu_functional.py::test_device_ser_harness_matches_host_count."""
    rng = np.random.default_rng(5)
    M, n = 16, 30000
    sig = synth.make_capture(M, n + 64, nmodes=2, snr_db=17, seed=11, dtype=np.complex128)
    tx = np.asarray(sig.symbols)
    al = np.ascontiguousarray(sig.coded_symbols, dtype=np.complex128)
    noise = (rng.normal(size=(2, n)) + 1j * rng.normal(size=(2, n))) * 0.12
    rx = np.stack([np.roll(tx[1], 7)[:n] * (-1j) + noise[0], np.roll(tx[0], -19)[:n] * (-1) + noise[1]])
    idx_tx = np.stack([ref.decide(row, al)[0] for row in tx])
    for row, want in zip(rx, ((1, 1, 7), (0, 2, -19))):
        errors, compared, mode, k, lag, matches, W = ref.ser(row, idx_tx, al, 64, 2048, 100)
        nerr, ncmp, hmode, hrot, hlag = synth.count_symbol_errors(row, tx, al, max_lag=64, trim=0)
        assert (mode, k, lag) == (hmode, hrot, hlag) == want
        d_r = synth.decide(row * np.exp(1j * hrot * np.pi / 2), al)[100:n - 100]
        d_t = synth.decide(tx[hmode], al)[100 - hlag:n - 100 - hlag]
        assert compared == d_r.size and errors == int(np.count_nonzero(d_r != d_t))
        assert 0 < errors < 0.1 * compared and W == 2048 and matches > 0.9 * W


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("name", list(ref.CASES))
def test_case_inputs_are_clear_of_ties_and_count_errors(name):
    c = ref.make(name)
    rx, al = c["rx"], c["alphabet"]
    assert np.array_equal(rx, np.round(rx * 4096) / 4096)                  # complex64 holds the same numbers
    assert c["moved"] <= 1e-3, c["moved"]
    keep = np.ones(rx.size, bool)
    keep[c["exempt"]] = False
    assert ref.min_margin(rx[keep], al) >= ref.BAR
    if c["exempt"].size:                                                     # the listed samples are exact ties, under every quarter turn
        assert all(np.all(ref.decide(rx[c["exempt"]] * 1j ** k, al)[1] == 0) for k in range(4))
    res, compared, wrong = ref.ser(rx, c["labels"], al, c["maxlag"], c["window"], c["trim"], detail=True)
    assert res == ref.expected(name)
    print("%s: moved %.2e, errors %d of %d (%.2e)" % (name, c["moved"], res[0], res[1], res[0] / max(res[1], 1)))
    if c["band"]:
        assert (res[2], res[3], res[4]) == (0 if c["identical"] else c["mode"], (-c["turns"]) % 4, c["lag"])
        assert 1e-4 <= res[0] / res[1] <= 0.1, res
    if c["N"] - 2 * c["trim"] >= ref.TRIP - 1:                               # errors in every pass of the counting kernel, the last one too
        per_trip = np.bincount((wrong - c["trim"]) // ref.TRIP, minlength=(c["N"] - 2 * c["trim"] + ref.TRIP - 1) // ref.TRIP)
        assert per_trip.min() > 0, per_trip
        last = wrong[wrong >= c["N"] - c["trim"] - 300]
        assert last.size > 0


def test_received_is_a_linear_shift():
    al = ref.alphabet("qam16")
    lab = ref.labels(1, 50, 16, 3)[0]
    for lag in (-5, 0, 9):
        x, _ = ref.received(lab, al, 2, lag, 60, None, 4)
        d = ref.decide(x * 1j ** 2, al)[0]
        i = np.arange(60)
        have = (i - lag >= 0) & (i - lag < 50)
        assert np.array_equal(d[have], lab[(i - lag)[have]]) and np.count_nonzero(have) == {-5: 45, 0: 50, 9: 50}[lag]


def test_clear_of_ties_moves_what_is_close_and_nothing_else():
    al = ref.alphabet("qam4")
    x = np.array([0.5 + 0.25j, 0.5 + 2e-5j, 3e-5 - 0.75j, -0.5 - 0.5j])     # the second and third sit on a boundary to 1e-4
    y, share = ref.clear_of_ties(x, al)
    assert share == 0.5 and y[0] == x[0] and y[3] == x[3]
    idx = ref.decide(x, al)[0]
    assert np.array_equal(y[1:3], np.round(al[idx[1:3]] * 4096) / 4096)
    assert ref.min_margin(y, al) >= ref.BAR


def test_count_errors_restatement():
    rx, tx = np.array([0, 1, 2, 3, 0, 1]), np.array([1, 2, 3, 9])
    assert ref.count_errors(rx, tx, 6, 0) == 4               # 0:1 1:2 2:3 3:9, two more without a partner
    assert ref.count_errors(rx, tx, 6, 1) == 1               # rx[1..4] against tx[0..3]: only 0 != 9
    assert ref.count_errors(rx, tx, 6, -1) == 3              # rx[0..2] against tx[1..3]
    assert ref.count_errors(rx, tx, 2, 1) == 0               # n cuts the received side
    assert ref.count_errors(rx, tx, 0, 0) == 0


# ------------------------------------------------------------------------------------------------ by hand
Q = np.array([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j]) / np.sqrt(2)          # point k is point 0 turned by j^k


def test_decide_takes_the_first_minimum_of_the_plain_distance():
    idx, margin = ref.decide(np.array([0.5 + 0.5j, 0j, 1j, -2.]), Q)
    assert list(idx) == [0, 0, 0, 1]                          # 0 is equally far from all four, 1j from points 0 and 1, -2 from 1 and 2
    a = 1 / np.sqrt(2)
    np.testing.assert_allclose(margin, [np.hypot(0.5 + a, 0.5 - a) - np.hypot(0.5 - a, 0.5 - a), 0, 0, 0], atol=1e-15)
    assert np.all(np.isinf(ref.decide(np.array([1., 2j]), np.array([0.3]))[1]))


def test_by_hand_first_maximum_between_identical_modes():
    lab = np.array([[0, 1, 2, 3, 0, 1]] * 2)
    # rotation k at lag -k (mod 4) matches too, but on 5 symbols only: the two modes at rotation 0, lag 0 tie with 6, and mode 0 comes first
    assert ref.ser(Q[lab[1]], lab, Q, 1, 0, 0) == (0, 6, 0, 0, 0, 6, 6)


def test_by_hand_first_maximum_between_lags():
    # a constant sequence longer than the row: lags -2, -1 and 0 all match the 5 symbols, lag 1 and 2 lose the first ones
    assert ref.ser(Q[np.zeros(5, int)], np.zeros((1, 9), int), Q, 2, 0, 0) == (0, 5, 0, 0, -2, 5, 5)


def test_by_hand_one_point_alphabet():
    # every hypothesis matches the whole window (symbols 3 and 4, two of maxlag clear of both ends): the first one wins, and at lag -2 the last
    # two symbols have no partner
    one = np.array([0.75 + 0.5j])
    assert ref.ser(np.full(8, 0.1 - 3j), np.zeros((3, 8), int), one, 2, 2, 0) == (0, 6, 0, 0, -2, 2, 2)


def test_by_hand_default_window_is_4096():
    lab = np.zeros((1, 8), int)
    for w in (0, -5):
        assert ref.ser(Q[lab[0]], lab, Q, 0, w, 0) == (0, 8, 0, 0, 0, 8, 8)                 # clamped to the row
        assert ref.window_of(5000, w, 0) == (4096, 452) and ref.window_of(5001, w, 0) == (4096, 452)
    lab = ref.labels(1, 5000, 4, 1)
    assert ref.ser(Q[lab[0]], lab, Q, 0, 0, 0) == (0, 5000, 0, 0, 0, 4096, 4096)


def test_by_hand_clamp_and_odd_start():
    tx = np.zeros((1, 8), int)
    # N - 2 trim = 4 < window: W = 4, start = 2; the four middle symbols match
    assert ref.ser(Q[[1, 1, 0, 0, 0, 0, 1, 1]], tx, Q, 0, 100, 2) == (0, 4, 0, 0, 0, 4, 4)
    # N - 2 trim - W = 3: start = 1 + 3 // 2 = 2, the window is symbols 2, 3, 4 - the only three in a row that match; a start of 1 or 3 sees two
    assert ref.ser(Q[[1, 1, 0, 0, 0, 1, 1, 1]], tx, Q, 0, 3, 1) == (3, 6, 0, 0, 0, 3, 3)
    assert ref.window_of(8, 3, 1) == (3, 2)


def test_by_hand_lag_rotation_and_mode():
    # the row is mode 1 delayed by two symbols and turned by j: turning it by j^3 gives the labels back; its first two symbols are unrelated
    lab = np.array([[0, 0, 1, 1, 2, 2, 3, 3], [0, 1, 3, 2, 0, 3, 1, 2]])
    row = np.concatenate([Q[[2, 2]], Q[lab[1][:6]]]) * 1j
    assert ref.ser(row, lab, Q, 2, 0, 0) == (0, 6, 1, 3, 2, 6, 8)
    assert ref.ser(row, lab, Q, 2, 0, 1) == (0, 5, 1, 3, 2, 5, 6)               # trim 1: symbols 1 .. 6, of which symbol 1 has no partner
