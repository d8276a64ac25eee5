"""
The restatement the device test of the phase search's tail is judged by (tests/bps_unwrap_ref.py), held to numpy and to rows worked out by
hand, and the conditions on the shared cases - checked on the oracle's indices, before anything runs on a device.
"""
import numpy as np
import pytest

from oracle import oracle
from qampy_amd.core import hip_dsp
import bps_unwrap_ref as ref
from bps_unwrap_ref import CASES, LONG_CASE, RT
from test_gpu_parity import _unwrap_quarter_turns

DTYPES = ["c64", "c128"]
_idx = {}


def oracle_idx(case, dn):
    """Indices of the oracle's search on every row of a shared case (formed once)."""
    key = (case["name"], dn)
    if key not in _idx:
        E, alphabet = ref.build(case, dn)
        grid = hip_dsp.test_angle_grid(case["A"], RT[dn])
        _idx[key] = np.stack([oracle.bps(np.ascontiguousarray(r), grid, alphabet, case["N"]) for r in E])
    return _idx[key]


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_equals_numpy_and_the_hand_written_rule(case, dn):
    A, N, L = case["A"], case["N"], case["L"]
    grid = ref.host_grid(A, dn)
    idx = oracle_idx(case, dn)
    assert not idx[:, :N].any() and not idx[:, L - N:].any() and idx.max() < A
    for row in idx:
        ph, K, val = ref.recover_ref(grid, row, N)
        assert ph.dtype == RT[dn] and not K[:N].any() and not K[L - N:].any() and K[N] == 0
        assert np.array_equal(ph[:N], grid[row[:N]]) and np.array_equal(ph[L - N:], grid[row[L - N:]])
        # the rule of numpy's unwrap, spelled out operation by operation
        assert np.array_equal(K[N:L - N], _unwrap_quarter_turns(grid, row, N))
        # float64 unwrap of the same grid values: the same decision wherever the jump is not exactly half the grid
        p4 = 4 * grid[row[N:L - N]].astype(np.float64)
        K64 = np.rint((np.unwrap(p4) - p4) / (2 * np.pi)).astype(np.int64)
        sure = 2 * np.abs(np.diff(row[N:L - N].astype(np.int64))) != A
        assert np.array_equal(np.diff(K[N:L - N])[sure], np.diff(K64)[sure])
        # the value of numpy's own ph, up to the rounding of its running sum: one rounding of at most u |4 ph| per wrap added, two more
        # for the sum with the raw phase and the division
        nw = np.count_nonzero(np.diff(K))
        assert np.abs(ph - val).max() <= (nw + 2) * ref.U[dn] * (1 + np.abs(val).max())


@pytest.mark.parametrize("dn", DTYPES)
def test_restatement_on_rows_written_out_by_hand(dn):
    """A = 4: 4 * grid is -pi, -pi/2, 0, pi/2.  A jump of three entries is 3 pi / 2 and wraps; entries 0 and 2 are -pi / 4 and 0, exact in
    both precisions, so that the jump between them is pi itself and numpy leaves it alone, up and down."""
    grid = ref.host_grid(4, dn)
    assert grid[2] == 0 and RT[dn](4) * grid[0] == -RT[dn](np.pi)
    # a step of pi itself: numpy's correction is 0 whether or not |dd| < pi lets it through (mod gives -pi, the fix makes it pi going up), so
    # the strictness of that comparison cannot be seen from outside
    for step in (np.pi, -np.pi):
        assert np.array_equal(np.unwrap(np.array([0, step], RT[dn])), np.array([0, step], RT[dn]))
    rows = [
        ([0, 0, 3, 3, 0, 0], 1, [0, 0, -1, -1, 0, 0]),                                 # +3 wraps down, -3 back up
        ([0, 3, 0, 3, 0], 1, [0, 0, 1, 0, 0]),                                         # -3 first: K goes positive
        ([0, 0, 2, 0, 2, 3, 0, 2, 0, 0], 1, [0, 0, 0, 0, 0, 0, 1, 1, 1, 0]),           # exactly 2 up and down: nothing; 3 -> 0: +1
        ([3, 3, 0, 3, 0, 0, 3, 3], 2, [0, 0, 0, -1, 0, 0, 0, 0]),                      # N = 2: the steps into and out of the edges do not count
    ]
    for idx, N, K in rows:
        ph, got, val = ref.recover_ref(grid, np.array(idx), N)
        assert got.tolist() == K, (idx, got)
        assert np.array_equal(val, grid[idx].astype(np.float64) + np.pi / 2 * np.array(K))
    for at in (1023, 1024):                                                            # a wrap on the last / first element of a chunk
        idx = np.zeros(1030, np.int64)
        idx[at:-1] = 3
        _, K, _ = ref.recover_ref(grid, idx, 1)
        assert not K[:at].any() and np.all(K[at:-1] == -1) and K[-1] == 0
        f = ref.features(idx, 4, 1, grid)
        assert (f["down"], f["up"], f["kmin"], f["kmax"]) == (1, 0, -1, 0)
        assert (f["last_down"], f["first_down"]) == ((1, 0) if at == 1023 else (0, 1))
    f = ref.features(np.array(rows[2][0]), 4, 1, grid)
    assert (f["half"], f["half_left"], f["half_corrected"], f["up"], f["down"]) == (5, 5, 0, 1, 0)
    for L, N in ((1, 8), (15, 8), (16, 8), (17, 8)):                                   # empty interior, empty, empty, one element
        ph, K, val = ref.recover_ref(grid, np.zeros(L, np.int64), N)
        assert not K.any() and np.all(ph == grid[0])


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_shared_cases_reach_the_edges_they_are_there_for(case, dn):
    f = ref.case_features(oracle_idx(case, dn), case["A"], case["N"], ref.host_grid(case["A"], dn))
    print(case["name"], dn, f)
    ref.check_features(case, f, dn)


def test_an_exact_half_jump_is_corrected_and_one_is_left_alone_in_double():
    """The rounding of the float64 grid puts some jumps of exactly A / 2 entries above pi and numpy corrects them: the device must follow
    numpy there, not the ideal grid.  At least one shared complex128 case holds both outcomes."""
    both = []
    for case in CASES:
        f = ref.case_features(oracle_idx(case, "c128"), case["A"], case["N"], ref.host_grid(case["A"], "c128"))
        if f["half_corrected"] and f["half_left"]:
            both.append((case["name"], f["half_corrected"], f["half_left"]))
    print(both)
    assert both


def test_long_row_wraps_across_more_than_1024_chunks():
    case = LONG_CASE
    f = ref.case_features(oracle_idx(case, "c64"), case["A"], case["N"], ref.host_grid(case["A"], "c64"))
    print(case["name"], f)
    assert -(-case["L"] // ref.CHUNK) == 1026
    ref.check_features(case, f, "c64")
    assert f["first_up"] and f["first_down"] and f["last_up"] and f["last_down"]
