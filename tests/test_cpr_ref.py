"""The float64 restatements of tests/cpr_ref.py against the reference's own results (tests/golden/cpr.npz, written by gen_golden_cpr.py), and
the conditions under which the parity of a kernel with the restatement is well defined, for every shared case.  No GPU."""
import os

import numpy as np
import pytest

import cpr_ref

VV_CASES, P16_CASES = cpr_ref.GOLDEN_VV, cpr_ref.GOLDEN_P16

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpr.npz"))
TOL = 1e-12


def _x(key):
    q = GOLD[key].astype(np.float64) / float(GOLD["scale"])
    return q[..., 0] + 1j * q[..., 1]


@pytest.mark.parametrize("case", VV_CASES, ids=[c[0] for c in VV_CASES])
def test_vv_restatement_is_the_reference(case):
    c, M, N, nm, L, seed = case
    x = _x("x_vv_" + c)
    assert x.shape == (nm, L)
    field, trace, umargin, _ = cpr_ref.viterbiviterbi(x, N, M)
    assert umargin >= 0.25
    ph = GOLD["vv_ph_" + c]
    assert trace.shape == ph.shape == (nm, L - N + 1)
    err_t = np.max(np.abs(trace - ph)) / max(1.0, np.max(np.abs(ph)))
    err_f = np.max(np.abs(field - GOLD["vv_E_" + c]))
    print("vv %s: trace %.3g field %.3g margin %.3g" % (c, err_t, err_f, umargin))
    assert err_t <= TOL and err_f <= TOL
    assert np.array_equal(GOLD["vv_phlast_" + c], ph[-1])                        # the 2-d call returns the last row's trace
    o = (N - 1) // 2
    edges = np.ones(L, bool)
    edges[o:o + L - N + 1] = False
    assert np.all(GOLD["vv_E_" + c][:, edges] == 0) and np.all(field[:, edges] == 0)


@pytest.mark.parametrize("case", P16_CASES, ids=[c[0] for c in P16_CASES])
def test_partition_restatement_is_the_reference(case):
    c, Nb, nm, L, seed = case
    x = _x("x_p16_" + c)
    field, trace, umargin, rmargin = cpr_ref.phase_partition_16qam(x, Nb)
    assert umargin >= 0.1 and rmargin >= 1e-9 and cpr_ref.tie_margin(x) >= 1e-4
    ph = GOLD["p16_ph_" + c]
    assert trace.shape == ph.shape == (nm, L)
    err_t = np.max(np.abs(trace - ph)) / max(1.0, np.max(np.abs(ph)))
    print("p16 %s: trace %.3g margins %.3g %.3g" % (c, err_t, umargin, rmargin))
    assert err_t <= TOL
    # the reference's field is every row turned by the RAW fourth-power angle of the last row; this repository turns every row by its own trace
    ref_field = x * np.exp(-4j * (ph[-1] + np.pi / 4))
    assert np.max(np.abs(GOLD["p16_E_" + c] - ref_field)) <= TOL
    assert np.max(np.abs(field - x * np.exp(-1j * ph))) <= TOL


def test_gamma_of_the_partition():
    assert cpr_ref.GAMMA_132 == 25 / 33


CASES = cpr_ref.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_conditions(case):
    """Conditions, not measurements: every shared case keeps its unwrap decisions and ring classes clear of a flip."""
    x = case["make"]()
    field, trace, umargin, rmargin = cpr_ref.run(case, x)
    assert np.array_equal(np.round(x * 4096), x * 4096) and np.abs(x).max() < 8      # complex64 holds the input exactly
    if case["kind"] == "vv":
        assert umargin >= 0.25
        assert trace.shape == (x.shape[0], x.shape[1] - case["N"] + 1)
    else:
        assert umargin >= 0.1 and rmargin >= 1e-9 and cpr_ref.tie_margin(x) >= 1e-4
        assert trace.shape == x.shape


def test_long_rows_conditions():
    for extra, nchunk in ((0, 1024), (1024, 1025)):
        _, trace, umargin, _ = cpr_ref.viterbiviterbi(cpr_ref.long_vv_row(extra), 11, 4)
        assert umargin >= 0.25 and -(-trace.shape[1] // 1024) == nchunk and np.ptp(trace) > 20     # many turns
    x = cpr_ref.long_p16_row()
    _, _, umargin, rmargin = cpr_ref.phase_partition_16qam(x, 64)
    assert umargin >= 0.1 and rmargin >= 1e-9 and cpr_ref.tie_margin(x) >= 1e-4


def test_wrap_ramp_wraps_on_the_chunk_boundary():
    x, idx = cpr_ref.wrap_ramp()
    theta = np.angle((x[0] / np.abs(x[0])) ** 4)
    c, K, margin = cpr_ref.wrap_counts(theta)
    assert [int(c[i - 1]) for i in idx] == [1, -1, 1] and idx == (1023, 1024, 1025)
    assert margin >= 0.25


def test_zero_sample_counts_as_one():
    x = np.array([[1 + 1j, 0, 1 - 1j, -1 + 1j]])
    field, trace, _, _ = cpr_ref.viterbiviterbi(x, 1, 4)
    raw = (trace[0, 1] * 4 + np.pi) % (2 * np.pi)                                 # the raw angle at the zero sample: angle(1) = 0
    assert min(raw, 2 * np.pi - raw) < 1e-12 and np.isfinite(trace).all() and field[0, 1] == 0
