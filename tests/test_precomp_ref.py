"""The numpy restatement of the digital pre-compensation (tests/precomp_ref.py) against the reference's results (tests/golden/precomp.npz,
recorded with ``python -O tests/golden/gen_golden_precomp.py``): pattern numbers and the dyadic tables compare equal, the arcsin and the DAC
pre-emphasis to 1e-11 of the largest reference value.  The GPU tests then hold the kernels against the restatement."""
import numpy as np
import pytest

import precomp_ref as pr


@pytest.fixture(scope="module")
def gold(golden):
    return golden["precomp"]


@pytest.fixture(scope="module")
def cs():
    return pr.cases()


def unscaled(v):
    return (v[..., 0] + 1j * v[..., 1]) / pr.Q


def test_the_inputs_are_the_stored_ones_and_dyadic(gold, cs):
    for i, c in enumerate(cs["index"]):
        assert np.array_equal(c["x"] * pr.Q, np.rint(c["x"] * pr.Q)) and c["L"] == c["x"].size <= 4099
        if c["L"] >= c["mem_len"]:
            assert np.array_equal(unscaled(gold["idx_%d_x" % i]), c["x"])
    for c in cs["lut"]:
        assert np.array_equal(unscaled(gold["lut_%s_tx" % c["name"]]), c["tx"]) and np.array_equal(unscaled(gold["lut_%s_rx" % c["name"]]), c["rx"])
        err = c["tx"] - c["rx"]
        assert max(np.abs(err.real).max(), np.abs(err.imag).max()) <= 1 and np.array_equal(err * pr.Q, np.rint(err * pr.Q))
        assert np.array_equal(c["tx"].astype(np.complex64).astype(np.complex128), c["tx"]) and np.array_equal(c["rx"].astype(np.complex64).astype(np.complex128), c["rx"])
    assert np.array_equal(unscaled(gold["tie_x"]), cs["tie"])
    assert np.array_equal(gold["nan_x"][:, 0], cs["nan"].real, equal_nan=True) and np.array_equal(gold["nan_x"][:, 1], cs["nan"].imag, equal_nan=True)


def test_the_cases_cover_what_they_are_meant_to(cs):
    kinds = {c["kind"] for c in cs["index"]}
    assert kinds == set(pr.RAIL) | set(pr.ALPHABET)
    assert {c["mem_len"] for c in cs["index"]} == {1, 2, 3, 5, 7}
    assert {1, 255, 256, 257, 4099} <= {c["L"] for c in cs["index"]} and any(c["L"] == 5 and c["mem_len"] == 7 for c in cs["index"])
    sizes = sorted(len(pr.ref_sym_of(c["kind"])[0]) ** c["mem_len"] if c["kind"] in pr.ALPHABET else pr.RAIL[c["kind"]] ** c["mem_len"] for c in cs["lut"])
    assert sizes == [64, 4096, 32768, 262144]


def test_no_sample_sits_near_a_decision_boundary_except_the_ties(cs):
    """2^-11 is half the grid of the inputs: a decision that a rounding could move would show here, on the restatement alone"""
    rows = [(c["kind"], c["x"]) for c in cs["index"]] + [(c["kind"], c["tx"]) for c in cs["lut"]]
    for kind, x in rows:
        lev_I, lev_Q, alphabet = pr.levels_of(kind)
        if alphabet is None:
            assert min(pr.margin(x.real, lev_I).min(), pr.margin(x.imag, lev_Q).min()) >= 2.0 ** -11
        else:
            assert pr.margin(x, alphabet).min() >= 2.0 ** -11
    lev = pr.rail_levels(4)
    x = cs["tie"]
    tied = (pr.margin(x.real, lev) == 0) | (pr.margin(x.imag, lev) == 0)
    assert 10 <= np.count_nonzero(tied) < 20
    assert min(pr.margin(x.real, lev)[pr.margin(x.real, lev) > 0].min(), pr.margin(x.imag, lev)[pr.margin(x.imag, lev) > 0].min()) >= 2.0 ** -11
    ok = np.isfinite(cs["nan"].real) & np.isfinite(cs["nan"].imag)
    assert np.count_nonzero(~ok) == 3 and pr.margin(cs["nan"].real[ok], lev).min() >= 2.0 ** -11 and pr.margin(cs["nan"].imag[ok], lev).min() >= 2.0 ** -11


def test_pattern_index_equals_the_reference(gold, cs):
    seen = 0
    for i, c in enumerate(cs["index"]):
        if c["L"] < c["mem_len"]:
            continue
        a, b = pr.pattern_index(c["x"], *pr.levels_of(c["kind"]), c["mem_len"])
        assert np.array_equal(a, gold["idx_%d_I" % i]) and np.array_equal(b, gold["idx_%d_Q" % i]), i
        seen += 1
    assert seen >= 15


def test_the_window_wraps_more_than_once():
    """L < mem_len, where the reference's rolling window reads past its buffer: the rule, spelled out"""
    lev = np.array([1, 0, 1, 1, 0])
    assert list(pr.window_index(lev, 2, 7)) == [int("".join(str(lev[(i - 3 + j) % 5]) for j in range(7)), 2) for i in range(5)]
    assert list(pr.window_index(np.array([2]), 3, 4)) == [2 * 27 + 2 * 9 + 2 * 3 + 2]


def test_a_tie_goes_to_the_lower_level_and_a_nan_to_level_0(gold, cs):
    lev = pr.rail_levels(4)
    assert list(pr.decide(np.array([-2., 0., 2., np.nan, -3., 3.]), lev)) == [0, 1, 2, 0, 0, 3]
    for name in ("tie", "nan"):
        a, b = pr.pattern_index(cs[name], lev, lev, None, 3)
        assert np.array_equal(a, gold[name + "_I"]) and np.array_equal(b, gold[name + "_Q"])
    a, _ = pr.pattern_index(cs["nan"], lev, lev, None, 3)
    assert (a[7] // 4) % 4 == 0 and (a[255] // 4) % 4 == 0


@pytest.mark.parametrize("which", pr.LUT_MASKS)
def test_the_dyadic_table_equals_the_reference(gold, cs, which):
    for c in cs["lut"]:
        lv = pr.levels_of(c["kind"])
        N = (lv[0].size if lv[2] is None else lv[2].size) ** c["mem_len"]
        a, b = pr.pattern_index(c["tx"], *lv, c["mem_len"])
        assert np.array_equal(a, gold["lut_%s_I" % c["name"]]) and np.array_equal(b, gold["lut_%s_Q" % c["name"]])
        mask = pr.mask_of(which, c["L"])
        ea, nI, nQ = pr.lut(c["tx"], c["rx"], a, b, N, mask)
        at, val = pr.nonzero_table(ea)
        assert ea.dtype == np.complex128 and ea.shape == (N,)
        assert np.array_equal(at, gold["lut_%s_%s_at" % (c["name"], which)]) and np.array_equal(val, gold["lut_%s_%s_ea" % (c["name"], which)])
        assert nI.sum() == nQ.sum() == (c["L"] if mask is None else np.count_nonzero(mask))
        if which == "empty":
            assert not ea.any()
        # the same values in complex64, the same table
        ea32, _, _ = pr.lut(c["tx"].astype(np.complex64), c["rx"].astype(np.complex64), a, b, N, mask)
        assert np.array_equal(ea32, ea)


def test_apply_is_the_users_statement(cs):
    c = cs["lut"][0]
    a, b = pr.pattern_index(c["tx"], *pr.levels_of(c["kind"]), c["mem_len"])
    ea, _, _ = pr.lut(c["tx"], c["rx"], a, b, 64)
    assert np.array_equal(pr.apply_lut(c["tx"], ea, a, b), c["tx"] + ea[a].real + 1j * ea[b].imag)
    assert np.array_equal(pr.apply_lut(c["tx"], ea, a, b, gain=-0.5), c["tx"] - 0.5 * (ea[a].real + 1j * ea[b].imag))


def test_comp_mod_sin_equals_the_reference(gold):
    x = pr.mod_sin_input()
    assert np.array_equal(x, gold["sin_x"])
    for key, vpi in (("sin_real", 1.14), ("sin_cplx", 1.2 + 0.9j)):
        want, got = gold[key], pr.comp_mod_sin(x, vpi)
        assert np.array_equal(np.isnan(got.real), np.isnan(want.real)) and np.array_equal(np.isnan(got.imag), np.isnan(want.imag))
        # numpy forms 1j * (the quadrature rail) as a complex product: a NaN there also lands in the real part
        out_re, out_im = ~(np.abs(x.real) <= 1), ~(np.abs(x.imag) <= 1)
        assert np.count_nonzero(out_re) == np.count_nonzero(out_im) == 5
        assert np.array_equal(np.isnan(want.real), out_re | out_im) and np.array_equal(np.isnan(want.imag), out_im)
        scale = np.nanmax(np.abs(np.concatenate([want.real, want.imag])))
        assert np.nanmax(np.abs(np.concatenate([got.real - want.real, got.imag - want.imag]))) <= 1e-11 * scale
    clipped = pr.comp_mod_sin(x, 1.14, clip=0.9)
    assert not np.isnan(clipped.real).any() and not np.isnan(clipped.imag).any()
    assert np.array_equal(clipped, pr.comp_mod_sin(np.clip(x.real, -0.9, 0.9) + 1j * np.clip(x.imag, -0.9, 0.9), 1.14))


@pytest.mark.parametrize("case", pr.DAC_CASES, ids=[c[0] for c in pr.DAC_CASES])
def test_comp_dac_resp_equals_the_reference(gold, case):
    name, fb, n, beta, papr, prms, os_ = case
    want, got = gold["dac_" + name], pr.comp_dac_resp(fb, n, beta, PAPR=papr, prms_dac=prms, os=os_)
    assert want.shape == got.shape == (n,) and np.all(np.isfinite(want))
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    assert np.count_nonzero(want) < n                                 # the stop band is exactly 0
    assert np.array_equal(got == 0, want == 0)
