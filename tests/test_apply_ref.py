"""The restatement of the butterfly FIR (tests/apply_ref.py) against the reference's outputs (tests/golden/apply.npz, all 14 vectors, the two
real-tap ones through the stacking), and the launch plans qh_apply_plan answers for the sizes tests/test_gpu_apply.py runs.  No GPU needed.

The bars are those of tests/test_gpu_parity.py::test_apply_filter_golden."""
import numpy as np
import pytest

import apply_ref as ref
from conftest import CT, golden_cases

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
KIB64 = 65536


@pytest.mark.parametrize("case", golden_cases("apply"), ids=lambda c: c["name"])
def test_restatement_matches_golden(golden, case):
    g = golden["apply"]
    n, dn = case["name"], case["dtype"]
    E, wx, want = golden.input(case["input"], CT[dn]), g[n + "__wx"], g[n + "__out"]
    assert wx.shape[-1] == case["ntaps"]
    if case.get("realtaps"):
        assert not np.iscomplexobj(wx) and wx.shape[0] == 2 * E.shape[0]
        out = ref.apply_filter(ref.stack_real(E), case["os"], wx, case["modes"])
        assert out.dtype == np.longdouble
        out = ref.unstack_real(out)
    else:
        out = ref.apply_filter(E, case["os"], wx, case["modes"])
    assert out.dtype == np.clongdouble and out.shape == want.shape
    np.testing.assert_allclose(out.astype(np.complex128), want, rtol=1e-12 if dn == "c128" else 2e-5, atol=1e-13 if dn == "c128" else 2e-6)


def test_restatement_is_the_plain_double_loop():
    """Against the formula written out sample by sample, with exactly representable values: the window view and the einsum index what they should."""
    rng = np.random.default_rng(3)
    for real in (False, True):
        for os_, ntaps, L, modes in ((1, 3, 11, None), (2, 4, 14, [2, 0]), (3, 5, 17, [1, 1, 0]), (4, 2, 9, [0]), (2, 5, 4, None)):
            E = rng.integers(-8, 9, (3, L)).astype(np.float64)
            wx = rng.integers(-8, 9, (3, 3, ntaps)).astype(np.float64)
            if not real:
                E, wx = E + 1j * rng.integers(-8, 9, E.shape), wx + 1j * rng.integers(-8, 9, wx.shape)
            rows = range(3) if modes is None else modes
            N = ref.n_out(L, ntaps, os_)
            want = np.zeros((len(rows), N), E.dtype)
            for j, m in enumerate(rows):
                for i in range(N):
                    for k in range(3):
                        for t in range(ntaps):
                            want[j, i] += E[k, i * os_ + t] * wx[m, k, t]
            got = ref.apply_filter(E, os_, wx, modes)
            assert got.dtype == (np.longdouble if real else np.clongdouble) and got.shape == want.shape
            assert np.array_equal(got, want)
    assert ref.n_out(4, 5, 2) == 0 and ref.n_out(5, 5, 2) == 0 and ref.n_out(6, 5, 2) == 1


def test_stacking_round_trip():
    E = np.arange(12).reshape(2, 6) + 1j * np.arange(12, 24).reshape(2, 6)
    S = ref.stack_real(E)
    assert S.shape == (4, 6) and not np.iscomplexobj(S) and S.flags.c_contiguous
    assert np.array_equal(S[:2], E.real) and np.array_equal(S[2:], E.imag) and np.array_equal(ref.unstack_real(S), E)


# (dtype, nmodes, os, ntaps, nsel) -> (per_thread, grid_y, lds): the forms tests/test_gpu_apply.py is there to reach, worked out by hand from the
# kernels' LDS layout - complex: nmodes rows of ((256 P - 1) os + ntaps + 2, rounded down to even) samples + 2 nmodes (ntaps + 1) samples of
# taps; real: nmodes rows of (256 P - 1) os + ntaps samples; P = 4 when that fits 160 KiB, else 1
PLANS = [
    ((C64, 2, 2, 41, 2), (4, 1, 34752)), ((C128, 2, 2, 41, 2), (4, 1, 69504)), ((C128, 2, 2, 40, 2), (4, 1, 69440)),
    ((C128, 8, 2, 21, 8), (1, 4, 73728)), ((C64, 4, 16, 33, 4), (1, 2, 133824)), ((C64, 16, 2, 37, 16), (1, 8, 79872)),
    ((C64, 3, 2, 7, 3), (4, 2, 49680)), ((C64, 5, 3, 7, 5), (4, 3, 123760)), ((C64, 5, 2, 7, 1), (4, 1, 82800)), ((C64, 4, 2, 7, 16), (4, 8, 66240)),
    ((F32, 4, 2, 9, 4), (4, 4, 32880)), ((F64, 4, 2, 9, 3), (4, 3, 65760)), ((F64, 8, 4, 9, 1), (1, 1, 65856)), ((F32, 16, 4, 9, 16), (1, 16, 65856)),
    ((C128, 2, 2, 1535, 2), (1, 1, 163776)), ((C64, 2, 2, 3242, 2), (1, 1, 163840)),
]


@pytest.mark.parametrize("args,want", PLANS, ids=["%s-%d-os%d-t%d-sel%d" % ((np.dtype(a[0]).name,) + a[1:]) for a, _ in PLANS])
def test_plan_of_the_tested_forms(args, want):
    p = ref.plan(*args)
    assert p is not None
    assert (p["per_thread"], p["grid_y"], p["lds"]) == want and p["tile"] == 256 * p["per_thread"]


def test_plan_boundary_and_refusals():
    """The accept / reject boundary in the tap count, found by search: the accepted plan fits the 160 KiB of a CU's LDS, and one more tap does not."""
    assert ref.largest_ntaps(C128, 2, 2, 2) == 1535 and ref.largest_ntaps(C64, 2, 2, 2) == 3242
    for dt, nm in ((C64, 2), (C128, 2), (C64, 16), (F32, 2), (F64, 2), (F64, 8)):
        n = ref.largest_ntaps(dt, nm, 2, nm)
        p = ref.plan(dt, nm, 2, n, nm)
        assert p["per_thread"] == 1 and KIB64 < p["lds"] <= 160 * 1024 and ref.plan(dt, nm, 2, n + 1, nm) is None
    # what the launch's argument check refuses, the plan refuses: no device is touched for either
    for bad in ((C64, 2, 0, 5, 2), (C64, 2, 2, 5, 0), (C64, 2, 2, 5, 17), (C64, 0, 2, 5, 1), (C64, 2, 2, 0, 1), (C64, 2, -1, 5, 1),
                (F64, 2, 2 ** 31 - 1, 5, 1), (C128, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1)):
        assert ref.plan(*bad) is None, bad
    from qampy_amd import _lib
    lib = _lib.load()
    assert lib.qh_apply_plan(1, 2, 2, 2, 5, 2, None, None, None, None) == _lib.QH_ERR_ARG          # no such element type
    assert lib.qh_apply_plan(1, 4, 2, 2, 5, 2, None, None, None, None) == _lib.QH_OK               # any pointer may be NULL
    assert lib.qh_apply_plan(1, 4, 2, 2, 3243, 2, None, None, None, None) == _lib.QH_ERR_ARG and b"LDS" in lib.qh_last_error()
