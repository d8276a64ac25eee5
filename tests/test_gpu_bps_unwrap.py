"""
The tail of ``qh_bps_recover_*_dev`` on a real MI355X - grid look-up, ``np.unwrap`` of the interior as an integer prefix scan over chunks of
1024, de-rotation (csrc/bps.hip from "unwrap + de-rotation" on) - against numpy's own unwrap (tests/bps_unwrap_ref.py), restated from the
indices the same call returns: the search itself is judged elsewhere.  Both precisions, the host's grid and the one formed on the device,
wraps of both signs on every element of a chunk, jumps of exactly half the grid, rows whose interior is empty or ends on a chunk boundary,
more rows than two and more chunks than the scan has threads.  Then the point-wise kernels at the end of bps.hip against numpy.
"""
import functools

import numpy as np
import pytest

from conftest import CT, RT, TOL
import bps_unwrap_ref as ref
from bps_unwrap_ref import CASES, EDGE_CASE, JUMP_CASES, LONG_CASE, U
from qampy_amd import _lib
from qampy_amd.core import hip_dsp
from qampy_amd.core.equalisation import hip_equalisation as hk

pytestmark = pytest.mark.gpu

D = _lib.DeviceArray
DTYPES = ["c64", "c128"]


def _close(a, b, dn):
    np.testing.assert_allclose(a, b, rtol=TOL[dn]["rtol"], atol=TOL[dn]["atol"])


@functools.lru_cache(maxsize=None)
def _built(name, dn):
    case = next(c for c in CASES + [LONG_CASE] if c["name"] == name)
    return ref.build(case, dn)


def recover(E, alphabet, A, N, dn, host_grid=True, nparts=1):
    """``hip_dsp.bps_recover_dev`` on host arrays: ``(idx, ph, Eout)`` as it leaves them in HBM."""
    dE, dsy = D.from_host(E), D.from_host(alphabet)
    dang = D.from_host(ref.host_grid(A, dn)) if host_grid else None
    idx, ph, out = D(E.shape, np.int32), D(E.shape, RT[dn]), D(E.shape, CT[dn])
    for part in range(nparts):
        hip_dsp.bps_recover_dev(dE, A, dsy, N, idx, ph, out, angles=dang, part=part, nparts=nparts)
    _lib.sync()
    return idx.to_host(), ph.to_host(), out.to_host()


def judge(E, got, grid, N, dn):
    """Every assertion on one call's ``(idx, ph, Eout)`` against the restatement on ``grid``; returns the largest ``|ph - value|`` in units of
    ``u (|value| + 1)`` and the largest field error as a share of what conftest's TOL allows."""
    idx, ph, out = got
    nm, L = E.shape
    u = U[dn]
    assert idx.shape == ph.shape == out.shape == E.shape and ph.dtype == RT[dn] and out.dtype == CT[dn]
    assert not idx[:, :N].any() and not idx[:, max(L - N, 0):].any() and idx.min() >= 0 and idx.max() < grid.size
    worst = 0.
    for m in range(nm):
        _, K, val = ref.recover_ref(grid, idx[m], N)
        raw = grid[idx[m]]
        Kdev = np.rint((ph[m].astype(np.float64) - raw.astype(np.float64)) / (np.pi / 2)).astype(np.int64)
        bad = np.flatnonzero(Kdev != K)
        assert not bad.size, "row %d: %d symbols carry another number of quarter turns, first at %d: %d for %d" % (m, bad.size, bad[0], Kdev[bad[0]], K[bad[0]])
        assert np.array_equal(ph[m][K == 0], raw[K == 0])                              # edges and uncorrected symbols: the grid entry, bit for bit
        err = np.abs(ph[m].astype(np.float64) - val) / (np.abs(val) + 1)
        assert err.max() <= 4 * u, (m, err.max() / u)
        worst = max(worst, float(err.max()) / u)
    want = E.astype(np.complex128) * np.exp(1j * ph.astype(np.float64))
    share = float((np.abs(out - want) / (TOL[dn]["atol"] + TOL[dn]["rtol"] * np.abs(want))).max())
    _close(out, want, dn)
    return worst, share


def report(name, dn, f, worst, share):
    print("%s %s: wraps up %d down %d, exact-half jumps %d (corrected %d), chunk-edge wraps first %d+%d last %d+%d, K in [%d, %d]; "
          "max |ph - float64| %.2f u (|value| + 1), field error %.3g of TOL"
          % (name, dn, f["up"], f["down"], f["half"], f["half_corrected"], f["first_up"], f["first_down"], f["last_up"], f["last_down"],
             f["kmin"], f["kmax"], worst, share))


# ------------------------------------------------------------------------------------------------ 1. the shared cases
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_unwrap_and_derotation_equal_numpy(case, dn):
    """Measured on an MI355X over these cases (the commit that added this file lists every case's counts): the largest |ph - float64 value| was
    1.40 u (|value| + 1) in complex64 (1.46 u on the long row below) and 1.97 u in complex128 against the bound of 4, the largest field error
    7.5e-4 and 2.5e-7 of TOL.  Exact-half jumps numpy corrects, complex128: 9 of 458 (A32 x3), 14 of 143 (A64 x3), 103 of 6181 (A32 x48).  The
    device's search settles the exact ties of these noise-free rows another way than the oracle does, so the counts differ from the host
    test's; the conditions are the same."""
    E, alphabet = _built(case["name"], dn)
    A, N = case["A"], case["N"]
    grid = ref.host_grid(A, dn)
    got = recover(E, alphabet, A, N, dn)
    f = ref.case_features(got[0], A, N, grid)
    worst, share = judge(E, got, grid, N, dn)
    report(case["name"], dn, f, worst, share)
    ref.check_features(case, f, dn)                                # the input conditions hold on the device's own indices too
    if case is EDGE_CASE:
        assert np.count_nonzero(got[0][:, N] > A // 2) >= 4         # first interior symbols that would wrap if the step from the edge counted


# ------------------------------------------------------------------------------------------------ 2. interior edges
def _edge_lengths(N):
    return [1, 2 * N - 1, 2 * N, 2 * N + 1, 2 * N + 2, 1024 + N - 1, 1024 + N, 1024 + N + 1, 2048 + N]


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("N", [8, 96])
def test_rows_whose_interior_is_empty_short_or_ends_on_a_chunk_boundary(N, dn):
    A, M = 16, 16
    grid = ref.host_grid(A, dn)
    for L in _edge_lengths(N):
        # the phase climbs a quarter turn in 400 symbols (N = 8) or 700 (N = 96: a window of 192 still follows it) and has reached 0.5 rad
        # (entry 13 of 16) at the first interior symbol: the step to it from the edge's entry 0 is longer than half the grid
        rate, phase0 = (400., 0.5) if N == 8 else (700., 0.3)
        E, alphabet = ref.drifting_rows(M, A, N, L, 2, 100 + L, CT[dn], wraps=L / rate, phase0=phase0)
        got = recover(E, alphabet, A, N, dn)
        idx, ph, out = got
        worst, share = judge(E, got, grid, N, dn)
        f = ref.case_features(idx, A, N, grid)
        print("N%d L%d %s: wraps %d+%d, %.2f u, field %.3g of TOL" % (N, L, dn, f["up"], f["down"], worst, share))
        if L <= 2 * N:                                             # nothing to search: every phase is the grid's first entry
            assert not idx.any() and np.all(ph == grid[0])
            _close(out, E.astype(np.complex128) * np.exp(1j * np.float64(grid[0])), dn)
        else:
            assert np.all(idx[:, N] > A // 2)                      # (condition on the input)
            assert np.array_equal(ph[:, N], grid[idx[:, N]])       # the first interior symbol never carries a correction
        if L > 1024:
            assert f["up"] + f["down"] >= 2, f                     # the running count reaches the end of the interior


# ------------------------------------------------------------------------------------------------ 3. grid formed on the device
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("A", [8, 32, 33, 64])
def test_grid_formed_on_the_device(A, dn):
    """``angles=None``.  The header allows the device's grid to differ from ``test_angle_grid`` in the last bit.  Entries that did on an MI355X:
    A = 8: none of 8 in either precision; A = 32: 10 (float32) and 11 (float64) of 32; A = 33: 16 and 15 of 33; A = 64: 22 and 26 of 64.  With
    them the outcome of exact-half jumps changes - float32, A = 32: 23 of 173 corrected, where the host's grid corrects none; float64, A = 32
    and 64: none corrected, where the host's grid corrects some - and from the first such jump on the row carries another count of quarter
    turns than it would on the host's grid (7411 to 13360 of 15381 symbols).  What holds, and is asserted: numpy's rule on the values of the
    grid the device formed, read back from the symbols that carry no correction."""
    rt, u = RT[dn], U[dn]
    N, L, nm = 1, 5127, 3
    E, alphabet = ref.rows(4 if A != 64 else 16, A, N, L, nm, 50 + A, CT[dn], opposite=0.25)
    idx, ph, out = got = recover(E, alphabet, A, N, dn, host_grid=False)
    ideal = np.linspace(-np.pi / 4, np.pi / 4, A, endpoint=False)
    host = ref.host_grid(A, dn)
    assert np.all(ph[:, :N] == rt(-np.pi) / rt(4)) and np.all(ph[:, L - N:] == rt(-np.pi) / rt(4))      # the device's angles[0]
    Kdev = np.rint((ph.astype(np.float64) - ideal[idx]) / (np.pi / 2)).astype(np.int64)
    # the device's grid, read back from the symbols that carry no correction: one value per entry
    dev = np.full(A, np.nan, rt)
    seen = np.zeros(A, bool)
    for a in range(A):
        v = np.unique(ph[(idx == a) & (Kdev == 0)])
        assert v.size <= 1, (a, v)
        if v.size:
            dev[a], seen[a] = v[0], True
    assert seen.all()                                              # (these inputs visit every entry without a correction somewhere)
    assert np.all(np.abs(dev.astype(np.float64) - ideal) <= 2 * u)                     # an entry's own rounding; |angle| < 1
    ndiff = int(np.count_nonzero(dev != host))
    other = 0
    for m in range(nm):
        # away from exact-half jumps: the float64 unwrap of the ideal grid
        p4 = 4 * ideal[idx[m, N:L - N]]
        K64 = np.rint((np.unwrap(p4) - p4) / (2 * np.pi)).astype(np.int64)
        sure = 2 * np.abs(np.diff(idx[m, N:L - N].astype(np.int64))) != A
        assert A % 2 == 0 or sure.all()
        assert np.array_equal(np.diff(Kdev[m, N:L - N])[sure], np.diff(K64)[sure])
        assert not Kdev[m, :N + 1].any() and not Kdev[m, L - N:].any()
        val = ideal[idx[m]] + (np.pi / 2) * Kdev[m]
        assert np.all(np.abs(ph[m] - val) <= 4 * u * (np.abs(val) + 1) + 2 * u)
        other += int(np.count_nonzero(Kdev[m] != ref.recover_ref(host, idx[m], N)[1]))
    # at the exact-half jumps too: numpy's rule on the values of the grid the device formed
    judge(E, got, dev, N, dn)
    f = ref.case_features(idx, A, N, dev)
    print("A%d %s: %d of %d grid entries seen differ from the host's in the last bit; %d exact-half jumps (%d corrected), %d symbols carry "
          "another count than on the host's grid" % (A, dn, ndiff, int(seen.sum()), f["half"], f["half_corrected"], other))
    assert f["row_up"] >= 100 and f["row_down"] >= 100 and (A % 2 or f["half"] >= 20)


# ------------------------------------------------------------------------------------------------ 4. more chunks than the scan has threads
def test_one_long_row_of_1026_chunks():
    case, dn = LONG_CASE, "c64"
    E, alphabet = _built(case["name"], dn)
    grid = ref.host_grid(case["A"], dn)
    got = recover(E, alphabet, case["A"], case["N"], dn)
    f = ref.case_features(got[0], case["A"], case["N"], grid)
    worst, share = judge(E, got, grid, case["N"], dn)
    report(case["name"], dn, f, worst, share)
    ref.check_features(case, f, dn)
    assert f["first_up"] and f["first_down"] and f["last_up"] and f["last_down"]


# ------------------------------------------------------------------------------------------------ 5. repeat and order
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_same_bits_again_and_after_a_longer_row():
    """The scratch of the chunk sums only grows: a short case gives the same bits a second time and once more after the long row has made
    the scratch 128 times as large."""
    short, dn = JUMP_CASES[2], "c64"
    E, alphabet = _built(short["name"], dn)
    first = recover(E, alphabet, short["A"], short["N"], dn)
    assert _same(first, recover(E, alphabet, short["A"], short["N"], dn))
    El, al = _built(LONG_CASE["name"], dn)
    recover(El, al, LONG_CASE["A"], LONG_CASE["N"], dn)
    assert _same(first, recover(E, alphabet, short["A"], short["N"], dn))
    judge(E, first, ref.host_grid(short["A"], dn), short["N"], dn)


@pytest.mark.parametrize("dn", DTYPES)
def test_three_parts_equal_one_call(dn):
    case = JUMP_CASES[0]
    E, alphabet = _built(case["name"], dn)
    assert _same(recover(E, alphabet, case["A"], case["N"], dn), recover(E, alphabet, case["A"], case["N"], dn, nparts=3))


# ------------------------------------------------------------------------------------------------ 6. rejections
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("what", ["nm=0", "L=0", "A=0", "part==nparts", "nparts=0"])
def test_bad_sizes_are_the_librarys_argument_error(what, dn):
    nm, L, A = 2, 64, 8
    E, alphabet = ref.rows(4, A, 1, L, nm, 3, CT[dn])
    dE, dsy, dang = D.from_host(E), D.from_host(alphabet), D.from_host(ref.host_grid(A, dn))
    idx, ph, out = D.from_host(np.full(E.shape, 7, np.int32)), D.from_host(np.full(E.shape, 5, RT[dn])), D.from_host(E * 0 + 3)
    _lib.sync()
    lib, c = _lib.load(), "c64" if dn == "c64" else "c128"
    args = dict(nm=nm, L=L, A=A)
    if "=0" in what and what != "nparts=0":
        args[what[:-2]] = 0
    head = (dE.ptr, args["nm"], args["L"], dang.ptr, args["A"], dsy.ptr, 4, 1, idx.ptr, ph.ptr, out.ptr)
    if what == "part==nparts":
        rc = getattr(lib, "qh_bps_recover_part_%s_dev" % c)(*head, 3, 3)
    elif what == "nparts=0":
        rc = getattr(lib, "qh_bps_recover_part_%s_dev" % c)(*head, 0, 0)
    else:
        rc = getattr(lib, "qh_bps_recover_%s_dev" % c)(*head)
    assert rc == _lib.QH_ERR_ARG and b"bps_recover" in lib.qh_last_error()
    _lib.sync()                                                                        # nothing ran: the outputs are as they were
    assert np.all(idx.to_host() == 7) and np.all(ph.to_host() == 5) and np.all(out.to_host() == 3)


# ------------------------------------------------------------------------------------------------ 7. pilot_phase_trace
def _knot_sets(L):
    if L == 1:
        return [[0], [0, 5], [2, 3]]
    return [[17],                              # one knot: a constant
            [5, 6, 40, L - 56],                # first knot after the start, two adjacent knots, last knot before the end
            [0, L // 2, L - 1],                # knots on the first and on the last symbol
            [3, 100, L],                       # last knot one past the end
            [3, 4, 100, L + 50]]               # ... and far beyond it


def _interp_two_roundings(L, knots, kph):
    """np.interp's expression ``slope * (x - xp[j]) + fp[j]`` with the product and the sum as two numpy operations, each rounded on its own
    on every host - np.interp itself is compiled code and may fuse the two where the host's numpy was built to."""
    knots, x = np.asarray(knots, dtype=np.int64), np.arange(L)
    j = np.clip(np.searchsorted(knots, x, side="right") - 1, 0, max(knots.size - 2, 0))
    if knots.size == 1:
        return np.repeat(kph[:, :1], L, axis=1)
    slope = (kph[:, j + 1] - kph[:, j]) / (knots[j + 1] - knots[j]).astype(np.float64)
    prod = slope * (x - knots[j]).astype(np.float64)
    val = prod + kph[:, j]
    return np.where(x <= knots[0], kph[:, :1], np.where(x >= knots[-1], kph[:, -1:], val))


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("L", [1, 255, 256, 257])
def test_pilot_phase_trace_equals_numpy_interp(L, dn):
    """The trace is exactly the cast of the interpolation evaluated with two roundings, product then sum, and within the 1 ulp of
    np.interp's own result (on an MI355X against an x86-64 numpy: no sample differs from np.interp either)."""
    rng = np.random.default_rng(7 + L)
    rt, nm = RT[dn], 3
    E = (rng.standard_normal((nm, L)) + 1j * rng.standard_normal((nm, L))).astype(CT[dn])
    for knots in _knot_sets(L):
        kph = 2 * rng.standard_normal((nm, len(knots)))
        out, trace = hip_dsp.pilot_phase_trace(E, np.array(knots), kph)
        assert out.shape == trace.shape == E.shape and out.dtype == trace.dtype == CT[dn] and not trace.imag.any()
        want = np.stack([np.interp(np.arange(L), knots, kph[m]) for m in range(nm)]).astype(rt)
        assert np.array_equal(trace.real, _interp_two_roundings(L, knots, kph).astype(rt))          # the kernel's own operations: exact
        off = trace.real != want
        ulps = np.abs(trace.real.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print("L%d %s knots %s: %d of %d samples off the cast of numpy's interpolation, by at most %.1f ulp" % (L, dn, knots, off.sum(), off.size, ulps.max()))
        assert ulps.max() <= 1
        for j, k in enumerate(knots):                              # on a knot: the knot's phase itself
            if k < L:
                assert np.array_equal(trace.real[:, k], kph[:, j].astype(rt))
        _close(out, E.astype(np.complex128) * np.exp(-1j * trace.real.astype(np.float64)), dn)


# ------------------------------------------------------------------------------------------------ 8. make_decision
QAM16 = (np.array([-3., -1., 1., 3.])[:, None] + 1j * np.array([-3., -1., 1., 3.])[None, :]).ravel()      # exact in float32
TIES = np.array([2 + 1j, 3j, -2 - 1j, 2 + 2j, 0, -2 + 2j])                             # midway between two symbols (x3), between four (x3)


def _points(L, rng):
    x = 2 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    n = min(L, TIES.size)
    x[:n] = TIES[3:3 + n] if L == 1 else TIES[:n]
    return x


def _decide_ref(x, sy):
    d = np.abs(x.astype(np.complex128)[:, None] - sy.astype(np.complex128)[None, :])
    return d, np.argmin(d, axis=1)                                 # first arg-min


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("L", [1, 256, 257])
@pytest.mark.parametrize("M", [16, 1])
def test_make_decision_on_exact_ties_and_one_symbol(M, L, dn):
    rng = np.random.default_rng(L + M)
    sy = (QAM16 if M == 16 else np.array([1 + 1j])).astype(CT[dn])
    x = _points(L, rng).astype(CT[dn])
    d, want = _decide_ref(x, sy)
    if M == 16:
        nt = min(L, TIES.size)
        ties = (d[:nt] == d[:nt].min(axis=1, keepdims=True)).sum(axis=1)
        assert ties.tolist() == ([4] if L == 1 else [2, 2, 2, 4, 4, 4])                # exact ties of the float64 distances
        two = np.sort(d[nt:], axis=1)[:, :2]
        assert not two.size or (two[:, 1] - two[:, 0]).min() > 1e-4                    # and nothing near a tie elsewhere
    det, dist, idx = hk.make_decision(x, sy)
    assert np.array_equal(idx, want) and np.array_equal(det, sy[want])                 # a tie keeps the first arg-min
    dmin = d[np.arange(L), want]
    # half an ulp of each difference, at most one of the distance together, and the hypot's own one to two
    assert np.all(np.abs(dist - dmin) <= 4 * np.spacing(dmin.astype(RT[dn])))
    # the device entry with det and / or dist left out writes what was asked for
    dx, dsy = D.from_host(x), D.from_host(sy)
    for with_det, with_dist in ((False, False), (True, False), (False, True), (True, True)):
        ddet, ddist, didx = D.from_host(np.full(L, 9, CT[dn])), D.from_host(np.full(L, 9, RT[dn])), D.from_host(np.full(L, 9, np.int32))
        hk.make_decision_dev(dx, dsy, ddet if with_det else None, ddist if with_dist else None, didx)
        _lib.sync()
        assert np.array_equal(didx.to_host(), idx)
        assert np.array_equal(ddet.to_host(), det) if with_det else np.all(ddet.to_host() == 9)
        assert np.array_equal(ddist.to_host(), dist) if with_dist else np.all(ddist.to_host() == 9)


# ------------------------------------------------------------------------------------------------ 9. select_angles
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("L", [1, 256, 257])
def test_select_angles_equals_numpy_indexing(L, dn):
    rng = np.random.default_rng(L)
    A, rt = 7, RT[dn]
    idx = rng.integers(0, A, L)
    idx[:1], idx[-1:] = 0, A - 1
    per = rng.standard_normal((max(L, 2), A)).astype(rt)           # a per-symbol grid has more than one row
    idx2 = rng.integers(0, A, per.shape[0])
    got = hip_dsp.select_angles(per, idx2)
    assert got.dtype == rt and np.array_equal(got, per[np.arange(per.shape[0]), idx2])
    one = rng.standard_normal((1, A)).astype(rt)
    got = hip_dsp.select_angles(one, idx)
    assert got.dtype == rt and np.array_equal(got, one[0, idx])


def test_select_angles_rejections():
    one, per = np.zeros((1, 7), np.float32), np.zeros((5, 7), np.float32)
    for bad in ([0, 7], [-1, 0]):
        with pytest.raises(ValueError, match="out of range"):
            hip_dsp.select_angles(one, np.array(bad))
    with pytest.raises(ValueError, match="needs as many indices"):
        hip_dsp.select_angles(per, np.zeros(4, np.int64))
    with pytest.raises(TypeError):
        hip_dsp.select_angles(np.zeros(7, np.float32), np.zeros(4, np.int64))
    with pytest.raises(TypeError):
        hip_dsp.select_angles(np.zeros((1, 7), np.int32), np.zeros(4, np.int64))
