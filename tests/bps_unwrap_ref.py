"""
Plain restatement of the tail of ``qh_bps_recover_*_dev`` (include/qampy_hip.h: grid look-up, ``np.unwrap`` of the interior, de-rotation),
the inputs that drive it to its edges and the cases the host test (test_bps_unwrap_ref.py) and the device test (test_gpu_bps_unwrap.py) share.

The restatement is numpy itself: ``ph = grid[idx]; ph[N:L-N] = np.unwrap(4 * ph[N:L-N]) / 4`` in the dtype of the grid.  From it come the integer
number ``K`` of quarter turns every symbol carries and the value ``float64(grid[idx]) + (pi / 2) K`` a device result is held to.
"""
import numpy as np

from conftest import CT, RT
from qampy_amd import theory
from qampy_amd.core import hip_dsp

CHUNK = 1024                       # elements of a row one workgroup of the unwrap launches owns (csrc/unwrap_scan.h: UW_CHUNK)
U = {"c64": 2. ** -24, "c128": 2. ** -53}          # unit roundoff of the real type


def recover_ref(grid, idx, N):
    """The contract of the header for one row: ``(ph, K, value)``.

    ``ph``: ``grid[idx]`` with ``np.unwrap(4 ph) / 4`` on ``[N, L - N)``, everything in the dtype of ``grid`` - numpy's own jump decisions on
    the grid's own roundings.  ``K`` (int64): the quarter turns numpy added to every symbol, 0 on the edges.  ``value`` (float64):
    ``float64(grid[idx]) + (pi / 2) K`` - numpy's ``ph`` without the rounding of its running sum."""
    grid = np.asarray(grid).ravel()
    idx = np.asarray(idx)
    rt = grid.dtype.type
    L = idx.size
    raw = grid[idx]
    ph = raw.copy()
    K = np.zeros(L, np.int64)
    if L - N > N:
        p4 = rt(4) * raw[N:L - N]
        un = np.unwrap(p4)
        assert un.dtype == grid.dtype
        ph[N:L - N] = un / rt(4)
        turns = (un.astype(np.float64) - p4.astype(np.float64)) / (2 * np.pi)
        K[N:L - N] = np.rint(turns).astype(np.int64)
        assert np.abs(turns - K[N:L - N]).max() < 0.25            # the rounding of numpy's running sum is nowhere near half a turn
    return ph, K, raw.astype(np.float64) + (np.pi / 2) * K


def features(idx, A, N, grid):
    """What one row of indices makes the unwrap of ``grid`` do, counted on the steps inside ``[N, L - N)`` (element ``i`` is "a wrap" when
    the step ``idx[i - 1] -> idx[i]`` changes ``K``: by -1 where the index rose by more than ``A / 2``, by +1 where it dropped by more):

    ``up`` / ``down``    wraps with ``K`` going up (+1) and down (-1), by :func:`recover_ref` on ``grid``
    ``half``             jumps of exactly ``A / 2`` (even ``A`` only) - what they do depends on the rounding of the grid;
                         ``half_corrected`` / ``half_left`` say what numpy made of them
    ``first_up`` ...     wraps on the first (``i % 1024 == 0``) and on the last (``i % 1024 == 1023``) element of a chunk, by sign
    ``kmin``, ``kmax``   range of ``K``"""
    idx = np.asarray(idx).astype(np.int64)
    L = idx.size
    f = dict(up=0, down=0, half=0, first_up=0, first_down=0, last_up=0, last_down=0, kmin=0, kmax=0, half_corrected=0, half_left=0)
    if L - N < N + 2:
        return f
    d = np.diff(idx[N:L - N])
    at = np.arange(N + 1, L - N)                                   # element each step ends on
    half = 2 * np.abs(d) == A
    K = recover_ref(grid, idx, N)[1][N:L - N]
    step = np.diff(K)
    assert np.all(step[2 * d > A] == -1) and np.all(step[2 * d < -A] == 1) and not step[2 * np.abs(d) < A].any()
    first, last = at % CHUNK == 0, at % CHUNK == CHUNK - 1
    f.update(up=int(np.sum(step > 0)), down=int(np.sum(step < 0)), half=int(half.sum()),
             half_corrected=int(np.count_nonzero(step[half])), half_left=int(np.count_nonzero(step[half] == 0)),
             first_up=int(np.sum(step[first] > 0)), first_down=int(np.sum(step[first] < 0)),
             last_up=int(np.sum(step[last] > 0)), last_down=int(np.sum(step[last] < 0)), kmin=int(K.min()), kmax=int(K.max()))
    return f


def case_features(idx, A, N, grid):
    """:func:`features` of every row of ``idx (nmodes, L)``: the sums over the rows, ``kmin`` / ``kmax`` over all of them, and
    ``row_up`` / ``row_down``, the smallest count of wraps of either sign any row has."""
    per = [features(r, A, N, grid) for r in np.atleast_2d(idx)]
    f = {k: sum(p[k] for p in per) for k in per[0] if k not in ("kmin", "kmax")}
    f.update(kmin=min(p["kmin"] for p in per), kmax=max(p["kmax"] for p in per),
             row_up=min(p["up"] for p in per), row_down=min(p["down"] for p in per))
    return f


def host_grid(A, dn):
    """The (A,) grid of the host layer in the real type of ``dn``."""
    return hip_dsp.test_angle_grid(A, RT[dn]).ravel()


def rows(M, A, N, L, nmodes, seed, dtype, seam=0., opposite=0.):
    """``nmodes`` rows of ``L`` noise-free M-QAM symbols, every run of ``N`` of them rotated by minus an entry of the host grid drawn at random.
    With ``N = 1`` the search window holds two symbols of unrelated rotations and the index it settles on - about half way between the two,
    on a grid that closes on itself after ``A`` entries - jumps by anything from ``-A / 2`` to ``A / 2`` at every step, plus or minus ``A`` (a
    wrap) where the way leads over the seam of the grid.  Uniform draws wrap at one step in six and hardly ever jump by exactly ``A / 2``:

    ``seam``      share of the draws replaced by one of the two end entries of the grid (evenly): more steps over the seam, for grids and
                  rows too short to wrap a hundred times either way otherwise
    ``opposite``  share of the draws whose two neighbours are replaced by the entry half a grid away from it (even ``A``): both windows
                  around such a symbol tie between the two entries a quarter of the grid to either side, and where they settle on
                  different ones the index jumps by exactly ``A / 2``

    Returns ``(E, alphabet)`` in ``dtype``."""
    rng = np.random.default_rng(seed)
    alphabet = theory.coded_symbols_qam(M, dtype=np.complex128)
    grid = np.linspace(-np.pi / 4, np.pi / 4, A, endpoint=False)
    n = -(-L // N)
    s = alphabet[rng.integers(0, M, size=(nmodes, L))]
    k = rng.integers(0, A, size=(nmodes, n))
    ends = (A - 1) * rng.integers(0, 2, size=(nmodes, n))
    k = np.where(rng.random((nmodes, n)) < seam, ends, k)
    if A % 2 == 0 and n > 2:
        centre = rng.random((nmodes, n)) < opposite
        centre[:, 0] = centre[:, -1] = False
        for m, j in zip(*np.nonzero(centre)):
            k[m, j - 1] = k[m, j + 1] = (k[m, j] + A // 2) % A
    k = np.repeat(k, N, axis=1)[:, :L]
    return np.ascontiguousarray((s * np.exp(-1j * grid[k])).astype(dtype)), alphabet.astype(dtype)


def drifting_rows(M, A, N, L, nmodes, seed, dtype, wraps=6.0, phase0=0.0):
    """``nmodes`` rows of ``L`` noisy M-QAM symbols under a Wiener phase walk plus a slope that carries the phase over ``wraps`` quarter turns
    in the row, from ``phase0`` on: long runs without a jump, then a wrap.  Returns ``(E, alphabet)`` in ``dtype``."""
    rng = np.random.default_rng(seed)
    alphabet = theory.coded_symbols_qam(M, dtype=np.complex128)
    s = alphabet[rng.integers(0, M, size=(nmodes, L))]
    snr_db = {4: 14., 16: 22., 64: 28.}[M]
    s = s + 10 ** (-snr_db / 20) * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape)) / np.sqrt(2)
    walk = np.cumsum(rng.normal(scale=0.01, size=(nmodes, L)), axis=1)
    slope = wraps * (np.pi / 2) / max(L, 1) * np.arange(L) * (1 + 0.3 * np.arange(nmodes)[:, None])
    return np.ascontiguousarray((s * np.exp(-1j * (phase0 + walk + slope))).astype(dtype)), alphabet.astype(dtype)


BUILDERS = {"jump": rows, "drift": drifting_rows}


def build(case, dn):
    return BUILDERS[case["kind"]](case["M"], case["A"], case["N"], case["L"], case["nmodes"], case["seed"], CT[dn], **case["kw"])


def _case(kind, M, A, N, L, nmodes, seed, **kw):
    return dict(kind=kind, M=M, A=A, N=N, L=L, nmodes=nmodes, seed=seed, kw=kw, name="%s-M%d-A%d-N%d-L%d-x%d" % (kind, M, A, N, L, nmodes))


# Random jumps, N = 1: 5127 symbols are five chunks of 1024 and 7 symbols of a sixth; 3073 and 2100 end one and 52 symbols into a chunk
# (measured with the oracle: uniform draws give about 400 wraps either way per row of 5127 at A = 32 and 64, 210 per row of 3073 at A = 8,
# but only 60 per row of 2100 at A = 4 and 80 at A = 3 - hence `seam` there, 150 to 190; exact-half jumps: 6 per row at A = 32 - hence
# `opposite`, 30 per row - 50 at A = 64 and A = 8, 120 at A = 4)
JUMP_CASES = [_case("jump", 4, 32, 1, 5127, 3, 11, opposite=0.25), _case("jump", 16, 64, 1, 5127, 3, 12), _case("jump", 4, 8, 1, 3073, 2, 13),
              _case("jump", 4, 4, 1, 2100, 2, 14, seam=0.5)]
# Many rows: a wrap of a given sign lands on a given element of a row about once in thirteen rows, so 48 rows of five chunk edges put
# some eighteen wraps of either sign on the first and on the last element of a chunk - the condition (four of each) holds with room for
# the search on the device settling its exact ties another way than the oracle does
EDGE_CASE = _case("jump", 4, 32, 1, 5127, 48, 15, opposite=0.25)
# Grids too small to wrap (A = 1: one angle; A = 2: every jump is exactly half the grid) and the smallest that can (A = 3: a jump of 2)
SMALL_CASES = [_case("jump", 4, 1, 1, 2100, 2, 21), _case("jump", 4, 2, 1, 2100, 2, 22), _case("jump", 4, 3, 1, 2100, 2, 23, seam=0.5)]
DRIFT_CASES = [_case("drift", 16, 32, 2, 5127, 2, 31), _case("drift", 16, 64, 20, 5127, 2, 32)]
CASES = JUMP_CASES + [EDGE_CASE] + SMALL_CASES + DRIFT_CASES
# complex128 cases that must hold an exact-half jump numpy corrects and one it leaves alone (oracle: 13 and 50 corrected)
HALF_CASES = [JUMP_CASES[1], EDGE_CASE]

# One long row: 1026 chunks, so that a thread of the scan of the chunk sums owns two of them (complex64 only)
LONG_CASE = _case("jump", 4, 64, 1, 1024 * 1025 + 5, 1, 41)


def check_features(case, f, dn):
    """The conditions a case's indices must meet to be worth running (asserted on the oracle's indices on the host and on the returned
    ones on the device); ``f`` from :func:`case_features` with the grid."""
    A = case["A"]
    if case["kind"] == "jump" and A >= 3:
        assert f["row_up"] >= 100 and f["row_down"] >= 100, f
        assert f["kmin"] < 0 < f["kmax"], f
    if case["kind"] == "jump" and A >= 4 and A % 2 == 0:
        assert f["half"] >= 20, f
    if case["kind"] == "jump" and A < 3:
        assert f["up"] == f["down"] == 0 and (A == 1 or f["half"] >= 20), f
    if case["kind"] == "drift":
        assert f["up"] + f["down"] >= 3 * case["nmodes"] and f["half"] == 0, f
    if case is EDGE_CASE:
        assert min(f["first_up"], f["first_down"], f["last_up"], f["last_down"]) >= 4, f
    if dn == "c128" and case in HALF_CASES:
        # the float64 grid puts some jumps of exactly A / 2 entries a hair past pi, where numpy corrects them, and leaves others at pi: a
        # kernel that followed the ideal grid (never a correction) would differ here
        assert f["half_corrected"] >= 1 and f["half_left"] >= 1, f
