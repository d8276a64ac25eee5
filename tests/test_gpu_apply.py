"""The butterfly FIR (csrc/apply.hip) in every launch form the host code can pick, against the extended-precision restatement
(tests/apply_ref.py, pinned to the reference's outputs by tests/test_apply_ref.py).

A form is chosen by the element type (complex64 / complex128 / float32 / float64; the real kernel is a separate one), the inner loop (complex64
at even ``os``: packed 16-byte reads with paired taps in LDS; everything else: the generic loop), the outputs per thread (P = 4, tiles of 1024,
or P = 1, tiles of 256, when four rows per thread do not fit 160 KiB of LDS), the pairing of selected modes (one mode: NJ = 1; more: pairs along
blockIdx.y, the last one half filled when their number is odd) and the opt-in above 64 KiB of dynamic LDS.  Every case first asserts through
qh_apply_plan the form it is there to reach, so a change of the constants in apply.hip fails these cases instead of moving them onto another form.

Bars: max-abs error over the rms of the expected output, 1e-5 for complex64 / float32 and 1e-11 for complex128 / float64.  Random-tap cases in
single precision keep nmodes * ntaps <= 600: a sequential fp32 sum of 572 terms errs by 2.7e-6 of the rms (tests/test_gpu_resample.py), a CPU
emulation of 16 modes x 37 taps (592 terms, no FMA) by 1.7e-6, and the same sum in double against long double by 4.6e-15 - the restatement alone
stays well inside both bars.  Where more terms are needed (the LDS boundary in single precision) the taps are one-hot and the check is exact.

Inputs: unit-power Gaussian samples rounded to a 2^-10 grid (the same values in all four types); taps random and different for every (j, k, t),
scaled by 1 / sqrt(nmodes * ntaps), rounded to float32 so that both precisions filter with the same taps; never symmetric.  ``L = N os + ntaps
- 1 + r`` with r = 0 unless a case says otherwise: the shortest row with N outputs under the reference's N = (L - ntaps + 1) // os (which leaves
the os - 1 samples behind the last window unused), and r < os more samples that change nothing."""
import numpy as np
import pytest

import apply_ref as ref
from qampy_amd import _lib
from qampy_amd._lib import DeviceArray
from qampy_amd.core.equalisation import equalisation as core_eq
from qampy_amd.core.equalisation import hip_equalisation as hk

pytestmark = pytest.mark.gpu

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
BAR = {C64: 1e-5, F32: 1e-5, C128: 1e-11, F64: 1e-11}
CPLX, REAL = (C64, C128), (F32, F64)
KIB64 = 65536
SENTINEL = -7.25 + 3.5j
_CACHE = {}


def name(dt):
    return np.dtype(dt).name


def length(N, os_, ntaps, r=0):
    return N * os_ + ntaps - 1 + r


def samples(nmodes, L, real=False, seed=0):
    """Unit-power Gaussian samples on a 2^-10 grid (float64 / complex128 holding values exact in float32), the same for every caller."""
    key = ("E", nmodes, L, real, seed)
    if key not in _CACHE:
        rng = np.random.default_rng([11, nmodes, L, seed])
        x = rng.standard_normal((nmodes, L)) if real else (rng.standard_normal((nmodes, L)) + 1j * rng.standard_normal((nmodes, L))) / np.sqrt(2)
        x = np.round(x * 1024) / 1024
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def taps(nrows, nmodes, ntaps, real=False, seed=0):
    """Random taps, every (j, k, t) its own value, exact in float32."""
    key = ("w", nrows, nmodes, ntaps, real, seed)
    if key not in _CACHE:
        rng = np.random.default_rng([13, nrows, nmodes, ntaps, seed])
        w = rng.standard_normal((nrows, nmodes, ntaps)) if real else rng.standard_normal((nrows, nmodes, ntaps)) + 1j * rng.standard_normal((nrows, nmodes, ntaps))
        w = (w / np.sqrt(nmodes * ntaps)).astype(F32 if real else C64).astype(F64 if real else C128)
        w.setflags(write=False)
        _CACHE[key] = w
    return _CACHE[key]


def expected(E, os_, wx, modes=None, key=None):
    """The restatement, computed once per case and shared by the types that run it."""
    if key is None:
        return ref.apply_filter(E, os_, wx, modes)
    key = ("ref",) + key
    if key not in _CACHE:
        out = ref.apply_filter(E, os_, wx, modes)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def run_dev(E, os_, wx, modes=None):
    """The kernel and nothing else: device arrays in, device array out (complex types)."""
    nsel = wx.shape[0] if modes is None else len(modes)
    dE, dw = DeviceArray.from_host(E), DeviceArray.from_host(wx)
    out = DeviceArray((nsel, ref.n_out(E.shape[1], wx.shape[-1], os_)), E.dtype)
    hk.apply_filter_to_signal_dev(dE, os_, dw, modes, out)
    return out.to_host()


def run(E, os_, wx, modes=None):
    """Complex types through the device entry point, real types through the host one (the real kernel has no other)."""
    if np.iscomplexobj(E):
        return run_dev(E, os_, wx, modes)
    return hk.apply_filter_to_signal(E, os_, wx, None if modes is None else np.asarray(modes))


def assert_plan(dt, nmodes, os_, ntaps, nsel, per_thread, grid_y, big_lds=None):
    p = ref.plan(dt, nmodes, os_, ntaps, nsel)
    assert p is not None, "the argument check refuses the case"
    assert (p["per_thread"], p["tile"], p["grid_y"]) == (per_thread, 256 * per_thread, grid_y), p
    if big_lds is not None:
        assert (p["lds"] > KIB64) == big_lds, p
    return p


def check(got, want, dt, what):
    assert got.shape == want.shape and got.dtype == dt, (what, got.shape, want.shape, got.dtype)
    err = ref.rel_max(got, want)
    print("apply %-58s %-10s rel_err = %.3g (bar %.0e)" % (what, name(dt), err, BAR[dt]))
    assert np.isfinite(got).all(), what
    assert err <= BAR[dt], (what, name(dt), err)
    return err


# ------------------------------------------------------------------------------------------------ a. tile edges, four outputs per thread
@pytest.mark.parametrize("ntaps", [41, 40])
@pytest.mark.parametrize("dt", CPLX, ids=name)
def test_tile_edges_four_per_thread(dt, ntaps):
    """N one symbol, and exactly on, one before and one after the edges of the 256-symbol rows and the 1024-symbol tiles; odd and even tap
    counts (the packed path pads an odd count with a zero tap against a spare zero sample).  Then with os - 1 leftover samples, these and the
    os - 1 unused ones before them set to NaN: they belong to no window and must not reach the output - the result has the bits of the run
    without them."""
    nm, os_ = 2, 2
    assert_plan(dt, nm, os_, ntaps, nm, per_thread=4, grid_y=1, big_lds=(dt == C128))
    wx = taps(nm, nm, ntaps)
    for N in (1, 255, 256, 257, 1023, 1024, 1025, 2049):
        L = length(N, os_, ntaps)
        E = samples(nm, length(2049, os_, 41))[:, :L]
        want = expected(E, os_, wx, key=("a", ntaps, N))
        got = run_dev(E.astype(dt), os_, wx.astype(dt))
        check(got, want, dt, "a P=4 ntaps=%d N=%d" % (ntaps, N))
        Er = np.concatenate([E[:, :L - (os_ - 1)], np.full((nm, 2 * (os_ - 1)), np.nan)], axis=1)
        got_r = run_dev(Er.astype(dt), os_, wx.astype(dt))
        assert got_r.shape == got.shape and np.array_equal(got_r, got), "leftover samples reached the output at N=%d" % N


# ------------------------------------------------------------------------------------------------ b. tile edges, one output per thread
@pytest.mark.parametrize("cfg", [(C128, 8, 2, 21), (C64, 4, 16, 33), (C64, 16, 2, 37)], ids=lambda c: "%s-%dm-os%d-t%d" % ((name(c[0]),) + c[1:]))
def test_tile_edges_one_per_thread(cfg):
    """The fallback form (tiles of 256) at its tile edges: many modes, or a large oversampling, do not fit four rows per thread."""
    dt, nm, os_, ntaps = cfg
    assert nm * ntaps <= 600
    assert_plan(dt, nm, os_, ntaps, nm, per_thread=1, grid_y=nm // 2, big_lds=True)
    wx = taps(nm, nm, ntaps)
    for N in (1, 255, 256, 257, 513):
        E = samples(nm, length(513, os_, ntaps))[:, :length(N, os_, ntaps)]
        check(run_dev(E.astype(dt), os_, wx.astype(dt)), expected(E, os_, wx), dt, "b P=1 %dm os=%d ntaps=%d N=%d" % (nm, os_, ntaps, N))


# ------------------------------------------------------------------------------------------------ c. mode pairing
PAIRING = [(3, None), (5, [4, 0, 2, 1, 3]), (5, [3]), (2, [1, 1]), (2, [1, 0]), (4, [3, 1, 1, 0, 2, 2, 3, 0, 0, 1, 3, 2, 1, 3, 0, 2])]
# (nmodes, os) at which complex128 with 7 taps does not fit four rows per thread - 5 (2046 + 8) + 10 * 8 = 10350 samples of 16 B are 165,600 B -
# and pairs its modes in the fallback form; every other case of the table runs four per thread
PAIRING_ONE_PER_THREAD = {(C128, 5, 2), (C128, 5, 3), (C128, 4, 3)}


@pytest.mark.parametrize("os_", [2, 3])
@pytest.mark.parametrize("dt", CPLX, ids=name)
def test_mode_pairing(dt, os_):
    """More than one pair of modes, a half-filled last pair, one mode alone, repeats and 16 selected rows.  Every output row has the bits of the
    single-mode call of its mode - first of a pair, second, or alone in a half-filled pair: the source accumulates every output in the same
    order - and a second call repeats the bits."""
    ntaps, N = 7, 1030
    for nm, modes in PAIRING:
        rows = list(range(nm)) if modes is None else modes
        nsel = len(rows)
        assert_plan(dt, nm, os_, ntaps, nsel, per_thread=1 if (dt, nm, os_) in PAIRING_ONE_PER_THREAD else 4, grid_y=1 if nsel == 1 else (nsel + 1) // 2)
        E, wx = samples(nm, length(N, os_, ntaps)), taps(nm, nm, ntaps)
        Ed, wd = E.astype(dt), wx.astype(dt)
        got = run_dev(Ed, os_, wd, modes)
        check(got, expected(E, os_, wx, modes, key=("c", os_, nm, tuple(rows))), dt, "c os=%d %dm modes=%s" % (os_, nm, modes))
        assert np.array_equal(run_dev(Ed, os_, wd, modes), got), "a second call gave other bits"
        single = {m: run_dev(Ed, os_, wd, [m]) for m in sorted(set(rows))}
        for j, m in enumerate(rows):
            assert single[m].shape == (1, N)
            assert np.array_equal(got[j], single[m][0]), "row %d (mode %d) of modes=%s differs from the single-mode call" % (j, m, modes)


# ------------------------------------------------------------------------------------------------ d. oversampling and tap counts
@pytest.mark.parametrize("dt,os_", [(C64, o) for o in (1, 2, 3, 4, 5, 8)] + [(C128, 1), (C128, 4)], ids=lambda v: name(v) if isinstance(v, type) else "os%d" % v)
def test_oversampling_and_tap_counts(dt, os_):
    """Packed reads at os = 2, 4, 8 and the generic loop at odd os, with one tap, fewer taps than os, odd and even counts; two tiles."""
    nm, N = 2, 1030
    for ntaps in (1, 2, 7, 8):
        assert_plan(dt, nm, os_, ntaps, nm, per_thread=4, grid_y=1)
        E, wx = samples(nm, length(N, 8, 8))[:, :length(N, os_, ntaps)], taps(nm, nm, ntaps)
        check(run_dev(E.astype(dt), os_, wx.astype(dt)), expected(E, os_, wx, key=("d", os_, ntaps)), dt, "d os=%d ntaps=%d" % (os_, ntaps))


# ------------------------------------------------------------------------------------------------ e. one-hot taps, exact
@pytest.mark.parametrize("dt", CPLX + REAL, ids=name)
def test_one_hot_taps_are_exact(dt):
    """wx[j, k, t] = 1 alone: row j is E[k, t : t + N os : os] to the bit and every other row is zero - a swapped mode, row or tap index has
    nowhere to hide."""
    nm, N, real = 3, 70, dt in REAL
    for os_ in (1, 2, 3):
        for ntaps in (4, 5):
            assert_plan(dt, nm, os_, ntaps, nm, per_thread=4, grid_y=nm if real else 2)
            E = np.ascontiguousarray(samples(nm, length(N, 3, 5), real=real)[:, :length(N, os_, ntaps)].astype(dt))
            for t in (0, ntaps // 2, ntaps - 1):
                for j in range(nm):
                    for k in range(nm):
                        wx = np.zeros((nm, nm, ntaps), dt)
                        wx[j, k, t] = 1
                        got = run(E, os_, wx)
                        want = np.zeros((nm, N), dt)
                        want[j] = E[k, t:t + N * os_:os_]
                        assert got.dtype == dt and np.array_equal(got, want), "os=%d ntaps=%d: the one tap (j=%d, k=%d, t=%d)" % (os_, ntaps, j, k, t)


# ------------------------------------------------------------------------------------------------ f. the real kernel, directly
@pytest.mark.parametrize("cfg", [(F32, 4, 2, 4, (1023, 1024, 1025)), (F64, 4, 2, 4, (1023, 1024, 1025)), (F64, 8, 4, 1, (255, 256, 257)),
                                 (F32, 16, 4, 1, (255, 256, 257))], ids=lambda c: "%s-%drows-os%d-P%d" % (name(c[0]), c[1], c[2], c[3]))
def test_real_kernel_with_mode_subsets(cfg):
    """Real arrays straight into the real kernel (the host layer reaches it only with every row selected): all rows, one row, a permuted subset;
    both tile sizes at their edges."""
    dt, nm, os_, P, Ns = cfg
    ntaps = 9
    wx = taps(nm, nm, ntaps, real=True)
    for modes in (None, [2], [3, 0, 1]):
        nsel = nm if modes is None else len(modes)
        assert_plan(dt, nm, os_, ntaps, nsel, per_thread=P, grid_y=nsel, big_lds=(P == 1 or dt == F64))
        for N in Ns:
            E = samples(nm, length(Ns[-1], os_, ntaps), real=True)[:, :length(N, os_, ntaps)]
            got = run(np.ascontiguousarray(E.astype(dt)), os_, wx.astype(dt), modes)
            check(got, expected(E, os_, wx, modes), dt, "f %d rows os=%d P=%d modes=%s N=%d" % (nm, os_, P, modes, N))


# ------------------------------------------------------------------------------------------------ g. the host layers on top
@pytest.mark.parametrize("dt", CPLX, ids=name)
def test_host_layers(dt):
    """Real-valued taps with a mode subset through core.equalisation.apply_filter (stacking, real kernel, unstacking) against the restatement
    through the same stacking; ResidentField.apply and the host-array entry point return the bits of the device form."""
    nm, os_, ntaps, N = 2, 2, 9, 1030
    rt = F32 if dt == C64 else F64
    E = samples(nm, length(N, os_, ntaps))
    wr = taps(2 * nm, 2 * nm, ntaps, real=True)
    for modes in ([1, 3], [3, 0, 1, 2], None):
        got = core_eq.apply_filter(E.astype(dt), os_, wr.astype(rt), modes=modes)
        want = ref.unstack_real(expected(ref.stack_real(E), os_, wr, modes))
        check(got, want, dt, "g real taps through apply_filter, modes=%s" % modes)
    wx = taps(3, 3, ntaps)
    E3 = samples(3, length(N, os_, ntaps))
    Ed, wd = np.ascontiguousarray(E3.astype(dt)), wx.astype(dt)
    for modes in (None, [2, 0], [1]):
        dev = run_dev(Ed, os_, wd, modes)
        check(dev, expected(E3, os_, wx, modes), dt, "g device form, modes=%s" % modes)
        assert np.array_equal(hk.apply_filter_to_signal(Ed, os_, wd, None if modes is None else np.array(modes)), dev)
        assert np.array_equal(hk.ResidentField(Ed).apply(os_, wd, modes), dev)
        assert np.array_equal(core_eq.apply_filter(Ed, os_, wd, modes=modes), dev)


# ------------------------------------------------------------------------------------------------ h. the LDS boundary
def raw_call(dt, E, os_, wx, modes, out, nmodes=None, L=None, ntaps=None, nsel=None):
    """The C entry point itself (device arrays for the complex types, host arrays for the real ones): its status, nothing raised."""
    fn = getattr(_lib.load(), "qh_apply_filter_" + {C64: "c64_dev", C128: "c128_dev", F32: "f32", F64: "f64"}[dt])
    modes = np.ascontiguousarray(modes, dtype=np.int64)
    return fn(_lib.ptr(E), E.shape[0] if nmodes is None else nmodes, E.shape[1] if L is None else L, os_, _lib.ptr(wx),
              wx.shape[-1] if ntaps is None else ntaps, _lib.ptr(modes), modes.size if nsel is None else nsel, _lib.ptr(out))


@pytest.mark.parametrize("dt", CPLX + REAL, ids=name)
def test_lds_boundary(dt):
    """The largest tap count the argument check admits (found by search) launches and computes - it asks for all, or all but a few bytes, of the
    160 KiB of a CU's LDS - and one tap more is refused with the LDS message before anything is written.  Double precision: random taps at the
    bar; single precision: one one-hot tap per row at t = ntaps - 1, exact (thousands of fp32 terms would not meet the bar by themselves)."""
    nm, os_, N, real = 2, 2, 300, dt in REAL
    ntaps = ref.largest_ntaps(dt, nm, os_, nm)
    p = assert_plan(dt, nm, os_, ntaps, nm, per_thread=1, grid_y=nm if real else 1, big_lds=True)
    assert p["lds"] <= 160 * 1024 and ref.plan(dt, nm, os_, ntaps + 1, nm) is None
    print("apply h %s: ntaps = %d accepted with %d B of dynamic LDS, %d refused" % (name(dt), ntaps, p["lds"], ntaps + 1))
    E = samples(nm, length(N, os_, ntaps), real=real)
    if dt in (C128, F64):
        wx = taps(nm, nm, ntaps, real=real)
        check(run(np.ascontiguousarray(E.astype(dt)), os_, wx.astype(dt)), expected(E, os_, wx), dt, "h ntaps=%d N=%d" % (ntaps, N))
    else:
        wx = np.zeros((nm, nm, ntaps), dt)
        wx[0, 1, -1] = wx[1, 0, -1] = 1
        Ed = np.ascontiguousarray(E.astype(dt))
        got = run(Ed, os_, wx)
        assert np.array_equal(got, Ed[::-1, ntaps - 1:ntaps - 1 + N * os_:os_])
    # one tap more, the same number of outputs
    E1 = np.ascontiguousarray(samples(nm, length(N, os_, ntaps + 1), real=real).astype(dt))
    w1 = np.ones((nm, nm, ntaps + 1), dt)
    fill = dt(SENTINEL.real) if real else dt(SENTINEL)
    if real:
        out = np.full((nm, N), fill)
        rc = raw_call(dt, E1, os_, w1, [0, 1], out)
        after = out
    else:
        out = DeviceArray.from_host(np.full((nm, N), fill))
        rc = raw_call(dt, DeviceArray.from_host(E1), os_, DeviceArray.from_host(w1), [0, 1], out)
        after = out.to_host()
    assert rc == _lib.QH_ERR_ARG and b"LDS" in _lib.load().qh_last_error()
    assert np.all(after == fill)


# ------------------------------------------------------------------------------------------------ i. writes stay inside out
def view(buf, first, shape):
    """A non-owning window of a flat device buffer, as DeviceArray.row makes them."""
    v = object.__new__(DeviceArray)
    v.shape, v.dtype = tuple(shape), buf.dtype
    v.nbytes = int(np.prod(shape)) * buf.dtype.itemsize
    v.ptr = buf.ptr + first * buf.dtype.itemsize
    v._own = False
    return v


@pytest.mark.parametrize("dt", CPLX, ids=name)
def test_writes_stay_inside_out(dt):
    """out as a window of a larger buffer filled with a sentinel: nothing before the first row or after the last one changes - with an odd
    number of selected modes (the guarded second store of a half-filled pair) and with a last tile of one symbol, in both tile sizes."""
    lead, tail = 64, 2048
    for nm, os_, ntaps, modes, N, P in ((3, 2, 7, None, 1025, 4), (3, 3, 7, [2, 0, 1], 1, 4), (4, 2, 8, [3], 1025, 4), (4, 2, 8, [1, 3, 0], 2049, 4),
                                        (16 if dt == C64 else 8, 2, 21, [5, 0, 7], 257, 1), (16 if dt == C64 else 8, 2, 21, [6], 1, 1)):
        nsel = nm if modes is None else len(modes)
        assert_plan(dt, nm, os_, ntaps, nsel, per_thread=P, grid_y=1 if nsel == 1 else (nsel + 1) // 2)
        E, wx = samples(nm, length(N, os_, ntaps)), taps(nm, nm, ntaps)
        whole = DeviceArray.from_host(np.full(lead + nsel * N + tail, dt(SENTINEL)))
        out = view(whole, lead, (nsel, N))
        hk.apply_filter_to_signal_dev(DeviceArray.from_host(E.astype(dt)), os_, DeviceArray.from_host(wx.astype(dt)), modes, out)
        back = whole.to_host()
        what = "i %dm os=%d modes=%s N=%d P=%d" % (nm, os_, modes, N, P)
        assert np.all(back[:lead] == dt(SENTINEL)) and np.all(back[lead + nsel * N:] == dt(SENTINEL)), what + ": wrote outside out"
        check(back[lead:lead + nsel * N].reshape(nsel, N), expected(E, os_, wx, modes), dt, what)


# ------------------------------------------------------------------------------------------------ j. argument errors through the C ABI
@pytest.mark.parametrize("dt", CPLX + REAL, ids=name)
def test_argument_errors(dt):
    """What the entry points refuse they refuse with QH_ERR_ARG and without writing; L < ntaps is no error: no output, nothing written."""
    nm, os_, ntaps, N, real = 2, 2, 5, 40, dt in REAL
    fill = dt(SENTINEL.real) if real else dt(SENTINEL)
    E = np.ascontiguousarray(samples(nm, length(N, os_, ntaps), real=real).astype(dt))
    wx = taps(nm, nm, ntaps, real=real).astype(dt)
    host_out = np.full((16, N), fill)
    dE, dw, out = (E, wx, host_out) if real else (DeviceArray.from_host(E), DeviceArray.from_host(wx), DeviceArray.from_host(host_out))
    untouched = lambda: np.all((out if real else out.to_host()) == fill)
    lib = _lib.load()
    for what, kw, modes, msg in (("os = 0", dict(), [0, 1], b"oversampling"), ("nsel = 0", dict(nsel=0), [0, 1], b"between 1 and 16"),
                                 ("nsel = 17", dict(nsel=17), [0] * 17, b"between 1 and 16"), ("mode = nmodes", dict(), [0, nm], b"largest mode number"),
                                 ("mode < 0", dict(), [-1], b"largest mode number"), ("nmodes = 0", dict(nmodes=0), [0], b"bad sizes"),
                                 ("ntaps = 0", dict(ntaps=0), [0], b"bad sizes"), ("L < 0", dict(L=-1), [0], b"bad sizes")):
        rc = raw_call(dt, dE, 0 if what == "os = 0" else os_, dw, modes, out, **kw)
        assert rc == _lib.QH_ERR_ARG and msg in lib.qh_last_error(), (what, rc, lib.qh_last_error())
        assert untouched(), what
    for L in (ntaps - 1, 0):
        assert raw_call(dt, dE, os_, dw, [0, 1], out, L=L) == _lib.QH_OK and untouched(), L
    # the Python layers raise what the reference raises
    with pytest.raises(ValueError, match="oversampling"):
        hk.apply_filter_to_signal(E, 0, wx)
    with pytest.raises(ValueError, match="largest mode number"):
        hk.apply_filter_to_signal(E, os_, wx, np.array([nm]))
    short = hk.apply_filter_to_signal(np.ascontiguousarray(E[:, :ntaps - 1]), os_, wx)
    assert short.shape == (nm, 0) and short.dtype == dt
