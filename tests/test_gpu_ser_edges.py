"""The device SER harness (qh_ser_c64_dev / qh_ser_c128_dev, qampy_amd/csrc/ser.hip) and the bare error counter (qh_count_errors_dev,
csrc/bps.hip) at their edges, against the float64 restatement of tests/ser_ref.py (itself pinned on the CPU by tests/test_ser_ref.py).

The C entry points are called directly, as core.ber_functions.cal_ser_dev calls them, so that the seven numbers of ``result`` are seen raw;
the transmitted labels are uploaded as they are, not decided on the device.  Every input is on the 2^-12 grid and clear of decision ties by
1e-4 (ser_ref.clear_of_ties), so a float32 kernel and the float64 restatement take the same decisions and ALL SEVEN NUMBERS ARE COMPARED
EXACTLY, for complex64 and complex128.  The samples of the two ``ties`` cases that sit exactly on a boundary are equidistant from
mirror-image points in any precision: there the first index must win.

qh_count_errors_dev ADDS the errors it counts to the counter it is given and never clears it: a counter that starts at 5 ends at 5 plus the
restated count, and n = 0 leaves it alone."""
import numpy as np
import pytest

import ser_ref as ref
from qampy_amd import _lib
from qampy_amd._lib import DeviceArray
from qampy_amd.core import ber_functions as ber

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
TRIP = 2048 * 256                       # symbols per pass of the counting kernels (grid cap x block)
UNTOUCHED = -77


class _Uploaded:
    """A case in HBM in one dtype, and the raw call."""

    def __init__(self, rx, lab, al, dn):
        self.dn, self.N, (self.nmodes, self.ntx), self.M = dn, rx.size, lab.shape, al.size
        self.E, self.T, self.A = (DeviceArray.from_host(np.ascontiguousarray(rx, dtype=CT[dn])), DeviceArray.from_host(np.ascontiguousarray(lab, dtype=np.int32)),
                                  DeviceArray.from_host(np.ascontiguousarray(al, dtype=CT[dn])))

    def call(self, maxlag, window, trim, **over):
        a = dict(E=self.E.ptr, N=self.N, T=self.T.ptr, nmodes=self.nmodes, ntx=self.ntx, A=self.A.ptr, M=self.M, result=True)
        a.update(over)
        h = np.full(7, UNTOUCHED, np.int64)
        _lib.call("qh_ser_%s_dev" % self.dn, a["E"], a["N"], a["T"], a["nmodes"], a["ntx"], a["A"], a["M"], maxlag, window, trim,
                  _lib.ptr(h) if a["result"] else None)
        return tuple(int(v) for v in h)


def _run(name, dn):
    c = ref.make(name)
    return _Uploaded(c["rx"], c["labels"], c["alphabet"], dn).call(c["maxlag"], c["window"], c["trim"])


PAIRS = [(n, dn) for n, c in ref.CASES.items() for dn in ("c64", "c128") if dn == "c64" or not c["c64_only"]]


# ------------------------------------------------------------------------------------------------ the harness
@pytest.mark.parametrize("name,dn", PAIRS)
def test_harness_equals_restatement(name, dn):
    """Lengths around one block and the default window, every window and trim edge, rows around one and two passes of the counting kernel,
    true lags at and beyond +-maxlag, maxlag 0 and 4096, ntx != N, 1 / 3 / 16 transmitted modes, identical modes (the first wins), the four
    quarter turns, nine alphabets, exact decision ties, labels outside [0, M)."""
    assert _run(name, dn) == ref.expected(name)


@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_cases_find_what_was_put_in(dn):
    """What the restatement itself was checked for on the CPU, on the device: the default case finds mode 1, rotation 1, lag 7; a true lag
    of maxlag + 1 is not found and matches little of its window; the overlap, not N, is compared when ntx is short."""
    res = _run("lag64", dn)
    assert res[2:5] == (1, 1, 64) and res[5] > 0.9 * res[6]
    res = _run("lag65", dn)
    assert res[5] < 0.2 * res[6]
    assert _run("ntx-short", dn)[1] == 5000
    assert _run("identical-modes", dn)[2] == 0
    assert _run("al-one", dn)[:5] == (0, 20000 - 64, 0, 0, -64)


@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_same_call_twice_gives_the_same_numbers(dn):
    c = ref.make("window257")
    up = _Uploaded(c["rx"], c["labels"], c["alphabet"], dn)
    first = up.call(c["maxlag"], c["window"], c["trim"])
    assert first == up.call(c["maxlag"], c["window"], c["trim"]) == ref.expected("window257")


@pytest.mark.parametrize("order", [("2trip+300", "N257"), ("N257", "2trip+300")])
def test_scratch_of_a_long_row_does_not_leak_into_a_short_one(order):
    """The scratch slot keeps its size and contents between calls: a short row after the longest one gives what it gives on its own."""
    for name in order:
        assert _run(name, "c64") == ref.expected(name), name


@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_cal_ser_dev_rows_are_the_single_row_calls(dn):
    N, al = 6000, ref.alphabet("qam16")
    lab = ref.labels(2, N, 16, 99)
    rows = np.stack([ref.received(lab[m], al, t, lag, N, ref.snr_for(16), 100 + i)[0] for i, (m, t, lag) in enumerate(((1, 3, 7), (0, 2, -19), (1, 0, 0)))])
    want = [ref.ser(r, lab, al, 64, 2048, 100) for r in rows]
    assert [w[2:5] for w in want] == [(1, 1, 7), (0, 2, -19), (1, 0, 0)] and all(w[0] > 0 for w in want)
    T, A = DeviceArray.from_host(lab), DeviceArray.from_host(al.astype(CT[dn]))
    got = ber.cal_ser_dev(DeviceArray.from_host(rows.astype(CT[dn])), T, A, maxlag=64, window=2048, trim=100)
    assert len(got) == 3
    for r, (g, w) in enumerate(zip(got, want)):
        one = ber.cal_ser_dev(DeviceArray.from_host(rows[r:r + 1].astype(CT[dn])), T, A, maxlag=64, window=2048, trim=100)
        assert one == [g]
        assert (g["errors"], g["compared"], g["tx_mode"], g["rotation"], g["lag"], g["window_matches"], g["window"]) == w
        assert g["ser"] == g["errors"] / max(g["compared"], 1)
    # a row without any partner: nothing compared, and the rate is 0 / 1
    g = ber.cal_ser_dev(DeviceArray.from_host(rows[:1].astype(CT[dn])), DeviceArray.from_host(lab[:, :1]), A, maxlag=0, window=16, trim=100)[0]
    assert (g["errors"], g["compared"], g["ser"]) == (0, 0, 0.0)


# ------------------------------------------------------------------------------------------------ the bare counter
def _count_inputs(n, lag, ntx, seed):
    rng = np.random.default_rng(seed)
    tx = rng.integers(0, 16, max(ntx, 1)).astype(np.int32)
    rx = rng.integers(0, 16, n).astype(np.int32)
    i = np.arange(n)
    have = (i - lag >= 0) & (i - lag < ntx)
    rx[have] = tx[(i - lag)[have]]
    hit = rng.random(n) < 0.03
    hit[[0, n - 1]] = True
    hit[TRIP::TRIP] = True                                   # the first symbol of every further pass, and the last symbol, are in error
    rx[hit] = (rx[hit] + 1 + rng.integers(0, 15, np.count_nonzero(hit))) % 16
    return rx, tx


@pytest.mark.parametrize("lag", [-19, 0, 7])
@pytest.mark.parametrize("n", [1, 255, 257, TRIP - 1, TRIP + 1, 2 * TRIP + 300])
def test_count_errors_adds_the_restated_count(n, lag):
    for ntx in (n, 2 * n // 3):
        rx, tx = _count_inputs(n, lag, ntx, 1000 * n + lag + 20)
        want = ref.count_errors(rx, tx[:ntx], n, lag)
        if ntx == n and n > abs(lag):
            assert want >= 1 + (n - 1) // TRIP
        R, T, cnt = DeviceArray.from_host(rx), DeviceArray.from_host(tx), DeviceArray.from_host(np.array([5], np.uint64))
        _lib.call("qh_count_errors_dev", R.ptr, T.ptr, n, lag, ntx, cnt.ptr)
        assert int(cnt.to_host()[0]) == 5 + want
        _lib.call("qh_count_errors_dev", R.ptr, T.ptr, n, lag, ntx, cnt.ptr)             # adds again: it never clears
        assert int(cnt.to_host()[0]) == 5 + 2 * want
        _lib.call("qh_count_errors_dev", R.ptr, T.ptr, 0, lag, ntx, cnt.ptr)             # n = 0 leaves the counter alone
        assert int(cnt.to_host()[0]) == 5 + 2 * want


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_bad_arguments_are_refused_before_anything_is_launched(dn):
    c = ref.make("N256")
    up = _Uploaded(c["rx"], c["labels"], c["alphabet"], dn)
    odd = ref.make("N257")
    up_odd = _Uploaded(odd["rx"], odd["labels"], odd["alphabet"], dn)
    bad = [(up, 64, 0, 0, dict(N=0)), (up, 64, 0, 0, dict(nmodes=0)), (up, 64, 0, 0, dict(nmodes=17)), (up, 64, 0, 0, dict(M=0)),
           (up, -1, 0, 0, {}), (up, 4097, 0, 0, {}), (up, 64, 0, -1, {}),
           (up, 64, 0, 128, {}),                              # 2 trim = N
           (up_odd, 64, 0, 129, {}),                          # 2 trim = N + 1
           (up, 64, 0, 0, dict(E=None)), (up, 64, 0, 0, dict(T=None)), (up, 64, 0, 0, dict(A=None)), (up, 64, 0, 0, dict(result=False))]
    for u, maxlag, window, trim, over in bad:
        with pytest.raises(ValueError):
            u.call(maxlag, window, trim, **over)
    assert up.call(64, 0, 127) == ref.ser(c["rx"], c["labels"], c["alphabet"], 64, 0, 127)      # the largest trim of 256 symbols, and the library still works
    assert up_odd.call(64, 0, 128) == ref.ser(odd["rx"], odd["labels"], odd["alphabet"], 64, 0, 128)


def test_bad_arguments_of_the_bare_counter():
    R, T, cnt = (DeviceArray.from_host(np.zeros(8, np.int32)), DeviceArray.from_host(np.ones(8, np.int32)), DeviceArray.from_host(np.array([5], np.uint64)))
    for args in ((None, T.ptr, 8, 0, 8, cnt.ptr), (R.ptr, None, 8, 0, 8, cnt.ptr), (R.ptr, T.ptr, 8, 0, 8, None), (R.ptr, T.ptr, 8, 0, -1, cnt.ptr)):
        with pytest.raises(ValueError):
            _lib.call("qh_count_errors_dev", *args)
    assert int(cnt.to_host()[0]) == 5
    _lib.call("qh_count_errors_dev", R.ptr, T.ptr, 8, 0, 8, cnt.ptr)
    assert int(cnt.to_host()[0]) == 13
