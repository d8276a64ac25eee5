"""Synchronisation of received and transmitted rows on the MI355X (csrc/sync.hip) against the float64 restatement (tests/sync_ref.py),
the host form and the reference's recorded results (tests/golden/sync.npz, tests/golden/metrics.npz)."""
import numpy as np
import pytest

import sync_ref
from qampy_amd import _lib, synth
from qampy_amd.core import ber_functions, hip_dsp
from qampy_amd.signals import SignalQAM

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
XTOL = {"c64": 1e-5, "c128": 1e-11}         # correlation: max-abs error over the rms of the expected row (tests/test_gpu_frontend.py's bar)
RTOL = {"c64": 1e-5, "c128": 1e-12}         # evm / snr / s0 / n0 (tests/test_gpu_metrics.py)
GABS = {"c64": 1e-5, "c128": 1e-10}         # gmi, gmi per bit, mi (tests/test_gpu_metrics.py)
TILE = hip_dsp.PEAK_TILE


def _dev(a):
    return _lib.DeviceArray.from_host(np.ascontiguousarray(a))


def _rms(a):
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden["sync"]


def _cx(q, scale):
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(scale)


# ------------------------------------------------------------------------------------------------ correlation
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("rows,nx,ny", [(1, 100, 100), (1, 1, 300), (1, 300, 1), (1, 4096, 4096), (1, 5000, 3000), (2, 100, 100), (2, 5000, 3000)])
def test_xcorr_against_numpy(rows, nx, ny, dn):
    """P = 2^8 (the floor), a single sample on either side, 2^13 (the last single-workgroup size), 2^14 (the first four-step size), two
    rows at once.  Measured max-abs error / rms, complex64: 3.1e-7 .. 7.0e-7 (5000 / 3000: 6.8e-7, two rows 7.0e-7); complex128:
    6.9e-16 .. 1.9e-15 (5000 / 3000: 1.8e-15)."""
    rng = np.random.default_rng(nx + 3 * ny + rows)
    x = (rng.standard_normal((rows, nx)) + 1j * rng.standard_normal((rows, nx))).astype(CT[dn])
    y = (rng.standard_normal(ny) + 1j * rng.standard_normal(ny)).astype(CT[dn])
    want = sync_ref.xcorr(x, y)
    out = _lib.DeviceArray((rows, nx + ny - 1), CT[dn])
    got = hip_dsp.xcorr_dev(_dev(x), _dev(y), out).to_host()
    err = max(float(np.max(np.abs(got[r] - want[r]))) / _rms(want[r]) for r in range(rows))
    print("xcorr %s rows %d nx %d ny %d: max-abs error / rms %.3g" % (dn, rows, nx, ny, err))
    assert err < XTOL[dn]
    again = hip_dsp.xcorr_dev(_dev(x), _dev(y), _lib.DeviceArray((rows, nx + ny - 1), CT[dn])).to_host()
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8))                       # bit-identical
    if rows == 1:                                                                        # a 1-d row is one row
        flat = hip_dsp.xcorr_dev(_dev(x[0]), _dev(y), _lib.DeviceArray((nx + ny - 1,), CT[dn])).to_host()
        assert np.array_equal(flat, got[0])


def test_xcorr_refuses_what_does_not_fit():
    c = np.complex64
    x = _lib.DeviceArray((8,), c)
    for nx, ny in ((2 ** 23 + 1, 2 ** 23 + 1), (0, 8), (8, 0)):
        with pytest.raises(ValueError):
            _lib.call("qh_xcorr_c64_dev", x.ptr, 1, nx, x.ptr, ny, x.ptr)


# ------------------------------------------------------------------------------------------------ peak search
def _peak(cc, n, dn):
    res = _lib.DeviceArray((6,), np.float64)
    return hip_dsp.xcorr_peak_dev(_dev(cc.astype(CT[dn])), n, res).to_host()


def _small(n, seed=0):
    """Small integers: magnitudes below 3, squares and sums exact."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1, 2, n) + 1j * rng.integers(-1, 2, n)).astype(np.complex128)


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("n", [1, 2, TILE, TILE + 1, 3 * TILE + 17, 300 * TILE + 5])
def test_peak_positions(n, dn):
    """One value, one tile, one tile and one value, several tiles, and more tiles than the second stage has threads (300 > 256)."""
    for k in sorted({0, n - 1, n // 2, min(TILE - 1, n - 1), min(TILE, n - 1)}):
        cc = _small(n, n)
        cc[k] = 3 + 4j
        res = _peak(cc, n, dn)
        assert np.array_equal(res, sync_ref.peak(cc)) and res[0] == k and res[5] == 5, (k, res)


@pytest.mark.parametrize("dn", CT)
def test_peak_ties_go_to_the_lower_index(dn):
    n = 300 * TILE
    for a, b in ((5, TILE + 9), (2 * TILE - 1, 2 * TILE), (7 * TILE + 3, 290 * TILE + 1), (70, 71), (63, 64), (100, 100 + 256)):
        cc = _small(n, 1)
        cc[a], cc[b] = 5, -4 + 3j                       # equal magnitudes: different tiles, waves, lanes and strides of one thread
        res = _peak(cc, n, dn)
        assert res[0] == a and np.array_equal(res, sync_ref.peak(cc)), (a, b, res)
        cc[a], cc[b] = cc[b], cc[a]
        assert _peak(cc, n, dn)[0] == a


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("n", [1, 100, TILE, TILE + 1])
def test_peak_ignores_the_padding(n, dn):
    cc = _small(n + 300, 2)
    cc[n - 1] = 3
    cc[n:] = 100 - 100j                                 # beyond n: must not be seen
    res = _peak(cc, n, dn)
    assert np.array_equal(res, sync_ref.peak(cc[:n])) and res[0] == n - 1


@pytest.mark.parametrize("dn", CT)
def test_peak_directional_maxima_come_from_four_elements(dn):
    n = 2 * TILE + 100
    cc = _small(n, 3)
    cc[10], cc[TILE + 5], cc[2 * TILE + 50], cc[300] = 7 + 1j, -1 + 6j, -5 - 1j, 1 - 4j
    cc[77] = 6 + 5j                                     # the magnitude peak is a fifth element
    res = _peak(cc, n, dn)
    assert list(res[:5]) == [77, 7, 6, 5, 4] and res[5] == np.sqrt(61.)


@pytest.mark.parametrize("dn", CT)
def test_peak_with_a_nan_is_numpys(dn):
    n = 2 * TILE + 100
    cc = _small(n, 4)
    cc[20] = 50
    cc[TILE + 33] = np.nan + 0j
    cc[TILE + 900] = 1j * np.nan
    res = _peak(cc, n, dn)
    assert res[0] == TILE + 33 == np.argmax(np.abs(cc)) and np.all(np.isnan(res[1:]))     # the first NaN; np.max gives NaN
    assert hip_dsp.peak_decision(res, 100) == (0, 0, 0.)                                  # what find_sequence_offset_complex returns
    x = np.ones(300, CT[dn])
    y = np.ones(100, CT[dn])
    y[50] = np.nan
    off, yy, turns, peak = ber_functions.find_sequence_offset_complex(x, y, method="hip")
    assert (off, turns, peak) == (0, 0, 0.) and yy is y
    assert ber_functions.find_sequence_offset_complex(x, y)[::2] == (0, 0)                # the host form


@pytest.mark.parametrize("dn", CT)
def test_peak_of_a_stack_of_rows(dn):
    n = TILE + 7
    cc = np.stack([_small(n, 5), _small(n, 6), _small(n, 7)])
    cc[0, 3], cc[1, n - 1], cc[2, TILE] = 4, 4j, -4
    res = hip_dsp.xcorr_peak_dev(_dev(cc.astype(CT[dn])), n, _lib.DeviceArray((3, 6), np.float64)).to_host()
    assert np.array_equal(res, np.stack([sync_ref.peak(c) for c in cc]))


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("dn", CT)
def test_gather_is_exact(dn):
    rng = np.random.default_rng(9)
    for nsrc, nouts in ((7, (3, 7, 20)), (100, (99, 100, 257)), (1025, (1024, 1025, 5000)), (1, (1, 5)), (3000, (1,))):
        src = (rng.standard_normal(nsrc) + 1j * rng.standard_normal(nsrc)).astype(CT[dn])
        d = _dev(src)
        for nout in nouts:
            for offset in (0, 1, -1, nsrc, -nsrc, 3 * nsrc, nsrc - 1, -(2 * nsrc + 3), 37, 10 ** 9 + 7):
                for turns in range(4):
                    got = hip_dsp.cyclic_gather_dev(d, offset, turns, _lib.DeviceArray((nout,), CT[dn])).to_host()
                    assert np.array_equal(got, sync_ref.gather(src, offset, turns, nout)), (nsrc, nout, offset, turns)
    got = hip_dsp.cyclic_gather_dev(d, 5, 6, _lib.DeviceArray((10,), CT[dn])).to_host()  # turns are taken modulo 4
    assert np.array_equal(got, sync_ref.gather(src, 5, 2, 10))


def test_gather_of_labels_and_labels_to_symbols():
    rng = np.random.default_rng(10)
    for nsrc, nout, offset in ((100, 257, -37), (257, 100, 300), (4096, 4096, 3000), (1000, 5000, 1000)):
        src = rng.integers(0, 16, nsrc).astype(np.int32)
        got = hip_dsp.cyclic_gather_dev(_dev(src), offset, 0, _lib.DeviceArray((nout,), np.int32)).to_host()
        assert np.array_equal(got, sync_ref.gather(src, offset, 0, nout))
    idx = rng.integers(-2, 19, (2, 1500)).astype(np.int32)                               # labels outside [0, 16) give 0
    for dn, ct in CT.items():
        al = sync_ref.qam16(1, 0)[1].astype(ct)
        got = hip_dsp.labels_to_symbols_dev(_dev(idx), _dev(al), _lib.DeviceArray(idx.shape, ct)).to_host()
        want = np.where((idx >= 0) & (idx < 16), al[np.clip(idx, 0, 15)], 0)
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ method="hip"
def _compare_with_host(tx, rx, adjust, dn, periodic):
    tx, rx = tx.astype(CT[dn]), rx.astype(CT[dn])
    (htx, hrx), hpeak = ber_functions.sync_and_adjust(tx, rx, adjust)
    (dtx, drx), dpeak = ber_functions.sync_and_adjust(tx, rx, adjust, method="hip")
    for h, d in ((htx, dtx), (hrx, drx)):
        assert h.dtype == d.dtype and h.shape == d.shape and np.array_equal(h, d)
    x, y = (rx, tx) if adjust == "tx" else (tx, rx)
    hoff, hy, hturns, hpk = ber_functions.find_sequence_offset_complex(x, y)
    doff, dy, dturns, dpk = ber_functions.find_sequence_offset_complex(x, y, method="hip")
    idx, cc = ber_functions.find_sequence_offset(x, y, show_cc=True)
    didx, dcc = ber_functions.find_sequence_offset(x, y, show_cc=True, method="hip")
    assert dcc.dtype == cc.dtype and dcc.shape == cc.shape
    bar = XTOL[dn] * _rms(sync_ref.xcorr(x, y))
    assert abs(dpeak - hpeak) <= bar and abs(dpk - hpk) <= bar and dpeak == dpk
    assert dturns == hturns and dy.dtype == hy.dtype
    a = np.abs(cc)
    runner_up = np.delete(a, int(np.argmax(a))).max() / a.max()
    if not periodic:                # several repetitions of the pattern: offsets one period apart give the same alignment
        assert runner_up < 0.9, runner_up
        assert doff == hoff == didx == idx and np.array_equal(dy, hy)



@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("adjust", ["tx", "rx"])
@pytest.mark.parametrize("ntx,nrx", sync_ref.LENGTHS)
def test_method_hip_equals_the_host_form(ntx, nrx, adjust, dn):
    """The aligned rows are equal exactly; the raw offset is compared wherever the correlation has one clear peak (runner-up below 0.9
    of it), which is every case but a pattern repeated several times inside the received row (100 / 257, 100 / 300, 1000 / 3500)."""
    for shift in (37, 3 * ntx // 4):
        for turns in ((shift + ntx) % 4, (shift + ntx + 1) % 4):
            tx, rx = sync_ref.case(ntx, nrx, shift, turns)
            _compare_with_host(tx, rx, adjust, dn, periodic=ntx < 0.7 * nrx)


@pytest.mark.parametrize("dn", CT)
def test_method_hip_equals_the_recorded_reference(fx, dn):
    for k, (ntx, nrx, shift, turns) in enumerate(fx["cases"]):
        tx, rx = _cx(fx["c%d_txq" % k], fx["scale"]).astype(CT[dn]), _cx(fx["c%d_rxq" % k], fx["scale"]).astype(CT[dn])
        for adjust in ("tx", "rx"):
            p = "c%d_%s_" % (k, adjust)
            (atx, arx), peak = ber_functions.sync_and_adjust(tx, rx, adjust, method="hip")
            assert np.array_equal(atx, _cx(fx[p + "txq"], fx["scale"])) and np.array_equal(arx, _cx(fx[p + "rxq"], fx["scale"])), (k, adjust)
            x, y = (rx, tx) if adjust == "tx" else (tx, rx)
            assert abs(peak - fx[p + "peak"]) <= XTOL[dn] * _rms(sync_ref.xcorr(x, y))
            offset, _, nturns, _ = ber_functions.find_sequence_offset_complex(x, y, method="hip")
            assert nturns == fx[p + "turns"]
            if fx[p + "runner_up"] < 0.9:
                assert offset == fx[p + "offset"], (k, adjust)
            else:
                assert ntx < 0.7 * nrx                                                   # the pattern repeats inside the received row


def test_real_and_integer_inputs_follow_the_host_form():
    rng = np.random.default_rng(12)
    x = rng.standard_normal(300)
    y = np.roll(x, -40)[:120]
    for xx, yy in ((x, y), (x.astype(np.float32), y.astype(np.float32)), ((x > 0), (y > 0)), ((8 * x).astype(np.int64), (8 * y).astype(np.int64))):
        idx, cc = ber_functions.find_sequence_offset(xx, yy, show_cc=True)
        didx, dcc = ber_functions.find_sequence_offset(xx, yy, show_cc=True, method="hip")
        assert didx == idx == 40 and dcc.dtype == cc.dtype and dcc.shape == cc.shape
        (htx, hrx), _ = ber_functions.sync_and_adjust(yy, xx)
        (dtx, drx), _ = ber_functions.sync_and_adjust(yy, xx, method="hip")
        assert htx.dtype == dtx.dtype and np.array_equal(htx, dtx) and np.array_equal(hrx, drx)
    tx, rx = sync_ref.case(100, 257, 37, 1)                                               # one side real: the complex path
    (htx, hrx), hp = ber_functions.sync_and_adjust(tx.real, rx)
    (dtx, drx), dp = ber_functions.sync_and_adjust(tx.real, rx, method="hip")
    assert htx.dtype == dtx.dtype and np.array_equal(htx, dtx) and abs(hp - dp) < 1e-9 * abs(hp)


# ------------------------------------------------------------------------------------------------ the point of the change
@pytest.fixture(scope="module")
def receiver():
    """A two-mode 16-QAM capture of 2^13 symbols through the resident receiver; rows and transmitted symbols on the host."""
    from qampy_amd.pipeline import ResidentReceiver
    sig = synth.make_capture(16, 2 ** 13, nmodes=2, snr_db=24, theta=0.5, dgd=20e-12, linewidth=10e3, seed=70, dtype=np.complex64)
    rx = ResidentReceiver(2, sig.shape[1], 2, 16, 15, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(2, 1), Mtestangles=32, Nbps=10,
                          alphabet=sig.coded_symbols)
    rx.load(sig)
    rx.run()
    out = rx.fetch()["out"]
    return rx, out, np.asarray(sig.symbols), np.asarray(sig.coded_symbols)


def _host_frame(per_bit, rotation):
    """Per-bit GMI as the host form orders it.  The device turns the received row onto the transmitted labels, the host form turns the
    transmitted row: with an odd quarter turn the in-phase and the quadrature half of a square alphabet's labels trade places."""
    per_bit = np.asarray(per_bit)
    return np.roll(per_bit, per_bit.size // 2) if rotation % 2 else per_bit


def _check_against_host(rx, out, pattern, coded, trim=0):
    met = rx.metrics(pattern, sync="full", trim=trim)
    ser = rx.ser(pattern, sync="full", trim=trim)
    host = SignalQAM(out, 16, symbols=pattern, coded_symbols=coded)
    _, errs, tx_al = host.cal_ser(verbose=True)
    _, bit_errs, _ = host.cal_ber(verbose=True)
    snr, s0, n0 = host.est_snr(verbose=True)
    evm, (gmi, per_bit), mi = host.cal_evm(), host.cal_gmi(), host.cal_mi()
    N, free = out.shape[1], [0, 1]
    assert trim == 0
    for r in range(2):
        m, s = met[r], ser[r]
        peaks = {i: ber_functions.find_sequence_offset_complex(out[r], pattern[i]) for i in free}
        mode = max(free, key=lambda i: (peaks[i][3], -i))
        free.remove(mode)
        offset, _, turns, peak = peaks[mode]
        assert (m["tx_mode"], m["rotation"]) == (mode, (-turns) % 4) == (s["tx_mode"], s["rotation"])
        assert (m["lag"] - offset) % pattern.shape[1] == 0 and s["lag"] == m["lag"]
        if pattern.shape[1] >= N:                                                        # one clear peak
            assert m["lag"] == offset
        assert abs(m["peak"] - peak) <= 1e-5 * _rms(sync_ref.xcorr(out[r], pattern[mode])) and s["peak"] == m["peak"]
        assert m["window"] is None and m["window_matches"] is None and s["window"] is None and s["window_matches"] is None
        assert m["compared"] == s["compared"] == N
        assert m["errors"] == s["errors"] == np.count_nonzero(errs[r]) and m["ser"] == s["ser"] == np.count_nonzero(errs[r]) / N
        assert m["bit_errors"] == np.count_nonzero(bit_errs[r]) and m["ber"] == np.count_nonzero(bit_errs[r]) / (4 * N)
        np.testing.assert_allclose([m["snr"], m["s0"], m["n0"], m["evm"]], [snr[r], s0[r], n0[r], evm[r]], rtol=RTOL["c64"])
        np.testing.assert_allclose(m["gmi"], gmi[r], rtol=0, atol=GABS["c64"])
        np.testing.assert_allclose(_host_frame(m["gmi_per_bit"], m["rotation"]), per_bit[r], rtol=0, atol=GABS["c64"])
        np.testing.assert_allclose(m["mi"], mi[r], rtol=0, atol=GABS["c64"])
    return met


def test_resident_metrics_with_full_sync_equal_the_host_metrics(receiver):
    """The transmitted pattern rolled by 3000 symbols, turned a quarter turn, its modes swapped: the full correlation finds it and the
    counts are the host's exactly; the bounded search on a window cannot."""
    rx, out, tx, coded = receiver
    pattern = np.ascontiguousarray(np.roll(tx[::-1] * 1j, 3000, axis=-1))
    met = _check_against_host(rx, out, pattern, coded)
    assert sorted(m["tx_mode"] for m in met) == [0, 1] and max(m["ser"] for m in met) < 0.02, met
    held = {k: v.ptr for k, v in rx._sync_workspace().items()}
    assert set(held) == {"symbols", "cc", "peaks", "labels0", "labels1"}
    again = rx.metrics(pattern, sync="full")
    assert {k: v.ptr for k, v in rx._sync_workspace().items()} == held                   # a repeated call allocates no buffer
    for a, b in zip(again, met):
        assert all(np.array_equal(a[k], b[k]) for k in a), (a, b)                        # bit-identical
    for w in rx.ser(pattern):                                                             # sync="window": the alignment is out of reach
        assert w["window"] == 4096 and w["window_matches"] < 0.25 * w["window"], w
        assert w["errors"] > 0.5 * w["compared"] and "peak" not in w
    for w in rx.metrics(pattern):
        assert w["errors"] > 0.5 * w["compared"] and "peak" not in w and "window" not in w


def test_resident_metrics_with_a_short_pattern(receiver):
    """A pattern of 1000 symbols against 2^13 received: continued periodically, every symbol compared."""
    rx, out, tx, coded = receiver
    rng = np.random.default_rng(21)
    pattern = coded[rng.integers(0, 16, (2, 1000))]
    rows = np.stack([pattern[1, (np.arange(out.shape[1]) + 300) % 1000] * -1j, pattern[0, (np.arange(out.shape[1]) + 77) % 1000]])
    rows = (rows + 0.05 * (rng.standard_normal(rows.shape) + 1j * rng.standard_normal(rows.shape))).astype(np.complex64)
    dev = rx.out if rx.Mtestangles else rx.eq
    keep = dev.to_host()
    try:
        dev.set(rows)
        met = _check_against_host(rx, rows, np.ascontiguousarray(pattern), coded)
        assert [m["tx_mode"] for m in met] == [1, 0] and [m["rotation"] for m in met] == [1, 0] and all(m["errors"] == 0 for m in met), met
        assert [m["lag"] % 1000 for m in met] == [700, 923]
    finally:
        dev.set(keep)


def test_more_rows_than_modes_is_refused(receiver):
    rx, out, tx, coded = receiver
    with pytest.raises(ValueError, match="modes"):
        rx.metrics(np.ascontiguousarray(tx[:1]), sync="full")


@pytest.mark.parametrize("dn", CT)
def test_golden_sync_case_of_the_metrics_through_full_sync(golden, dn):
    """The ``sync_*`` arrays of metrics.npz (quarter turn, shift of 37, swapped modes) through ``cal_metrics_dev(sync="full")``."""
    g = golden["metrics"]
    M, ct = int(g["sync_M"]), CT[dn]
    rxq = g["sync_rxq"]
    rows = ((rxq[..., 0] + 1j * rxq[..., 1].astype(np.float64)) / float(g["rx_scale"])).astype(ct)
    coded = g["M%d_%s_coded" % (M, dn)]
    d_al, d_rows = _dev(coded.astype(ct)), _dev(rows)
    idx_tx = _dev(g["sync_%s_tx_label" % dn].astype(np.int32))
    met = ber_functions.cal_metrics_dev(d_rows, idx_tx, d_al, sync="full")
    ser = ber_functions.cal_ser_dev(d_rows, idx_tx, d_al, sync="full")
    pre, N = "sync_%s_" % dn, rows.shape[1]
    assert [m["tx_mode"] for m in met] == [1, 0] and all(m["lag"] == 37 and m["compared"] == N for m in met)
    for r, (m, s) in enumerate(zip(met, ser)):
        assert m["errors"] / N == g[pre + "ser"][r] == s["ser"] and m["ber"] == g[pre + "ber"][r]
        np.testing.assert_allclose([m["snr"], m["s0"], m["n0"], m["evm"]], [g[pre + k][r] for k in ("snr", "s0", "n0", "evm")], rtol=RTOL[dn])
        np.testing.assert_allclose(m["gmi"], g[pre + "gmi"][r], rtol=0, atol=GABS[dn])
        assert m["rotation"] == 3                                                         # the received rows were turned by 1j
        np.testing.assert_allclose(_host_frame(m["gmi_per_bit"], m["rotation"]), g[pre + "gmi_per_bit"][r], rtol=0, atol=GABS[dn])
        np.testing.assert_allclose(m["mi"], g[pre + "mi"][r], rtol=0, atol=GABS[dn])
        labels = hip_dsp.cyclic_gather_dev(idx_tx.row(m["tx_mode"]), m["lag"], 0, _lib.DeviceArray((N,), np.int32)).to_host()
        turned = coded[labels] * 1j ** ((-m["rotation"]) % 4)                             # the reference recorded the turned row's labels
        assert np.array_equal(np.argmin(np.abs(turned[:, None] - coded[None, :]), axis=-1), g["sync_%s_tx_aligned_label" % dn][r])


@pytest.mark.parametrize("dn", CT)
def test_signal_methods_with_sync_method_hip(fx, dn):
    """``SignalQAM`` with the alignment on the device equals the default and the reference on the golden case: 4096 16-QAM symbols,
    pattern rolled by 3000, a quarter turn, swapped modes."""
    ct = CT[dn]
    coded = fx["qam_%s_coded" % dn]
    sig = SignalQAM(_cx(fx["qam_rxq"], fx["scale"]).astype(ct), 16, symbols=coded[fx["qam_%s_pattern_label" % dn]], coded_symbols=coded)
    ser, _, tx_al = sig.cal_ser(verbose=True, sync_method="hip")
    assert np.array_equal(ser, sig.cal_ser()) and np.array_equal(ser, fx["qam_%s_ser" % dn])
    assert np.array_equal(tx_al, coded[fx["qam_%s_aligned_label" % dn]])
    assert np.array_equal(sig.cal_ber(sync_method="hip"), fx["qam_%s_ber" % dn])
    for name in ("cal_evm", "est_snr", "cal_mi"):
        assert np.array_equal(getattr(sig, name)(sync_method="hip"), getattr(sig, name)()), name
    assert np.array_equal(sig.cal_gmi(sync_method="hip")[1], sig.cal_gmi()[1])


def test_channel_bank_metrics_with_full_sync():
    """The channel bank's twins pass ``sync`` through: per channel the host's error counts on the fetched rows."""
    from qampy_amd.pipeline import ChannelBank
    sigs = [synth.make_capture(16, 2 ** 13, nmodes=2, snr_db=24, theta=0.5 + 0.1 * c, dgd=20e-12, linewidth=10e3, seed=70 + c, dtype=np.complex64)
            for c in range(2)]
    bank = ChannelBank(2, 2, sigs[0].shape[1], 2, 16, 15, (2e-3, 5e-4), methods=("mcma", "sbd"), Niter=(2, 1), Mtestangles=32, Nbps=10,
                       alphabet=sigs[0].coded_symbols)
    for c, sg in enumerate(sigs):
        bank.load(c, sg)
    bank.run()
    for c, sg in enumerate(sigs):
        pattern = np.ascontiguousarray(np.roll(np.asarray(sg.symbols)[::-1] * -1j, 5000 + c, axis=-1))
        met, ser = bank.metrics(c, pattern, sync="full"), bank.ser(c, pattern, sync="full")
        host = SignalQAM(bank.fetch(c)["out"], 16, symbols=pattern, coded_symbols=np.asarray(sg.coded_symbols))
        _, errs, _ = host.cal_ser(verbose=True)
        _, bit_errs, _ = host.cal_ber(verbose=True)
        assert sorted(m["tx_mode"] for m in met) == [0, 1]
        for r in range(2):
            assert met[r]["errors"] == ser[r]["errors"] == np.count_nonzero(errs[r]) and met[r]["bit_errors"] == np.count_nonzero(bit_errs[r])
            assert met[r]["compared"] == errs.shape[1] and met[r]["peak"] > 0 and met[r]["ser"] < 0.02
