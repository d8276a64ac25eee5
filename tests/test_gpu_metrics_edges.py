"""The signal-quality kernels (qampy_amd/csrc/metrics.hip) at their edges, against the float64 restatement of tests/metrics_ref.py
(itself checked against the reference by tests/test_metrics_ref.py): lengths around the grid-stride trip (1024 blocks x 256
threads = 262 144 symbols), every nbits 1..10, the alignment arguments of the _dev entry points, labels outside [0, M), SNRs from
-5 to 60 dB, the device-row paths, repeat calls and bad arguments; and 8- / 512- / 1024-QAM against the reference
(tests/golden/metrics_orders.npz).

Tolerances (kernel against the float64 restatement):
- counts: complex128 exact; complex64 decides in float32, so the number of differing decisions may not exceed the number of
  near-ties (best and second-best distance within 1e-6 relative); the inputs are random, so that is 0 nearly everywhere.
- sums: the error power to rtol 1e-11 (complex128) / 1e-6 (complex64: float32 distances, summed in double).
- LLRs: complex128 rtol 1e-9, atol 1e-8 where both subset sums shifted by the global minimum are normal doubles; beyond that
  its documented range is +-inf with the restatement's sign (or, while a sum is subnormal, within 1 of it with that sign).
  complex64 rtol 1e-5, atol 1e-4 + 2^-21 snr max(m0, m1) (float32 distances: snr m carries float32's relative error) and
  finite everywhere (per-subset shifts).
- GMI and MI: atol 1e-10 (complex128) / 1e-5 (complex64): means of terms computed in float32 and summed in double.
- SNR, S0, N0: rtol 1e-11 (complex128) / 1e-10 (complex64): the class statistics are accumulated in double from the samples,
  complex64 ones widened exactly, so only the order of the sums differs."""
import numpy as np
import pytest

import metrics_ref as ref
from qampy_amd import _lib, synth, theory
from qampy_amd._lib import DeviceArray
from qampy_amd.core import ber_functions, hip_dsp
from qampy_amd.signals import SignalQAM

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
TRIP = 1024 * 256                            # symbols per grid-stride trip (MET_MAXBLK x MET_THREADS)
LENGTHS = (1, 2, 255, 256, 257, TRIP - 1, TRIP, TRIP + 1, 3 * TRIP + 17)
TOL = {"c128": dict(pow=1e-11, llr_rtol=1e-9, llr_atol=1e-8, info=1e-10, snr=1e-11),
       "c64": dict(pow=1e-6, llr_rtol=1e-5, llr_atol=1e-4, info=1e-5, snr=1e-10)}


# ------------------------------------------------------------------------------------------------ inputs
def _alphabet(M, ct, synthetic=False):
    """The square / cross QAM alphabet in label order, or (synthetic) M random points of unit power, labels = index."""
    if not synthetic:
        return np.ascontiguousarray(theory.coded_symbols_qam(M).astype(ct))
    rng = np.random.default_rng(M)
    al = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    return np.ascontiguousarray((al / np.sqrt(np.mean(np.abs(al) ** 2))).astype(ct))


def _noisy(al, t, snr_db, rng):
    n = 10 ** (-snr_db / 20) * (rng.standard_normal(t.shape) + 1j * rng.standard_normal(t.shape)) / np.sqrt(2)
    return np.asarray(al, np.complex128)[t] + n


def _case(M, N, snr_db, ct, seed, synthetic=False, bad_frac=0.):
    """(rx (N,) ct, labels (N,) int32, alphabet): uniform labels, AWGN at snr_db, a fraction bad_frac of labels set to -1 or M."""
    rng = np.random.default_rng(seed)
    al = _alphabet(M, ct, synthetic)
    t = rng.integers(0, M, N).astype(np.int32)
    rx = _noisy(al, t, snr_db, rng).astype(ct)
    if bad_frac:
        bad = rng.random(N) < bad_frac
        t[bad] = np.where(rng.random(np.count_nonzero(bad)) < 0.5, -1, M)
    return rx, t, al


def _dn(ct):
    return "c64" if np.dtype(ct) == np.complex64 else "c128"


# ------------------------------------------------------------------------------------------------ the C ABI
def _fused(rx, t, al, rot=0, lag=0, trim=0, ntx=None, snr=1., minmax=False):
    dn = _dn(rx.dtype)
    E, T, A = DeviceArray.from_host(rx), DeviceArray.from_host(t), DeviceArray.from_host(al)
    counts, sums = np.zeros(3, np.int64), np.zeros(2 + ref.nbits(al.size), np.float64)
    _lib.call("qh_metrics_%s_dev" % dn, E.ptr, rx.size, T.ptr, t.size if ntx is None else ntx, A.ptr, al.size, rot, lag, trim, float(snr),
              int(minmax), _lib.ptr(counts), _lib.ptr(sums))
    return counts, sums


def _snr_dev(rx, t, al, rot=0, lag=0, trim=0, ntx=None):
    dn = _dn(rx.dtype)
    E, T, A = DeviceArray.from_host(rx), DeviceArray.from_host(t), DeviceArray.from_host(al)
    res = np.zeros(3, np.float64)
    _lib.call("qh_estimate_snr_%s_dev" % dn, E.ptr, rx.size, T.ptr, t.size if ntx is None else ntx, A.ptr, al.size, rot, lag, trim, _lib.ptr(res))
    return res


def _llr_dev(rx, al, snr, minmax, nbits=None):
    dn = _dn(rx.dtype)
    nb = ref.nbits(al.size) if nbits is None else nbits
    E, A, L = DeviceArray.from_host(rx), DeviceArray.from_host(al), DeviceArray((max(rx.size, 1), nb), np.float64)
    _lib.call("qh_soft_l_value_demapper_%s_dev" % dn, E.ptr, rx.size, nb, float(snr), A.ptr, al.size, int(minmax), L.ptr)
    return L.to_host()[:rx.size]


def _llr_host(rx, al, snr, minmax):
    L = np.zeros((rx.size, ref.nbits(al.size)), np.float64)
    _lib.call("qh_soft_l_value_demapper_%s%s" % ("minmax_" if minmax else "", _dn(rx.dtype)), _lib.ptr(rx), rx.size, ref.nbits(al.size), float(snr),
              _lib.ptr(al), al.size, _lib.ptr(L))
    return L


# ------------------------------------------------------------------------------------------------ checks
def _check_counts(counts, r, dn, nb):
    assert counts[2] == r["compared"]
    if dn == "c128":
        assert (counts[0], counts[1]) == (r["errors"], r["bit_errors"])
    else:
        assert abs(int(counts[0]) - r["errors"]) <= r["near_ties"], (counts, r["errors"], r["near_ties"])
        assert abs(int(counts[1]) - r["bit_errors"]) <= nb * r["near_ties"]


def _check_fused(counts, sums, r, dn, M):
    nb, tol = ref.nbits(M), TOL[dn]
    _check_counts(counts, r, dn, nb)
    n = max(r["compared"], 1)
    np.testing.assert_allclose(sums[0], r["err_pow"], rtol=tol["pow"])
    np.testing.assert_allclose(np.log2(M) - sums[1] / n, r["mi"], rtol=0, atol=tol["info"], err_msg="mi")
    np.testing.assert_allclose(1 - sums[2:] / n, r["gmi_per_bit"], rtol=0, atol=tol["info"], err_msg="gmi per bit")


def _check_snr(res, want, dn):
    want = np.asarray(want, np.float64)
    if np.isnan(want[0]):
        assert np.isnan(res[0]), res
        return
    np.testing.assert_allclose(res, want, rtol=TOL[dn]["snr"], err_msg="snr, s0, n0")


def _side_minima(x, al):
    d = ref.dist2(np.asarray(x, np.complex128), np.asarray(al, np.complex128))
    nb = ref.nbits(al.size)
    return np.stack([d.reshape(-1, 1 << k, 2, 1 << (nb - 1 - k)).min(axis=(1, 3)) for k in range(nb)], axis=1)    # (n, nb, 2)


def _check_llr(got, x, al, snr, dn, minmax):
    """Kernel LLRs against the restatement (module docstring); returns the largest deviation where compared tightly."""
    x = np.asarray(x, np.complex128)
    want = ref.llr_maxlog(x, al, snr) if minmax else ref.llr_exact(x, al, snr)
    tol = TOL[dn]
    assert got.shape == want.shape
    if dn == "c64":
        assert np.all(np.isfinite(got))
        atol = tol["llr_atol"] + 2.0 ** -21 * snr * _side_minima(x, al).max(axis=2)
        dev = np.abs(got - want)
        bad = dev > atol + tol["llr_rtol"] * np.abs(want)
        assert not np.any(bad), (got[bad][:5], want[bad][:5], np.count_nonzero(bad))
        return float(dev.max(initial=0.))
    if minmax:
        np.testing.assert_allclose(got, want, rtol=tol["llr_rtol"], atol=tol["llr_atol"])
        return float(np.abs(got - want).max(initial=0.))
    sums = ref.side_sums_global_shift(x, al, snr)
    normal = sums.min(axis=2) >= np.finfo(np.float64).tiny
    np.testing.assert_allclose(got[normal], want[normal], rtol=tol["llr_rtol"], atol=tol["llr_atol"])
    g, w = got[~normal], want[~normal]
    assert np.all(np.sign(g) == np.sign(w)), "an LLR beyond the normal range has the wrong sign"
    assert np.all(np.isinf(g) | (np.abs(g - w) <= 1)), "a finite LLR beyond the normal range is off by more than 1"
    return float(np.abs(got[normal] - want[normal]).max(initial=0.))


# ------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("N", LENGTHS)
def test_lengths_around_the_grid_stride_trip(dn, N):
    """Fused pass, two-pass SNR estimate, LLR kernel (exact and max-log) and fast MI at lengths around the grid-stride trip."""
    M, snr_db = 16, 18.
    rx, t, al = _case(M, N, snr_db, CT[dn], seed=N)
    rx = rx * CT[dn](-1j)                    # a quarter turn back (exact), undone by rot = 1
    snr = 10 ** (snr_db / 10)
    r = ref.metrics(rx, t, al, rot=1, snr=snr)
    assert r["errors"] <= 0.05 * r["compared"] + 1
    _check_fused(*_fused(rx, t, al, rot=1, snr=snr), r, dn, M)
    x, tt = ref.aligned(rx, t, M, rot=1)
    est = ref.snr_estimate(x, tt, M, N)
    _check_snr(_snr_dev(rx, t, al, rot=1), est, dn)
    for minmax in (False, True):
        _check_llr(_llr_dev(rx, al, snr, minmax), rx, al, snr, dn, minmax)
    mi = hip_dsp.cal_mi_mc_fast(rx, np.ascontiguousarray(al[t]), al, 1 / snr)
    np.testing.assert_allclose(mi, np.log2(M) - ref.mi_fast_sum(rx.astype(np.complex128), al[t], al, snr) / N, rtol=0, atol=TOL[dn]["info"])


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("ML", [(64, 4095), (64, 4097), (64, 12289), (1024, 255), (1024, 257)])
def test_mi_mc_around_the_grid_stride_trip(dn, ML):
    """cal_mi_mc's grid runs over L * M (noise sample, transmitted point) pairs: L * M on both sides of 262 144, and 3 trips."""
    M, L = ML
    rng = np.random.default_rng(L)
    al = _alphabet(M, CT[dn])
    noise = (0.05 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(CT[dn])
    N0 = 2 * 0.05 ** 2
    np.testing.assert_allclose(hip_dsp.cal_mi_mc(noise, al, N0), ref.mi_mc(noise, al, N0), rtol=0, atol=TOL[dn]["info"])


# ------------------------------------------------------------------------------------------------ orders
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("nb", range(1, 11))
def test_every_nbits_at_the_abi(dn, nb):
    """nbits 1..10 on a synthetic alphabet (labels = index): fused pass (both LLR forms), SNR estimate and both demappers."""
    M = 1 << nb
    N = TRIP + 1000 if nb <= 6 else 40000
    snr_db = 3. * nb + 6
    rx, t, al = _case(M, N, snr_db, CT[dn], seed=100 + nb, synthetic=True, bad_frac=0.01)
    snr = 10 ** (snr_db / 10)
    for minmax in (False, True):
        r = ref.metrics(rx, t, al, lag=0, trim=3, snr=snr, minmax=minmax)
        _check_fused(*_fused(rx, t, al, trim=3, snr=snr, minmax=minmax), r, dn, M)
    x, tt = ref.aligned(rx, t, M, trim=3)
    _check_snr(_snr_dev(rx, t, al, trim=3), ref.snr_estimate(x, tt, M, N - 6), dn)
    n = min(N, 8192)
    for minmax in (False, True):
        _check_llr(_llr_host(rx[:n], al, snr, minmax), rx[:n], al, snr, dn, minmax)


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", [256, 512, 1024])
def test_class_statistics_layouts(dn, M):
    """class_stats_kernel's thread layouts - S = 64 (M <= 64), 128, 256 threads per class group and the M > 256 layout (each
    thread owns classes g, g + 256, ...) - over many tiles and three grid trips, with labels outside [0, M) and an alignment."""
    for m in sorted({M, 32, 128}) if M == 256 else (M,):
        N = 3 * TRIP + 999
        rx, t, al = _case(m, N, 25., CT[dn], seed=m, bad_frac=0.01)
        rot, lag, trim, ntx = 3, -7, 11, N - 5
        x, tt = ref.aligned(rx, t, m, rot, lag, trim, ntx)
        _check_snr(_snr_dev(rx, t, al, rot, lag, trim, ntx), ref.snr_estimate(x, tt, m, ref.overlap(N, ntx, lag, trim)), dn)


# ------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("rot", range(4))
def test_alignment_arguments(dn, rot):
    """Every rot x lag x trim x ntx combination of the _dev entry points on rows built for that rot and lag (outside the
    transmitted sequence: random points), 1 % of labels -1 or M."""
    M, N = 16, 4099
    rng = np.random.default_rng(7 + rot)
    al = _alphabet(M, CT[dn])
    t = rng.integers(0, M, N + 300).astype(np.int32)
    snr = 10 ** 1.5
    for lag in (-300, -1, 0, 1, 257):
        i = np.arange(N)
        src = rng.integers(0, M, N)
        ok = (i - lag >= 0) & (i - lag < t.size)
        src[ok] = t[i[ok] - lag]
        rx = (_noisy(al, src, 15., rng) * 1j ** (-rot % 4)).astype(CT[dn])
        tb = t.copy()
        bad = rng.random(tb.size) < 0.01
        tb[bad] = np.where(rng.random(np.count_nonzero(bad)) < 0.5, -1, M)
        for trim in (0, 1, 1000):
            for ntx in (N, N // 2, N + 300):
                tx = np.ascontiguousarray(tb[:ntx])
                r = ref.metrics(rx, tx, al, rot, lag, trim, ntx, snr=snr)
                assert r["errors"] < 0.1 * r["compared"]
                _check_fused(*_fused(rx, tx, al, rot, lag, trim, snr=snr), r, dn, M)
                x, tt = ref.aligned(rx, tx, M, rot, lag, trim)
                _check_snr(_snr_dev(rx, tx, al, rot, lag, trim), ref.snr_estimate(x, tt, M, ref.overlap(N, ntx, lag, trim)), dn)


def _impaired_rows(M, N, dn, seed, rot, lag):
    """(out (2, N) DeviceArray, idx_tx (2, N) DeviceArray, tx labels, rows, alphabet): row r carries tx mode 1 - r (swapped modes)
    delayed by ``lag`` and turned by j^-rot, so that rx[i] j^rot is close to the point of tx[1 - r, i - lag]."""
    rng = np.random.default_rng(seed)
    al = _alphabet(M, CT[dn])
    t = rng.integers(0, M, (2, N)).astype(np.int32)
    rows = np.empty((2, N), CT[dn])
    for r in range(2):
        src = rng.integers(0, M, N)                          # where i - lag is outside the transmitted sequence
        i = np.arange(N)
        ok = (i - lag >= 0) & (i - lag < N)
        src[ok] = t[1 - r, i[ok] - lag]
        rows[r] = (_noisy(al, src, 18., rng) * (1j ** (-rot % 4))).astype(CT[dn])
    return DeviceArray.from_host(rows), DeviceArray.from_host(t), t, rows, al


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("rot,lag,trim", [(0, 0, 0), (1, -1, 1), (2, 257, 1000), (3, -300, 0)])
def test_cal_metrics_dev_finds_and_applies_the_alignment(dn, rot, lag, trim):
    """cal_metrics_dev on rows with swapped modes, a quarter turn and a lag: it finds them and every field equals the restatement."""
    M, N = 64, 20000
    out, idx, t, rows, al = _impaired_rows(M, N, dn, seed=rot * 7 + trim, rot=rot, lag=lag)
    A = DeviceArray.from_host(al)
    res = ber_functions.cal_metrics_dev(out, idx, A, maxlag=300, trim=trim)
    for r in range(2):
        m = res[r]
        assert (m["tx_mode"], m["rotation"], m["lag"]) == (1 - r, rot, lag)
        w = ref.metrics(rows[r], t[1 - r], al, rot, lag, trim)
        _check_counts(np.array([m["errors"], m["bit_errors"], m["compared"]]), w, dn, 6)
        _check_snr(np.array([m["snr"], m["s0"], m["n0"]]), [w["snr"], w["s0"], w["n0"]], dn)
        np.testing.assert_allclose(m["evm"], w["evm"], rtol=TOL[dn]["pow"])
        np.testing.assert_allclose(m["gmi_per_bit"], w["gmi_per_bit"], rtol=0, atol=TOL[dn]["info"])
        np.testing.assert_allclose([m["gmi"], m["mi"]], [w["gmi"], w["mi"]], rtol=0, atol=TOL[dn]["info"] * 6)


@pytest.mark.parametrize("dn", CT)
def test_empty_class_gives_nan(dn):
    M, N = 16, 5000
    rx, t, al = _case(M, N, 20., CT[dn], seed=3)
    t[t == 5] = 6
    assert np.isnan(_snr_dev(rx, t, al)[0])
    assert np.isnan(hip_dsp.estimate_snr(rx, np.ascontiguousarray(al[t]), al)[0])
    x, tt = ref.aligned(rx, t, M)
    assert np.isnan(ref.snr_estimate(x, tt, M, N)[0])


# ------------------------------------------------------------------------------------------------ SNR range
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("snr_db", [-5., 0., 10., 30., 45., 60.])
@pytest.mark.parametrize("M", [64, 1024])
def test_snr_range(dn, snr_db, M):
    """Exact and max-log LLRs from -5 to 60 dB (complex128 beyond the normal range: +-inf with the right sign), and the fused
    pass's GMI / MI there."""
    N = 4096
    rx, t, al = _case(M, N, snr_db, CT[dn], seed=int(snr_db) + 50 + M)
    snr = 10 ** (snr_db / 10)
    for minmax in (False, True):
        _check_llr(_llr_dev(rx, al, snr, minmax), rx, al, snr, dn, minmax)
        r = ref.metrics(rx, t, al, snr=snr, minmax=minmax)
        counts, sums = _fused(rx, t, al, snr=snr, minmax=minmax)
        _check_counts(counts, r, dn, ref.nbits(M))
        np.testing.assert_allclose(sums[0], r["err_pow"], rtol=TOL[dn]["pow"])
        np.testing.assert_allclose(np.log2(M) - sums[1] / N, r["mi"], rtol=0, atol=TOL[dn]["info"], err_msg="mi")
        if dn == "c64" or minmax:
            np.testing.assert_allclose(1 - sums[2:] / N, r["gmi_per_bit"], rtol=0, atol=TOL[dn]["info"], err_msg="gmi")
        else:               # complex128 exact: an infinite LLR of the right sign adds 0 where the restatement adds ~exp(-|L|)
            got = 1 - sums[2:] / N
            assert np.all(np.isfinite(got))
            np.testing.assert_allclose(got, r["gmi_per_bit"], rtol=0, atol=TOL[dn]["info"], err_msg="gmi")


# ------------------------------------------------------------------------------------------------ orders through SignalQAM
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", [8, 4, 16, 32, 64, 128, 256, 512, 1024])
def test_orders_through_signalqam_and_cal_metrics_dev(dn, M):
    N = 20000
    snr_db = {8: 12., 4: 9., 16: 15., 32: 18., 64: 21., 128: 24., 256: 27., 512: 30., 1024: 33.}[M]
    rng = np.random.default_rng(M)
    al = _alphabet(M, CT[dn])
    t = rng.integers(0, M, (2, N)).astype(np.int32)
    rx = np.stack([_noisy(al, t[m], snr_db, rng) for m in range(2)]).astype(CT[dn])
    sig = SignalQAM(rx, M, symbols=al[t], coded_symbols=al)
    want = [ref.metrics(rx[m], t[m], al) for m in range(2)]
    for m, w in enumerate(want):
        assert abs(round(sig.cal_ser(synced=True)[m] * N) - w["errors"]) <= w["near_ties"]
        assert abs(round(sig.cal_ber(synced=True)[m] * N * ref.nbits(M)) - w["bit_errors"]) <= ref.nbits(M) * w["near_ties"]
    snr, s0, n0 = sig.est_snr(synced=True, verbose=True)
    for m, w in enumerate(want):
        _check_snr(np.array([snr[m], s0[m], n0[m]]), [w["snr"], w["s0"], w["n0"]], dn)
    np.testing.assert_allclose(sig.cal_evm(synced=True), [w["evm"] for w in want], rtol=TOL[dn]["pow"])
    gmi, per_bit = sig.cal_gmi(synced=True)
    np.testing.assert_allclose(per_bit, [w["gmi_per_bit"] for w in want], rtol=0, atol=TOL[dn]["info"])
    np.testing.assert_allclose(sig.cal_mi(synced=True), [w["mi"] for w in want], rtol=0, atol=TOL[dn]["info"])
    res = ber_functions.cal_metrics_dev(DeviceArray.from_host(rx), DeviceArray.from_host(t), DeviceArray.from_host(al), trim=0)
    for m, w in enumerate(want):
        assert (res[m]["tx_mode"], res[m]["rotation"], res[m]["lag"]) == (m, 0, 0)
        _check_counts(np.array([res[m]["errors"], res[m]["bit_errors"], res[m]["compared"]]), w, dn, ref.nbits(M))
        np.testing.assert_allclose(res[m]["gmi_per_bit"], w["gmi_per_bit"], rtol=0, atol=TOL[dn]["info"])
        np.testing.assert_allclose(res[m]["mi"], w["mi"], rtol=0, atol=TOL[dn]["info"])


# ------------------------------------------------------------------------------------------------ 8 / 512 / 1024-QAM: the reference
def _orders_rx(fx, M, j):
    base = np.round(fx["M%d_c128_coded" % M][fx["M%d_s%d_tx_label" % (M, j)]] * float(fx["rx_scale"]))
    q = fx["M%d_s%d_rxd" % (M, j)] + np.stack([base.real, base.imag], axis=-1)
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(fx["rx_scale"])


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("M", [8, 512, 1024])
def test_orders_match_the_reference(golden, M, j, dn):
    """SignalQAM's metric methods and both demappers against the reference at the orders metrics.npz lacks."""
    from test_gpu_metrics import GABS, RTOL, _close_where_finite, _normal_sums
    fx = golden["metrics_orders"]
    pre = "M%d_s%d_%s_" % (M, j, dn)
    coded = fx["M%d_%s_coded" % (M, dn)]
    rx = _orders_rx(fx, M, j)
    sig = SignalQAM(rx.astype(CT[dn]), M, symbols=coded[fx["M%d_s%d_tx_label" % (M, j)]], coded_symbols=coded)
    np.testing.assert_array_equal(sig.cal_ser(), fx[pre + "ser"])
    np.testing.assert_array_equal(sig.cal_ber(), fx[pre + "ber"])
    snr, s0, n0 = sig.est_snr(verbose=True)
    for name, v in (("snr", snr), ("s0", s0), ("n0", n0)):
        np.testing.assert_allclose(v, fx[pre + name], rtol=RTOL[dn], err_msg=name)
    np.testing.assert_allclose(sig.cal_evm(), fx[pre + "evm"], rtol=RTOL[dn])
    np.testing.assert_allclose(sig.cal_evm(blind=True), fx[pre + "evm_blind"], rtol=RTOL[dn])
    for suf, minmax in (("", False), ("_minmax", True)):
        gmi, per_bit = sig.cal_gmi(llr_minmax=minmax)
        _close_where_finite(gmi, fx[pre + "gmi" + suf], GABS[dn], pre + "gmi" + suf)
        _close_where_finite(per_bit, fx[pre + "gmi_per_bit" + suf], GABS[dn], pre + "gmi_per_bit" + suf)
    _close_where_finite(sig.cal_mi(), fx[pre + "mi"], GABS[dn], pre + "mi")
    if j == 0:
        n = int(fx["M%d_mi_slow_n" % M])
        r_, tx = np.asarray(sig), sig.symbols
        got = [hip_dsp.cal_mi_mc(np.ascontiguousarray(r_[m, :n] - tx[m, :n]), coded, 1 / fx[pre + "snr"][m]) for m in range(2)]
        _close_where_finite(got, fx[pre + "mi_slow"], GABS[dn], pre + "mi_slow")
    nllr, nb = int(fx["nllr"]), int(np.log2(M))
    r0 = np.ascontiguousarray(rx[0, :nllr].astype(CT[dn]))
    bitmap, s = fx["M%d_%s_bitmap_sig" % (M, dn)], fx[pre + "snr"][0]
    tol = dict(rtol=1e-5, atol=1e-4) if dn == "c64" else dict(rtol=1e-9, atol=1e-8)
    for suf, fn in (("llr", hip_dsp.soft_l_value_demapper), ("llr_minmax", hip_dsp.soft_l_value_demapper_minmax)):
        got, want = fn(r0, nb, s, bitmap), fx[pre + suf]
        fin = np.isfinite(want)
        assert np.all(np.isfinite(got[fin])), suf
        cmp = fin & (_normal_sums(r0, coded, s, nb) if suf == "llr" else True)
        np.testing.assert_allclose(got[cmp], want[cmp], err_msg=suf, **tol)


# ------------------------------------------------------------------------------------------------ device-row paths
def _receiver_case(nch=2):
    from qampy_amd.pipeline import ChannelBank, ResidentReceiver
    M = 16
    sigs = [synth.make_capture(M, 2 ** 13, nmodes=2, snr_db=22, theta=0.5 + 0.1 * c, dgd=20e-12, linewidth=10e3, seed=90 + c, dtype=np.complex64)
            for c in range(nch)]
    kw = dict(methods=("mcma", "sbd"), Niter=(2, 2), Mtestangles=32, Nbps=10)
    L = sigs[0].shape[1]
    bank = ChannelBank(nch, 2, L, 2, M, 15, (2e-3, 5e-4), alphabet=sigs[0].coded_symbols, **kw)
    for c, sg in enumerate(sigs):
        bank.load(c, sg)
    bank.run()
    rxs = []
    for sg in sigs:
        rx = ResidentReceiver(2, L, 2, M, 15, (2e-3, 5e-4), alphabet=sg.coded_symbols, **kw)
        rx.load(sg)
        rx.run()
        rxs.append(rx)
    return sigs, bank, rxs


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_resident_receiver_metrics_minmax_and_given_snr():
    """ResidentReceiver.metrics with max-log LLRs and with a given SNR (then s0 = n0 = NaN) against the restatement on the
    fetched rows; ChannelBank.metrics(ch) equals a single receiver's .metrics bit for bit on the same capture."""
    sigs, bank, rxs = _receiver_case()
    trim = 200
    for c, (sg, rx) in enumerate(zip(sigs, rxs)):
        tx = np.asarray(sg.symbols)
        al = np.asarray(sg.coded_symbols, np.complex64)
        labels = np.argmin(np.abs(tx[..., None] - al), axis=-1)
        out = rx.fetch()["out"]
        for kw in (dict(llr_minmax=True), dict(snr_db=17.5), dict(snr_db=17.5, llr_minmax=True)):
            met = rx.metrics(tx, trim=trim, **kw)
            _same_rows = bank.metrics(c, tx, trim=trim, **kw)
            for r in range(2):
                _same(met[r], _same_rows[r])
                m = met[r]
                given = kw.get("snr_db")
                w = ref.metrics(out[r], labels[m["tx_mode"]], al, m["rotation"], m["lag"], trim,
                                snr=None if given is None else 10 ** (given / 10), minmax=kw.get("llr_minmax", False))
                if given is not None:
                    assert np.isnan(m["s0"]) and np.isnan(m["n0"]) and m["snr"] == 10 ** (given / 10)
                else:
                    _check_snr(np.array([m["snr"], m["s0"], m["n0"]]), [w["snr"], w["s0"], w["n0"]], "c64")
                _check_counts(np.array([m["errors"], m["bit_errors"], m["compared"]]), w, "c64", 4)
                np.testing.assert_allclose(m["gmi_per_bit"], w["gmi_per_bit"], rtol=0, atol=1e-5)
                np.testing.assert_allclose(m["mi"], w["mi"], rtol=0, atol=1e-5)
                np.testing.assert_allclose(m["evm"], w["evm"], rtol=1e-6)
        _same_rows = bank.metrics(c, tx, trim=trim)
        for r, m in enumerate(rx.metrics(tx, trim=trim)):
            _same(m, _same_rows[r])


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("dn", CT)
def test_repeat_calls_are_bit_identical(dn):
    """Every entry point twice, at multi-trip sizes: bit-identical."""
    ct = CT[dn]
    for M in (64, 1024):
        N = 3 * TRIP + 5 if M == 64 else TRIP + 5
        rx, t, al = _case(M, N, 20., ct, seed=M, bad_frac=0.01)
        tx = np.ascontiguousarray(al[np.clip(t, 0, M - 1)])
        calls = [lambda: _fused(rx, t, al, 1, 3, 2, snr=50.), lambda: _fused(rx, t, al, 1, 3, 2, snr=50., minmax=True),
                 lambda: _snr_dev(rx, t, al, 2, -3, 5), lambda: _llr_dev(rx[:TRIP + 3], al, 50., False),
                 lambda: _llr_dev(rx[:TRIP + 3], al, 50., True), lambda: hip_dsp.estimate_snr(rx, tx, al),
                 lambda: hip_dsp.cal_mi_mc_fast(rx, tx, al, 0.02), lambda: hip_dsp.cal_mi_mc(rx[:300] - tx[:300], al, 0.02)]
        for k, f in enumerate(calls):
            a, b = f(), f()
            a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
            for u, v in zip(a, b):
                assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True), (M, k)


# ------------------------------------------------------------------------------------------------ bad input
@pytest.mark.parametrize("dn", CT)
def test_bad_arguments_raise_before_launching(dn):
    """M > 1024, nbits != log2 M, 2 trim >= N and an alignment without overlap: ValueError, and the outputs are untouched."""
    ct = CT[dn]
    rx, t, al = _case(16, 1000, 20., ct, seed=1)
    big = np.ascontiguousarray(np.resize(_alphabet(1024, ct), 2048) * 1.001 ** np.arange(2048))
    E, T = DeviceArray.from_host(rx), DeviceArray.from_host(t)

    def fused(alpha, rot=0, lag=0, trim=0):
        A = DeviceArray.from_host(alpha)
        counts, sums = np.full(3, -7, np.int64), np.full(2 + 11, -7.)
        with pytest.raises(ValueError):
            _lib.call("qh_metrics_%s_dev" % dn, E.ptr, rx.size, T.ptr, t.size, A.ptr, alpha.size, rot, lag, trim, 10., 0,
                      _lib.ptr(counts), _lib.ptr(sums))
        assert np.all(counts == -7) and np.all(sums == -7.)

    def snr_dev(alpha, lag=0, trim=0):
        A = DeviceArray.from_host(alpha)
        res = np.full(3, -7.)
        with pytest.raises(ValueError):
            _lib.call("qh_estimate_snr_%s_dev" % dn, E.ptr, rx.size, T.ptr, t.size, A.ptr, alpha.size, 0, lag, trim, _lib.ptr(res))
        assert np.all(res == -7.)

    def llr(alpha, nbits):
        A, L = DeviceArray.from_host(alpha), DeviceArray.from_host(np.full((rx.size, 11), -7.))
        with pytest.raises(ValueError):
            _lib.call("qh_soft_l_value_demapper_%s_dev" % dn, E.ptr, rx.size, nbits, 10., A.ptr, alpha.size, 0, L.ptr)
        assert np.all(L.to_host() == -7.)
        Lh = np.full((rx.size, 11), -7.)
        with pytest.raises(ValueError):
            _lib.call("qh_soft_l_value_demapper_%s" % dn, _lib.ptr(rx), rx.size, nbits, 10., _lib.ptr(alpha), alpha.size, _lib.ptr(Lh))
        assert np.all(Lh == -7.)

    fused(big)                                           # M > 1024
    snr_dev(big)
    llr(big, 11)
    llr(al, 3)                                           # nbits != log2 M
    llr(al, 5)
    fused(al, trim=500)                                  # 2 trim >= N
    snr_dev(al, trim=500)
    fused(al, lag=rx.size + 10)                          # no overlap
    fused(al, lag=-t.size - 1)
    snr_dev(al, lag=rx.size + 10)
    mi = np.full(1, -7.)
    with pytest.raises(ValueError):
        _lib.call("qh_cal_mi_mc_%s" % dn, _lib.ptr(rx), 10, _lib.ptr(big), big.size, 0.1, _lib.ptr(mi))
    with pytest.raises(ValueError):
        _lib.call("qh_cal_mi_mc_fast_%s" % dn, _lib.ptr(rx), _lib.ptr(rx), 10, _lib.ptr(big), big.size, 0.1, _lib.ptr(mi))
    res = np.full(3, -7.)
    with pytest.raises(ValueError):
        _lib.call("qh_estimate_snr_%s" % dn, _lib.ptr(rx), rx.size, _lib.ptr(rx), rx.size, _lib.ptr(big), big.size, _lib.ptr(res))
    assert mi[0] == -7. and np.all(res == -7.)
