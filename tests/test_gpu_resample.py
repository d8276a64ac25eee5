"""Polyphase resampler on the GPU (csrc/resample.hip): the kernel against the float64 restatement (tests/resample_ref.py), the drop-ins
against the reference's outputs (tests/golden/resample.npz), renormalisation on the device, and a raw capture into the resident receiver.

Bars are max-abs errors relative to the reference rms: 1e-5 for complex64 and 1e-11 for complex128 (those of tests/test_gpu_cd.py for "same
algorithm").  A sequential fp32 accumulation over J = ceil(taps / up) terms errs by 7e-7 (J = 36) to 2.7e-6 (J = 572) and 5.1e-6 at
J = 2001, so complex64 cases keep J <= 600."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as ref
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import resample as rs
from table_cache_check import assert_sequence_matches_fresh_calls

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
RATIOS = [(2, 1), (1, 2), (3, 1), (7, 10), (10, 7), (28, 25), (1, 1)]
TAPS = [1, 2, 255, 400, 401, 4001]
LENGTHS = [37, 1000, 1003, 4099]
_CACHE = {}


def rel_max(got, want):
    return np.abs(got - want).max() / np.sqrt(np.mean(np.abs(want) ** 2))


def taps_of(T, seed=0):
    """A low-pass-like tap set of length T that is not symmetric (a swapped tap order would show)."""
    m = np.arange(T) - (T - 1) // 2
    return np.sinc(m / 3.3) * np.exp(-(m / (0.3 * T + 2)) ** 2) * (1 + 0.1 * np.cos(0.37 * m + seed)) + (0.01 if T > 1 else 0) * (m > 0)


def case(up, down, T, n, nm, gain):
    """Input (values exact in float32) and restatement, computed once for both precisions."""
    key = (up, down, T, n, nm, gain)
    if key not in _CACHE:
        x = ref.unit_noise(nm, n, 7 * n + T + up).astype(np.complex64)
        h = taps_of(T)
        _CACHE[key] = (x, h, ref.resample(x, h, up, down, gain))
    return _CACHE[key]


def run_dev(x, h, up, down, gain, Lout=None):
    Lout = ref.n_out(x.shape[1], up, down) if Lout is None else Lout
    E = DeviceArray.from_host(x)
    out = DeviceArray((x.shape[0], Lout), x.dtype)
    rs.resample_dev(E, out, h, up, down, gain)
    return out.to_host()


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_kernel_matches_restatement(ratio, dtype):
    up, down = ratio
    ran = 0
    for it, T in enumerate(TAPS):
        for il, n in enumerate(LENGTHS):
            if T > up * n or (dtype == np.complex64 and -(-T // up) > 600):
                continue
            nm, gain = 1 + (it + il) % 3, (1.0 if (it + il) % 2 else float(up))
            x, h, want = case(up, down, T, n, nm, gain)
            got = run_dev(x.astype(dtype), h, up, down, gain)
            assert got.shape == want.shape and got.dtype == dtype
            assert rel_max(got, want) <= BAR[dtype], (T, n, nm, gain, rel_max(got, want))
            ran += 1
    assert ran >= 12


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_short_output_and_untiled_lengths(dtype):
    for up, down, T, n, cut in ((7, 10, 401, 4099, 13), (2, 1, 255, 1003, 1), (28, 25, 255, 1000, 501), (1, 2, 400, 4099, 1999)):
        x, h, want = case(up, down, T, n, 2, 1.0)
        Lout = want.shape[1] - cut
        got = run_dev(x.astype(dtype), h, up, down, 1.0, Lout)
        assert got.shape == (2, Lout) and rel_max(got, want[:, :Lout]) <= BAR[dtype]


def test_short_output_leaves_the_rest_of_out_alone():
    x, h, want = case(7, 10, 401, 4099, 2, 1.0)
    E = DeviceArray.from_host(x)
    full = DeviceArray((2 * want.shape[1],), np.complex64)
    full.set(np.full(2 * want.shape[1], 7 - 3j, np.complex64))
    Lout = want.shape[1] - 100
    view = full.row(0)                                          # (a 1-d array's "row" is a scalar view: shape it by hand)
    view.shape, view.nbytes = (2, Lout), 2 * Lout * 8
    rs.resample_dev(E, view, h, 7, 10, 1.0)
    got = full.to_host()
    assert rel_max(got[:2 * Lout].reshape(2, Lout), want[:, :Lout]) <= 1e-5
    assert np.all(got[2 * Lout:] == np.complex64(7 - 3j))


def deq(g, key):
    return (g[key][..., 0] + 1j * g[key][..., 1]) / g["scale"]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_drop_ins_match_fixture(dtype):
    from qampy_amd.core.filter import rrcos_pulseshaping
    g = dict(np.load(GOLD))
    fold, Ts, beta = float(g["fold"]), float(g["Ts"]), float(g["beta"])
    seen = 0
    for key in sorted(g):
        part = key.split("_")
        if part[0] == "rrc":
            up, down, n, taps = (int(v) for v in part[1:5])
            x = deq(g, "x_%d" % n).astype(dtype)
            got = rs.rrcos_resample(x, fold, fold * up / down, Ts=Ts, beta=beta, taps=taps, fftconv=part[5] == "fft")
            if (up, down) == (1, 1) and part[5] == "poly":
                assert np.array_equal(got, x) and got is not x   # scipy's copy at a ratio of 1
        elif part[0] == "rrcb1":
            x = deq(g, "x_1000").astype(dtype)
            got = rs.rrcos_resample(x, fold, fold * 0.7, Ts=Ts, beta=1, taps=401)
        elif part[0] == "poly":
            up, down = int(part[1]), int(part[2])
            x = deq(g, "x_1000").astype(dtype)
            got = rs.resample_poly(x, fold, fold * up / down)
            assert np.array_equal(got, rs.rrcos_resample(x, fold, fold * up / down))          # beta=None is the same call
        elif part[0] == "renorm":
            x = deq(g, "x_1000").astype(dtype)
            got = rs.rrcos_resample(x, fold, fold * 0.7, Ts=Ts, beta=beta, taps=401, renormalise=True)
        elif key == "shape_out":
            x = deq(g, "shape_in").astype(dtype)
            got = rrcos_pulseshaping(x, 56e9, Ts, beta, taps=101)
        else:
            continue
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == g[key].shape, key
        assert rel_max(got, g[key]) <= BAR[dtype], (key, rel_max(got, g[key]))
        seen += 1
    assert seen == 17
    # input that is neither precision runs as complex128; a window given as taps is resample_poly(window=...)
    x = deq(g, "x_1000")
    got = rs.resample_poly(x.astype(np.clongdouble), fold, fold * 0.7, window=g["taps_7_10_1000_401"])
    assert got.dtype == np.complex128 and rel_max(got, g["rrc_7_10_1000_401_poly"]) <= 1e-11
    two = rs.resample_poly(np.stack([x, 2 * x]), fold, fold * 2)
    assert two.shape == (2, 2000) and rel_max(two[1], 2 * g["poly_2_1_1000"]) <= 1e-11


def test_signal_object_resample():
    from qampy_amd.signals import SignalQAM

    class Sub(SignalQAM):
        pass
    g = dict(np.load(GOLD))
    sig = Sub(deq(g, "sig_in"), 16, fb=28e9, fs=28e9, symbols=g["sig_sym"])
    out = sig.resample(2 * sig.fb, beta=0.1, renormalise=True)
    assert type(out) is Sub and out.fs == 2 * sig.fb and out.fb == sig.fb and out.M == 16 and out.dtype == sig.dtype
    assert np.array_equal(out.symbols, sig.symbols) and out.symbols is not sig.symbols
    assert out.shape == (2, 4096) and rel_max(np.asarray(out), g["sig_out"]) <= 1e-11
    same = sig.resample(sig.fs * (1 + 1e-12), beta=0.1)
    assert type(same) is Sub and np.array_equal(same, sig) and not np.shares_memory(same, sig) and same.fs == sig.fs


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_renormalisation_on_the_device(dtype):
    x = (ref.unit_noise(3, 4099, 77) * np.array([[0.5], [1.0], [3.0]]) + np.array([[0.2 - 0.1j], [0], [1j]])).astype(dtype)
    h = ref.rrcos_taps(401, 7 * 80e9, 1 / 28e9, 0.1)
    got = rs.rrcos_resample(x, 80e9, 56e9, Ts=1 / 28e9, beta=0.1, taps=401, renormalise=True)
    want = ref.renormalise(ref.resample(x, h, 7, 10, 1.0), x)
    pin = np.mean(np.abs(x.astype(np.complex128)) ** 2, axis=1)
    g64 = got.astype(np.complex128)
    assert np.all(np.abs(g64.mean(axis=1)) <= 1e-6 * np.sqrt(pin))
    assert np.abs(np.mean(np.abs(g64) ** 2, axis=1) / pin - 1).max() <= 1e-5
    assert got.dtype == dtype
    for r in range(3):                                          # (rows of power 0.25 .. 10: each against its own rms)
        assert rel_max(got[r], want[r]) <= BAR[dtype], (r, rel_max(got[r], want[r]))
    # the pieces: moments against numpy, a target power instead of a second array
    E = DeviceArray.from_host(x)
    mom = rs.row_moments_dev(E).to_host()
    x128 = x.astype(np.complex128)
    assert np.allclose(mom[:, 0], x128.real.mean(axis=1), rtol=0, atol=1e-13 * 9)
    assert np.allclose(mom[:, 1], x128.imag.mean(axis=1), rtol=0, atol=1e-13 * 9)
    assert np.allclose(mom[:, 2], np.mean(np.abs(x128) ** 2, axis=1), rtol=1e-13, atol=0)
    rs.center_scale_dev(E, rs.row_moments_dev(E), power=2.0)
    y = E.to_host().astype(np.complex128)
    assert np.abs(np.mean(np.abs(y) ** 2, axis=1) - 2.0).max() <= 2e-5 and np.abs(y.mean(axis=1)).max() <= 2e-6


def test_repeat_calls_bit_identical_across_tap_sets():
    x = ref.unit_noise(2, 20011, 3).astype(np.complex64)
    h1, h2 = taps_of(401), taps_of(401, seed=1)
    a1 = run_dev(x, h1, 7, 10, 1.0)
    b1 = run_dev(x, h2, 7, 10, 1.0)
    c1 = run_dev(x, h1, 28, 25, 1.0)
    a2 = run_dev(x, h1, 7, 10, 1.0)
    b2 = run_dev(x, h2, 7, 10, 1.0)
    d1 = run_dev(x.astype(np.complex128), h1, 7, 10, 1.0)
    a3 = run_dev(x, h1, 7, 10, 1.0)
    assert np.array_equal(a1, a2) and np.array_equal(a1, a3) and np.array_equal(b1, b2)
    assert not np.array_equal(a1, b1) and c1.shape != a1.shape
    assert rel_max(a1, ref.resample(x, h1, 7, 10)) <= 1e-5 and rel_max(b2, ref.resample(x, h2, 7, 10)) <= 1e-5
    assert rel_max(d1, ref.resample(x, h1, 7, 10)) <= 1e-11
    # the table follows its key (taps, up, precision) on the smallest shapes: tap set A, B, A again; the other precision in between; a larger
    # table, which regrows the slot, in between - every call gives the bits it gives as the first call after qh_release_scratch
    x = ref.unit_noise(2, 64, 5).astype(np.complex64)
    h5, h7, h5b = taps_of(5), taps_of(7), taps_of(5, seed=1)
    for dt, other in ((np.complex64, np.complex128), (np.complex128, np.complex64)):
        calls = {"5": lambda: run_dev(x.astype(dt), h5, 2, 1, 2.0), "7": lambda: run_dev(x.astype(dt), h7, 2, 1, 2.0),
                 "5 other taps": lambda: run_dev(x.astype(dt), h5b, 2, 1, 2.0), "5 other precision": lambda: run_dev(x.astype(other), h5, 2, 1, 2.0),
                 "5 up 3": lambda: run_dev(x.astype(dt), h5, 3, 1, 3.0), "401": lambda: run_dev(x.astype(dt), h1, 2, 1, 2.0)}
        want = assert_sequence_matches_fresh_calls(calls, ["5", "7", "5", "5 other taps", "5", "5 other precision", "5", "5 other precision",
                                                           "5 up 3", "5", "401", "5", "7"])
        assert not np.array_equal(want["5"], want["7"]) and not np.array_equal(want["5"], want["5 other taps"])
        assert rel_max(want["5"], ref.resample(x, h5, 2, 1, 2.0)) <= BAR[dt] and rel_max(want["7"], ref.resample(x, h7, 2, 1, 2.0)) <= BAR[dt]


def test_bad_arguments_rejected_by_the_library():
    lib = _lib.load()
    x = DeviceArray((2, 1000), np.complex64)
    y = DeviceArray((2, 2000), np.complex64)
    h = np.ones(8192)

    def rc(up=7, down=10, ntaps=401, Lout=700, out=None, L=1000, taps=h):
        return lib.qh_resample_c64_dev(C.c_void_p(x.ptr), 2, L, C.c_void_p(taps.ctypes.data), ntaps, up, down, 1.0, Lout,
                                       C.c_void_p(y.ptr if out is None else out))
    assert rc() == _lib.QH_OK
    for bad in (dict(up=0), dict(up=65), dict(down=0), dict(down=65), dict(up=-1)):
        assert rc(**bad) == _lib.QH_ERR_ARG and b"1 to 64" in lib.qh_last_error()
    for bad in (dict(ntaps=0), dict(ntaps=8192)):
        assert rc(**bad) == _lib.QH_ERR_ARG and b"8191" in lib.qh_last_error()
    assert rc(ntaps=8191) == _lib.QH_OK and rc(up=64, down=64, Lout=1000) == _lib.QH_OK
    assert rc(out=x.ptr) == _lib.QH_ERR_ARG and b"other than E" in lib.qh_last_error()
    assert rc(Lout=701) == _lib.QH_ERR_ARG and b"Lout" in lib.qh_last_error()
    assert rc(Lout=-1) == _lib.QH_ERR_ARG
    with pytest.raises(ValueError):
        rs.resample_dev(x, y, h[:401], 7, 10)                   # y holds 2000 per row, the filter yields 700
    with pytest.raises(TypeError):
        rs.resample_dev(x, DeviceArray((2, 700), np.complex128), h[:401], 7, 10)
    _lib.sync()


def _receiver(d, nsym):
    from qampy_amd.pipeline import ResidentReceiver
    return ResidentReceiver(2, 2 * nsym, 2, 16, 21, (1e-3,), methods=("mcma",), Niter=(2,), adaptive_stepsize=(False,), TrSyms=(None,),
                            Mtestangles=32, Nbps=20, alphabet=d["alphabet_host"], tier="a")


def _ser(rx, d):
    from qampy_amd.core import ber_functions as ber
    rx.run()
    res = ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, maxlag=256, window=4096, trim=8000)
    return max(r["ser"] for r in res)


def test_receiver_takes_a_raw_capture():
    nsym = 2 ** 16
    d = synth.make_capture_dev(16, nsym, nmodes=2, snr_db=17, theta=np.pi / 5.6, dgd=30e-12, seed=1000)
    E = d["E"].to_host()
    fs = d["fs"]
    rx = _receiver(d, nsym)
    rx.load(E)
    plain = _ser(rx, d)
    raw = ref.resample(E, ref.default_window(10, 7), 10, 7, 10.0).astype(np.complex64)          # the capture at 10/7 of its rate
    assert raw.shape == (2, ref.n_out(2 * nsym, 10, 7))
    rx2 = _receiver(d, nsym)
    with pytest.raises(ValueError):
        rx2.load_resampled(raw[:, :-8], fs * 10 / 7, fs=fs)       # too short for the receiver's L
    with pytest.raises(ValueError):
        rx2.load_resampled(raw, fs * 10 / 7)                      # no rate to resample to
    rx2.load_resampled(raw, fs * 10 / 7, beta=None, fs=fs)
    back = rx2.E.to_host().astype(np.complex128)
    assert np.abs(np.mean(np.abs(back) ** 2, axis=1) - 1).max() <= 1e-5 and np.abs(back.mean(axis=1)).max() <= 1e-6
    want = ref.renormalise(ref.resample(raw, ref.default_window(7, 10), 7, 10, 7.0, nout=2 * nsym), np.ones((2, 1)))
    assert rel_max(back, want) <= 1e-5
    res = _ser(rx2, d)
    print("SER plain %.3e, through load_resampled %.3e" % (plain, res))
    assert 1e-4 < plain < 1e-2, plain
    assert res <= 1.5 * plain + 2e-4 and plain <= 1.5 * res + 2e-4, (plain, res)


def test_receiver_tier_b_rule_sees_unit_power():
    from qampy_amd.pipeline import ResidentReceiver
    nsym = 2 ** 12
    raw = ref.unit_noise(2, ref.n_out(2 * nsym, 10, 7), 9).astype(np.complex64) * 3
    kw = dict(methods=("mcma",), Niter=(1,), adaptive_stepsize=(False,), TrSyms=(None,), Mtestangles=None, tier="b")
    rx = ResidentReceiver(2, 2 * nsym, 2, 16, 21, (1e-3,), **kw)
    rx.fs = 56e9
    rx.load_resampled(raw, 80e9, beta=0.1, taps=401)
    got = rx.pit[0]["acq_chunk"]
    rx.load_resampled(raw, 80e9, beta=0.1, taps=401, next_capture=True)
    assert rx._next_loaded and np.array_equal(rx.E_next.to_host(), rx.E.to_host())
    rx3 = ResidentReceiver(2, 2 * nsym, 2, 16, 21, (1e-3,), **kw)
    rx3.load(rx.E.to_host())                                     # the same rows through load(): the rule reads their power, 1.0
    assert got == rx3.pit[0]["acq_chunk"] and got > 0
