"""Chromatic-dispersion filter on the GPU (csrc/cd.hip): the kernel against the float64 restatement (tests/cd_ref.py), the drop-ins against
the reference's outputs (tests/golden/cd.npz), and compensation in front of the resident receiver.

Bars are max-abs errors relative to the signal rms: 1e-5 for complex64 and 1e-11 for complex128 where the algorithms are the same;
where the block filter stands in for one transform of the whole row, the truncation bars of tests/test_cd_host.py."""
import ctypes as C
import os

import numpy as np
import pytest

import cd_ref
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import filter as cdf
from table_cache_check import assert_sequence_matches_fresh_calls

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cd.npz")
KM = {"100": 100e3, "1000": 1000e3, "m1000": -1000e3}
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
FS, D, WL = 40e9, 17e-6, 1550e-9


def rel_max(got, ref):
    return np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))


def rel_rms(got, ref):
    return np.sqrt(np.mean(np.abs(got - ref) ** 2) / np.mean(np.abs(ref) ** 2))


def run_dev(x, N, coeffs, mode):
    n = N // 2
    Lout = x.shape[1] if mode == "circular" else (x.shape[1] // n) * n
    if Lout == 0:
        return np.empty((x.shape[0], 0), x.dtype)
    E = DeviceArray.from_host(x)
    out = DeviceArray((x.shape[0], Lout), x.dtype)
    cdf.cd_filter_coeffs_dev(E, out, N, coeffs, mode)
    return out.to_host()


def lengths(N):
    return [N, N // 2 + 3, 3 * N + N // 4 + 5, 2 * N + 1, 5 * N // 2]     # L = N, L < N, L not a multiple of n, odd L, a multiple of n


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mode", ["circular", "linear"])
def test_kernel_matches_restatement(N, dtype, mode):
    coeffs = (-(N / 16) / (4 * np.pi), 0.3, 0.7)              # spread N / 16 samples; a linear and a constant phase too
    for i, L in enumerate(lengths(N)):
        nm = 1 + i % 4
        x = cd_ref.bandlimited(nm, L, 10 * N + i).astype(dtype)
        want = cd_ref.cd_filter(x, N, *coeffs, mode=mode)
        got = run_dev(x, N, coeffs, mode)
        assert got.shape == want.shape and got.dtype == dtype
        if want.size:
            assert rel_max(got, want) <= BAR[dtype], (L, nm, rel_max(got, want))


def gold_x(g, n):
    q = g["x%d" % n]
    return (q[..., 0] + 1j * q[..., 1]) / g["scale"]


def test_cdcomp_and_add_dispersion_match_fixture():
    from qampy_amd.core.equalisation import CDcomp
    from qampy_amd.core.impairments import add_dispersion
    g = dict(np.load(GOLD))
    for k in sorted(g):
        if not (k.startswith("cdcomp_") or k.startswith("adddisp_")):
            continue
        fn, n, km, dt = k.split("_")
        n, ct = int(n), {"c64": np.complex64, "c128": np.complex128}[dt]
        x = gold_x(g, n).astype(ct)
        if fn == "cdcomp":
            got, H = CDcomp(x, FS, 0, KM[km], D, WL)
            assert H.shape == (n,)
        else:
            got = add_dispersion(x, FS, D, KM[km], WL)
        assert got.dtype == ct and got.shape == (n,)
        if n in (4096,):                                       # one exact transform
            assert rel_max(got, g[k]) <= BAR[ct], (k, rel_max(got, g[k]))
        else:                                                  # blocks at the default size
            assert rel_rms(got, g[k]) < 6e-5, (k, rel_rms(got, g[k]))
            assert rel_max(got, g[k]) < 3e-4, (k, rel_max(got, g[k]))


def test_cdcomp_blocks_compensate():
    from qampy_amd.core.equalisation import CDcomp
    g = dict(np.load(GOLD))
    blk = (g["blk_in"][..., 0] + 1j * g["blk_in"][..., 1]) / g["scale"]
    want = cd_ref.cdcomp_blocks(blk, FS, 1024, -1000e3, D, WL)
    got, H = CDcomp(blk, FS, 1024, -1000e3, D, WL)
    assert H.shape == (1024,) and got.shape == want.shape
    assert rel_max(got, want) <= 1e-11
    assert rel_rms(got, gold_x(g, 4096)) < 0.2 < rel_rms(g["blk_ref"], gold_x(g, 4096))


def test_signal_object_add_dispersion():
    from qampy_amd import impairments
    sig = synth.make_capture(16, 2 ** 12, nmodes=2, seed=3, dtype=np.complex128)
    out = impairments.add_dispersion(sig, D, 100e3)
    assert type(out) is type(sig) and out.fs == sig.fs
    want = cd_ref.add_dispersion(np.asarray(sig), sig.fs, D, 100e3, WL)
    assert rel_max(np.asarray(out), want) <= 1e-11


@pytest.mark.parametrize("km", [100, 500, 1000, 2000])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_round_trip(km, dtype):
    x = cd_ref.bandlimited(2, 2 ** 15, km).astype(dtype)
    E = DeviceArray.from_host(x)
    a, b = DeviceArray(x.shape, dtype), DeviceArray(x.shape, dtype)
    cdf.cd_filter_dev(E, a, FS, D, km * 1e3, WL)
    cdf.cd_filter_dev(a, b, FS, D, -km * 1e3, WL)
    back = b.to_host()
    bar = {100: 7e-5, 500: 1e-4, 1000: 5e-5, 2000: 3e-5}[km]
    assert rel_rms(back, x) < bar, rel_rms(back, x)
    # and the forward filter alone against the exact circular one
    assert rel_rms(a.to_host(), cd_ref.add_dispersion(x, FS, D, km * 1e3, WL)) < bar / 2 + 1e-6


def test_repeat_calls_bit_identical():
    x = cd_ref.bandlimited(2, 100003, 5).astype(np.complex64)
    outs = []
    for mode in ("circular", "linear", "circular", "linear"):
        outs.append(run_dev(x, 2048, cdf.cd_coeffs_exact(FS, D, 500e3, WL), mode))
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[3])
    E = DeviceArray.from_host(x)
    a, b = DeviceArray(x.shape, np.complex64), DeviceArray(x.shape, np.complex64)
    cdf.cd_filter_dev(E, a, FS, D, 1000e3, WL)
    cdf.cd_filter_dev(E, b, FS, D, 1000e3, WL)
    assert np.array_equal(a.to_host(), b.to_host())
    # the table follows its key (N, coefficients, precision): key A, key B, A again; the other precision in between; a larger table, which
    # regrows the slot, in between - every call gives the bits it gives as the first call after qh_release_scratch
    x = cd_ref.bandlimited(2, 389, 6)
    co = (-16 / (4 * np.pi), 0.3, 0.7)
    for dt, other in ((np.complex64, np.complex128), (np.complex128, np.complex64)):
        calls = {"256": lambda: run_dev(x.astype(dt), 256, co, "circular"), "512": lambda: run_dev(x.astype(dt), 512, co, "circular"),
                 "256 other coefficients": lambda: run_dev(x.astype(dt), 256, (co[0], 0.2, 0.7), "circular"),
                 "256 other precision": lambda: run_dev(x.astype(other), 256, co, "circular"),
                 "8192": lambda: run_dev(x.astype(dt), 8192, co, "circular")}
        want = assert_sequence_matches_fresh_calls(calls, ["256", "512", "256", "256 other coefficients", "256", "256 other precision", "256",
                                                           "256 other precision", "8192", "256", "512"])
        assert not np.array_equal(want["256"], want["512"]) and not np.array_equal(want["256"], want["256 other coefficients"])
        assert rel_max(want["256"], cd_ref.cd_filter(x.astype(dt), 256, *co)) <= BAR[dt]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("L", [1, 100, 256, 257, 3 * 128 + 5])
def test_circular_edges_at_the_smallest_block(L, dtype):
    """N = 256: a row shorter than the block, whose halo wraps round it several times; the whole row; one sample more; a partial last block."""
    coeffs = (-(256 / 16) / (4 * np.pi), 0.3, 0.7)
    x = cd_ref.bandlimited(2, L, 40 + L).astype(dtype)
    want = cd_ref.cd_filter(x, 256, *coeffs)
    got = run_dev(x, 256, coeffs, "circular")
    assert got.shape == want.shape and got.dtype == dtype
    print("cd edge", L, np.dtype(dtype).name, rel_max(got, want))
    assert rel_max(got, want) <= BAR[dtype], (L, rel_max(got, want))


def test_bad_arguments_rejected_by_the_library():
    lib = _lib.load()
    x = DeviceArray((2, 4096), np.complex64)
    y = DeviceArray((2, 4096), np.complex64)
    for N in (128, 1000, 16384, 0):
        assert lib.qh_cd_filter_c64_dev(C.c_void_p(x.ptr), 2, 4096, N, 0., 0., 0., 0, C.c_void_p(y.ptr)) == _lib.QH_ERR_ARG
        assert b"power of two" in lib.qh_last_error()
    assert lib.qh_cd_filter_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1024, 0., 0., 0., 2, C.c_void_p(y.ptr)) == _lib.QH_ERR_ARG
    assert lib.qh_cd_filter_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1024, 0., 0., 0., 0, C.c_void_p(x.ptr)) == _lib.QH_ERR_ARG
    with pytest.raises(ValueError):
        cdf.cd_filter_dev(x, y, FS, D, 10000e3, WL)
    with pytest.raises(ValueError):
        cdf.cd_filter_dev(x, y, FS, D, 100e3, WL, N=3000)


def test_make_capture_dev_cd_matches_host_filter():
    base = synth.make_capture_dev(16, 2 ** 14, nmodes=2, snr_db=20, seed=11)["E"].to_host()
    disp = synth.make_capture_dev(16, 2 ** 14, nmodes=2, snr_db=20, seed=11, cd=(D, 1000e3, WL))["E"].to_host()
    # the noise fills the whole band, where the truncated response is least accurate: twice the band-limited bar
    assert rel_rms(disp, cd_ref.add_dispersion(base, 40e9, D, 1000e3, WL)) < 2e-4
    host = synth.make_capture(16, 2 ** 12, nmodes=2, snr_db=20, seed=4, dtype=np.complex128, cd=(D, 300e3, WL))
    plain = synth.make_capture(16, 2 ** 12, nmodes=2, snr_db=20, seed=4, dtype=np.complex128)
    assert rel_max(np.asarray(host), cd_ref.add_dispersion(np.asarray(plain), 40e9, D, 300e3, WL)) < 1e-11


def _receiver_ser(tier, cd_km, compensate):
    from qampy_amd.core import ber_functions as ber
    from qampy_amd.pipeline import ResidentReceiver
    nsym = 2 ** 18
    d = synth.make_capture_dev(16, nsym, nmodes=2, snr_db=17, theta=np.pi / 5.6, dgd=30e-12, seed=1000,
                               cd=None if cd_km is None else (D, cd_km * 1e3, WL))
    rx = ResidentReceiver(2, 2 * nsym, 2, 16, 21, (1e-3,), methods=("mcma",), Niter=(2,), adaptive_stepsize=(False,), TrSyms=(None,),
                          Mtestangles=32, Nbps=20, alphabet=d["alphabet_host"], tier=tier)
    rx.load(d["E"].to_host())
    if compensate:
        rx.compensate_cd(d["fs"], D, cd_km * 1e3, WL)
    rx.run()
    res = ber.cal_ser_dev(rx.out, d["idx_tx"], rx.alphabet, maxlag=256, window=4096, trim=20000)
    return max(r["ser"] for r in res)


@pytest.mark.parametrize("tier", ["a", "b"])
def test_receiver_end_to_end_1000km(tier):
    base = _receiver_ser(tier, None, False)
    assert 1e-4 < base < 1e-2, base
    comp = _receiver_ser(tier, 1000, True)
    assert abs(comp - base) <= 0.1 * base + 1e-4, (base, comp)
    if tier == "a":
        assert _receiver_ser(tier, 1000, False) > 0.1
