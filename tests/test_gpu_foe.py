"""Blind frequency-offset estimate and removal on the GPU (csrc/foe.hip) against the float64 restatement (tests/foe_ref.py).

Inputs are square M-QAM symbols plus noise at 25 dB, rotated by exp(2 pi j f n) and rounded to multiples of 2^-12 (tests/foe_ref.py qam_tone),
so complex64 and complex128 hold the same values.  Bins and offsets are compared exactly; every such case first shows, on the restatement, that
its largest bin exceeds the second largest by a factor of 1.2 or more (the all-zero row apart, whose spectrum is zero in every bin on both
sides).  The spectrum is compared as sqrt(P), max-abs relative to the restatement's rms: 1e-5 (complex64) and 1e-11 (complex128) up to
N = 8192 - the bar of tests/test_gpu_cd.py for the same transform - times log2(N) / 13 above; peak and total power to twice that.  The
spectrum of a rotated constellation is a line on a floor: the line stands sqrt(N) above the rms while its rounding error grows with its own
size, so the comparison relative to the rms is made at 16-QAM up to the default size 2^16 and not at 2^20.

The sizes of this file are 256, 512, 1024, 4096, 8192, 2^14, 2^16 and 2^20: every four-step size among them is a square split (128^2, 256^2,
1024^2), where a kernel that exchanged N1 and N2 in its store or its read-back would compute the same.  tests/test_gpu_foe_sizes.py runs
every size 2^8 .. 2^20 with the helpers of this file, the non-square splits 2^15, 2^17 and 2^19 among them, and calls that need more than
one chunk of blocks; the bars it measured at 2^17 .. 2^19 are in its docstring."""
import ctypes as C

import numpy as np
import pytest

import foe_ref
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import hip_dsp, phaserecovery

pytestmark = pytest.mark.gpu

DT = [np.complex64, np.complex128]
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}


def bar(dtype, N):
    return BAR[dtype] * max(1.0, np.log2(N) / 13)


def run_dev(x, os, N, blocks, avg, spectrum=False):
    E = DeviceArray.from_host(x)
    fo, st = DeviceArray((x.shape[0],), np.float64), DeviceArray((x.shape[0], 3), np.float64)
    sp = DeviceArray((x.shape[0], N), x.real.dtype) if spectrum else None
    hip_dsp.find_freq_offset_dev(E, os, N, blocks, avg, fo, stats=st, spectrum=sp)
    _lib.sync()
    return fo.to_host(), st.to_host(), (sp.to_host() if spectrum else None)


def check_exact(x64, os, N, blocks, dtype, avg=False, zero=False, want_bins=None):
    """Bin, offset (and the mean over the modes) exactly as the restatement's; peak and total power to twice the spectrum's bar."""
    fo_r, bins_r, stats_r, P = foe_ref.find_freq_offset(x64, os, N, blocks, avg, full=True)
    if zero:
        assert not P.any()
    else:
        print("peak ratio", foe_ref.peak_ratio(P))
        assert foe_ref.peak_ratio(P).min() >= 1.2, foe_ref.peak_ratio(P)
    if want_bins is not None:
        assert list(bins_r) == list(want_bins)
    fo, st, _ = run_dev(x64.astype(dtype), os, N, blocks, avg)
    assert np.array_equal(st[:, 0], bins_r.astype(np.float64)), (st[:, 0], bins_r)
    assert np.array_equal(fo, fo_r), (fo, fo_r)
    if not zero:
        assert np.abs(st[:, 1:] / stats_r[:, 1:] - 1).max() <= 2 * bar(dtype, N), np.abs(st[:, 1:] / stats_r[:, 1:] - 1).max()
    else:
        assert not st.any()
    return fo


def tone(M, nm, L, bins, N, seed):
    """Rows whose fourth power has its line in the given bins of an N-point transform."""
    return foe_ref.qam_tone(M, nm, L, np.asarray(bins, dtype=np.float64) / (4.0 * N), seed)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N", [256, 8192, 16384, 65536])
def test_sizes_modes_and_mean(N, dtype):
    x = tone(16, 2, N, [5, N - 9], N, N + 1)
    for avg in (False, True):
        fo = check_exact(x, 2, N, 1, dtype, avg=avg, want_bins=[5, N - 9])
    assert fo[0] == fo[1] == np.mean([5 * 2 / N / 4, -9 * 2 / N / 4])


def test_largest_size():
    N = 2 ** 20
    check_exact(tone(4, 1, N, [N - 12345], N, 3), 1, N, 1, np.complex64, want_bins=[N - 12345])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,L", [(256, 200), (8192, 8000), (16384, 9001)])
def test_short_rows_are_zero_padded(N, L, dtype):
    check_exact(tone(4, 2, L, [7, N - 3], N, L), 1, N, 1, dtype, want_bins=[7, N - 3])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,amp", [(256, 2.0), (16384, 5.0)])
def test_long_rows_are_read_up_to_N(N, amp, dtype):
    """L = N + 37 with a stronger line in another bin in the last 37 samples: an estimator that reads them (here: folds them onto the start of
    the block) finds that bin."""
    x = tone(4, 1, N + 37, [11], N, N + 2)
    x[:, N:] = amp * tone(4, 1, 37, [N // 4 + 1], N, N + 3)
    folded = x[:, :N].copy()
    folded[:, :37] = (folded[:, :37] ** 4 + x[:, N:] ** 4) ** 0.25
    wrong = np.argmax(foe_ref.power_spectrum(folded, N, 1)[0])
    assert wrong != 11 and abs(wrong - (N // 4 + 1)) <= N // 37          # (37 samples make a line N / 37 bins wide)
    check_exact(x, 1, N, 1, dtype, want_bins=[11])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("nm", [1, 2, 3])
@pytest.mark.parametrize("N", [1024, 16384])
def test_rows_alone_and_averaged(N, nm, dtype):
    bins = [5, N - 40, 300][:nm]
    x = tone(16, nm, N, bins, N, 10 * nm + 1)
    check_exact(x, 1, N, 1, dtype, avg=False, want_bins=bins)
    check_exact(x, 1, N, 1, dtype, avg=True, want_bins=bins)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N", [256, 16384])
def test_tone_bins(N, dtype):
    x = tone(4, 4, N, [0, 5, N - 5, N // 2], N, 77)
    fo = check_exact(x, 2, N, 1, dtype, want_bins=[0, 5, N - 5, N // 2])
    assert list(fo) == [0.0, 5 * 2 / N / 4, -5 * 2 / N / 4, -2 / 8]


@pytest.mark.parametrize("dtype", DT)
def test_zero_input_gives_bin_zero(dtype):
    for N, L in ((256, 300), (16384, 16384)):
        fo = check_exact(np.zeros((2, L), np.complex128), 2, N, 1, dtype, zero=True, want_bins=[0, 0])
        assert not fo.any()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N", [256, 16384])
def test_blocks(N, dtype):
    L = 5 * N + 100
    x = tone(16, 2, L, [9, N - 21], N, N + 5)
    for blocks in (1, 2, 5, "all"):
        check_exact(x, 1, N, blocks, dtype, want_bins=[9, N - 21])
    with pytest.raises(ValueError):
        run_dev(x.astype(dtype), 1, N, 6, False)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N", [512, 16384])
def test_tone_in_block_three_only(N, dtype):
    x = tone(4, 1, 4 * N + 50, [0], N, N + 7)
    x[:, 3 * N:4 * N] = 2 * tone(4, 1, N, [40], N, N + 8)
    a = check_exact(x, 1, N, 1, dtype, want_bins=[0])
    b = check_exact(x, 1, N, 4, dtype, want_bins=[40])
    assert a[0] != b[0]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,blocks", [(256, 1), (8192, 1), (16384, 2), (65536, 1)])
def test_spectrum_output(N, blocks, dtype):
    x = tone(16, 2, blocks * N + 3, [5, N - 9], N, N + 11)
    _, _, stats_r, P = foe_ref.find_freq_offset(x, 1, N, blocks, False, full=True)
    fo, st, sp = run_dev(x.astype(dtype), 1, N, blocks, False, spectrum=True)
    assert sp.shape == P.shape and sp.dtype == np.dtype(dtype).type(0).real.dtype
    ref = np.sqrt(P)
    err = np.abs(np.sqrt(sp.astype(np.float64)) - ref).max() / np.sqrt(np.mean(ref ** 2))
    print("N", N, np.dtype(dtype).name, "sqrt(P) max-abs / rms", err, "stats rel", np.abs(st[:, 1:] / stats_r[:, 1:] - 1).max())
    assert err <= bar(dtype, N), err
    assert np.abs(st[:, 1:] / stats_r[:, 1:] - 1).max() <= 2 * bar(dtype, N)
    assert np.array_equal(st[:, 1], sp[np.arange(2), st[:, 0].astype(int)].astype(np.float64))         # the peak is the spectrum's own value


def test_repeat_calls_bit_identical():
    x = tone(16, 2, 3 * 65536 + 17, [5, 65000], 65536, 5).astype(np.complex64)
    a = run_dev(x, 2, 65536, 3, True, spectrum=True)
    b = run_dev(x, 2, 65536, 3, True, spectrum=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c = run_dev(x[:, :5000], 2, 4096, 1, False, spectrum=True)
    d = run_dev(x[:, :5000], 2, 4096, 1, False, spectrum=True)
    for u, v in zip(c, d):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("dtype", DT)
def test_host_array_entry_points(dtype):
    N = 4096
    x = tone(16, 2, 2 * N + 9, [33, N - 70], N, 21)
    want = foe_ref.find_freq_offset(x, 2, N, 2, False)
    assert np.array_equal(hip_dsp.find_freq_offset(x.astype(dtype), 2, N, 2, False), want)
    got = phaserecovery.find_freq_offset(x.astype(dtype), 2, False, N, method="hip", blocks=2)
    assert got.shape == (2, 1) and got.dtype == np.float64 and np.array_equal(got[:, 0], want)
    got = phaserecovery.find_freq_offset(x.astype(dtype), 2, True, N - 100, method="hip", blocks="all")         # rounded up to N
    assert np.array_equal(got[:, 0], foe_ref.find_freq_offset(x, 2, N, "all", True))
    # one block: what the host path (the reference's code) finds
    assert np.array_equal(phaserecovery.find_freq_offset(x.astype(dtype), 2, False, N, method="hip"),
                          phaserecovery.find_freq_offset(x.astype(dtype), 2, False, N))


def exact_turns(fo, L, os):
    """(len(fo), L) float64: (n + 1) fo / os modulo one turn, n = 0 .. L - 1, from the offsets' exact ratios in whole numbers."""
    rows = []
    for f in fo:
        num, den = float(f).as_integer_ratio()
        den *= os
        rows.append([((n * num) % den) / den for n in range(1, L + 1)])
    return np.array(rows)


@pytest.mark.parametrize("dtype", DT)
def test_removal_with_a_device_offset(dtype):
    L = 100003
    x = tone(16, 3, L, [5, 100, 7], 4096, 31).astype(dtype)
    fo = np.array([0.0123, -0.25, 1 / 3])
    want = hip_dsp.comp_freq_offset(x, fo, 2)
    E, dfo, out = DeviceArray.from_host(x), DeviceArray.from_host(fo), DeviceArray(x.shape, dtype)
    hip_dsp.comp_freq_offset_dev(E, dfo, 2, out)
    _lib.sync()
    assert np.array_equal(out.to_host(), want)
    hip_dsp.comp_freq_offset_dev(E, dfo, 2, E)
    _lib.sync()
    assert np.array_equal(E.to_host(), want)
    # Against the exact rotation.  The turns (n + 1) fo / os reach 33 334 here, where a double is spaced 7.3e-12: the kernel's product and
    # quotient are each rounded once (half a spacing each, before the reduction modulo one turn), so its phase may be off by
    # 2 pi spacing(L max|fo| / os ... L max|fo|) <= 2 pi spacing(L max|fo|), times the largest sample; the rest (sine, cosine, the complex
    # product, the cast) is the bar of the precision.  The reference's turns are reduced modulo one in whole-number arithmetic, so they are exact.
    ref = x.astype(np.complex128) * np.exp(-2j * np.pi * exact_turns(fo, L, 2))
    tol = BAR[dtype] * np.sqrt(np.mean(np.abs(x) ** 2)) + 2 * np.pi * np.spacing(L * np.abs(fo).max()) * np.abs(x).max()
    err = np.abs(want - ref).max()
    print(np.dtype(dtype).name, "removal max-abs error", err, "bound", tol)
    assert err <= tol, (err, tol)


def test_bad_arguments_rejected_by_the_library():
    lib = _lib.load()
    x, fo = DeviceArray((2, 4096), np.complex64, zero=True), DeviceArray((2,), np.float64)
    for N in (128, 1000, 2 ** 21, 0, -256):
        assert lib.qh_find_freq_offset_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1, N, 1, 0, C.c_void_p(fo.ptr), None, None) == _lib.QH_ERR_ARG
        assert b"power of two" in lib.qh_last_error()
    for blocks in (0, 17, -1):
        assert lib.qh_find_freq_offset_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1, 256, blocks, 0, C.c_void_p(fo.ptr), None, None) == _lib.QH_ERR_ARG
    assert lib.qh_find_freq_offset_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1, 256, 16, 0, None, None, None) == _lib.QH_ERR_ARG
    assert lib.qh_find_freq_offset_c64_dev(C.c_void_p(x.ptr), 2, 4096, 1, 256, 16, 0, C.c_void_p(fo.ptr), None, None) == _lib.QH_OK
    _lib.sync()
    assert not fo.to_host().any()


# ------------------------------------------------------------------------------------------------ resident chain
NSYM, FFT = 2 ** 15, 2 ** 14


@pytest.fixture(scope="module")
def chain():
    """16-QAM, 2 modes, 2^15 symbols at 2 samples per symbol (generator and recipe of the receiver test of tests/test_gpu_cd.py), unrotated."""
    d = synth.make_capture_dev(16, NSYM, nmodes=2, snr_db=17, theta=np.pi / 5.6, dgd=30e-12, seed=1000)
    return dict(E=d["E"].to_host(), idx_tx=d["idx_tx"], alphabet=d["alphabet_host"])


def receiver(chain):
    from qampy_amd.pipeline import ResidentReceiver
    return ResidentReceiver(2, 2 * NSYM, 2, 16, 21, (1e-3,), methods=("mcma",), Niter=(2,), adaptive_stepsize=(False,), TrSyms=(None,),
                            Mtestangles=32, Nbps=20, alphabet=chain["alphabet"])


def symbol_errors(rx, chain):
    from qampy_amd.core import ber_functions as ber
    rx.run()
    res = ber.cal_ser_dev(rx.out, chain["idx_tx"], rx.alphabet, maxlag=256, window=4096, trim=4000)
    return [r["ser"] for r in res], [r["errors"] for r in res]


def rotate(E, f, os=2):
    return (E.astype(np.complex128) * np.exp(2j * np.pi * f * np.arange(1, E.shape[1] + 1) / os)).astype(np.complex64)


def test_receiver_takes_the_offset_out(chain):
    f = 1500 * 2 / FFT / 4                              # bin 1500 of the estimator's grid: 0.0458 of the symbol rate
    rx = receiver(chain)
    rx.load(chain["E"])
    base_ser, base_err = symbol_errors(rx, chain)
    assert max(base_ser) < 2e-2, base_ser
    rx.load(rotate(chain["E"], f))
    rx.compensate_foe(fft_size=FFT)
    fo, stats = rx.foe
    assert fo.shape == (2,) and stats.shape == (2, 3)
    assert np.array_equal(fo, [f, f]) and np.array_equal(stats[:, 0], [1500., 1500.]), (fo, stats)
    back = rx.E.to_host()
    err = np.abs(back - chain["E"]).max() / np.sqrt(np.mean(np.abs(chain["E"]) ** 2))
    print("corrected capture max-abs / rms", err, "peak over mean", stats[:, 1] / (stats[:, 2] / FFT))
    assert err <= bar(np.complex64, FFT), err
    ser, nerr = symbol_errors(rx, chain)
    print("symbol errors unrotated", base_err, "corrected", nerr)
    assert all(abs(a - b) <= 3 for a, b in zip(nerr, base_err)), (nerr, base_err)
    rx.load(rotate(chain["E"], f))
    ser_raw, _ = symbol_errors(rx, chain)
    assert min(ser_raw) > 0.1, ser_raw


def test_receiver_off_grid_offset_within_half_a_bin(chain):
    f = 0.0301234
    rx = receiver(chain)
    rx.load(rotate(chain["E"], f))
    rx.compensate_foe(fft_size=FFT, average_over_modes=False)
    fo, _ = rx.foe
    assert np.abs(fo - f).max() <= 2 / (8 * FFT), fo - f
