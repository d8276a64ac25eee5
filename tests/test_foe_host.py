"""CPU checks of the frequency-offset restatement (tests/foe_ref.py) against the reference's outputs (tests/golden/foe.npz), of the argument
checks of the Python layer, which run before the library is touched, and of the new entry points' place in the C ABI."""
import os
import re

import numpy as np
import pytest

import foe_ref
from conftest import ROOT
from qampy_amd import _lib, phaserec
from qampy_amd.core import hip_dsp, phaserecovery

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foe.npz")
NEW = ["qh_find_freq_offset_c64", "qh_find_freq_offset_c128", "qh_find_freq_offset_c64_dev", "qh_find_freq_offset_c128_dev",
       "qh_comp_freq_offset_c64_dev", "qh_comp_freq_offset_c128_dev"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def cases(g):
    return sorted(k[2:] for k in g if k.startswith("x_"))


def x_of(g, c):
    q = g["x_" + c]
    return (q[..., 0] + 1j * q[..., 1]) / g["scale"]


def test_fixture_covers_the_shapes(gold):
    cs = [tuple(int(v) for v in c.split("_")) for c in cases(gold)]
    assert {c[0] for c in cs} == {4, 16, 64} and {c[1] for c in cs} == {1, 2} and {c[2] for c in cs} == {256, 4096}
    for M in (4, 16, 64):
        for osf in (1, 2):
            for N in (256, 4096):
                Ls = sorted(c[3] for c in cs if c[:3] == (M, osf, N))
                assert len(Ls) == 3 and Ls[0] < N == Ls[1] < Ls[2]


def test_restatement_equals_reference_offsets(gold):
    g = gold
    for c in cases(g):
        M, osf, N, L = (int(v) for v in c.split("_"))
        x = x_of(g, c)
        assert x.shape[1] == L
        fo = foe_ref.find_freq_offset(x, osf, N, 1, False)
        assert np.array_equal(fo.reshape(-1, 1), g["fo_" + c]), c
        assert np.array_equal(foe_ref.find_freq_offset(x, osf, N, 1, True).reshape(-1, 1), g["foavg_" + c]), c
        if M == 4:                                   # (a strong line: the estimate is the rotation that went in on the grid, in units of the symbol rate)
            assert np.array_equal(fo, g["f_" + c] * osf), c


def test_restatement_equals_reference_removal(gold):
    g = gold
    n = 0
    for c in cases(g):
        if "comp_" + c not in g:
            continue
        osf = int(c.split("_")[1])
        got = foe_ref.comp_freq_offset(x_of(g, c), g["fo_" + c], osf)
        assert np.abs(got - g["comp_" + c]).max() <= 1e-13, c
        n += 1
    assert n == 18


def test_host_path_is_the_reference_bit_for_bit(gold):
    """method="pyt" (the default) is the host code as it was; a size that is no power of two is rounded up as the reference rounds it."""
    g = gold
    for c in cases(g):
        M, osf, N, L = (int(v) for v in c.split("_"))
        x = x_of(g, c)
        assert np.array_equal(phaserecovery.find_freq_offset(x, osf, average_over_modes=False, fft_size=N), g["fo_" + c])
        assert np.array_equal(phaserecovery.find_freq_offset(x, osf, True, N, method="pyt", blocks=1), g["foavg_" + c])
    x = x_of(g, "16_1_4096_2500")
    assert np.array_equal(phaserecovery.find_freq_offset(x, 1, False, 3000), g["odd_16_1_3000_2500"])
    assert np.array_equal(foe_ref.find_freq_offset(x, 1, 4096, 1, False).reshape(-1, 1), g["odd_16_1_3000_2500"])
    assert hip_dsp.foe_plan(2500, 3000, 1) == (4096, 1)


def test_restatement_blocks_padding_and_first_maximum():
    N = 256
    t = np.arange(3 * N + 11)
    x = np.exp(2j * np.pi * (3 / (4 * N)) * t)[None, :]
    assert foe_ref.find_freq_offset(x, 1, N, 1)[0] == 3 / (4 * N)
    assert foe_ref.n_blocks(x.shape[1], N, "all") == 3 and foe_ref.n_blocks(100, N, "all") == 1
    P1, P3 = foe_ref.power_spectrum(x, N, 1), foe_ref.power_spectrum(x, N, "all")
    assert np.allclose(P3, 3 * P1, rtol=1e-9, atol=1e-6)
    short = foe_ref.power_spectrum(x[:, :100], N, 1)                      # zero-padded
    ref = np.abs(np.fft.fft(x[0, :100] ** 4, N)) ** 2
    assert np.allclose(short[0], ref, rtol=1e-12, atol=1e-9)
    long_ = foe_ref.power_spectrum(x, N, 1)                               # truncated to the first N samples
    assert np.allclose(long_[0], np.abs(np.fft.fft(x[0] ** 4, N)) ** 2, rtol=1e-12, atol=1e-9)
    fo, bins, stats, P = foe_ref.find_freq_offset(np.zeros((2, 300), complex), 2, N, 1, False, full=True)
    assert list(bins) == [0, 0] and list(fo) == [0., 0.] and np.all(stats == 0)
    # the bin N / 2 is the negative Nyquist frequency of fftfreq: -os / 8
    ny = np.exp(2j * np.pi * (1 / 8) * np.arange(N))[None, :]
    assert foe_ref.find_freq_offset(ny, 2, N, 1)[0] == -2 / 8
    # mean over the modes
    two = np.stack([x[0, :N], np.exp(2j * np.pi * (-7 / (4 * N)) * np.arange(N))])
    assert list(foe_ref.find_freq_offset(two, 1, N, 1, False)) == [3 / (4 * N), -7 / (4 * N)]
    assert list(foe_ref.find_freq_offset(two, 1, N, 1, True)) == [-2 / (4 * N)] * 2


def test_split_helpers_follow_the_kernel_rule():
    assert [foe_ref.four_step_split(2 ** lg) for lg in (8, 13, 14, 15, 16, 17, 18, 19, 20)] == \
        [(1, 256), (1, 8192), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024)]
    for lg in range(8, 21):
        N = 2 ** lg
        N1, N2 = foe_ref.four_step_split(N)
        bins = foe_ref.split_bins(N)
        assert len(set(bins)) == len(bins) and all(0 < k < N for k in bins)
        if N1 == 1:
            assert {1, N - 1, N // 2 + 3} <= set(bins)
        else:
            assert set(bins) == {N1, N2, N1 + 1, N - 1, 2 * N1 - 1, 3 + 5 * N1, N // 2 + N1 + 2}
            assert len(bins) == (7 if N1 != N2 else 6)
    # the two permutations against the index formulas they stand for, at a small non-square split
    N1, N2 = 4, 8
    N = N1 * N2
    P = np.arange(2 * N, dtype=np.float64).reshape(2, N)
    S = np.empty_like(P)
    for k in range(N):
        S[:, (k % N1) * N2 + k // N1] = P[:, k]                     # the kernel's store
    rb = np.stack([S[:, (k % N2) * N1 + k // N2] for k in range(N)], axis=1)
    assert np.array_equal(foe_ref.swapped_readback(P, N1, N2), rb)
    by_peak_search = np.empty_like(P)
    for q in range(N):
        by_peak_search[:, (q // N1) + N2 * (q % N1)] = S[:, q]      # the peak search's bin of position q, exchanged
    assert np.array_equal(by_peak_search, rb)
    for k in range(N):
        S[:, (k % N2) * N1 + k // N2] = P[:, k]                     # the store, exchanged
    st = np.stack([S[:, (k % N1) * N2 + k // N1] for k in range(N)], axis=1)
    assert np.array_equal(foe_ref.swapped_store(P, N1, N2), st)
    assert np.array_equal(foe_ref.swapped_store(rb, N1, N2), P) and not np.array_equal(rb, P) and not np.array_equal(st, P)


@pytest.mark.parametrize("lg", range(14, 21))
def test_exchanged_split_moves_the_bins_only_at_non_square_sizes(lg):
    """The inputs of the GPU tests can fail: a spectrum stored at k1 N2 + k2 and read back with N1 and N2 exchanged (or stored exchanged and
    read back correctly) puts the lines of ``split_bins`` elsewhere at 2^15, 2^17 and 2^19 - every row but the one at N - 1 - and nowhere else at
    the square sizes, where the exchange is the identity: the sizes the suite compared values at before (2^14, 2^16, 2^20) could not tell."""
    N = 2 ** lg
    N1, N2 = foe_ref.four_step_split(N)
    bins = foe_ref.split_bins(N)
    x = foe_ref.qam_tone(4, len(bins), N, np.asarray(bins, dtype=np.float64) / (4.0 * N), lg)
    _, got, _, P = foe_ref.find_freq_offset(x, 1, N, 1, False, full=True)
    assert list(got) == bins and foe_ref.peak_ratio(P).min() >= 1.2, (got, foe_ref.peak_ratio(P))
    for form in (foe_ref.swapped_readback, foe_ref.swapped_store):
        moved = np.argmax(form(P, N1, N2), axis=1) != np.asarray(bins)
        if N1 == N2:
            assert np.array_equal(form(P, N1, N2), P) and not moved.any()
        else:
            assert list(moved) == [k != N - 1 for k in bins], (form.__name__, moved)


class _Stub:
    """A stand-in with a DeviceArray's attributes: the checks must fire before any library call."""
    def __init__(self, shape, dtype, ptr=1):
        self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), ptr


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


@pytest.mark.parametrize("fft_size", [128, 100, 2 ** 20 + 1, 2 ** 21, 0])
def test_size_outside_the_range_is_refused(no_library, fft_size):
    x = np.zeros((2, 4096), np.complex64)
    with pytest.raises(ValueError):
        phaserecovery.find_freq_offset(x, 1, True, fft_size, method="hip")
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset(x, 1, fft_size)
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset_dev(_Stub((2, 4096), np.complex64), 1, fft_size, 1, True, _Stub((2,), np.float64))


def test_blocks_that_do_not_fit_are_refused(no_library):
    x = np.zeros((2, 1000), np.complex128)
    for blocks in (4, 2 ** 20):
        with pytest.raises(ValueError):
            phaserecovery.find_freq_offset(x, 1, True, 256, method="hip", blocks=blocks)
        with pytest.raises(ValueError):
            hip_dsp.find_freq_offset_dev(_Stub((2, 1000), np.complex128), 1, 256, blocks, True, _Stub((2,), np.float64))
    for blocks in (0, -1, 1.5, "some"):
        with pytest.raises(ValueError):
            phaserecovery.find_freq_offset(x, 1, True, 256, method="hip", blocks=blocks)
    assert hip_dsp.foe_plan(1000, 256, 3) == (256, 3) and hip_dsp.foe_plan(1000, 256, "all") == (256, 3)
    assert hip_dsp.foe_plan(100, 256, "all") == (256, 1) and hip_dsp.foe_plan(100, 256, 1) == (256, 1)
    with pytest.raises(ValueError):
        hip_dsp.foe_plan(100, 256, 2)


def test_host_method_takes_one_block(no_library):
    x = np.zeros((1, 1000), np.complex128)
    for blocks in (2, "all"):
        with pytest.raises(ValueError):
            phaserecovery.find_freq_offset(x, 1, True, 256, method="pyt", blocks=blocks)
    with pytest.raises(ValueError):
        phaserecovery.find_freq_offset(x, 1, True, 256, method="fft")

    class Sig(np.ndarray):
        os = 2
    with pytest.raises(ValueError):
        phaserec.find_freq_offset(x.view(Sig), fft_size=256, method="pyt", blocks=3)
    with pytest.raises(ValueError):
        phaserec.find_freq_offset(x.view(Sig), fft_size=64, method="hip")


def test_device_wrappers_check_their_buffers(no_library):
    E = _Stub((2, 4096), np.complex64)
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset_dev(E, 1, 256, 1, True, _Stub((3,), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset_dev(E, 1, 256, 1, True, _Stub((2,), np.float64), stats=_Stub((2, 2), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset_dev(E, 1, 256, 1, True, _Stub((2,), np.float64), spectrum=_Stub((2, 256), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.find_freq_offset_dev(E, 1.5, 256, 1, True, _Stub((2,), np.float64))
    with pytest.raises(ValueError):
        hip_dsp.comp_freq_offset_dev(E, _Stub((2,), np.float64), 1, _Stub((2, 4000), np.complex64))
    with pytest.raises(ValueError):
        hip_dsp.comp_freq_offset_dev(E, _Stub((2,), np.float32), 1, E)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    declared = set(re.findall(r"\b(qh_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert _lib.SIGNATURES["qh_find_freq_offset_c64_dev"] == _lib.SIGNATURES["qh_find_freq_offset_c128"] and len(_lib.SIGNATURES["qh_find_freq_offset_c64"]) == 10
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.qh_abi_version() == 11
