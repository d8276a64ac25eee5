"""The frequency-offset transform (csrc/foe.hip) at every size, at the non-square four-step splits and past one chunk of blocks, against
the float64 restatement (tests/foe_ref.py), with the helpers and the bars of tests/test_gpu_foe.py.

Above 2^13 the kernel transforms N = N1 N2 points in four steps, N1 = 2^floor(lg N / 2), and keeps the spectrum at position k1 N2 + k2 of
bin k1 + N1 k2; the peak search and the spectrum output turn positions back into bins.  At a square split (2^14, 2^16, 2^18, 2^20) each of
those formulas is unchanged when N1 and N2 change places, so a kernel with any of them exchanged computes the same there; at 128 x 256,
256 x 512 and 512 x 1024 (2^15, 2^17, 2^19) it does not.  The rows' lines stand in the bins of ``foe_ref.split_bins``, whose k1 and k2
differ: tests/test_foe_host.py shows on the CPU that an exchanged store or read-back moves every one of them but N - 1 at the three
non-square sizes and none at the square ones.  Every size 2^8 .. 2^20 is run, which reaches every instantiation the host code can choose:
the single transform at 256 .. 8192, step 1 at N1 = 128, 256, 512, 1024 and step 2 at N2 = 128 .. 1024.

A call works in chunks of ``FOE_CHUNK / (nmodes N)`` blocks (``chunk_of`` below restates the rule): the cases of ``CHUNKED`` need a second
chunk, a partial last chunk and the clamp of the chunk to one block, and each asserts that it does.

Inputs are ``qam_tone`` rows (multiples of 2^-12: complex64 and complex128 hold the same values); bins and offsets are compared exactly after
the restatement has shown a peak ratio of 1.2 or more, peak and total power to ``2 bar(dtype, N)``.

sqrt(P) against the restatement, max-abs relative to its rms, 16-QAM, measured on an MI355X (complex64, complex128):

    N = 2^11, 7 rows             1.36e-6, 5.6e-15     bar(dtype, N) = 1.00e-5, 1.00e-11
    N = 2^15, 7 rows, 2 blocks   5.50e-6, 1.6e-14     bar(dtype, N) = 1.15e-5, 1.15e-11
    N = 2^17, 7 rows             1.49e-5, 4.5e-14     bar(dtype, N) = 1.31e-5, 1.31e-11
    N = 2^18, 6 rows             1.62e-5, 3.2e-14     bar(dtype, N) = 1.38e-5, 1.38e-11
    N = 2^19, 4 rows             2.57e-5, 4.5e-14     bar(dtype, N) = 1.46e-5, 1.46e-11

The bars of 2^17 .. 2^19, which no earlier test had measured, are ``bar(dtype, N)`` where the measured error is at most half of it - complex128
at all three - and twice the measured error otherwise - complex64 at all three, in ``SPECTRUM_BAR``: the line stands about 0.4 sqrt(N) above
the rms and its rounding error grows with it, so relative to the rms complex64 leaves the inherited bar between 2^16 and 2^17.  (With 4-QAM
rows, whose line is stronger still, complex64 measured 3.5e-5, 4.9e-5 and 8.7e-5 at the three sizes; no test compares those.)  Peak and total
power, which are relative to themselves, stayed at 2.5e-7 (complex64) and 2e-15 (complex128) or below at every size."""
import functools

import numpy as np
import pytest

import foe_ref
from qampy_amd.core import hip_dsp, phaserecovery
from test_gpu_foe import DT, bar, check_exact, run_dev, tone

pytestmark = pytest.mark.gpu

FOE_CHUNK = 2 ** 22                     # csrc/foe.hip FOE_CHUNK: elements of intermediate per chunk of blocks

# (dtype, N) -> the bar of sqrt(P) relative to the rms where it was measured and not inherited (see the docstring)
SPECTRUM_BAR = {(np.complex64, 2 ** 17): 2 * 1.491e-5,          # measured 1.491e-5; bar(dtype, N) is 1.31e-5
                (np.complex64, 2 ** 18): 2 * 1.617e-5,          # measured 1.617e-5;                  1.38e-5
                (np.complex64, 2 ** 19): 2 * 2.572e-5}          # measured 2.572e-5;                  1.46e-5


def chunk_of(nmodes, N, B):
    """Blocks per chunk, as find_freq_offset_dev of csrc/foe.hip forms it: max(1, min(B, FOE_CHUNK / (nmodes N)))."""
    return max(1, min(B, FOE_CHUNK // (nmodes * N)))


@functools.lru_cache(maxsize=4)
def rows(M, L, bins, N, seed):
    """``tone`` rows shared by the two dtypes of a case; read-only."""
    x = tone(M, len(bins), L, list(bins), N, seed)
    x.setflags(write=False)
    return x


def size_bins(N):
    """The rows of a size: all of ``split_bins`` below 2^19; from there four of them, none of which an exchanged split leaves in place."""
    bins = foe_ref.split_bins(N)
    return tuple(bins if N < 2 ** 19 else bins[:2] + bins[-2:])


# ------------------------------------------------------------------------------------------------ every size
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("lg", range(8, 21))
def test_every_size_at_the_split_bins(lg, dtype):
    N = 2 ** lg
    bins = size_bins(N)
    x = rows(16 if lg <= 16 else 4, N, bins, N, 100 + lg)
    a = check_exact(x, 1, N, 1, dtype, avg=False, want_bins=bins)
    b = check_exact(x, 1, N, 1, dtype, avg=True, want_bins=bins)
    assert len(set(a)) == len(bins) and np.all(b == np.mean(a))


# ------------------------------------------------------------------------------------------------ the spectrum in bin order
def check_spectrum(x64, N, blocks, dtype, spec_bar, label):
    """Every row: the spectrum's maximum is in the restatement's bin, the returned peak is the spectrum's own value there and the returned
    total its sum to 2 bar; sqrt(P) against the restatement relative to its rms within ``spec_bar``.  Returns what the device gave."""
    _, bins_r, stats_r, P = foe_ref.find_freq_offset(x64, 1, N, blocks, False, full=True)
    assert foe_ref.peak_ratio(P).min() >= 1.2, foe_ref.peak_ratio(P)
    got = run_dev(x64.astype(dtype), 1, N, blocks, False, spectrum=True)
    fo, st, sp = got
    nm = x64.shape[0]
    assert sp.shape == P.shape and sp.dtype == np.dtype(dtype).type(0).real.dtype
    assert np.array_equal(np.argmax(sp, axis=1), bins_r), (np.argmax(sp, axis=1), bins_r)
    assert np.array_equal(st[:, 0], bins_r.astype(np.float64)), (st[:, 0], bins_r)
    assert np.array_equal(st[:, 1], sp[np.arange(nm), bins_r].astype(np.float64))
    tot = np.abs(st[:, 2] / sp.astype(np.float64).sum(axis=1) - 1).max()
    ref = np.sqrt(P)
    err = np.abs(np.sqrt(sp.astype(np.float64)) - ref).max() / np.sqrt(np.mean(ref ** 2))
    rel = np.abs(st[:, 1:] / stats_r[:, 1:] - 1).max()
    print(label, "N", N, np.dtype(dtype).name, "sqrt(P) max-abs / rms %.3e" % err, "bar %.3e" % spec_bar, "stats rel %.3e" % rel,
          "total against the spectrum's sum %.3e" % tot)
    assert tot <= 2 * bar(dtype, N), tot
    assert rel <= 2 * bar(dtype, N), rel
    assert err <= spec_bar, (err, spec_bar)
    return got


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("lg,blocks", [(11, 1), (15, 2), (17, 1), (18, 1), (19, 1)])
def test_spectrum_in_bin_order(lg, blocks, dtype):
    N = 2 ** lg
    bins = size_bins(N)
    x = rows(16, blocks * N + 3, bins, N, 200 + lg)
    _, st, _ = check_spectrum(x, N, blocks, dtype, SPECTRUM_BAR.get((dtype, N), bar(dtype, N)), "spectrum")
    assert list(st[:, 0]) == list(bins)


# ------------------------------------------------------------------------------------------------ row ends at a non-square split
@pytest.mark.parametrize("dtype", DT)
def test_short_row_at_a_non_square_split(dtype):
    """The mask n < valid runs over n = n1 N2 + n2: 20001 samples end inside row n1 = 78 of the (128, 256) view."""
    N, L = 2 ** 15, 20001
    check_exact(rows(4, L, (130, N - 3), N, L), 1, N, 1, dtype, want_bins=[130, N - 3])


@pytest.mark.parametrize("dtype", DT)
def test_long_row_at_a_non_square_split(dtype):
    """L = N + 37 with a stronger line in another bin in the last 37 samples, as test_long_rows_are_read_up_to_N builds it."""
    N, amp = 2 ** 17, 10.0
    x = tone(4, 1, N + 37, [N // 256 + 11], N, N + 2)
    x[:, N:] = amp * tone(4, 1, 37, [N // 4 + 1], N, N + 3)
    folded = x[:, :N].copy()
    folded[:, :37] = (folded[:, :37] ** 4 + x[:, N:] ** 4) ** 0.25
    wrong = np.argmax(foe_ref.power_spectrum(folded, N, 1)[0])
    assert wrong != N // 256 + 11 and abs(wrong - (N // 4 + 1)) <= N // 37
    check_exact(x, 1, N, 1, dtype, want_bins=[N // 256 + 11])


# ------------------------------------------------------------------------------------------------ several blocks at a non-square split
@pytest.mark.parametrize("dtype", DT)
def test_blocks_at_a_non_square_split(dtype):
    N = 2 ** 15
    bins = (N // 128 + 3, N - 257)
    x = rows(16, 3 * N + 100, bins, N, N + 5)
    for blocks in (1, 3, "all"):
        fo = check_exact(x, 2, N, blocks, dtype, want_bins=bins)
        assert list(fo) == [bins[0] * 2 / N / 4, -257 * 2 / N / 4]
    with pytest.raises(ValueError):
        run_dev(x.astype(dtype), 2, N, 4, False)


@pytest.mark.parametrize("dtype", DT)
def test_tone_in_block_three_only_at_a_non_square_split(dtype):
    N = 2 ** 17
    x = tone(4, 1, 4 * N + 50, [0], N, N + 7)
    x[:, 3 * N:4 * N] = 2 * tone(4, 1, N, [N // 256 + 40], N, N + 8)
    a = check_exact(x, 1, N, 1, dtype, want_bins=[0])
    b = check_exact(x, 1, N, 4, dtype, want_bins=[N // 256 + 40])
    assert a[0] != b[0]


# ------------------------------------------------------------------------------------------------ more than one chunk of blocks
CHUNKED = [  # N, nmodes, B, blocks per chunk, dtypes
    (4096, 3, 343, [341, 2], DT),
    (2 ** 16, 4, 17, [16, 1], DT),
    (2 ** 19, 3, 5, [2, 2, 1], DT),
    (2 ** 20, 5, 2, [1, 1], [np.complex64]),          # FOE_CHUNK / (nmodes N) < 1: the chunk is clamped to one block
]
CHUNK_CASES = [pytest.param(N, nm, B, tuple(parts), dt, id="%d-%d-%d-%s" % (N, nm, B, np.dtype(dt).name))
               for N, nm, B, parts, dts in CHUNKED for dt in dts]


def chunk_parts(nmodes, N, B):
    c = chunk_of(nmodes, N, B)
    assert B > c, "the case no longer needs a second chunk"
    return tuple(min(c, B - b0) for b0 in range(0, B, c))


def chunk_bins(N, nmodes):
    bins = foe_ref.split_bins(N)
    return tuple((bins[:2] + bins[-3:])[:nmodes] if len(bins) > 5 else bins[:nmodes])


@pytest.mark.parametrize("N,nmodes,B,parts,dtype", CHUNK_CASES)
def test_more_than_one_chunk(N, nmodes, B, parts, dtype):
    assert chunk_parts(nmodes, N, B) == parts
    if nmodes * N > FOE_CHUNK:
        assert FOE_CHUNK // (nmodes * N) == 0 and parts == (1,) * B
    bins = chunk_bins(N, nmodes)
    x = rows(4, B * N + 11, bins, N, N + nmodes)
    check_exact(x, 1, N, B, dtype, want_bins=bins)


@functools.lru_cache(maxsize=2)
def last_block_rows(N, nmodes, B, amp):
    """Every block has its line in bin 0 but the last, whose line, ``amp`` times as large, decides the sum over the blocks:
    amp^8 (the fourth power, squared) against B - 1 blocks."""
    bins = chunk_bins(N, nmodes)
    assert amp ** 8 >= 4 * (B - 1)
    x = tone(4, nmodes, B * N + 11, [0] * nmodes, N, N + 21)
    x[:, (B - 1) * N:B * N] = amp * tone(4, nmodes, N, list(bins), N, N + 22)
    x.setflags(write=False)
    return x, bins


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,nmodes,B,amp", [(4096, 3, 343, 3.0), (2 ** 16, 4, 17, 2.0)])
def test_line_in_the_last_partial_chunk(N, nmodes, B, amp, dtype):
    """An accumulator that starts again at a later chunk loses the total power; a chunk that ignores its first block number reads blocks
    0 .. again and never sees the line."""
    parts = chunk_parts(nmodes, N, B)
    assert len(parts) == 2 and parts[1] < parts[0]
    x, bins = last_block_rows(N, nmodes, B, amp)
    a = check_exact(x, 1, N, 1, dtype, want_bins=[0] * nmodes)
    b = check_exact(x, 1, N, B, dtype, want_bins=bins)
    assert not a.any() and np.all(b != 0)


# ------------------------------------------------------------------------------------------------ scratch across splits
def test_scratch_layout_across_splits():
    """One scratch slot holds tables, accumulator, per-block powers and intermediate at offsets that depend on the size: a call at
    512 x 1024, one at 128 x 256, the first again, then a single transform."""
    dtype = np.complex64
    got = []
    for lg, seed in ((19, 0), (15, 1), (19, 0), (13, 2)):
        N = 2 ** lg
        x = rows(16, N + 3, size_bins(N)[:2], N, 300 + lg)
        got.append(check_spectrum(x, N, 1, dtype, SPECTRUM_BAR.get((dtype, N), bar(dtype, N)), "scratch"))
    for u, v in zip(got[0], got[2]):
        assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------ host entry points
@pytest.mark.parametrize("dtype", DT)
def test_host_array_entry_points_at_a_non_square_size(dtype):
    N = 2 ** 15
    bins = (N // 128 + 33, N - 300)
    x = rows(16, 2 * N + 9, bins, N, 23)
    want, got_bins, _, P = foe_ref.find_freq_offset(x, 2, N, 2, False, full=True)
    assert list(got_bins) == list(bins) and foe_ref.peak_ratio(P).min() >= 1.2
    assert np.array_equal(hip_dsp.find_freq_offset(x.astype(dtype), 2, N, 2, False), want)
    got = phaserecovery.find_freq_offset(x.astype(dtype), 2, False, N, method="hip", blocks=2)
    assert got.shape == (2, 1) and got.dtype == np.float64 and np.array_equal(got[:, 0], want)
    got = phaserecovery.find_freq_offset(x.astype(dtype), 2, False, N - 100, method="hip", blocks=2)            # rounded up to N
    assert np.array_equal(got[:, 0], want)
    got = phaserecovery.find_freq_offset(x.astype(dtype), 2, True, N - 100, method="hip", blocks="all")
    assert np.array_equal(got[:, 0], foe_ref.find_freq_offset(x, 2, N, "all", True))
    assert np.array_equal(hip_dsp.find_freq_offset(x.astype(dtype), 2, N - 100, 1, True), foe_ref.find_freq_offset(x, 2, N, 1, True))
