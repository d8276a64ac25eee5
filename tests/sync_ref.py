"""Float64 restatement of the device synchronisation (csrc/sync.hip): the full cross-correlation by ``np.fft``, the peak rule of
``find_sequence_offset_complex`` and the one gather formula that stands for the roll, the roll-and-cut and the periodic extension of
``sync_and_adjust``.  Independent of the library: the CPU tests hold it against the host form, the GPU tests hold the kernels against it."""
import numpy as np

#: lengths (ntx, nrx) of the alignment grid: equal, tx longer, rx longer (one and several periods), powers of two, off by one
LENGTHS = [(100, 100), (257, 100), (100, 257), (100, 300), (4096, 4096), (1000, 3500), (3500, 1000), (128, 129)]


def shifts(n):
    """The shifts of the grid for a sequence of ``n`` samples."""
    return [0, 1, 37, n - 1, 3 * n // 4]


def xcorr(x, y):
    """``fftconvolve(x, conj(y)[::-1], "full")`` in complex128 on the power of two at or above ``max(nx + ny - 1, 256)``."""
    x, y = np.asarray(x, np.complex128), np.asarray(y, np.complex128)
    n = x.shape[-1] + y.shape[0] - 1
    P = 256
    while P < n:
        P *= 2
    return np.fft.ifft(np.fft.fft(x, P, axis=-1) * np.fft.fft(y.conj()[::-1], P), axis=-1)[..., :n]


def peak(cc):
    """The (6,) result row of the peak search: first maximum of ``|cc|``, ``max Re, max Im, max -Re, max -Im``, ``|cc|`` there."""
    k = int(np.argmax(np.abs(cc)))
    return np.array([k, cc.real.max(), cc.imag.max(), (-cc.real).max(), (-cc.imag).max(), np.abs(cc[k])], dtype=np.float64)


def decide(res, ny):
    """``(offset, turns, peak)`` from a result row: the largest directional maximum names the turn; none positive: ``(0, 0, 0.)``."""
    peaks = np.asarray(res[1:5], dtype=np.float64)
    if not peaks.max() > 0:
        return 0, 0, 0.
    turns = int(np.argmax(peaks))
    return int(res[0]) - (ny - 1), turns, float(peaks[turns])


def gather(src, offset, turns, nout):
    """``out[i] = 1j**turns * src[(i - offset) mod len(src)]``."""
    out = src[(np.arange(nout) - offset) % src.shape[0]]
    return out if turns % 4 == 0 and not np.iscomplexobj(src) else out * 1.j ** (turns % 4)


def sync_and_adjust(tx, rx, adjust="tx"):
    """``((tx, rx), peak)``: the row named by ``adjust`` gathered onto the other one."""
    fixed, moved = (rx, tx) if adjust == "tx" else (tx, rx)
    offset, turns, pk = decide(peak(xcorr(fixed, moved)), moved.shape[0])
    out = gather(moved, offset, turns, fixed.shape[0])
    return ((out, rx) if adjust == "tx" else (tx, out)), pk


def qam16(n, seed):
    """``n`` random 16-QAM symbols (unit mean power over the alphabet) and their alphabet."""
    rng = np.random.default_rng(seed)
    levels = np.array([-3., -1., 1., 3.]) / np.sqrt(10.)
    alphabet = (levels[:, None] + 1j * levels[None, :]).ravel()
    return alphabet[rng.integers(0, 16, n)], alphabet


def case(ntx, nrx, shift, turns, seed=0, noise=0.05):
    """A transmitted pattern and what a receiver sees of it: the pattern made periodic, started ``shift`` samples in, turned back by
    ``turns`` quarter turns, ``nrx`` samples long, with a little noise."""
    tx, _ = qam16(ntx, seed + 1000 * ntx + nrx)
    rng = np.random.default_rng(seed + 7)
    rx = tx[(np.arange(nrx) + shift) % ntx] * 1.j ** (-turns)
    return tx, rx + noise * (rng.standard_normal(nrx) + 1j * rng.standard_normal(nrx))
