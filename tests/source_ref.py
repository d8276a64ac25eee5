"""
Numpy restatement of the bit source and the Gray mapper (csrc/source.hip), pinned to the reference by tests/test_source_ref.py through
tests/golden/source.npz.  No GPU, no reference.

External XOR (``pythran_dsp.prbs_ext``, taps ``[o, k]``): with the virtual history ``b[-o + p] = bit p of the seed``, ``p < o``, the output is
``b[i] = b[i - o] ^ b[i - k]`` for every ``i >= 0``.  Internal XOR (``pythran_dsp.prbs_int(seed, mask, o, N)``): the Galois register itself for
the first ``o`` outputs, then ``g[i] = g[i - o] ^ g[i - (o - k)]``.  Both recurrences are run in blocks: squaring a two-term recurrence over
GF(2) doubles both lags, ``b[i] = b[i - 2^j o] ^ b[i - 2^j k]`` for ``i >= 2^j o`` past the start of the data, so the blocks grow with it.
"""
import numpy as np

TAPS = {7: 6, 15: 14, 23: 18, 31: 28}


def seed_int(order, seed=None):
    """The seed as an integer: None is all ones, a bool array is read with element 0 as bit 0 (the reference's ``bool2bin``)."""
    if seed is None:
        return 2 ** order - 1
    if np.ndim(seed) > 0:
        return int(sum(int(bool(v)) << i for i, v in enumerate(np.asarray(seed).ravel())))
    return int(seed)


def _extend(first, n, a, b):
    """``first`` continued to ``n`` values by ``c[i] = c[i - a] ^ c[i - b]``, ``a > b``, ``len(first) >= a``."""
    have = len(first)
    out = np.zeros(max(n, have), np.uint8)
    out[:have] = first
    while have < n:
        j = 0
        while (a << (j + 1)) <= have:
            j += 1
        A, B = a << j, b << j
        cnt = min(B, n - have)
        out[have:have + cnt] = out[have - A:have - A + cnt] ^ out[have - B:have - B + cnt]
        have += cnt
    return out[:n]


def prbs_ext(order, n, seed=None, start=0):
    """Bits ``start .. start + n - 1`` of the external-XOR sequence, uint8."""
    s = seed_int(order, seed)
    history = np.array([(s >> p) & 1 for p in range(order)], np.uint8)
    return _extend(history, order + start + n, order, TAPS[order])[order + start:]


def galois_steps(order, n, seed=None):
    """``pythran_dsp.prbs_int(seed, 2^o + 2^k + 1, o, n)`` step by step."""
    state, mask = seed_int(order, seed), 2 ** order + 2 ** TAPS[order] + 1
    out = np.zeros(n, np.uint8)
    for i in range(n):
        state <<= 1
        x = state >> order
        if x:
            state ^= mask
        out[i] = x
    return out


def prbs_int(order, n, seed=None, start=0):
    """Bits ``start .. start + n - 1`` of the internal-XOR sequence, uint8."""
    return _extend(galois_steps(order, order, seed), start + n, order, order - TAPS[order])[start:]


def prbs(kind, order, n, seed=None, start=0):
    return {"ext": prbs_ext, "int": prbs_int}[kind](order, n, seed, start)


def bits_to_labels(bits, nb):
    """Labels, MSB first per symbol, of rows of whole symbols (``SignalQAMGrayCoded._modulate``)."""
    bits = np.asarray(bits).astype(np.int64)
    return (bits.reshape(bits.shape[:-1] + (-1, nb)) @ (2 ** np.arange(nb - 1, -1, -1))).astype(np.int32)


def labels_to_bits(labels, nb):
    labels = np.asarray(labels).astype(np.int64)
    return ((labels[..., None] >> np.arange(nb - 1, -1, -1)) & 1).astype(np.uint8).reshape(labels.shape[:-1] + (-1,))
