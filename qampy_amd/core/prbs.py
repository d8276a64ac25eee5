"""
Pseudo-random bit sequences, the call surface of ``qampy.core.prbs`` with the generator on the GPU (csrc/source.hip).

The reference steps a shift register one bit at a time (``pythran_dsp.prbs_ext`` / ``prbs_int``).  Both registers obey a two-term linear
recurrence over GF(2), so every workgroup jumps to its own first bit and the bits are produced in parallel; the values are the reference's bit
for bit.  Two departures, both on input the reference mishandles:

* a seed outside ``[0, 2**order)`` raises ``ValueError`` - in the reference its stray high bits drift into the taps;
* ``make_prbs_intXOR`` works: the reference's passes three arguments to the four-argument ``prbs_int`` and raises ``TypeError``; this one
  returns what ``pythran_dsp.prbs_int(seed, mask, order, nbits)`` returns.

For a sequence that stays in HBM use :func:`qampy_amd.core.hip_dsp.prbs_bits_dev`.
"""
import numpy as np

from .. import _lib
from . import hip_dsp


def _make(order, nbits, seed, kind):
    assert order in [7, 15, 23, 31], """Only orders 7, 15, 23, 31 are implemented"""
    nbits = int(nbits)
    seed = hip_dsp.prbs_seed(order, seed)
    if nbits < 1:
        return np.zeros(0, dtype=bool)
    out = np.empty(nbits, dtype=bool)
    for a in range(0, nbits, hip_dsp.PRBS_ROW_MAX):
        n = min(hip_dsp.PRBS_ROW_MAX, nbits - a)
        d = _lib.DeviceArray((n,), np.uint8)
        hip_dsp.prbs_bits_dev(d, order, seed, kind=kind, start=a)
        out[a:a + n] = d.to_host().view(bool)
    return out


def make_prbs_extXOR(order, nbits, seed=None):
    """
    Pseudo-random bit sequence of a linear feedback shift register with external (Fibonacci) XOR (qampy/core/prbs.py:27-58).

    Parameters
    ----------
    order : one of 7, 15, 23, 31
    nbits : length of the sequence
    seed : int in ``[0, 2**order)`` or bool array (element 0 is bit 0); None: all ones

    Returns
    -------
    bool array of ``nbits`` values
    """
    return _make(order, nbits, seed, "ext")


def make_prbs_intXOR(order, nbits, seed=None):
    """
    Pseudo-random bit sequence of a linear feedback shift register with internal (Galois) XOR: ``pythran_dsp.prbs_int(seed, mask, order,
    nbits)`` with the masks of qampy/core/prbs.py:81-86.  Arguments and result as :func:`make_prbs_extXOR`.
    """
    return _make(order, nbits, seed, "int")
