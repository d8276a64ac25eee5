"""
Bit source and Gray mapper: csrc/source.hip on DeviceArrays, for qampy.core.prbs, PRBSBits and SignalQAMGrayCoded._modulate /
_demodulate (qampy/signals.py:89-137, :678-731).  Bits are one byte each (uint8 or bool DeviceArrays, 0 / 1); labels are int32, the
first bit of a symbol the most significant.
"""
import numpy as np

from ... import _lib
from ._args import bit_rows, buffer, cplx, rows_of

PRBS_ORDERS = (7, 15, 23, 31)
PRBS_KINDS = {"ext": 0, "int": 1}  # external (Fibonacci) / internal (Galois) XOR
PRBS_W = 65536                     # bits per workgroup of prbs_bits_dev (csrc/source.hip SRC_W)
SOURCE_SYMS = 8192                 # symbols per workgroup of prbs_symbols_dev, 32 per thread, whatever the bits per symbol (SRC_SYMS)
PRBS_ROW_MAX = 2 ** 31             # most bits of a row, most symbols of a mapping call
PRBS_START_MAX = 2 ** 62
SOURCE_NB = (2, 10)                # bits per symbol


def prbs_seed(order, seed=None):
    """The seed of a PRBS as an integer in ``[0, 2**order)``: ``None`` is all ones, a bool array is read as the reference's ``bool2bin`` reads
    it (element 0 is bit 0).  Anything outside the range raises ``ValueError`` (in the reference the stray high bits drift into the taps)."""
    if order not in PRBS_ORDERS:
        raise ValueError("Only orders 7, 15, 23, 31 are implemented")
    if seed is None:
        return 2 ** order - 1
    if np.ndim(seed) > 0:
        seed = sum(int(bool(v)) << i for i, v in enumerate(np.asarray(seed).ravel()))
    if int(seed) != seed:
        raise ValueError("the seed must be an integer or an array of bools")
    seed = int(seed)
    if not 0 <= seed < 2 ** order:
        raise ValueError("the seed of a PRBS of order %d must lie in [0, 2**%d), got %d" % (order, order, seed))
    return seed


def _prbs_args(order, seed, kind, start):
    seed = prbs_seed(order, seed)
    if kind not in PRBS_KINDS:
        raise ValueError("kind must be 'ext' (external XOR) or 'int' (internal XOR), not %r" % (kind,))
    if int(start) != start or not 0 <= int(start) <= PRBS_START_MAX:
        raise ValueError("start must be an integer in [0, 2**62]")
    return int(order), PRBS_KINDS[kind], seed, int(start)


def _bits_per_symbol(nb, what):
    if int(nb) != nb or not SOURCE_NB[0] <= nb <= SOURCE_NB[1]:
        raise ValueError("%s: between %d and %d bits per symbol" % ((what,) + SOURCE_NB))
    return int(nb)


def _alphabet_bits(alphabet, what):
    M = int(np.prod(alphabet.shape))
    nb = int(round(np.log2(M))) if M >= 1 else 0
    if 2 ** nb != M:
        raise ValueError("%s: the alphabet must have a power of two of points, got %d" % (what, M))
    return M, _bits_per_symbol(nb, what)


def prbs_bits_dev(out, order, seed=None, kind="ext", start=0, invert=False):
    """Bits ``start .. start + n - 1`` of the PRBS of ``order`` (7, 15, 23, 31) into the 1-d uint8 / bool DeviceArray ``out`` of ``n`` bits:
    ``kind="ext"`` what ``make_prbs_extXOR(order, start + n, seed)[start:]`` holds, ``"int"`` the internal-XOR form.  ``seed``: None (all
    ones), an int in ``[0, 2**order)`` or a bool array (element 0 is bit 0); ``start`` up to 2**62 at no extra cost (every workgroup jumps to
    its first bit); ``invert`` complements the output.  Nothing is read back."""
    order, k, seed, start = _prbs_args(order, seed, kind, start)
    if len(out.shape) != 1:
        raise ValueError("prbs_bits_dev: out must be one row (use DeviceArray.row for a stack)")
    rows, n = bit_rows(out, "prbs_bits_dev", "out")
    if n > PRBS_ROW_MAX:
        raise ValueError("prbs_bits_dev: at most 2**31 bits per call")
    _lib.call("qh_prbs_bits_dev", order, k, seed, start, int(bool(invert)), n, out.ptr)
    return out


def _map_shapes(bits, labels, nb, what):
    """Number of symbols of ``bits`` (rows of whole symbols) and the check of ``labels`` against it."""
    rows, n = bit_rows(bits, what, "bits")
    if n % nb:
        raise ValueError("%s: the rows of bits must hold whole symbols of %d bits" % (what, nb))
    shape = tuple(bits.shape[:-1]) + (n // nb,)
    if labels is not None:
        if np.dtype(labels.dtype) != np.int32:
            raise TypeError("%s: labels must be int32" % what)
        if tuple(labels.shape) != shape:
            raise ValueError("%s: labels must be %s" % (what, shape))
    if rows * (n // nb) > PRBS_ROW_MAX:
        raise ValueError("%s: at most 2**31 symbols per call" % what)
    return rows * (n // nb), shape


def bits_to_labels_dev(bits, nb, labels):
    """``labels = bits.reshape(..., -1, nb) @ 2**arange(nb - 1, -1, -1)`` (``_modulate``'s index, MSB first) for a row or a stack of rows of
    whole symbols; ``labels`` int32, one per symbol."""
    nb = _bits_per_symbol(nb, "bits_to_labels_dev")
    if labels is None:
        raise ValueError("bits_to_labels_dev: labels must be given")
    nsym, _ = _map_shapes(bits, labels, nb, "bits_to_labels_dev")
    _lib.call("qh_bits_to_labels_dev", bits.ptr, nsym, nb, labels.ptr)
    return labels


def labels_to_bits_dev(labels, nb, bits):
    """The inverse of :func:`bits_to_labels_dev`: the low ``nb`` bits of every int32 label, most significant first, one byte each."""
    nb = _bits_per_symbol(nb, "labels_to_bits_dev")
    if labels is None:
        raise ValueError("labels_to_bits_dev: labels must be given")
    nsym, _ = _map_shapes(bits, labels, nb, "labels_to_bits_dev")
    _lib.call("qh_labels_to_bits_dev", labels.ptr, nsym, nb, bits.ptr)
    return bits


def modulate_bits_dev(bits, alphabet, symbols, labels=None, nb=None):
    """``symbols = alphabet[label]`` of every ``nb`` bits of ``bits`` (``SignalQAMGrayCoded._modulate`` with ``alphabet`` the coded symbols):
    one launch, ``labels`` written too when given.  ``nb``: ``log2`` of the alphabet's size; given explicitly, the alphabet may be shorter than
    ``2**nb`` and a label outside it gives 0, as in :func:`labels_to_symbols_dev`."""
    c = cplx(alphabet, "modulate_bits_dev", "alphabet")
    M = int(np.prod(alphabet.shape))
    nb = _alphabet_bits(alphabet, "modulate_bits_dev")[1] if nb is None else _bits_per_symbol(nb, "modulate_bits_dev")
    if M < 1:
        raise ValueError("modulate_bits_dev: at least one alphabet point")
    nsym, shape = _map_shapes(bits, labels, nb, "modulate_bits_dev")
    buffer(symbols, "modulate_bits_dev", "symbols", shape, alphabet.dtype)
    _lib.call("qh_modulate_bits_%s_dev" % c, bits.ptr, nsym, nb, alphabet.ptr, M, symbols.ptr, None if labels is None else labels.ptr)
    return symbols


def prbs_symbols_dev(symbols, alphabet, order, seed=None, kind="ext", start=0, labels=None, bits=None):
    """The fused source of one row: PRBS bits ``start .. start + nsym * nb - 1`` (arguments as :func:`prbs_bits_dev`) -> labels -> ``symbols
    = alphabet[label]`` in one launch.  ``symbols``: 1-d, ``nsym`` values of the alphabet's dtype; ``alphabet``: ``2**nb`` points; ``labels``
    (nsym,) int32 and ``bits`` (nsym * nb,) uint8 / bool are written only when given - symbols alone cost no bit traffic."""
    c = cplx(alphabet, "prbs_symbols_dev", "alphabet")
    M, nb = _alphabet_bits(alphabet, "prbs_symbols_dev")
    order, k, seed, start = _prbs_args(order, seed, kind, start)
    if len(symbols.shape) != 1 or symbols.shape[0] < 1 or np.dtype(symbols.dtype) != np.dtype(alphabet.dtype):
        raise ValueError("prbs_symbols_dev: symbols must be one non-empty row of the alphabet's dtype")
    nsym = symbols.shape[0]
    if nsym * nb > PRBS_ROW_MAX:
        raise ValueError("prbs_symbols_dev: at most 2**31 bits per row")
    buffer(labels, "prbs_symbols_dev", "labels", (nsym,), np.int32, optional=True)
    if bits is not None and (bit_rows(bits, "prbs_symbols_dev", "bits") != (1, nsym * nb) or len(bits.shape) != 1):
        raise ValueError("prbs_symbols_dev: bits must be (%d,)" % (nsym * nb))
    _lib.call("qh_prbs_symbols_%s_dev" % c, order, k, seed, start, nsym, nb, alphabet.ptr, M, symbols.ptr, None if labels is None else labels.ptr,
              None if bits is None else bits.ptr)
    return symbols


def demodulate_dev(E, alphabet, bits, labels=None):
    """Bits of the decisions of ``E`` (a row or a stack of rows): the nearest alphabet point of every sample (``qh_make_decision_*_dev``), then
    its label's bits, MSB first, into ``bits`` (``E``'s shape with the last axis times ``nb``).  ``labels``: the int32 decisions, kept when
    given (a buffer of ``E``'s shape)."""
    from ..equalisation import hip_equalisation as hk
    cplx(alphabet, "demodulate_dev", "alphabet")
    M, nb = _alphabet_bits(alphabet, "demodulate_dev")
    if np.dtype(E.dtype) != np.dtype(alphabet.dtype):
        raise TypeError("demodulate_dev: E and the alphabet must have one dtype")
    rows_of(E, "demodulate_dev", "E")
    if tuple(bits.shape) != tuple(E.shape[:-1]) + (E.shape[-1] * nb,):
        raise ValueError("demodulate_dev: bits must be %s" % (tuple(E.shape[:-1]) + (E.shape[-1] * nb,),))
    if labels is None:
        _map_shapes(bits, None, nb, "demodulate_dev")
        labels = _lib.DeviceArray(E.shape, np.int32)
    else:
        _map_shapes(bits, labels, nb, "demodulate_dev")
    hk.make_decision_dev(E, alphabet, None, None, labels)
    return labels_to_bits_dev(labels, nb, bits)
