"""
What every unit of the device DSP binding checks its arguments with: is this a complex DeviceArray of the right rank and size, is this
output buffer of this shape and dtype (or shall one be made), and the few argument rules more than one unit shares.  Every check raises
before anything is launched.  A mistake in the dtype is a ``TypeError`` and one in the shape a ``ValueError``, unless ``exc`` says
otherwise: the units differ there, and their callers rely on it.
"""
import numpy as np

from ... import _lib


def cplx(a, what, name="E", exc=TypeError):
    """``"c64"`` / ``"c128"``, the suffix of the entry points, of a complex DeviceArray of any shape."""
    suf, rt, ct = _lib.suffix(a.dtype)
    if np.dtype(a.dtype) != ct:
        raise exc("%s: %s must be a complex64 or complex128 DeviceArray" % (what, name))
    return _lib.cname(suf)


def rows_of(a, what, name="E"):
    """``(rows, length)`` of a non-empty 1-d row or 2-d stack of rows of any dtype."""
    if len(a.shape) not in (1, 2) or min(a.shape) < 1:
        raise ValueError("%s: %s must be a non-empty 1-d row or 2-d stack of rows" % (what, name))
    return (1, a.shape[0]) if len(a.shape) == 1 else tuple(a.shape)


def field(a, what, name="E", *, ndim=(2,), rows=None, like=None, max_rows=None, max_len=None, empty=False, exc=None):
    """``(c, rows, L)`` of a complex DeviceArray, ``c`` as :func:`cplx` gives it.  ``ndim``: the ranks it may have, ``(1, 2)`` for a row (one
    row then) or a stack of rows; ``rows``: the number of rows it must have; ``like``: the dtype it must have; ``max_rows``, ``max_len``: the
    most the kernels index; ``empty``: whether an axis of length 0 passes; ``exc``: one exception type for dtype and rank instead of the two of
    the module's rule."""
    c = cplx(a, what, name, exc or TypeError)
    if len(a.shape) not in ndim or not (empty or min(a.shape) >= 1):
        raise (exc or ValueError)("%s: %s must be a%s %s complex DeviceArray" % (what, name, "" if empty else " non-empty", " or ".join("%d-d" % n for n in ndim)))
    nrows, L = (1, a.shape[0]) if len(a.shape) == 1 else tuple(a.shape)
    if rows is not None and nrows != rows:
        raise ValueError("%s: %s must have %d rows" % (what, name, rows))
    if like is not None and np.dtype(a.dtype) != np.dtype(like):
        raise TypeError("%s: %s must be %s like the field" % (what, name, np.dtype(like).name))
    if (max_rows is not None and nrows > max_rows) or (max_len is not None and L > max_len):
        raise ValueError("%s: %s is too large" % (what, name))
    return c, nrows, L


def buffer(a, what, name, shape, dtype, *, make=False, optional=False, by_size=False):
    """``a`` if it is a DeviceArray of this shape and dtype, else ValueError.  When ``a`` is None: ``make`` gives a fresh one, ``optional`` lets
    the None pass.  ``by_size``: any shape of as many elements passes."""
    if a is None and (make or optional):
        return _lib.DeviceArray(shape, dtype) if make else None
    if a is None or np.dtype(a.dtype) != np.dtype(dtype) or (int(np.prod(a.shape)) != int(np.prod(shape)) if by_size else tuple(a.shape) != tuple(shape)):
        raise ValueError("%s: %s must be %s %s" % (what, name, tuple(shape), np.dtype(dtype).name))
    return a


def resident(E, what):
    """``c`` of an (nmodes, L) field as the channel, transmitter, front-end and fibre units take it: an axis may be empty, and a wrong rank
    is a TypeError like a wrong dtype."""
    return field(E, what, empty=True, exc=TypeError)[0]


def same_as(E, out, what):
    """``out`` must be a buffer of ``E``'s shape and dtype (it may be ``E``)."""
    return buffer(out, what, "out", E.shape, E.dtype)


def bit_rows(a, what, name):
    """``(rows, length)`` of a row or a stack of rows of bits, one byte each."""
    if np.dtype(a.dtype) not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError("%s: %s must be a uint8 or bool DeviceArray" % (what, name))
    return rows_of(a, what, name)


def two_modes(E, what):
    if E.shape[0] != 2:
        raise ValueError("%s needs two modes" % what)


def modes_upto(E, what, most):
    if not 1 <= E.shape[0] <= most:
        raise ValueError("%s works on 1 to %d modes" % (what, most))


def seed64(seed):
    """The low 64 bits of an integer seed, as the counter-based generators take it."""
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def thread_table(local, key, make, keep=None):
    """``make()`` - device copies of small host tables, staging buffers - kept by ``key`` in the ``threading.local()`` ``local``, so that a loop
    which asks for the same again uploads and allocates nothing.  ``keep``: the most entries kept; the oldest go, and are released, before
    a new one is made."""
    kept = local.__dict__.setdefault("kept", {})                 # (the dictionary of a threading.local is the calling thread's own)
    if key not in kept:
        while keep is not None and len(kept) >= keep:
            kept.pop(next(iter(kept)))
        kept[key] = make()
    return kept[key]
