"""Signal-object filters (qampy/filtering.py): the wrappers of :mod:`qampy_amd.core.filter` that take a signal object at its own ``fs`` and
return ``signal.recreate_from_np_array(...)``."""
from .core import filter as _core
from .core.filter import moving_average          # noqa: F401


def filter_signal(signal, cutoff, ftype="bessel", order=2, analog=False):
    """Low-pass a signal object by a digital Bessel or Butterworth filter with the 3 dB ``cutoff``: see
    :func:`qampy_amd.core.filter.filter_signal` ('gauss', 'exp' and ``analog=True`` raise NotImplementedError)."""
    return signal.recreate_from_np_array(_core.filter_signal(signal, signal.fs, cutoff, ftype=ftype, order=order, analog=analog))


def rrcos_pulseshaping(sig, beta, T=None):
    """Root-raised-cosine filtering of a signal object with roll-off ``beta`` and symbol period ``T`` (None: ``1 / sig.fb`` - the reference
    passes ``sig.fb`` itself there, which is a rate, not a period), by the tap filter of :func:`qampy_amd.core.filter.rrcos_pulseshaping`."""
    if T is None:
        T = 1 / sig.fb
    return sig.recreate_from_np_array(_core.rrcos_pulseshaping(sig, sig.fs, T, beta))


def pre_filter(signal, bw):
    """Brick-wall pre-filter of a signal object: :func:`qampy_amd.core.filter.pre_filter`, handed to ``signal.recreate_from_np_array``."""
    return signal.recreate_from_np_array(_core.pre_filter(signal, bw))
