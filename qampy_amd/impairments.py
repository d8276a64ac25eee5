"""Signal-object impairments (qampy/impairments.py:104-125): chromatic dispersion."""
from .core import impairments as _core


def add_dispersion(sig, D, L, wl0=1550e-9):
    """Add the dispersion of ``L`` metres of fibre (``D`` in s/m/m) to a signal object at its own ``fs``: see
    :func:`qampy_amd.core.impairments.add_dispersion`."""
    return sig.recreate_from_np_array(_core.add_dispersion(sig, sig.fs, D, L, wl0=wl0))
