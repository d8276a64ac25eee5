"""Small helpers under the names of qampy/helpers.py (:26-57): unit conversions, |x|^2 and the per-row normalisation."""
import numpy as np

from .synth import normalise_and_center          # noqa: F401  (re-exported: per-mode mean removal and unit-power scaling, always 2-d)


def cabssquared(x):
    """``x.real**2 + x.imag**2``"""
    return x.real ** 2 + x.imag ** 2


def dB2lin(x):
    """dB -> linear: ``10**(x / 10)``"""
    return 10 ** (x / 10)


def lin2dB(x):
    """linear -> dB: ``10 log10(x)``"""
    return 10 * np.log10(x)
