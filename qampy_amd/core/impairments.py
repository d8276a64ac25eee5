"""Chromatic dispersion on plain ndarrays (qampy/core/impairments.py:673-703 add_dispersion), through the GPU's block filter."""
import numpy as np

from . import filter as _filter


def add_dispersion(sig, fs, D, L, wl0=1550e-9):
    """
    Add the dispersion of ``L`` metres of fibre (``D`` in s/m/m, centre wavelength ``wl0``) to every row of ``sig``: circular filtering
    by exp(-0.5j beta2 L omega^2) on the fftfreq grid of the row length, in the input's dtype (complex64 or complex128).

    A row length that is a power of two up to 8192 is one exact transform per row; longer or other lengths run as overlap-save blocks of
    the default size of :func:`qampy_amd.core.filter.cd_filter_dev`, with its truncation error (about 2e-5 to 5e-5 of the signal rms).
    Every row is filtered on its own: the reference's 2-d input goes through a final ``fftshift`` over all axes, which also rolls the
    rows (two modes come back swapped); that is not reproduced.
    """
    x = np.asarray(sig)
    one = x.ndim == 1
    X = np.atleast_2d(x)
    if X.dtype not in (np.complex64, np.complex128):
        X = X.astype(np.complex128)
    n = X.shape[-1]
    N = n if (n & (n - 1)) == 0 and _filter.CD_NMIN <= n <= _filter.CD_NMAX else _filter.cd_block_size(_filter.cd_spread(fs, D, L, wl0))
    out = _filter.cd_filter_host(X, N, _filter.cd_coeffs_exact(fs, D, L, wl0))
    return out[0] if one else out
