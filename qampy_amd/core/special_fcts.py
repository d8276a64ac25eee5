"""Special functions of the pulse-shaping filters (the call surface of qampy/core/special_fcts.py)."""
import numpy as np


def rrcos_time(t, beta, T):
    """
    Impulse response of the root-raised-cosine filter with roll-off ``beta`` (0 < beta <= 1) and symbol period ``T`` at the times ``t``:

        h(t) = [sin(pi x (1 - beta)) + 4 beta x cos(pi x (1 + beta))] / [pi x (1 - (4 beta x)^2)] / T,   x = t / T

    with its two removable singularities filled in by their limits: h(0) = (1 + beta (4 / pi - 1)) / T and
    h(+-T / (4 beta)) = beta / (T sqrt 2) [(1 + 2 / pi) sin(pi / (4 beta)) + (1 - 2 / pi) cos(pi / (4 beta))].  A sample counts as
    singular when it lies within a quarter of the grid spacing of the point, so a grid that hits it up to rounding is handled.
    """
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    x = t / T
    eps = abs(x.flat[1] - x.flat[0]) / 4 if x.size > 1 else 1e-9
    at0 = np.abs(x) < eps
    atq = np.abs(np.abs(x) - 1 / (4 * beta)) < eps
    xs = np.where(at0 | atq, 0.5 / (4 * beta), x)            # any regular point: overwritten below
    h = (np.sin(np.pi * xs * (1 - beta)) + 4 * beta * xs * np.cos(np.pi * xs * (1 + beta))) / (np.pi * xs * (1 - (4 * beta * xs) ** 2)) / T
    h[at0] = (1 + beta * (4 / np.pi - 1)) / T
    a = np.pi / (4 * beta)
    h[atq] = beta / (T * np.sqrt(2)) * ((1 + 2 / np.pi) * np.sin(a) + (1 - 2 / np.pi) * np.cos(a))
    return h


def q_function(x):
    """Tail probability of the standard normal distribution, ``0.5 erfc(x / sqrt 2)`` (the Gaussian co-error function of the BER formulas)."""
    from scipy.special import erfc
    return erfc(np.asarray(x, dtype=np.float64) * np.sqrt(0.5)) / 2
