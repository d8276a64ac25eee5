"""Signal-object wrappers of :mod:`qampy_amd.core.analog_frontend` (qampy/analog_frontend.py)."""
from .core import analog_frontend as _core
from .core.analog_frontend import comp_IQ_inbalance          # noqa: F401


def comp_rf_delay(signal, delay):
    """Delay a signal object by ``delay`` seconds at its own sampling rate ``signal.fs``: :func:`qampy_amd.core.analog_frontend.comp_rf_delay`,
    handed to ``signal.recreate_from_np_array``."""
    return signal.recreate_from_np_array(_core.comp_rf_delay(signal, delay, signal.fs))


def orthonormalize_signal(signal):
    """Orthonormalise a signal object at its own oversampling ``signal.os``: :func:`qampy_amd.core.analog_frontend.orthonormalize_signal`
    (a plain array, as the reference returns)."""
    return _core.orthonormalize_signal(signal, signal.os)
