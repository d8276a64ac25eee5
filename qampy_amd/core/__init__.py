"""Core API (plain ndarrays in/out), mirror of ``qampy.core`` for the equaliser + BPS hot path."""
from . import analog_frontend, equalisation, phaserecovery, ber_functions, filter, impairments, pilotbased_receiver, prbs, resample, special_fcts  # noqa: F401
from . import digital_pre_compensation, fibre  # noqa: F401
