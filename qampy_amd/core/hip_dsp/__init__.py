"""
The Python side of every non-trainer kernel of ``libqampy_hip.so``, one module per unit; the kernels live in qampy_amd/csrc.  This file only
re-exports: the public names of the units are the attributes of ``qampy_amd.core.hip_dsp``, as callers and tests look them up.  What the
units check their arguments with is in ``_args``; a unit imports the public functions of another, never its underscore names.
(``hip_dsp.bps`` is the function: the ``from`` import below binds it over the module of that name.)
"""
# flake8: noqa: F401
from .bps import bps, bps_recover, bps_recover_dev, bps_twostage_recover, bps_twostage_recover_dev, select_angles, test_angle_grid, twostage_offsets
from .foe import FOE_NMAX, FOE_NMIN, comp_freq_offset, comp_freq_offset_dev, find_freq_offset, find_freq_offset_dev, foe_plan
from .cpr import P16_NBLOCK_MAX, VV_MMAX, VV_NMAX, partition16_recover, partition16_recover_dev, pilot_phase_trace, vv_recover, vv_recover_dev
from .metrics import bits_map_labels, cal_mi_mc, cal_mi_mc_fast, estimate_snr, soft_l_value_demapper, soft_l_value_demapper_minmax
from .impair import (IMPAIR_TILE, PMD_N, PMD_NMIN, apply_pmd_dev, impair_pointwise_dev, modal_delay_dev, phase_noise_dev, rotate_field_dev,
                     simulate_transmission_dev, snr_noise_factor, snr_power_factor)
from .txresp import (SOS_CHUNK, SOS_MAXSEC, SOS_TILE, TX_MAXMODES, dac_pointwise_dev, design_lowpass_sos, enob_sigma, filter_signal_dev,
                     modulator_response_dev, row_extrema_dev, sim_dac_response_dev, sim_tx_response_check, sim_tx_response_dev, sos_transition,
                     sosfilt_dev)
from .frontend import (FFT_ANY_MAX, FFT_POW2_MAX, FFT_POW2_MIN, FH_BAND, FH_BRICK, FH_COMPLEX, FH_RAMP, FH_REAL, FH_TWORAIL, IQ_CENTRE, IQ_IMBALANCE,
                       IQ_ORTHONORMALIZE, IQ_TILE, comp_iq_imbalance_dev, delay_dev, fft_dev, fft_length_ok, fft_plan, ifft_dev, iq_affine_dev,
                       iq_coeffs_dev, iq_moments_dev, orthonormalize_dev, pre_filter_bins, pre_filter_dev, pre_filter_wdm_dev, skew_dev,
                       spectral_filter_dev)
from .sync import (PEAK_FIELDS, PEAK_TILE, SYNC_ROW_MAX, XCORR_MAX, cyclic_gather_dev, find_sequence_offset_complex_dev, labels_to_symbols_dev,
                   peak_decision, sync_and_adjust_dev, xcorr_dev, xcorr_peak_dev)
from .source import (PRBS_KINDS, PRBS_ORDERS, PRBS_ROW_MAX, PRBS_START_MAX, PRBS_W, SOURCE_NB, SOURCE_SYMS, bits_to_labels_dev, demodulate_dev,
                     labels_to_bits_dev, modulate_bits_dev, prbs_bits_dev, prbs_seed, prbs_symbols_dev)
from .pilot import (PILOT_NMAX, PILOT_ROW_MAX, PILOT_TABLES_KEPT, pilot_const_phase, pilot_const_phase_dev, pilot_counts, pilot_cpe, pilot_cpe_dev,
                    pilot_foe, pilot_foe_dev, pilot_frame_dev, pilot_frame_list, pilot_knots_dev, pilot_ordinals, pilot_phase_dev, pilot_positions,
                    pilot_split_dev, pilot_used, rotate_rows_dev)
from .precomp import (PRECOMP_LDS_N, PRECOMP_LEN_MAX, PRECOMP_LUT_LMAX, PRECOMP_M_MAX, PRECOMP_MEM_MAX, PRECOMP_N_MAX, PRECOMP_ROW_MAX, PatternLevels,
                      cal_lut_dev, comp_dac_resp_dev, comp_mod_sin_dev, dac_preemphasis_dev, lut_accumulate_dev, lut_apply_dev, lut_predistort_dev,
                      pattern_index_dev, pattern_levels)
from .theory import (MC_NS_MAX, MC_NSNR_MAX, MC_TILE, MC_TRIP, PS_LMAX, PS_ROW_MAX, PS_TILE, awgn_mc, awgn_mc_dev, awgn_mc_noise_dev, cal_gmi_mc,
                     fresh_seed, ps_cdf, ps_symbols_dev)
from .blind import (BLIND_M_MAX, BLIND_SLICE, BLIND_SLICES, BLIND_STATS, blind_evm_dev, blind_ideal, blind_moments_dev, blind_stats_dev, cal_gamma,
                    norm_to_s0_dev, qpsk_blind_snr_dev, stats_from_moments)
from .hybrid import (TDH_FM_MAX, TDH_M_MAX, TDH_ROW_MAX, TDH_SUMS, TDH_TILE, tdh_align_dev, tdh_align_host, tdh_assemble_dev, tdh_class_sums_dev,
                     tdh_divide, tdh_geometry, tdh_metrics_dev, tdh_power_ratio, tdh_rates, tdh_split_dev)
from .fibre import C_LIGHT, FIBRE_MAX, H_PLANCK, ase_power, dbp_dev, fibre_alpha, fibre_nl_dev, fibre_plan, ssfm_dev
