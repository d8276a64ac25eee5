"""Host side of the signal-quality metrics (no GPU): the bit map and its inversion, the tx / rx alignment restated from the
reference, and the C ABI of the metric kernels.  Fixture: tests/golden/metrics.npz (gen_golden_metrics.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qampy_amd import _lib
from qampy_amd.core import ber_functions, hip_dsp, signal_quality
from qampy_amd.signals import SignalQAM

MS = (4, 16, 32, 64, 128, 256)
CT = {"c64": np.complex64, "c128": np.complex128}


@pytest.fixture(scope="module")
def fx(golden):
    return golden["metrics"]


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", MS)
def test_generate_bitmapping_mtx_equals_the_reference(fx, M, dn):
    coded, bits = fx["M%d_%s_coded" % (M, dn)], fx["M%d_%s_coded_bits" % (M, dn)]
    bm = signal_quality.generate_bitmapping_mtx(coded, bits, M, dtype=CT[dn])
    assert bm.dtype == CT[dn]
    np.testing.assert_array_equal(bm, fx["M%d_%s_bitmap" % (M, dn)])
    np.testing.assert_array_equal(bm, fx["M%d_%s_bitmap_sig" % (M, dn)])


@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", MS)
def test_bits_map_inverts_to_the_coded_alphabet(fx, M, dn):
    """Point g of coded_symbols carries label g: inverting the reference's map gives the alphabet back in coded order."""
    coded = fx["M%d_%s_coded" % (M, dn)]
    np.testing.assert_array_equal(hip_dsp.bits_map_labels(fx["M%d_%s_bitmap" % (M, dn)]), coded)
    # and the labels are the Gray labels of the reference's own demodulation
    bits = fx["M%d_%s_coded_bits" % (M, dn)].reshape(M, -1).astype(int)
    np.testing.assert_array_equal(bits @ (1 << np.arange(bits.shape[1] - 1, -1, -1)), np.arange(M))


def test_bits_map_inversion_rejects_a_corrupted_map(fx):
    bm = np.array(fx["M16_c128_bitmap"])
    both = bm.copy()
    both[2, 0, 1] = bm[2, 0, 0]                                          # one point on both sides of bit 2
    with pytest.raises(ValueError):
        hip_dsp.bits_map_labels(both)
    dup = bm.copy()
    dup[0, 1, 0] = dup[0, 0, 0]                                          # 15 distinct points
    with pytest.raises(ValueError):
        hip_dsp.bits_map_labels(dup)
    moved = bm.copy()
    moved[3] = bm[2]                                                     # bits 2 and 3 equal: labels collide
    with pytest.raises(ValueError):
        hip_dsp.bits_map_labels(moved)
    with pytest.raises(ValueError):
        hip_dsp.bits_map_labels(bm[:3])                                  # 16 points cannot carry 3 bits
    with pytest.raises(ValueError):
        hip_dsp.bits_map_labels(bm[..., :1])


def _cx(q, fx):
    """Complex samples from the fixture's int16 (re, im) * rx_scale."""
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(fx["rx_scale"])


@pytest.mark.parametrize("dn", CT)
def test_sync_and_adjust_reproduces_the_reference_alignment(fx, dn):
    """Quarter turn, cyclic shift and swapped modes: the restated _sync_and_adjust assigns, rotates and rolls like the reference."""
    M, ct = int(fx["sync_M"]), CT[dn]
    coded = fx["M%d_%s_coded" % (M, dn)]
    tx = coded[fx["sync_%s_tx_label" % dn]]
    rx = _cx(fx["sync_rxq"], fx).astype(ct)
    sig = SignalQAM(rx, M, symbols=tx, coded_symbols=coded)
    t, r = sig._sync_and_adjust(sig.symbols, np.asarray(sig))
    assert t.dtype == r.dtype == ct
    np.testing.assert_array_equal(t, coded[fx["sync_%s_tx_aligned_label" % dn]])
    np.testing.assert_array_equal(r, _cx(fx["sync_%s_rx_alignedq" % dn], fx).astype(ct))


def test_adjust_helpers():
    x = np.arange(5)
    np.testing.assert_array_equal(ber_functions._adjust_to(x, 12), [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1])
    np.testing.assert_array_equal(ber_functions._adjust_to(x, 7, back=False), [3, 4, 0, 1, 2, 3, 4])
    np.testing.assert_array_equal(ber_functions._adjust_to(x, 10, back=False), np.r_[x, x, x])     # data[-0:] is all of data
    np.testing.assert_array_equal(ber_functions._adjust_to(x, 3), [0, 1, 2])
    t, r = ber_functions.adjust_data_length(np.arange(8), np.arange(5), method="truncate")
    assert len(t) == len(r) == 5
    t, r = ber_functions.adjust_data_length(np.arange(3), np.arange(8), method="extend", offset=1)
    np.testing.assert_array_equal(t, [2, 0, 1, 2, 0, 1, 2, 0])
    t, r = ber_functions.adjust_data_length(np.arange(8), np.arange(3))
    np.testing.assert_array_equal(t, [0, 1, 2])


def test_header_declares_the_metric_entry_points():
    text = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    assert int(re.search(r"#define QH_ABI_VERSION (\d+)", text).group(1)) == 11 == _lib.ABI_VERSION
    for base in ("soft_l_value_demapper", "soft_l_value_demapper_minmax", "estimate_snr", "cal_mi_mc", "cal_mi_mc_fast"):
        for suf in ("c64", "c128"):
            assert re.search(r"\bint qh_%s_%s\(" % (base, suf), text), base
            assert "qh_%s_%s" % (base, suf) in _lib.SIGNATURES
    for name in ("qh_metrics_c64_dev", "qh_metrics_c128_dev", "qh_estimate_snr_c64_dev", "qh_estimate_snr_c128_dev"):
        assert re.search(r"\bint %s\(" % name, text) and name in _lib.SIGNATURES


def test_metric_drop_ins_keep_the_reference_names():
    for name in ("soft_l_value_demapper", "soft_l_value_demapper_minmax", "estimate_snr", "cal_mi_mc", "cal_mi_mc_fast"):
        assert callable(getattr(hip_dsp, name)) and getattr(signal_quality, name) is getattr(hip_dsp, name)
    for meth in ("cal_ser", "cal_ber", "cal_evm", "est_snr", "cal_gmi", "cal_mi"):
        assert callable(getattr(SignalQAM, meth))
    assert SignalQAM(np.zeros((1, 4), np.complex64), 64).Nbits == 6
