"""The float64 restatement of the metric kernels (tests/metrics_ref.py) reproduces the reference's numbers in
tests/golden/metrics.npz and metrics_orders.npz at the tolerances tests/test_gpu_metrics.py holds the kernels to, so the GPU edge
tests (tests/test_gpu_metrics_edges.py) compare the kernels with a checked reference rather than with a second copy of them."""
import numpy as np
import pytest

import metrics_ref as ref

CT = {"c64": np.complex64, "c128": np.complex128}
RTOL = {"c64": 1e-5, "c128": 1e-12}         # evm / snr / s0 / n0
GABS = {"c64": 1e-5, "c128": 1e-10}         # gmi, gmi per bit, mi
LLR_TOL = {"c64": dict(rtol=1e-5, atol=1e-4), "c128": dict(rtol=1e-9, atol=1e-8)}
FILES = {"metrics": (4, 16, 32, 64, 128, 256), "metrics_orders": (8, 512, 1024)}
CASES = [(f, M, j, dn) for f, Ms in FILES.items() for M in Ms for j in (0, 1) for dn in CT]


def _cx(q, fx):
    return (q[..., 0] + 1j * q[..., 1].astype(np.float64)) / float(fx["rx_scale"])


def _rx(fx, M, j):
    base = np.round(fx["M%d_c128_coded" % M][fx["M%d_s%d_tx_label" % (M, j)]] * float(fx["rx_scale"]))
    return _cx(fx["M%d_s%d_rxd" % (M, j)] + np.stack([base.real, base.imag], axis=-1), fx)


def _close_where_finite(got, want, atol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin])), what
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=atol, err_msg=what)


def _check(fx, pre, rx, labels, al, dn):
    """Per mode: the restatement of est_snr / cal_ser / cal_ber / cal_evm (known and blind) / cal_gmi (both LLRs) / cal_mi."""
    got = {k: [] for k in ("snr", "s0", "n0", "ser", "ber", "evm", "evm_blind", "gmi", "gmi_per_bit", "gmi_minmax", "gmi_per_bit_minmax", "mi")}
    for m in range(rx.shape[0]):
        row = rx[m].astype(CT[dn])
        r = ref.metrics(row, labels[m], al)
        rm = ref.metrics(row, labels[m], al, snr=r["snr"], minmax=True)
        for k in ("snr", "s0", "n0", "ser", "ber", "evm", "gmi", "gmi_per_bit", "mi"):
            got[k].append(r[k])
        got["gmi_minmax"].append(rm["gmi"])
        got["gmi_per_bit_minmax"].append(rm["gmi_per_bit"])
        got["evm_blind"].append(np.sqrt(np.mean(np.abs(r["x"] - np.asarray(al, np.complex128)[r["dec"]]) ** 2)))
    np.testing.assert_array_equal(got["ser"], fx[pre + "ser"])
    np.testing.assert_array_equal(got["ber"], fx[pre + "ber"])
    for k in ("snr", "s0", "n0", "evm", "evm_blind"):
        np.testing.assert_allclose(got[k], fx[pre + k], rtol=RTOL[dn], err_msg=pre + k)
    for k in ("gmi", "gmi_per_bit", "gmi_minmax", "gmi_per_bit_minmax", "mi"):
        _close_where_finite(got[k], fx[pre + k], GABS[dn], pre + k)


def _normal_sums(r0, al, snr):
    """(n, nb): both of the reference's unshifted double sums are normal numbers (below that its own LLR is off)."""
    d = ref.dist2(np.asarray(r0, np.complex128), np.asarray(al, np.complex128))
    e = np.exp(-snr * d)
    bits = ref.bit_table(al.size)
    tiny = np.finfo(np.float64).tiny
    return np.stack([np.minimum(e[:, b == 0].sum(1), e[:, b == 1].sum(1)) >= tiny for b in bits.T], axis=1)


@pytest.mark.parametrize("f,M,j,dn", CASES, ids=["%s-M%d-s%d-%s" % c for c in CASES])
def test_restatement_reproduces_the_reference(golden, f, M, j, dn):
    fx = golden[f]
    pre = "M%d_s%d_%s_" % (M, j, dn)
    al = fx["M%d_%s_coded" % (M, dn)]
    rx, labels = _rx(fx, M, j), fx["M%d_s%d_tx_label" % (M, j)]
    _check(fx, pre, rx, labels, al, dn)
    nllr, snr = int(fx["nllr"]), float(fx[pre + "snr"][0])
    r0 = rx[0, :nllr].astype(CT[dn]).astype(np.complex128)
    L = ref.llr_exact(r0, al, snr)
    ok = np.isfinite(fx[pre + "llr"]) & _normal_sums(r0, al, snr)
    np.testing.assert_allclose(L[ok], fx[pre + "llr"][ok], err_msg=pre + "llr", **LLR_TOL[dn])
    np.testing.assert_allclose(ref.llr_maxlog(r0, al, snr), fx[pre + "llr_minmax"], err_msg=pre + "llr_minmax", **LLR_TOL[dn])
    if j == 0:                               # the Monte-Carlo MI on the reference's slice and N0
        n = int(fx["M%d_mi_slow_n" % M])
        tx = np.asarray(al, np.complex128)[labels]
        got = [ref.mi_mc(rx[m, :n].astype(CT[dn]) - tx[m, :n], al, 1 / fx[pre + "snr"][m]) for m in range(2)]
        _close_where_finite(got, fx[pre + "mi_slow"], GABS[dn], pre + "mi_slow")


@pytest.mark.parametrize("dn", CT)
def test_restatement_reproduces_the_unsynchronised_case(golden, dn):
    """metrics.npz's quarter turn / cyclic shift / swapped modes: the restatement on the reference's own alignment."""
    fx = golden["metrics"]
    M = int(fx["sync_M"])
    al = fx["M%d_%s_coded" % (M, dn)]
    _check(fx, "sync_%s_" % dn, _cx(fx["sync_%s_rx_alignedq" % dn], fx), fx["sync_%s_tx_aligned_label" % dn], al, dn)


def test_restatement_reproduces_the_high_snr_llrs(golden):
    """64-QAM at 25 dB: exact LLRs far beyond fp32's exp range, the reference's double sums still normal."""
    fx = golden["metrics"]
    M, snr = int(fx["hisnr_M"]), 10 ** (float(fx["hisnr_snr_db"]) / 10)
    r0 = _cx(fx["hisnr_rxq"], fx)
    al = fx["M%d_c128_coded" % M]
    np.testing.assert_allclose(ref.llr_exact(r0, al, snr), fx["hisnr_c128_llr"], **LLR_TOL["c128"])
    np.testing.assert_allclose(ref.llr_maxlog(r0, al, snr), fx["hisnr_c128_llr_minmax"], **LLR_TOL["c128"])


def test_restatement_conventions():
    """Labels and alignment as the kernels take them: bit k MSB first, j^rot, lag, trim, ntx, out-of-range labels skipped but
    counted in the SNR estimate's overlap length."""
    assert ref.bit_table(8).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]
    row = np.arange(10) + 0j
    x, t = ref.aligned(row, np.array([0, 1, 2, 3, -1, 5, 6]), 8, rot=1, lag=2, trim=1, ntx=6)
    np.testing.assert_array_equal(x, np.array([2, 3, 4, 5, 7]) * 1j)
    np.testing.assert_array_equal(t, [0, 1, 2, 3, 5])
    assert ref.overlap(10, 6, 2, 1) == 6 and ref.overlap(10, 6, -7, 0) == 0
    assert np.isnan(ref.snr_estimate(np.ones(3, complex), np.array([0, 0, 1]), 4, 3)[0])
