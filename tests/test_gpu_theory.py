"""The theory kernels on the GPU: the Monte-Carlo GMI / MI of csrc/metrics.hip (awgn_mc_kernel, awgn_mc_noise_kernel) and the shaped source of
csrc/source.hip (ps_symbols_kernel), against the reference's values (tests/golden/theory.npz) and the float64 restatement (tests/theory_ref.py,
itself held to the reference by tests/test_theory_ref.py).

Tolerances.  GMI per bit and MI: ``test_gpu_metrics_edges.TOL[dn]["info"]`` - 1e-10 (complex128) / 1e-5 (complex64), the bar of the resident
metrics, whose sums these are (means of O(1) terms computed in the row's precision and added in double); the total GMI is a sum of nbits such
means, so its bar is nbits times that.  Draws: the bars of tests/test_gpu_impair.py for the same Box-Muller - 8 * 2^-52 r per complex128 draw (the
scale sqrt(1 / (2 snr)) adds one rounding of the product here and one of the test's division, 2^-52 r together, to the 4 * 2^-52 r derived there),
4 * C64_DRAW_DEVIATION for complex64 (the test divides by the float32 scale the device multiplied by).  The shaped source is integer work and
table look-ups: exact.

Inputs of the parity tests against the restatement lie on a 2^-10 grid, so complex64 and complex128 hold the same values and share one
reference, computed once per case and left unchanged."""
import os

import numpy as np
import pytest

import impair_ref as ir
import theory_ref as tr
from conftest import GOLDEN
from qampy_amd import synth, theory
from qampy_amd._lib import DeviceArray
from qampy_amd.core import hip_dsp
from test_gpu_impair import BAR, C64_DRAW_DEVIATION
from test_gpu_metrics_edges import TOL

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
G = np.load(os.path.join(GOLDEN, "theory.npz"))
CASES = [(int(M), int(ns), float(db)) for M, ns, db in G["mc_cases"]]
TILE = hip_dsp.MC_TILE             # (sent point, draw) pairs of one workgroup: 256
TRIP = hip_dsp.MC_TRIP             # pairs the capped grid covers before it loops: 1024 workgroups
GRID = 2.0 ** -10
_REF = {}


def on_grid(x):
    return np.round(np.asarray(x) / GRID) * GRID


def synthetic(nb, seed=0):
    """2^nb random points near unit power on the 2^-10 grid, all distinct; the label is the index"""
    rng = np.random.default_rng(1000 * nb + seed)
    M = 1 << nb
    while True:
        al = rng.standard_normal(M) + 1j * rng.standard_normal(M)
        al = on_grid(al / np.sqrt(np.mean(np.abs(al) ** 2)))
        if np.unique(al).size == M:
            return al


def draws(ns, snr_db, seed):
    rng = np.random.default_rng(seed)
    return on_grid(10 ** (-snr_db / 20) * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) / np.sqrt(2))


def restated(key, al, snr, z):
    """[gmi, mi, per bit ...] of the restatement, computed once per key"""
    if key not in _REF:
        gmi, per_bit, mi = tr.gmi_mc(al, snr, z)
        _REF[key] = np.concatenate([[gmi, mi], per_bit])
        _REF[key].setflags(write=False)
    return _REF[key]


def device(al, snr, z, ct):
    """(nsnr, 2 + nbits) of the kernel for explicit draws z (nsnr, ns)"""
    z = np.atleast_2d(z)
    return hip_dsp.awgn_mc(np.ascontiguousarray(al, dtype=ct), snr, z.shape[1], noise=z)


def check(got, want, dn, what="", extra=0.0):
    """extra: what the size of the exponents adds to the bar (test_far_outliers_in_complex128), 0 for terms of O(1)"""
    nb = want.size - 2
    tol = TOL[dn]["info"] + extra
    print(what, dn, "gmi %.3g  mi %.3g  per bit %.3g" % (abs(got[0] - want[0]), abs(got[1] - want[1]), np.abs(got[2:] - want[2:]).max()))
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got[2:], want[2:], rtol=0, atol=tol, err_msg="gmi per bit " + what)
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=tol, err_msg="mi " + what)
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=nb * tol, err_msg="gmi " + what)


def bit_map_of(al):
    """the reference's (nbits, M / 2, 2) map of an alphabet in label order"""
    nb = tr.nbits(al.size)
    g = np.arange(al.size)
    return np.stack([np.stack([al[((g >> (nb - 1 - k)) & 1) == b] for b in (0, 1)], axis=-1) for k in range(nb)])


# ------------------------------------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("c", range(len(CASES)))
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_explicit_noise_against_the_reference(dn, c):
    M, ns, db = CASES[c]
    ct, nb, snr = CT[dn], tr.nbits(M), 10 ** (db / 10)
    bm, z = G["bitmap_%d" % M], G["mc%d_z" % c]
    gmi = hip_dsp.cal_gmi_mc(G["coded_%d" % M].astype(ct), snr, ns, bm, noise=z)
    al = hip_dsp.bits_map_labels(bm)
    out = device(al, snr, z, ct)[0]
    want = restated(("gold", c), al, snr, z)
    print(dn, M, "gmi - reference %.3g, mi - reference %.3g" % (gmi - float(G["mc%d_gmi" % c]), out[1] - float(G["mc%d_mi" % c])))
    assert isinstance(gmi, float) and gmi == out[0]
    np.testing.assert_allclose(gmi, float(G["mc%d_gmi" % c]), rtol=0, atol=nb * TOL[dn]["info"])
    np.testing.assert_allclose(out[1], float(G["mc%d_mi" % c]), rtol=0, atol=TOL[dn]["info"])
    check(out, want, dn, "golden case %d" % c)
    np.testing.assert_allclose(out[2:].sum(), out[0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("nb", range(1, 11))
def test_every_bit_width(nb, ns):
    al, db = synthetic(nb), 3.0 * nb
    z = draws(ns, db, 77 + nb)
    want = restated(("nb", nb, ns), al, 10 ** (db / 10), z)
    for dn, ct in CT.items():
        check(device(al, 10 ** (db / 10), z, ct)[0], want, dn, "nbits %d ns %d" % (nb, ns))


@pytest.mark.parametrize("nb,ns", [(1, TILE // 2 - 1), (1, TILE // 2), (1, TILE // 2 + 1), (3, TILE // 8 + 1), (1, TRIP // 2 - 1), (1, TRIP // 2),
                                   (1, TRIP // 2 + 1), (4, TRIP // 16 + 3), (1, TRIP + 5)])
def test_launch_geometry(nb, ns):
    """M ns one draw below, at and one draw above a workgroup's tile of TILE = 256 (point, draw) pairs; around one trip of the capped grid
    (TRIP = 1024 tiles) and beyond two."""
    al, db = synthetic(nb, seed=1), 4.0 + 2 * nb
    z = draws(ns, db, ns)
    want = restated(("geom", nb, ns), al, 10 ** (db / 10), z)
    for dn, ct in CT.items():
        check(device(al, 10 ** (db / 10), z, ct)[0], want, dn, "M ns = %d" % (ns << nb))


@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("nsnr", [1, 2, 7])
def test_multi_snr_launch_equals_per_point_launches(nsnr, dn):
    ct, ns = CT[dn], 100
    al = np.ascontiguousarray(theory.coded_symbols_qam(16, dtype=ct))
    snr = 10 ** (np.linspace(2, 20, nsnr) / 10)
    out, z = hip_dsp.awgn_mc(al, snr, ns, seed=11, return_noise=True)
    assert out.shape == (nsnr, 6) and z.shape == (nsnr, ns) and z.dtype == ct
    for p in range(nsnr):
        assert np.array_equal(hip_dsp.awgn_mc(al, snr[p], ns, noise=z[p])[0], out[p]), p
    if nsnr > 1:
        assert not np.array_equal(z[0] * np.sqrt(snr[0]), z[1] * np.sqrt(snr[1]))          # every point has draws of its own


def test_snr_points_beyond_one_batch_of_partials():
    """The workgroup partials of one batch are capped at 2^22 doubles: 1024-QAM with a full grid (1025 x 11 doubles per point) takes 372 points a
    batch.  400 points: those either side of the seam and the last one equal their own single-point launches bit for bit."""
    al = np.ascontiguousarray(theory.coded_symbols_qam(1024, dtype=np.complex64))
    ns, nsnr = TRIP // 1024, 400
    per_batch = 2 ** 22 // ((TRIP // TILE + 1) * 11)
    assert per_batch == 372 < nsnr
    snr = 10 ** (np.linspace(10, 30, nsnr) / 10)
    out, z = hip_dsp.awgn_mc(al, snr, ns, seed=21, return_noise=True)
    assert out.shape == (nsnr, 12) and np.all(np.isfinite(out))
    for p in (0, per_batch - 1, per_batch, nsnr - 1):
        assert np.array_equal(hip_dsp.awgn_mc(al, snr[p], ns, noise=z[p])[0], out[p]), p


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("ns", [1, TILE - 1, TILE, TILE + 1, 1000])
def test_draws_against_the_restatement(ns, dn):
    ct, seed = CT[dn], 4321 + ns
    snr = np.array([0.5, 10 ** 0.6, 10 ** 2.2])
    Z = DeviceArray((snr.size, ns), ct)
    hip_dsp.awgn_mc_noise_dev(Z, snr, seed)
    z = Z.to_host().astype(np.complex128)
    worst = 0.0
    for p in range(snr.size):
        g0, g1, r = ir.gauss(seed, p, np.arange(ns), tr.STREAM_MC, dn == "c128")
        sigma = np.sqrt(1.0 / (2.0 * snr[p]))
        g = z[p] / (sigma if dn == "c128" else np.float64(np.float32(sigma)))
        d = np.maximum(np.abs(g.real - g0), np.abs(g.imag - g1))
        worst = max(worst, d.max())
        if dn == "c128":
            assert np.all(d <= 8 * 2.0 ** -52 * r), (p, d.max())
        else:
            assert d.max() <= 4 * C64_DRAW_DEVIATION, (p, d.max())
    print("draw deviation", dn, ns, worst)


@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_seeded_run_equals_explicit_run_and_repeats(dn):
    ct, ns = CT[dn], 300
    al = np.ascontiguousarray(theory.coded_symbols_qam(64, dtype=ct))
    snr = 10 ** (np.array([5., 14.]) / 10)
    a, z = hip_dsp.awgn_mc(al, snr, ns, seed=2024, return_noise=True)
    b = hip_dsp.awgn_mc(al, snr, ns, seed=2024)
    assert np.array_equal(a, b)                                                       # a repeated call: the same bits
    assert np.array_equal(hip_dsp.awgn_mc(al, snr, ns, noise=z), a)                   # the seeded run is the explicit run on its draws
    c, z2 = hip_dsp.awgn_mc(al, snr, ns, seed=2025, return_noise=True)
    assert not np.array_equal(z, z2) and not np.array_equal(a, c)
    bm = bit_map_of(al)
    assert hip_dsp.cal_gmi_mc(al, snr[0], ns, bm, seed=2024) == a[0, 0]
    assert hip_dsp.cal_gmi_mc(al, snr[0], ns, bm) != hip_dsp.cal_gmi_mc(al, snr[0], ns, bm)      # seed=None: fresh draws


# ------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("what", ["40dB", "-10dB", "outlier"])
def test_range(what, dn):
    """64-QAM at 40 dB and at -10 dB on seeded draws, and at 15 dB with one draw of modulus 10: finite, and the restatement's value."""
    ct, ns = CT[dn], 64
    al = np.ascontiguousarray(theory.coded_symbols_qam(64, dtype=ct))
    db = {"40dB": 40.0, "-10dB": -10.0, "outlier": 15.0}[what]
    snr = 10 ** (db / 10)
    if what == "outlier":
        z = draws(ns, db, 5).astype(ct)
        z[17] = ct(10 * np.exp(0.3j))
        out = device(al, snr, z, ct)[0]
    else:
        o, z = hip_dsp.awgn_mc(al, snr, ns, seed=99, return_noise=True)
        out, z = o[0], z[0]
    want = restated(("range", what, dn), al, snr, z)
    assert np.all(np.isfinite(want))
    check(out, want, dn, what)


def test_far_outliers_in_complex128():
    """The per-side shifts in double, well inside their range: 64-QAM at 30 dB with draws of modulus 10 and 100 - exponents of 10^5 and 10^6 between
    the sides' nearest points, where sums about the global minimum are 0 in any format.  complex128 only: a float32 distance of 10^2 .. 10^4 carries
    4e-6 .. 5e-4 absolute, times snr log2 e = 1443 that is far beyond the complex64 bar for those draws, whatever the kernel does.

    The bar.  The terms are no longer O(1): a term is a difference of exponents E = snr log2(e) |y - s|^2 of up to E_max = 1.5e7 here, and in
    double each exponent carries about four roundings of its own size (the two squares and their sum, the product with snr log2 e), on the device
    and in the restatement alike: 8 * 2^-53 E_max, about 1.3e-8, is added to the bar of the O(1) terms.  The mean over the draws would allow less
    (two of sixteen draws are large); no credit is taken for it.  A wrong shift shows as an infinity or an error of the order of the terms."""
    al = np.ascontiguousarray(theory.coded_symbols_qam(64))
    snr = 10 ** 3.0
    z = draws(16, 30.0, 6)
    z[3], z[11] = 10 * np.exp(-1.1j), 100 * np.exp(2.5j)
    want = restated(("far",), al, snr, z)
    assert np.all(np.isfinite(want))
    e_max = snr * np.log2(np.e) * np.max(np.abs(al[:, None] + np.conj(z)[None, :]) + np.abs(al).max()) ** 2
    check(device(al, snr, z, np.complex128)[0], want, "c128", "far outliers", extra=8 * 2.0 ** -53 * e_max)


@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_qpsk_gmi_equals_mi(dn):
    """For Gray-labelled QPSK the bit sides factor the sum over the alphabet, so GMI = MI on every realisation."""
    ct = CT[dn]
    al = np.ascontiguousarray(theory.coded_symbols_qam(4, dtype=ct))
    out = hip_dsp.awgn_mc(al, 10 ** (np.array([-5., 5., 15., 30.]) / 10), 200, seed=8)
    print(dn, np.abs(out[:, 0] - out[:, 1]).max())
    np.testing.assert_allclose(out[:, 0], out[:, 1], rtol=0, atol=3 * TOL[dn]["info"])      # the GMI's bar (2 bits) plus the MI's


# ------------------------------------------------------------------------------------------------ host layer
def test_cal_gmi_end_to_end():
    g, per_bit = theory.cal_gmi(16, [8, 12], N=64, seed=5, per_bit=True)
    assert g.shape == (2,) and per_bit.shape == (2, 4) and g.dtype == np.float64
    al = theory.coded_symbols_qam(16)
    lin = 10 ** (np.array([8., 12.]) / 10)
    Z = DeviceArray((2, 64), np.complex128)
    hip_dsp.awgn_mc_noise_dev(Z, lin, 5)
    z = Z.to_host()
    for p in range(2):
        assert hip_dsp.cal_gmi_mc(al, lin[p], 64, bit_map_of(al), noise=z[p]) == g[p]
    assert np.array_equal(theory.cal_gmi(16, [8, 12], N=64, seed=5), g)
    assert theory.cal_gmi(16, 8, N=64, seed=5)[0] == g[0] and 0 < g[0] < g[1] < 4


def test_sim_mi_mc_on_the_device():
    al = theory.coded_symbols_qam(16)
    lin = 10 ** (np.array([6., 12.]) / 10)
    mi = theory.sim_mi_mc(2 * al, [6., 12.], 64, seed=3)
    assert np.array_equal(mi, hip_dsp.awgn_mc(al / np.sqrt(np.mean(abs(al) ** 2)), lin, 64, seed=3)[:, 1])
    assert theory.sim_mi_mc(al, 6., 64, seed=3) == mi[0]
    # an alphabet that is no power of two: the same draws through cal_mi_mc
    psk = theory.cal_symbols_psk(12)
    got = theory.sim_mi_mc(psk, 9., 50, seed=3)
    Z = DeviceArray((1, 50), np.complex128)
    hip_dsp.awgn_mc_noise_dev(Z, [10 ** 0.9], 3)
    z = Z.to_host()[0]
    d = psk[:, None] - psk[None, :]
    e = -(np.abs(d[:, None, :]) ** 2 + 2 * np.real(d[:, None, :] * z[None, :, None])) * 10 ** 0.9
    want = np.log2(12) - np.mean(np.log2(np.sum(np.exp(e), axis=-1)))
    np.testing.assert_allclose(got, want, rtol=0, atol=TOL["c128"]["info"])


# ------------------------------------------------------------------------------------------------ shaped source
PS_NS = [1, hip_dsp.PS_TILE - 1, hip_dsp.PS_TILE, hip_dsp.PS_TILE + 1, 3 * hip_dsp.PS_TILE + 5]


@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("nmodes", [1, 2, 3])
def test_shaped_source_equals_the_restatement(nmodes, dn):
    ct, M, nu = CT[dn], 64, 0.05
    table = theory.gray_code_qam(M).reshape(8, 8)
    for N in PS_NS:
        seed = 31 * N + nmodes
        s = synth.make_ps_symbols_dev(M, nu, N, nmodes=nmodes, seed=seed, dtype=ct)
        sym, idx, al = s["symbols"].to_host(), s["idx_tx"].to_host(), s["alphabet"].to_host()
        assert sym.shape == (nmodes, N) and sym.dtype == ct and idx.dtype == np.int32 and np.array_equal(al, s["alphabet_host"]) and s["M"] == M
        np.testing.assert_allclose(np.sum(s["px"][:, None] * s["px"][None, :] * np.abs(s["levels"][:, None] + 1j * s["levels"][None, :]) ** 2), 1, rtol=1e-14)
        assert np.array_equal(al[idx], sym)
        for m in range(nmodes):
            i, q = tr.shaped_indices(seed, m, np.arange(N), s["px"])
            assert np.array_equal(idx[m], table[i, q]), (N, m)
            assert np.array_equal(sym[m], (s["levels"][i] + 1j * s["levels"][q]).astype(ct)), (N, m)
    # the coded alphabet of the uniform source, rescaled: same points, same labels
    np.testing.assert_allclose(al / np.sqrt(np.mean(np.abs(al) ** 2)), theory.coded_symbols_qam(M), rtol=1e-6 if dn == "c64" else 1e-14)


def test_generate_ps_symbols_on_the_device():
    lev, px = theory.cal_ps_probablts(theory.coded_symbols_qam(64), 2.0)
    raw = theory.generate_ps_symbols(3000, lev, px, normalize=False, seed=12, method="hip")
    i, q = tr.shaped_indices(12, 0, np.arange(3000), px)
    assert raw.shape == (3000,) and raw.dtype == np.complex128 and np.array_equal(raw, lev[i] + 1j * lev[q])
    x = theory.generate_ps_symbols((3, 5000), lev, px, normalize=True, seed=12, method="hip")
    assert x.shape == (3, 5000)
    print(np.abs(x.mean(axis=-1)).max(), np.abs(np.mean(np.abs(x) ** 2, axis=-1) - 1).max())
    assert np.abs(x.mean(axis=-1)).max() <= BAR[np.complex128] and np.abs(np.mean(np.abs(x) ** 2, axis=-1) - 1).max() <= BAR[np.complex128]
    assert np.array_equal(x, theory.generate_ps_symbols((3, 5000), lev, px, normalize=True, seed=12, method="hip"))
