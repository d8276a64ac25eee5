"""The blind signal-quality kernels on the GPU (csrc/blind.hip) against the float64 restatement tests/blind_ref.py and the reference's values
(tests/golden/blind.npz).

Tolerances.
- Moments against the restatement in double on the same samples: rtol 1e-12.  A tree sum of at most 2^22 non-negative doubles plus four roundings
  per term stays below 1e-14 relative; 1e-12 leaves room for any order of combining.  The means of re and im are sums of signed terms: the same
  bound holds relative to the mean of |re| (|im|), so they are compared with that as the absolute tolerance.  S1 and S2 follow from the moments
  by a dozen roundings: rtol 1e-12 against the restatement's formula on the device's own moments, and on the fixture rows against the
  restatement on the samples.
- snr, s0, EVM and the QPSK SNR against the reference's values: the fixture's measured tolerances (tests/golden/gen_golden_blind.py) -
  complex128: 10 x the spread two summation orders give the reference's value; complex64, per quantity: 2 x what the reference's own float32
  arithmetic contributes, which a device that sums in double does not follow.
- ``norm_to_s0_dev``: one division rounded to the row's precision, against a root that may differ by an ulp of double: 2^-51 / 2^-23 relative.
- snr and s0 of the receiver's rows against the restatement: S1 and S2 amplify the moments' 1e-12 by the condition number |gamma k / (gamma k - 1)|,
  k = r2^2 / r4 carries three of them and the quotients add: 1e-12 max(1, 4 x condition).
- The distance sums of complex64 rows against the restatement in double (the receiver test): a coordinate rounded to float moves a squared
  distance d by at most 2 sqrt(d) |p| 2^-24 and the four float operations that form it by 4 d 2^-24; over a row that is at most
  (2 max|p| / evm + 4) 2^-24 relative on the mean, half of it on its root.

Inputs lie on a dyadic grid, so complex64 and complex128 hold the same values; every reference is computed once per case and left unchanged."""
import os

import numpy as np
import pytest

import blind_ref
from conftest import GOLDEN
from qampy_amd import helpers, pipeline, synth, theory
from qampy_amd._lib import DeviceArray
from qampy_amd.core import hip_dsp, signal_quality as sq
from qampy_amd.signals import SignalQAMGrayCoded

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
G = np.load(os.path.join(GOLDEN, "blind.npz"))
CASES = [(int(M), float(db)) for M, db in G["cases"]]
NO_SNR = set(int(M) for M in G["no_snr_M"])
BLOCK = int(G["block"])
SLICE, SLICES = hip_dsp.BLIND_SLICE, hip_dsp.BLIND_SLICES        # samples a workgroup sums before a row is cut; most workgroups per row
RT = 1e-12
_ROWS, _REF = {}, {}


def tol(dt, q):
    return float(G["tol_c128"]) if dt == "c128" else float(G["tol_c64_" + q])


def fixture_rows(c):
    """``(received, known)`` of fixture case c in complex128 (exact in complex64 too)."""
    if c not in _ROWS:
        M = CASES[c][0]
        s = float(G["rx_scale"])
        q = G["c%d_rx" % c].astype(np.float64) / s
        k = np.rint(G["alphabet_%d" % M][G["c%d_idx" % c]].view(np.float64).reshape(-1, 2) * s) / s
        _ROWS[c] = (q[:, 0] + 1j * q[:, 1], k[:, 0] + 1j * k[:, 1])
    return _ROWS[c]


def gamma_of(M):
    """The library's own gamma (held to the reference's by tests/test_blind_host.py): the restatement then repeats the device's formula."""
    return hip_dsp.cal_gamma(M)


def noisy_rows(nrows, L, M=16, seed=0):
    """``nrows`` rows of M-QAM at about 15 dB, scaled by 1.3, on the odd points of the 2^-11 grid: no sample lies on an axis, the branch cut of
    the fourth root, where the sign of a zero decides numpy's side."""
    rng = np.random.default_rng(7 * L + nrows + seed)
    al = theory.cal_symbols_qam(M).ravel() / np.sqrt(theory.cal_scaling_factor_qam(M))
    x = 1.3 * (al[rng.integers(0, M, (nrows, L))] + 0.126 * (rng.standard_normal((nrows, L)) + 1j * rng.standard_normal((nrows, L))))
    return (np.floor(x.real * 1024) + 0.5) / 1024 + 1j * (np.floor(x.imag * 1024) + 0.5) / 1024


def ref_moments(key, E, block=None):
    """The restatement's moments of every row (or block) of E, computed once per key."""
    if key not in _REF:
        _REF[key] = np.array([blind_ref.moments(r) if block is None else blind_ref.block_moments(r, block) for r in E])
    return _REF[key]


def check_moments(got, want, E):
    np.testing.assert_allclose(got[..., :2], want[..., :2], rtol=RT, atol=0)
    scale = np.mean(abs(E.real)) + np.mean(abs(E.imag))
    np.testing.assert_allclose(got[..., 2:], want[..., 2:], rtol=0, atol=RT * scale)


def check_qpsk(got, want):
    """P like a moment; var = P - |mean|^2 within the same bound relative to P; the dB value where var is not all cancellation (var > 1e-6 P: the
    quotient then holds 1e-14 1e6 relative, 4.4e-8 dB)."""
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=RT)
    np.testing.assert_allclose(got[..., 1], want[..., 1], rtol=0, atol=RT * np.max(want[..., 0]))
    ok = want[..., 1] > 1e-6 * want[..., 0]
    np.testing.assert_allclose(got[..., 2][ok], want[..., 2][ok], rtol=0, atol=1e-7)


def stats_of(mom, gamma):
    return np.array([blind_ref.stats(m[0], m[1], gamma) for m in mom.reshape(-1, 4)]).reshape(mom.shape[:-1] + (6,))


# ------------------------------------------------------------------------------------------------ moments, S1, S2
@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("c", range(len(CASES)))
def test_moments_and_S_on_the_fixture_rows(c, dt):
    M = CASES[c][0]
    E = fixture_rows(c)[0]
    want = ref_moments(("fx", c), E[None])
    dE = DeviceArray.from_host(E.astype(CT[dt]))
    mom = hip_dsp.blind_moments_dev(dE).to_host()
    assert mom.shape == (1, 4)
    check_moments(mom, want, E)
    st = hip_dsp.blind_stats_dev(dE, M).to_host()
    assert st.shape == (1, 6)
    np.testing.assert_array_equal(st[:, :2], mom[:, :2])
    np.testing.assert_allclose(st[0, 2:4], blind_ref.stats(want[0, 0], want[0, 1], gamma_of(M))[2:4], rtol=RT)
    np.testing.assert_allclose(st[0, :2], G["c%d_c128_mom" % c], rtol=RT)
    np.testing.assert_allclose(st[0, 2:4], G["c%d_c128_S" % c], rtol=RT)


LENGTHS = [1, 63, 64, 65, 255, 257, SLICE - 1, SLICE + 1, SLICES * SLICE + 1]


@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("i", range(len(LENGTHS)))
def test_reduction_shapes(i, dt):
    """Every length at which the slicing of a row changes, with 1, 2 and 3 rows."""
    L, nrows = LENGTHS[i], 1 + i % 3
    E = noisy_rows(nrows, L)
    want = ref_moments(("len", L, nrows), E)
    dE = DeviceArray.from_host(E.astype(CT[dt]))
    mom = hip_dsp.blind_moments_dev(dE).to_host()
    check_moments(mom, want, E)
    st = hip_dsp.blind_stats_dev(dE, 16).to_host()
    np.testing.assert_allclose(st, stats_of(mom, gamma_of(16)), rtol=RT, equal_nan=True)
    q = hip_dsp.qpsk_blind_snr_dev(dE).to_host()
    check_qpsk(q, [blind_ref.qpsk_snr(r) for r in E])


@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("block", [1, 64, 1000])
def test_blocks(block, dt):
    """Per-block sums; 4500 samples leave a tail of 500 out of the blocks of 1000."""
    L, nrows = 4500, 2
    E = noisy_rows(nrows, L, seed=block)
    want = ref_moments(("blk", block), E, block)
    dE = DeviceArray.from_host(E.astype(CT[dt]))
    mom = hip_dsp.blind_moments_dev(dE, block=block).to_host()
    assert mom.shape == (nrows, L // block, 4)
    check_moments(mom, want, E)
    st = hip_dsp.blind_stats_dev(dE, 16, block=block).to_host()
    assert st.shape == (nrows, L // block, 6)
    np.testing.assert_allclose(st, stats_of(mom, gamma_of(16)), rtol=RT, equal_nan=True)
    if block == 1:
        np.testing.assert_allclose(mom[..., 0] ** 2 / mom[..., 1], 1, rtol=1e-15)        # k = 1 for a single sample
    q = hip_dsp.qpsk_blind_snr_dev(dE, block=block).to_host()
    assert q.shape == (nrows, L // block, 3)
    wq = np.array([[blind_ref.qpsk_snr(r[b * block:(b + 1) * block]) for b in range(L // block)] for r in E])
    check_qpsk(q, wq)


@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_edge_rows(dt):
    """An all-zero row: NaN wherever the formula gives NaN.  A constant-modulus row: k = 1 exactly, S2 = gamma - 1."""
    L = 3000
    rng = np.random.default_rng(3)
    E = np.zeros((3, L), dtype=np.complex128)
    E[1] = 0.5 * (rng.choice([-1, 1], L) + 1j * rng.choice([-1, 1], L))
    E[2] = noisy_rows(1, L)[0]
    dE = DeviceArray.from_host(E.astype(CT[dt]))
    for M in (4, 16):
        st = hip_dsp.blind_stats_dev(dE, M).to_host()
        want = np.array([blind_ref.row_stats(r, gamma_of(M)) for r in E])
        assert np.all(np.isnan(want[0, 2:])) and want[1, 0] ** 2 / want[1, 1] == 1.0
        np.testing.assert_allclose(st, want, rtol=RT, equal_nan=True)
        assert st[1, 0] == 0.5 and st[1, 1] == 0.25 and st[1, 3] == gamma_of(M) * 1.0 - 1
        evm = hip_dsp.blind_evm_dev(dE, M)
        assert np.isnan(evm[0]) and np.isfinite(evm[2])
        out = hip_dsp.norm_to_s0_dev(dE, M, DeviceArray(E.shape, CT[dt])).to_host()
        assert np.all(np.isnan(out[0].real)) and np.all(np.isfinite(out[2]))
    q = hip_dsp.qpsk_blind_snr_dev(dE).to_host()
    assert q[0, 0] == 0 and np.isnan(q[0, 2])
    assert q[1, 0] == 0.5 and abs(q[1, 1]) < 1e-15 and np.isfinite(q[2]).all()      # every point folds onto one: no variance


@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_two_calls_give_the_same_bits(dt):
    E = noisy_rows(2, SLICES * SLICE + 1, M=4)
    dE, dK = DeviceArray.from_host(E.astype(CT[dt])), DeviceArray.from_host(np.roll(E, 1, axis=1).astype(CT[dt]))

    def once():
        st = hip_dsp.blind_stats_dev(dE, 4)
        sums = DeviceArray((2,), np.float64), DeviceArray((2,), np.float64)
        hip_dsp.blind_evm_dev(dE, 4, stats=st, evm_sum=sums[0])
        hip_dsp.blind_evm_dev(dE, 4, known=dK, stats=st, evm_sum=sums[1])
        return [a.to_host() for a in (hip_dsp.blind_moments_dev(dE), st, hip_dsp.blind_moments_dev(dE, block=5000), hip_dsp.qpsk_blind_snr_dev(dE),
                                      sums[0], sums[1])]
    for a, b in zip(once(), once()):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ against the reference's values
@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("c", range(len(CASES)))
def test_estimates_equal_the_reference(c, dt):
    M = CASES[c][0]
    E, K = fixture_rows(c)
    pre = "c%d_%s_" % (c, dt)
    dE, dK = DeviceArray.from_host(E.astype(CT[dt])), DeviceArray.from_host(K.astype(CT[dt]))
    st = hip_dsp.blind_stats_dev(dE, M)
    assert hip_dsp.blind_evm_dev(dE, M, stats=st)[0] == pytest.approx(float(G[pre + "evm"]), rel=tol(dt, "evm"))
    if M in NO_SNR:
        return
    s = st.to_host()[0]
    assert s[4] == pytest.approx(float(G[pre + "snr"]), rel=tol(dt, "snr"))
    assert s[5] == pytest.approx(float(G[pre + "s0"]), rel=tol(dt, "s0"))
    assert hip_dsp.blind_evm_dev(dE, M, known=dK, stats=st)[0] == pytest.approx(float(G[pre + "evmk"]), rel=tol(dt, "evmk"))
    if M == 4:
        assert hip_dsp.qpsk_blind_snr_dev(dE).to_host()[0, 2] == pytest.approx(float(G[pre + "qpsk"]), rel=tol(dt, "qpsk"))
    if c in G["block_cases"]:
        b = hip_dsp.blind_stats_dev(dE, M, block=BLOCK).to_host()[0]
        np.testing.assert_allclose(b[:, 4], G[pre + "bsnr"], rtol=tol(dt, "snr"))
        np.testing.assert_allclose(b[:, 5], G[pre + "bs0"], rtol=tol(dt, "s0"))


@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_method_hip_of_the_module(dt):
    """core.signal_quality with method="hip": a scalar for a row, one value per row for a stack, the reference's values."""
    (a, ka), (b, kb) = fixture_rows(1), fixture_rows(0)
    E, K = np.stack([a, b]).astype(CT[dt]), np.stack([ka, kb]).astype(CT[dt])
    want = lambda q: [float(G["c1_%s_%s" % (dt, q)]), float(G["c0_%s_%s" % (dt, q)])]
    np.testing.assert_allclose(sq.cal_snr_qam(E, 4, method="hip"), want("snr"), rtol=tol(dt, "snr"))
    np.testing.assert_allclose(sq.cal_s0(E, 4, method="hip"), want("s0"), rtol=tol(dt, "s0"))
    np.testing.assert_allclose(sq.cal_evm(E, 4, method="hip"), want("evm"), rtol=tol(dt, "evm"))
    np.testing.assert_allclose(sq.cal_evm(E, 4, known=K, method="hip"), want("evmk"), rtol=tol(dt, "evmk"))
    np.testing.assert_allclose(sq.cal_snr_blind_qpsk(E, method="hip"), want("qpsk"), rtol=tol(dt, "qpsk"))
    one = sq.cal_snr_qam(E[0], 4, method="hip")
    assert np.ndim(one) == 0 and one == sq.cal_snr_qam(E, 4, method="hip")[0]
    n = sq.norm_to_s0(E[0], 4, method="hip")
    assert n.shape == E[0].shape and n.dtype == E.dtype
    np.testing.assert_allclose(n, E[0] / np.sqrt(sq.cal_s0(E[0], 4, method="hip")), rtol=2.0 ** (-23 if dt == "c64" else -51))


@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_norm_to_s0_in_place_and_out_of_place(dt):
    E = noisy_rows(3, SLICE + 1).astype(CT[dt])
    dE = DeviceArray.from_host(E)
    st = hip_dsp.blind_stats_dev(dE, 16)
    out = hip_dsp.norm_to_s0_dev(dE, 16, DeviceArray(E.shape, E.dtype), stats=st).to_host()
    s0 = st.to_host()[:, 5]
    want = E.astype(np.complex128) / np.sqrt(s0)[:, None]
    np.testing.assert_allclose(out, want, rtol=2.0 ** (-23 if dt == "c64" else -51))
    assert np.array_equal(dE.to_host(), E)                                   # the source is untouched
    assert hip_dsp.norm_to_s0_dev(dE, 16, dE, stats=st) is dE
    assert dE.to_host().tobytes() == out.tobytes()
    fresh = DeviceArray.from_host(E)                                         # stats formed inside
    assert hip_dsp.norm_to_s0_dev(fresh, 16, fresh).to_host().tobytes() == out.tobytes()
    # the normalised signal has unit estimated signal power
    np.testing.assert_allclose(hip_dsp.blind_stats_dev(dE, 16).to_host()[:, 5], 1, rtol=1e-6 if dt == "c64" else 1e-14)


# ------------------------------------------------------------------------------------------------ the resident pipeline
def _receiver_case(nch=2):
    from qampy_amd.pipeline import ChannelBank, ResidentReceiver
    M = 16
    sigs = [synth.make_capture(M, 2 ** 14, nmodes=2, snr_db=22, theta=0.5 + 0.1 * c, dgd=20e-12, linewidth=10e3, seed=90 + c, dtype=np.complex64)
            for c in range(nch)]
    kw = dict(methods=("mcma", "sbd"), Niter=(2, 2), Mtestangles=32, Nbps=10)
    L = sigs[0].shape[1]
    bank = ChannelBank(nch, 2, L, 2, M, 15, (2e-3, 5e-4), alphabet=sigs[0].coded_symbols, **kw)
    for c, sg in enumerate(sigs):
        bank.load(c, sg)
    bank.run()
    rxs = []
    for sg in sigs:
        rx = ResidentReceiver(2, L, 2, M, 15, (2e-3, 5e-4), alphabet=sg.coded_symbols, **kw)
        rx.load(sg)
        rx.run()
        rxs.append(rx)
    return M, bank, rxs


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_receiver_and_bank_blind_metrics():
    """``ResidentReceiver.blind_metrics`` equals the kernels on the fetched rows put back on the device bit for bit and the restatement in
    double on those rows within the bounds of the header; ``ChannelBank.blind_metrics(ch)`` equals the single receiver's values bit for bit."""
    M, bank, rxs = _receiver_case()
    gamma, ideal = gamma_of(M), theory.cal_symbols_qam(M).ravel()
    for ch, rx in enumerate(rxs):
        got = rx.blind_metrics(block=2048)
        rows = rx.fetch()["out"]
        assert len(got) == rows.shape[0] == 2
        dR = DeviceArray.from_host(rows)
        st = hip_dsp.blind_stats_dev(dR, M)
        evm = hip_dsp.blind_evm_dev(dR, M, stats=st)
        tr = hip_dsp.blind_stats_dev(dR, M, block=2048).to_host()
        st = st.to_host()
        for i, d in enumerate(got):
            assert set(d) == {"snr", "snr_db", "s0", "evm_blind", "snr_trace", "s0_trace"}
            assert d["snr"] == st[i, 4] and d["s0"] == st[i, 5] and d["evm_blind"] == evm[i] and d["snr_db"] == 10 * np.log10(st[i, 4])
            assert d["snr_trace"].shape == (rows.shape[1] // 2048,) and np.array_equal(d["snr_trace"], tr[i, :, 4], equal_nan=True)
            assert np.array_equal(d["s0_trace"], tr[i, :, 5], equal_nan=True)
            want = blind_ref.row_stats(rows[i], gamma)
            cond = abs(gamma * want[0] ** 2 / want[1] / want[3])
            assert d["snr"] == pytest.approx(want[4], rel=RT * max(1., 4 * cond)) and d["s0"] == pytest.approx(want[5], rel=RT * max(1., 4 * cond))
            e = blind_ref.evm(rows[i], ideal, gamma)
            pmax = np.max(abs(rows[i])) / np.sqrt(want[5])
            assert d["evm_blind"] == pytest.approx(e, rel=(2 * pmax / e + 4) * 2.0 ** -24)
            assert np.isfinite(d["evm_blind"]) and d["evm_blind"] > 0
        assert set(rx.blind_metrics()[0]) == {"snr", "snr_db", "s0", "evm_blind"}
        for a, b in zip(bank.blind_metrics(ch, block=2048), got):
            _same(a, b)


def test_blind_metrics_of_qpsk_rows():
    """The row function behind both ``blind_metrics`` on QPSK rows: ``snr_qpsk_db`` appears, every value is the reference's."""
    (a, _), (b, _) = fixture_rows(1), fixture_rows(2)
    got = pipeline._blind_metrics(DeviceArray.from_host(np.stack([a, b]).astype(np.complex64)), 4, BLOCK, {})
    for d, c in zip(got, (1, 2)):
        pre = "c%d_c64_" % c
        assert d["snr"] == pytest.approx(float(G[pre + "snr"]), rel=tol("c64", "snr")) and d["s0"] == pytest.approx(float(G[pre + "s0"]), rel=tol("c64", "s0"))
        assert d["evm_blind"] == pytest.approx(float(G[pre + "evm"]), rel=tol("c64", "evm"))
        assert d["snr_qpsk_db"] == pytest.approx(float(G[pre + "qpsk"]), rel=tol("c64", "qpsk"))
        assert d["snr_trace"].shape == d["s0_trace"].shape == (a.size // BLOCK,)
    np.testing.assert_allclose(got[0]["snr_trace"], G["c1_c64_bsnr"], rtol=tol("c64", "snr"))


# ------------------------------------------------------------------------------------------------ SignalQAM.normalize_and_center
@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_normalize_and_center(dt):
    sig = SignalQAMGrayCoded(16, 2 ** 12, nmodes=2, dtype=CT[dt])
    rng = np.random.default_rng(11)
    noisy = sig * 0.4 + 0.05 * (rng.standard_normal(sig.shape) + 1j * rng.standard_normal(sig.shape)) + (0.3 - 0.1j)
    noisy = sig.recreate_from_np_array(np.asarray(noisy).astype(CT[dt]))
    want = helpers.normalise_and_center(np.asarray(noisy).astype(np.complex128))
    plain = noisy.copy()
    assert plain.normalize_and_center() is None
    np.testing.assert_allclose(np.asarray(plain), want, rtol=0, atol=(2.0 ** -23 if dt == "c64" else 1e-14) * np.max(abs(want)))
    based = noisy.copy()
    centred = np.asarray(noisy) - np.asarray(noisy).mean(axis=-1)[:, None]
    p = noisy.recreate_from_np_array(centred).est_snr(synced=False, verbose=True)[1]
    based.normalize_and_center(symbol_based=True)
    np.testing.assert_allclose(np.asarray(based), centred / np.sqrt(p)[:, None], rtol=1e-6 if dt == "c64" else 1e-13)
    assert based.dtype == plain.dtype == CT[dt]
