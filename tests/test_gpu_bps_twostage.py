"""
The device-resident two-stage blind phase search (``method="fused"``, ``hip_dsp.bps_twostage_recover[_dev]``, ``ResidentReceiver(Bbps=..)``)
on a real MI355X: against the vectors captured from the reference, against the composed path (``method="pyt"``) on drifting inputs
whose ``4 ph`` wraps several times, at the edges of a row, through the resident receiver and the channel bank, and its rejections.
"""
import numpy as np
import pytest

from conftest import CT, RT, TOL, golden_cases
from oracle import oracle
import qampy_amd
from qampy_amd import synth, theory, _lib
from qampy_amd.signals import SignalQAM
from qampy_amd.core import hip_dsp, phaserecovery as core_ph

pytestmark = pytest.mark.gpu

D = _lib.DeviceArray

# Largest |np.unwrap(4 sel) / 4 in the array's dtype - the same in float64| over the selected angles `sel` of every case of CASES below,
# measured on the CPU with the oracle standing in for the index kernels (the composed path, whose host unwrap the bar belongs to), whole
# quarter turns set aside (case M64 L257 N20 A16 B4 holds a jump of 4 ph that float32 sees on the other side of pi than float64 does):
# float32 1.04e-6 - the running correction is rounded once per wrap, on phases of up to 12 rad; float64 identically 0.
# The bar on fused - composed is twice that, or 1e-6 if that is larger.
UNWRAP_HOST_ERR = {"c64": 1.04e-6, "c128": 0.}
PH_BAR = {dn: max(2 * v, 1e-6) for dn, v in UNWRAP_HOST_ERR.items()}
EPS = {"c64": 2. ** -24, "c128": 2. ** -53}


def tie_bound(dn, N, sums, emax):
    """How far apart the float64 window sums of two fine angles may lie for the two paths to order them differently.  Both paths sum the
    same rounded distances in another order: direct + sliding sums of at most ~300 terms, 300 eps relative.  The float64 sums they are
    judged by here differ from the sums of the rounded distances by at most 2N distance errors of 8 eps (|E| + 1)^2 each, per sum."""
    return 300 * EPS[dn] * sums + 2 * (2 * N) * 8 * EPS[dn] * (emax + 1) ** 2


DIFF_CAP = {"c64": 1e-2, "c128": 2e-3}          # share of samples that may differ: the bar of test_bps_twostage_on_gpu


def _close(a, b, dn):
    np.testing.assert_allclose(a, b, rtol=TOL[dn]["rtol"], atol=TOL[dn]["atol"])


def drifting_rows(M, L, nmodes, dn, seed, wraps=5.0, snr_db=None):
    """``nmodes`` rows of ``L`` noisy M-QAM symbols under a Wiener phase walk plus a slope that carries the phase over ``wraps`` quarter turns
    in the row (so that ``4 ph`` wraps about that often).  Returns ``(E, alphabet)`` in the dtype ``dn``."""
    rng = np.random.default_rng(seed)
    alphabet = theory.coded_symbols_qam(M, dtype=np.complex128)
    s = alphabet[rng.integers(0, M, size=(nmodes, L))]
    snr_db = {4: 14., 16: 22., 32: 25., 64: 28.}[M] if snr_db is None else snr_db
    s = s + 10 ** (-snr_db / 20) * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape)) / np.sqrt(2)
    walk = np.cumsum(rng.normal(scale=0.01, size=(nmodes, L)), axis=1)
    slope = wraps * (np.pi / 2) / max(L, 1) * np.arange(L) * (1 + 0.3 * np.arange(nmodes)[:, None])
    return np.ascontiguousarray((s * np.exp(-1j * (walk + slope))).astype(CT[dn])), alphabet.astype(CT[dn])


def fused_dev(E, A, B, alphabet, N):
    """``hip_dsp.bps_twostage_recover_dev`` on host arrays: everything it leaves in HBM."""
    rt = E.real.dtype
    dE, dsy, dang = D.from_host(E), D.from_host(alphabet), D.from_host(hip_dsp.test_angle_grid(A, rt))
    idx1, idx2, ph, out = D(E.shape, np.int32), D(E.shape, np.int32), D(E.shape, rt), D(E.shape, E.dtype)
    hip_dsp.bps_twostage_recover_dev(dE, A, B, dsy, N, idx1, idx2, ph, out, angles=dang)
    _lib.sync()
    return dict(idx1=idx1.to_host(), idx2=idx2.to_host(), ph=ph.to_host(), out=out.to_host())


def fine_table(A, B, rt):
    return (hip_dsp.test_angle_grid(A, rt)[0].astype(np.float64)[:, None] + hip_dsp.twostage_offsets(A, B)[None, :]).astype(rt)


def composed(row, A, B, alphabet, N):
    """The composed path of core/phaserecovery.py:48-53 for one row, step by step, keeping what it selects on the way."""
    rt = row.real.dtype
    coarse = hip_dsp.test_angle_grid(A, rt)
    idx1 = hip_dsp.bps(row, coarse, alphabet, N)
    first = hip_dsp.select_angles(np.copy(coarse), idx1)
    steps = np.linspace(-B / 2, B / 2, B)
    fine = (first[:, np.newaxis] + steps[np.newaxis, :] / (B * A) * np.pi / 2).astype(rt)
    idx2 = hip_dsp.bps(row, fine, alphabet, N)
    second = hip_dsp.select_angles(np.copy(fine), idx2)
    return dict(idx1=idx1, idx2=idx2, fine=fine, second=second, ph=np.unwrap(second * 4, discont=np.pi) / 4)


def window_sums64(row, fine, alphabet, N):
    """Second-stage window sums in float64 with the limits of the per-symbol-grid branch (rows i - N + 1 .. i + N for N <= i < L - N):
    ``(L, B)``, rows outside the interior NaN."""
    x = row.astype(np.complex128)[:, None] * np.exp(1j * fine.astype(np.float64))
    d = np.minimum((np.abs(x[:, :, None] - alphabet.astype(np.complex128)[None, None, :]) ** 2).min(axis=2), 100.)
    L = row.size
    c = np.vstack([np.zeros((1, d.shape[1])), np.cumsum(d, axis=0)])
    out = np.full(d.shape, np.nan)
    i = np.arange(N, L - N)
    if i.size:
        out[i] = c[i + N + 1] - c[i - N + 1]
    return out


# ------------------------------------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("case", golden_cases("twostage"), ids=lambda c: c["name"])
def test_fused_matches_the_reference_vectors(golden, case):
    g = golden["twostage"]
    dn = case["dtype"]
    A, N, B = case["A"], case["N"], case["B"]
    E = g[case["base"] + "__E"].astype(CT[dn])
    sig = SignalQAM(E, case["M"], coded_symbols=g[case["base"] + "__alphabet"].astype(CT[dn]))
    Eout, ph = qampy_amd.phaserec.bps_twostage(sig, A, N, B=B, method="fused")
    assert type(Eout) is SignalQAM and Eout.dtype == CT[dn] and ph.dtype == RT[dn] and ph.shape == E.shape
    e1, p1 = core_ph.bps_twostage(E[0], A, sig.coded_symbols, N, B=B, method="fused")
    assert e1.ndim == 1 and p1.ndim == 1 and type(e1) is np.ndarray
    step = np.pi / 2 / A
    for got, ref in ((ph, g[case["name"] + "__ph"]), (p1, g[case["name"] + "__ph1d"])):
        bad = np.abs(got - ref) > 1e-6
        print(case["name"], "share of samples off the reference by more than 1e-6:", bad.mean())
        assert bad.mean() < DIFF_CAP[dn]
        assert np.all(np.abs(np.angle(np.exp(4j * (got - ref))) / 4) <= 1.01 * step)
    _close(np.asarray(Eout), E * np.exp(1j * ph), dn)
    _close(e1, E[0] * np.exp(1j * p1), dn)


# ------------------------------------------------------------------------------------------------ 2. fused against composed
# (M, L, N, A, B, nmodes): every L of {2N, 2N + 1, 257, 4096 + 3}, N of {1, 8, 20}, (A, B) of {(8, 1), (8, 2), (16, 4), (32, 6), (64, 64)},
# M of {4, 16, 64} + 32-QAM (cross), nmodes of {1, 2, 3} occurs; 4099 symbols are 9 runs of 512 and five unwrap chunks of 1024
CASES = [
    (16, 2, 1, 8, 1, 1), (4, 3, 1, 8, 2, 2), (16, 16, 8, 16, 4, 1), (64, 17, 8, 32, 6, 3), (16, 40, 20, 16, 4, 2), (4, 41, 20, 64, 64, 1),
    (4, 257, 1, 8, 1, 3), (16, 257, 8, 8, 2, 2), (64, 257, 20, 16, 4, 1), (32, 257, 8, 32, 6, 2), (4, 257, 8, 64, 64, 1),
    (16, 4099, 20, 16, 4, 3), (64, 4099, 8, 32, 6, 1), (32, 4099, 20, 8, 2, 2), (4, 4099, 1, 16, 4, 2), (16, 4099, 8, 64, 64, 1),
]


@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("M,L,N,A,B,nmodes", CASES)
def test_fused_equals_composed_on_drifting_phase(M, L, N, A, B, nmodes, dn):
    E, alphabet = drifting_rows(M, L, nmodes, dn, seed=1000 + 7 * L + A + B + M)
    rt = RT[dn]
    f = fused_dev(E, A, B, alphabet, N)
    Ec, phc = core_ph.bps_twostage(E, A, alphabet, N, B=B, method="pyt")
    Ef, phf = core_ph.bps_twostage(E, A, alphabet, N, B=B, method="fused")
    assert np.array_equal(phf, f["ph"]) and np.array_equal(Ef, f["out"])           # the host wrapper is the device call
    _close(f["out"], E * np.exp(1j * f["ph"]), dn)
    table = fine_table(A, B, rt)
    ndiff = nwrap = 0
    worst_ph = worst_host = 0.
    for m in range(nmodes):
        c = composed(E[m], A, B, alphabet, N)
        assert np.array_equal(c["ph"].astype(rt), phc[m])                           # the replica IS the composed path
        assert np.array_equal(f["idx1"][m], c["idx1"])                              # coarse stage: the same kernel on the same data
        assert np.array_equal(c["fine"], table[c["idx1"]])                          # the table row a symbol looks up is its fine grid
        # the oracle in float64 on the same inputs: no exact ties, and its indices are the arg-min of the float64 sums up to near-ties
        w = window_sums64(E[m], c["fine"], alphabet, N)
        inner = np.arange(N, L - N)
        if inner.size and B > 1:
            two = np.sort(w[inner], axis=1)[:, :2]
            assert np.all(two[:, 1] > two[:, 0]), "exact tie of the two best float64 window sums"
            o2 = oracle.bps(np.ascontiguousarray(E[m].astype(np.complex128)), np.ascontiguousarray(c["fine"].astype(np.float64)),
                            alphabet.astype(np.complex128), N)
            off = np.flatnonzero(o2[inner] != np.argmin(w[inner], axis=1)) + N
            assert np.all(w[off, o2[off]] - np.nanmin(w[off], axis=1) <= 1e-9 * np.nanmin(w[off], axis=1))
        # fine stage: the composed path's indices except at near-ties
        differ = np.flatnonzero(f["idx2"][m] != c["idx2"])
        assert np.all((differ >= N) & (differ < L - N))                             # never at the edges
        if differ.size:
            a, b = w[differ, f["idx2"][m][differ]], w[differ, c["idx2"][differ]]
            assert np.all(np.abs(a - b) <= tie_bound(dn, N, np.maximum(a, b), np.abs(E[m]).max())), (differ[:8], a[:8], b[:8])
        ndiff += differ.size
        # phases where the indices agree: same wrap count, values within the host unwrap's own rounding
        same = f["idx2"][m] == c["idx2"]
        assert np.all(np.round((f["ph"][m][same] - c["ph"][same]) / (np.pi / 2)) == 0)
        worst_ph = max(worst_ph, float(np.abs(f["ph"][m][same].astype(np.float64) - c["ph"][same].astype(np.float64)).max()))
        dh = c["ph"].astype(np.float64) - np.unwrap(c["second"].astype(np.float64) * 4, discont=np.pi) / 4
        worst_host = max(worst_host, float(np.abs(dh - np.round(dh / (np.pi / 2)) * (np.pi / 2)).max()))
        nwrap += int(np.count_nonzero(np.abs(np.diff(c["second"].astype(np.float64) * 4)) >= np.pi))
    print("M%d L%d N%d A%d B%d nm%d %s: fine indices differing %d of %d, wraps %d, |fused - composed| %.3g (bar %.3g), host unwrap vs float64 %.3g"
          % (M, L, N, A, B, nmodes, dn, ndiff, nmodes * L, nwrap, worst_ph, PH_BAR[dn], worst_host))
    assert ndiff <= DIFF_CAP[dn] * nmodes * L
    assert worst_ph <= PH_BAR[dn]
    if L >= 257:
        assert nwrap >= 3 * nmodes, "the drift does not wrap 4 ph three times per row"


# ------------------------------------------------------------------------------------------------ 3. edge rule
@pytest.mark.parametrize("dn", ["c64", "c128"])
def test_edges_keep_index_zero_and_carry_the_wrap(dn):
    L, N, A, B, M = 64, 8, 16, 4, 16
    rt = RT[dn]
    E, alphabet = drifting_rows(M, L, 1, dn, seed=5, wraps=3.0)
    f = fused_dev(E, A, B, alphabet, N)
    c = composed(E[0], A, B, alphabet, N)
    assert np.array_equal(f["idx2"][0][:N], c["idx2"][:N]) and np.array_equal(f["idx2"][0][-N:], c["idx2"][-N:])
    assert not f["idx2"][0][:N].any() and not f["idx2"][0][-N:].any() and not f["idx1"][0][:N].any() and not f["idx1"][0][-N:].any()
    assert f["idx2"][0][N:-N].any()                                                 # (the interior is searched)
    table = fine_table(A, B, rt)
    sel = table[f["idx1"][0], f["idx2"][0]]
    u = np.unwrap(sel * 4, discont=np.pi)                                           # in the array's dtype, as the composed path unwraps
    wraps = np.round((u.astype(np.float64) - sel.astype(np.float64) * 4) / (2 * np.pi)).astype(np.int64)      # 2 pi corrections carried up to each sample
    assert wraps[-1] != 0 and np.all(wraps[:N] == 0)
    assert np.all(f["ph"][0][:N] == table[0, 0])                                    # no wrap yet: the fine angle itself, bit for bit
    want = sel.astype(np.float64) + np.float64(rt(np.pi) / rt(2)) * wraps
    ulp = np.spacing((np.abs(sel) + np.abs(wraps) * rt(np.pi / 2)).astype(rt))
    assert np.all(np.abs(f["ph"][0] - want) <= 2 * ulp)                             # fine[j, idx2[j]] + wraps pi/2, rounded once or twice
    assert np.all(f["ph"][0][-N:] == f["ph"][0][-1]) and wraps[-N:].min() == wraps[-N:].max()


# ------------------------------------------------------------------------------------------------ 4. resident path
RX_KW = dict(methods=("mcma", "sbd"), Niter=(2, 2), Nbps=10)


def _capture(seed, nsym=2 ** 13):
    return synth.make_capture(16, nsym, nmodes=2, snr_db=18, theta=0.6, dgd=20e-12, linewidth=100e3, seed=seed, dtype=np.complex64)


def test_resident_receiver_two_stage():
    from qampy_amd.pipeline import ResidentReceiver
    sig = _capture(77)
    L = sig.shape[1]                                                                # 2^14 samples at 2 samples per symbol
    mk = lambda **kw: ResidentReceiver(2, L, 2, 16, 11, (2e-3, 5e-4), alphabet=sig.coded_symbols, **RX_KW, **kw)
    two, one, plain, none = mk(Mtestangles=16, Bbps=4), mk(Mtestangles=64, Bbps=None), mk(Mtestangles=64), mk(Mtestangles=16, Bbps=None)
    res = []
    for rx in (two, one, plain, none):
        rx.load(sig)
        rx.run()
        res.append(rx.fetch())
    r2, r1, rp, rn = res
    out, ph = hip_dsp.bps_twostage_recover(r2["eq"], 16, sig.coded_symbols, 10, B=4)
    assert np.array_equal(r2["out"], out) and np.array_equal(r2["ph"], ph) and r2["idx2"].shape == r2["idx"].shape and r2["idx2"].max() < 4
    assert two.bytes_per_symbol()["bps"] > one.bytes_per_symbol()["bps"] and "idx2" not in r1
    for k in ("eq", "out", "ph", "idx"):                                            # Bbps=None is the receiver without the argument
        assert np.array_equal(r1[k], rp[k]), k
    assert np.array_equal(rn["eq"], r2["eq"]) and np.array_equal(rn["idx"], r2["idx"])          # same coarse stage
    e2 = [d["errors"] for d in two.ser(sig.symbols)]
    e1 = [d["errors"] for d in one.ser(sig.symbols)]
    own = [synth.count_symbol_errors(r1["out"][m], sig.symbols, sig.coded_symbols)[0] for m in range(2)]
    # 16 x 4 angles resolve the phase as finely as 64: the two error counts are two draws of one statistic, and may differ by what the
    # test itself counts on the single-stage output
    for m in range(2):
        assert e2[m] <= e1[m] + own[m], "mode %d: two-stage %d symbol errors, single-stage (64 angles) %d, counted here %d" % (m, e2[m], e1[m], own[m])
    print("symbol errors per mode: two-stage %s, single-stage %s, counted on the host %s" % (e2, e1, own))
    mt = two.metrics(sig.symbols)
    assert len(mt) == 2 and all(np.isfinite(d["ser"]) for d in mt)
    two.run(overlap=True)                                                           # the pending search goes as one launch
    assert np.array_equal(two.fetch()["out"], r2["out"])


def test_channel_bank_two_stage():
    from qampy_amd.pipeline import ChannelBank, ResidentReceiver
    sigs = [_capture(81 + c, nsym=2 ** 12) for c in range(2)]
    L = sigs[0].shape[1]
    kw = dict(alphabet=sigs[0].coded_symbols, Mtestangles=16, Bbps=4, **RX_KW)
    bank = ChannelBank(2, 2, L, 2, 16, 11, (2e-3, 5e-4), **kw)
    for c, sg in enumerate(sigs):
        bank.load(c, sg)
    bank.run()
    for c, sg in enumerate(sigs):
        rx = ResidentReceiver(2, L, 2, 16, 11, (2e-3, 5e-4), **kw)
        rx.load(sg)
        rx.run()
        a, b = bank.fetch(c), rx.fetch()
        for k in ("eq", "out", "ph", "idx", "idx2"):
            assert np.array_equal(a[k], b[k]), (c, k)
        assert [d["errors"] for d in bank.ser(c, sg.symbols)] == [d["errors"] for d in rx.ser(sg.symbols)]


# ------------------------------------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("dn", ["c64", "c128"])
@pytest.mark.parametrize("B,N", [(0, 4), (65, 4), (4, 0)])
def test_bad_sizes_are_the_librarys_argument_error(B, N, dn):
    E, alphabet = drifting_rows(4, 64, 1, dn, seed=1)
    rt = RT[dn]
    dE, dsy = D.from_host(E), D.from_host(alphabet)
    idx1, idx2, ph, out = D.from_host(np.full(E.shape, 7, np.int32)), D.from_host(np.full(E.shape, 7, np.int32)), D(E.shape, rt), D.from_host(E * 0 + 3)
    _lib.sync()
    rc = getattr(_lib.load(), "qh_bps_twostage_recover_c%s_dev" % dn[1:])(dE.ptr, 1, 64, None, 8, B, dsy.ptr, 4, N, idx1.ptr, idx2.ptr, ph.ptr, out.ptr)
    assert rc == _lib.QH_ERR_ARG and b"bps_twostage" in _lib.load().qh_last_error()
    with pytest.raises(ValueError, match="bps_twostage"):
        hip_dsp.bps_twostage_recover_dev(dE, 8, B, dsy, N, idx1, idx2, ph, out)
    _lib.sync()                                                                     # nothing ran: the outputs are as they were
    assert np.all(idx1.to_host() == 7) and np.all(idx2.to_host() == 7) and np.all(out.to_host() == 3)
    with pytest.raises(ValueError, match="Eout must not be E"):
        hip_dsp.bps_twostage_recover_dev(dE, 8, 4, dsy, 4, idx1, idx2, ph, dE)


def test_real_input_is_a_type_error():
    with pytest.raises(TypeError):
        hip_dsp.bps_twostage_recover(np.zeros((1, 64), np.float32), 8, np.ones(4, np.complex64), 4)
    with pytest.raises(TypeError):
        core_ph.bps_twostage(np.zeros(64, np.float64), 8, np.ones(4, np.complex128), 4, method="fused")


def test_row_pipeline_returns_what_the_one_stream_path_returns(monkeypatch):
    """``hip_dsp.bps_recover`` / ``bps_twostage_recover`` on a (3, 2**16) complex64 field: 1.5 MiB, just above ``_lib.PINNED_MIN_BYTES``, so the rows go
    through the three-stream pipeline - a first, a middle and a last row, every one different; bit for bit what the same calls return on the
    one-stream path (the threshold moved out of reach)."""
    rng = np.random.default_rng(7)
    M, nm, L = 16, 3, 2 ** 16
    sy = theory.cal_symbols_qam(M).astype(np.complex64)
    sy /= np.sqrt(np.mean(np.abs(sy) ** 2))
    ph = np.cumsum(rng.normal(0, 2e-2, (nm, L)), axis=1)
    E = (sy[rng.integers(0, M, (nm, L))] * np.exp(1j * ph) + 0.05 * (rng.normal(size=(nm, L)) + 1j * rng.normal(size=(nm, L)))).astype(np.complex64)
    assert E.nbytes >= _lib.PINNED_MIN_BYTES

    def both():
        return [np.array(a) for a in hip_dsp.bps_recover(E, 32, sy, 12) + hip_dsp.bps_twostage_recover(E, 16, sy, 12, B=4)]
    piped = both()
    monkeypatch.setattr(_lib, "PINNED_MIN_BYTES", 1 << 40)
    plain = both()
    assert all(a.shape == (nm, L) and np.any(a) for a in piped)
    for name, a, b in zip(("bps out", "bps ph", "two-stage out", "two-stage ph"), piped, plain):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
