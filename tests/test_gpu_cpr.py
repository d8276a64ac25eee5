"""Viterbi-Viterbi and QPSK-partition carrier recovery on the GPU (csrc/cpr.hip) against the float64 restatements of tests/cpr_ref.py.

Inputs are multiples of 2^-12, so complex64 and complex128 hold the same values, and every case keeps its unwrap decisions and ring classes
clear of a flip, and no class-2 sample of a 16-QAM row within 1e-4 of a tie of the partition's complex minimum (the conditions
tests/test_cpr_ref.py asserts on the restatement alone; cpr_ref.tie_margin): kernel and restatement then take the same decisions and differ
by rounding.  Bars, those of tests/test_gpu_foe.py: 1e-5 (complex64) and 1e-11 (complex128), for the trace as max-abs over
max(1, max |trace|) and for the field as max-abs over the restatement's rms; the zero edges of the V&V field are exactly zero.

Measured maxima on an MI355X over the shared cases and the long rows (trace, field):
    Viterbi-Viterbi   complex64 2.3e-7, 1.2e-6    complex128 1.5e-14, 7.7e-14
    QPSK partition    complex64 5.7e-8, 4.2e-7    complex128 2.1e-16, 1.3e-15
Functional, 2 x 2^16 symbols: QPSK through CMA and V&V (N = 11) 0 errors in 2 x 65126 symbols; 16-QAM at 25 dB 50 errors in 130252 symbols with
the partition (blocks of 64) against 27 with the blind phase search (64 angles, N = 20): a ratio of 1.85.
"""
import numpy as np
import pytest

import cpr_ref
from qampy_amd import _lib, phaserec, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import hip_dsp, phaserecovery
from qampy_amd.pipeline import ResidentReceiver
from qampy_amd.signals import SignalQAM

pytestmark = pytest.mark.gpu

DT = [np.complex64, np.complex128]
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
CASES = cpr_ref.cases()
_REF = {}


def ref_of(case):
    """The input and the restatement of a shared case, computed once and left unchanged."""
    if case["name"] not in _REF:
        x = case["make"]()
        _REF[case["name"]] = (x,) + cpr_ref.run(case, x)
    return _REF[case["name"]]


def run_dev(x, case):
    E = DeviceArray.from_host(x)
    nm, L = x.shape
    rt = x.real.dtype
    out = DeviceArray((nm, L), x.dtype)
    if case["kind"] == "vv":
        tr = DeviceArray((nm, L - case["N"] + 1), rt)
        hip_dsp.vv_recover_dev(E, case["N"], case["M"], tr, out)
    else:
        tr = DeviceArray((nm, L), rt)
        hip_dsp.partition16_recover_dev(E, case["Nblock"], tr, out)
    _lib.sync()
    return out.to_host(), tr.to_host()


def compare(name, dtype, got, want, case=None):
    field, trace = got
    rfield, rtrace = want
    assert trace.dtype == np.dtype(dtype).type(0).real.dtype and field.dtype == dtype
    assert trace.shape == rtrace.shape and field.shape == rfield.shape
    err_t = np.max(np.abs(trace.astype(np.float64) - rtrace)) / max(1.0, np.max(np.abs(rtrace)))
    err_f = np.max(np.abs(field.astype(np.complex128) - rfield)) / np.sqrt(np.mean(np.abs(rfield) ** 2))
    print("%s %s: trace %.3g field %.3g" % (name, np.dtype(dtype).name, err_t, err_f))
    if case is not None and case["kind"] == "vv":
        L, N = field.shape[1], case["N"]
        o = (N - 1) // 2
        edges = np.ones(L, bool)
        edges[o:o + L - N + 1] = False
        assert edges.sum() == N - 1 and not field[:, edges].any()
    assert err_t <= BAR[dtype], (name, err_t)
    assert err_f <= BAR[dtype], (name, err_f)


@pytest.mark.parametrize("dtype", DT, ids=["c64", "c128"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_against_the_restatement(case, dtype):
    x, rfield, rtrace, umargin, rmargin = ref_of(case)
    assert umargin >= (0.25 if case["kind"] == "vv" else 0.1) and rmargin >= 1e-9
    assert case["kind"] == "vv" or cpr_ref.tie_margin(x) >= 1e-4
    compare(case["name"], dtype, run_dev(x.astype(dtype), case), (rfield, rtrace), case)


def test_the_wrap_ramp_wraps_where_it_was_built_to():
    """The constructed row corrects by +1, -1, +1 turns at outputs 1023, 1024 and 1025 - the last of a chunk, the first of the next, its second."""
    case = next(c for c in CASES if c["name"] == "vv-wrap-ramp")
    x, _, rtrace, _, _ = ref_of(case)
    _, tr = run_dev(x.astype(np.complex128), case)
    raw = np.angle((x[0] / np.abs(x[0])) ** 4)
    K = np.rint((tr[0] * 4 + np.pi - raw) / (2 * np.pi)).astype(int)
    assert list(np.diff(K)[1022:1025]) == [1, -1, 1] and K[0] == 0


@pytest.mark.parametrize("extra", [0, 1024], ids=["1024-chunks", "1025-chunks"])
def test_vv_long_row(extra):
    """2^20 + 3 samples, N = 11, complex64: 1024 unwrap chunks; with 1024 samples more 1025, so that the threads of the scan of the chunk sums
    hold more than one chunk each."""
    x = cpr_ref.long_vv_row(extra)
    rfield, rtrace, umargin, _ = cpr_ref.viterbiviterbi(x, 11, 4)
    assert umargin >= 0.25 and np.ptp(rtrace) > 20
    case = dict(kind="vv", N=11, M=4)
    compare("vv-long+%d" % extra, np.complex64, run_dev(x.astype(np.complex64), case), (rfield, rtrace), case)


def test_partition_long_row():
    x = cpr_ref.long_p16_row()
    rfield, rtrace, umargin, rmargin = cpr_ref.phase_partition_16qam(x, 64)
    assert umargin >= 0.1 and rmargin >= 1e-9 and cpr_ref.tie_margin(x) >= 1e-4
    case = dict(kind="p16", Nblock=64)
    compare("p16-long", np.complex64, run_dev(x.astype(np.complex64), case), (rfield, rtrace), case)


# ------------------------------------------------------------------------------------------------ host API
@pytest.mark.parametrize("dtype", DT, ids=["c64", "c128"])
def test_core_entry_points(dtype):
    rt = np.dtype(dtype).type(0).real.dtype
    x = cpr_ref.psk_rows(4, 3, 1500, 5, 18.).astype(dtype)
    case = dict(kind="vv", N=11, M=4)
    dfield, dtrace = run_dev(x, case)
    out, ph = phaserecovery.viterbiviterbi(x, 11, 4)
    assert out.shape == (3, 1500) and ph.shape == (1490,) and ph.dtype == rt and out.dtype == dtype
    assert np.array_equal(out, dfield) and np.array_equal(ph, dtrace[-1])
    out, ph = phaserecovery.viterbiviterbi(x, 11, 4, all_modes=True)
    assert np.array_equal(ph, dtrace)
    out, ph = phaserecovery.viterbiviterbi(x[1], 11, 4)
    assert out.shape == (1500,) and ph.shape == (1490,) and np.array_equal(out, dfield[1]) and np.array_equal(ph, dtrace[1])
    y = cpr_ref.qam16_rows(2, 2000, 6).astype(dtype)
    case = dict(kind="p16", Nblock=48)
    dfield, dtrace = run_dev(y, case)
    out, ph = phaserecovery.phase_partition_16qam(y, 48)
    assert out.shape == ph.shape == (2, 2000) and ph.dtype == rt and np.array_equal(out, dfield) and np.array_equal(ph, dtrace)
    out, ph = phaserecovery.phase_partition_16qam(y[0], 48)
    assert out.shape == ph.shape == (2000,) and np.array_equal(out, dfield[0]) and np.array_equal(ph, dtrace[0])


def test_phaserec_entry_points_keep_the_signal_class():
    sig = SignalQAM(cpr_ref.psk_rows(4, 2, 2048, 3, 18.).astype(np.complex64), 4, fb=10e9)
    out, ph = phaserec.viterbiviterbi(sig, 11)
    want, wph = phaserecovery.viterbiviterbi(np.asarray(sig), 11, 4)
    assert type(out) is SignalQAM and out.M == 4 and out.fb == 10e9 and np.array_equal(np.asarray(out), want) and np.array_equal(ph, wph)
    sig = SignalQAM(cpr_ref.qam16_rows(2, 2048, 4), 16, fb=10e9)
    out, ph = phaserec.phase_partition_16qam(sig, 64)
    want, wph = phaserecovery.phase_partition_16qam(np.asarray(sig), 64)
    assert type(out) is SignalQAM and out.M == 16 and ph.dtype == np.float64 and np.array_equal(np.asarray(out), want) and np.array_equal(ph, wph)
    assert ph.shape == sig.shape


# ------------------------------------------------------------------------------------------------ the resident receiver
NSYM = 2 ** 16


def _receiver(clean, M, methods, mu, Niter, impair, **kw):
    E = np.ascontiguousarray(np.asarray(clean))
    rx = ResidentReceiver(2, E.shape[1], 2, M, 21, mu, methods=methods, Niter=Niter, alphabet=clean.coded_symbols, **kw)
    rx.load(E)
    rx.impair(clean.fs, **impair)
    rx.run()
    return rx


def test_qpsk_cma_then_vv_recovers_every_symbol():
    """The reference's QPSK recipe (test/test_signal_recover_functional.py: CMA, then viterbiviterbi(sout, 11)) on the resident receiver:
    2 polarisations, 2^16 symbols at 2 samples per symbol, PMD and 100 kHz of linewidth applied on the device, no noise as there."""
    clean = synth.make_capture(4, NSYM, nmodes=2, snr_db=None, theta=None, dgd=None, linewidth=0., seed=31, dtype=np.complex64)
    rx = _receiver(clean, 4, ("cma",), (2e-3,), (2,), dict(lwdth=100e3, dgd=100e-12, theta=np.pi / 5.9, seed=8), carrier="vv", Nbps=11)
    res = rx.ser(clean.symbols, trim=200)
    got = rx.fetch()
    N = rx.N
    assert got["out"].shape == (2, N) and got["ph"].shape == (2, N - 10) and "idx" not in got
    assert not got["out"][:, :5].any() and not got["out"][:, N - 5:].any() and got["out"][:, 5:N - 5].all()
    print("QPSK, CMA + V&V:", [(r["errors"], r["compared"]) for r in res])
    assert all(r["compared"] > N // 2 for r in res) and {r["tx_mode"] for r in res} == {0, 1}
    assert all(r["errors"] == 0 for r in res)
    # metrics() on the same output
    m = rx.metrics(clean.symbols, trim=200)
    assert len(m) == 2


def test_16qam_partition_against_the_blind_phase_search():
    """16-QAM at 25 dB on the same impaired capture: the partition estimator (blocks of 64) makes at most twice the symbol errors of the
    blind phase search; and carrier="bps" is the receiver as it was, bit for bit."""
    clean = synth.make_capture(16, NSYM, nmodes=2, snr_db=None, theta=None, dgd=None, linewidth=0., seed=32, dtype=np.complex64)
    imp = dict(snr=25., lwdth=100e3, dgd=30e-12, theta=np.pi / 5.6, seed=9)
    args = (clean, 16, ("mcma", "sbd"), (2e-3, 5e-4), (2, 1), imp)
    rp = _receiver(*args, carrier="partition", Nbps=64)
    rb = _receiver(*args, carrier="bps")
    r0 = _receiver(*args)
    ep = rp.ser(clean.symbols, trim=200)
    eb = rb.ser(clean.symbols, trim=200)
    a, b = rb.fetch(), r0.fetch()
    assert sorted(a) == sorted(b)
    for k in a:
        for u, v in zip(a[k], b[k]) if isinstance(a[k], tuple) else [(a[k], b[k])]:
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), k
    assert rp.fetch()["ph"].shape == (2, rp.N)
    np_, nb_ = sum(r["errors"] for r in ep), sum(r["errors"] for r in eb)
    cp, cb = sum(r["compared"] for r in ep), sum(r["compared"] for r in eb)
    print("16-QAM 25 dB: partition %d / %d errors, blind phase search %d / %d" % (np_, cp, nb_, cb))
    assert cp == cb and np_ / cp <= 2 * nb_ / cb
