"""Time-domain hybrid QAM, PSK and resampled signals on the GPU (csrc/hybrid.hip) against the float64 restatement of tests/hybrid_ref.py and the
reference's arrays (tests/golden/hybrid.npz).

Shapes.  The class sums cut a row into tiles of 4096 samples whatever the frame length; the shared cases of hybrid_ref.CASES are rows of 4130
(f_M = 10 = 7 + 3), 4098 (f_M = 2) and 4132 symbols (f_M = 4 = 1 + 3, the higher order in format 2): each crosses the tile boundary, and 10 does
not divide the tile.  A power-of-two tile is a multiple of every power-of-two frame, so two more rows join them: f_M = 7 = 4 + 3 (4102 symbols)
and f_M = 256 = 100 + 156 (4352 symbols, the longest frame, one group of threads).  One row of exactly one frame (L = f_M = 10) is the smallest
call.  Received rows are golden rows plus seeded numpy noise at 12, 18 and 12 dB, rolled by 7, 1 and 3 (third row: one more): the alignments are
3, 1, 1 (third row 2, 0, 0).  tests/test_hybrid_ref.py asserts on the restatement that every alignment leads its runner-up by 2 % and that no
sample lies within 1e-4 (squared distance) of a decision boundary, so kernel and restatement take the same decisions in both precisions.

Bars.  Class sums: 1e-11 relative (double accumulation of at most 2^18 terms) and two calls bit-identical.  Shifts, the six counts per row,
assembled rows and labels: exact.  Split: exact in complex128 (the same product of the same doubles) and for part 1; part 2 in complex64 and the
squared-error sums: the field bars of tests/test_gpu_cpr.py, 1e-5 / 1e-11 (max-abs over rms; relative for the sums).

Measured maxima on an MI355X over all cases:
    class sums (relative)            complex64 5.6e-16    complex128 6.7e-16
    split, part 2 (over rms)         complex64 8.1e-8     complex128 0
    squared-error sums (relative)    complex64 4.5e-8     complex128 2.2e-16
    resampled row (over rms)         complex64 6.2e-7     complex128 1.6e-15
    shifts, counts, assembled rows and labels: equal in every case
8-PSK at 14 dB, 2^18 symbols: SER 6.767e-3 against 6.680e-3 from theory, 0.55 binomial sigma.
Resident sweep, (16, 4) at fr = 0.25, 2^18 symbols, 12 dB: combined BER 0.018174 over theory.hybrid_qam_ber_vs_esn0's 0.018280: 0.9942 (bar 1 +- 0.039).
"""
import numpy as np
import pytest

import hybrid_ref as ref
from qampy_amd import _lib, phaserec, signals, synth, theory
from qampy_amd._lib import DeviceArray
from qampy_amd.core import hip_dsp

pytestmark = pytest.mark.gpu

DTS = sorted(ref.DT)
BAR = {"c64": 1e-5, "c128": 1e-11}
CASE_IDS = [c["name"] for c in ref.CASES]
PREFIXES = ["t%d_n%d_" % (k, nm) for k in range(4) for nm in (1, 2)] + ["tfs_", "tpsk_"]
SEEN = {}


def note(key, dt, value):
    SEEN[(key, dt)] = max(SEEN.get((key, dt), 0.0), float(value))


def synthetic(fM, fM1, nframes, M, nm, dt, snr, rolls, seed):
    """A hybrid row that is not in the golden file: random labels on the golden (16, 4) / (4, 16) / 16-QAM alphabets, noise, a roll per row."""
    g = ref.golden_signal("t0_n1_", dt)
    alph = {16: g["coded1"], 4: g["coded2"]}
    coded1, coded2 = alph[M[0]], alph[M[1]]
    powratio = float(ref.power_ratio(coded1, coded2))
    rng = np.random.default_rng(seed)
    l1, l2 = rng.integers(0, M[0], (nm, nframes * fM1)), rng.integers(0, M[1], (nm, nframes * (fM - fM1)))
    clean = ref.assemble(coded1[l1], coded2[l2], fM, fM1, powratio)
    x = np.array([np.roll(ref.noisy_row(clean[m], snr, seed + 1 + m), -rolls[m]) for m in range(nm)]).astype(ref.DT[dt])
    idx = np.empty(clean.shape, np.int32)
    i1, i2 = ref.positions(clean.shape[1], fM, fM1)
    idx[:, i1], idx[:, i2] = l1, l2
    return dict(x=x, clean=clean, idx_tx=idx, fM=fM, fM1=fM1, powratio=powratio, coded1=coded1, coded2=coded2, M=M, labels1=l1.astype(np.int32),
                labels2=l2.astype(np.int32))


def all_rows(dt):
    """``(name, rows, fM, fM1, M)`` of every row shape the class sums and the alignment are run on."""
    out = []
    for case in ref.CASES:
        for nm in ref.NMODES:
            s, x, _, _ = ref.received(case, nm, dt)
            out.append(("%s_n%d" % (case["name"], nm), x, s["fM"], s["fM1"], s["M"]))
    s, x, _, _ = ref.received(ref.CASES[0], 2, dt)
    out.append(("one_frame", np.ascontiguousarray(np.roll(x, 7, axis=1)[:, :10]), 10, 7, (16, 4)))
    for fM, fM1, nframes, rolls in ((7, 4, 586, (3, 0, 6)), (256, 100, 17, (37, 0, 255))):
        y = synthetic(fM, fM1, nframes, (16, 4), 3, dt, 14.0, rolls, seed=fM)
        out.append(("fM%d" % fM, y["x"], fM, fM1, (16, 4)))
    return out


def test_the_rows_cross_a_tile_boundary():
    for name, x, fM, fM1, M in all_rows("c64"):
        assert x.shape[1] % fM == 0
        if name != "one_frame":
            assert x.shape[1] > hip_dsp.TDH_TILE
    assert hip_dsp.TDH_TILE % 10 and hip_dsp.TDH_TILE % 7 and 256 == hip_dsp.TDH_FM_MAX


@pytest.mark.parametrize("dt", DTS)
def test_class_sums_and_alignment(dt):
    for name, x, fM, fM1, M in all_rows(dt):
        E = DeviceArray.from_host(x)
        a = hip_dsp.tdh_class_sums_dev(E, fM)
        b = hip_dsp.tdh_class_sums_dev(E, fM, DeviceArray((x.shape[0], fM), np.float64))
        got, again = a.to_host(), b.to_host()
        want = ref.class_sums(x, fM)
        assert got.shape == want.shape and got.tobytes() == again.tobytes(), name
        err = np.abs(got / want - 1).max()
        note("class sums", dt, err)
        assert err <= 1e-11, (name, err)
        shift = hip_dsp.tdh_align_dev(a, fM1, M)
        assert shift.dtype == np.int32 and list(shift.to_host()) == list(ref.align(x, fM, fM1, M)), name
    for case in ref.CASES:                                               # what the cases were built for
        for nm in ref.NMODES:
            s, x, _, shifts = ref.received(case, nm, dt)
            E = DeviceArray.from_host(x)
            assert list(hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(E, s["fM"]), s["fM1"], s["M"]).to_host()) == list(shifts)
            assert shifts[0] == case["shift"]


@pytest.mark.parametrize("dt", DTS)
def test_alignment_of_aligned_rows_and_of_a_tie(dt):
    for k in range(3):
        s = ref.golden_signal("t%d_n2_" % k, dt)
        E = DeviceArray.from_host(s["row"])
        assert list(hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(E, s["fM"]), s["fM1"], s["M"]).to_host()) == [0, 0]
    # exact data: both formats with |x| = 1, every alignment has the same mean - the first one wins
    x = np.tile(np.array([1, -1, 1j, -1j, 1, 1j, -1j, -1, 1j, 1], dtype=ref.DT[dt]), (2, 500))
    for fM, fM1, M in ((10, 7, (16, 4)), (10, 7, (4, 16)), (4, 1, (4, 16)), (2, 1, (64, 16))):
        sums = hip_dsp.tdh_class_sums_dev(DeviceArray.from_host(x), fM)
        assert np.array_equal(sums.to_host(), np.full((2, fM), 5000 // fM, dtype=np.float64))
        assert list(hip_dsp.tdh_align_dev(sums, fM1, M).to_host()) == [0, 0] == list(ref.align(x, fM, fM1, M))
    # a lead in one alignment only: the strict comparison keeps the first of two equal maxima
    sums = DeviceArray.from_host(np.array([[1., 3., 3., 1.], [2., 2., 2., 5.]]))
    assert list(hip_dsp.tdh_align_dev(sums, 3, (4, 16)).to_host()) == [2, 0]        # format 2 sits at residue 3: j = 2 brings residue 1 there first
    assert list(hip_dsp.tdh_align_dev(sums, 1, (16, 4)).to_host()) == [1, 3]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("prefix", PREFIXES)
def test_assemble_of_the_golden_parts_is_bit_for_bit(prefix, dt):
    s = ref.golden_signal(prefix, dt)
    D = DeviceArray
    out, idx = D(s["row"].shape, s["row"].dtype), D(s["row"].shape, np.int32)
    hip_dsp.tdh_assemble_dev(D.from_host(s["part1"]), D.from_host(s["part2"]), s["fM"], s["fM1"], s["powratio"], out, D.from_host(s["labels1"]),
                             D.from_host(s["labels2"]), idx)
    assert np.array_equal(out.to_host(), s["row"]) and np.array_equal(idx.to_host(), s["idx_tx"])
    plain = D(s["row"].shape, s["row"].dtype)
    hip_dsp.tdh_assemble_dev(D.from_host(s["part1"]), D.from_host(s["part2"]), s["fM"], s["fM1"], s["powratio"], plain)
    assert np.array_equal(plain.to_host(), s["row"])


def split_rows(dt):
    out = []
    for case in ref.CASES:
        for nm in ref.NMODES:
            s, x, labels, shifts = ref.received(case, nm, dt)
            out.append(dict(s, x=x, idx_tx=labels, shifts=shifts, name="%s_n%d" % (case["name"], nm)))
    s, x, labels, shifts = ref.received(ref.CASES[0], 2, dt, rolled=False)
    out.append(dict(s, x=np.ascontiguousarray(x[:, :10]), idx_tx=np.ascontiguousarray(labels[:, :10]), shifts=shifts, name="one_frame"))
    for fM, fM1, nframes, rolls in ((7, 4, 586, (3, 0, 6)), (256, 100, 17, (37, 0, 255))):
        y = synthetic(fM, fM1, nframes, (16, 4), 3, dt, 14.0, rolls, seed=fM)
        sh = np.array([(fM - r) % fM for r in rolls], dtype=np.int32)
        y["idx_tx"] = np.ascontiguousarray([np.roll(y["idx_tx"][m], -(rolls[m] + sh[m])) for m in range(3)])
        out.append(dict(y, shifts=sh, name="fM%d" % fM))
    return out


@pytest.mark.parametrize("dt", DTS)
def test_split_with_a_device_and_a_host_shift(dt):
    D = DeviceArray
    for c in split_rows(dt):
        x, fM, fM1 = c["x"], c["fM"], c["fM1"]
        nm, L = x.shape
        E = D.from_host(x)
        w1, w2 = ref.split(x, fM, fM1, c["powratio"], c["shifts"])
        p1, p2 = D((nm, L // fM * fM1), x.dtype), D((nm, L // fM * (fM - fM1)), x.dtype)
        hip_dsp.tdh_split_dev(E, fM, fM1, c["powratio"], p1, p2, D.from_host(c["shifts"]))
        g1, g2 = p1.to_host(), p2.to_host()
        assert np.array_equal(g1, w1.astype(x.dtype)), c["name"]
        err = np.abs(g2 - w2).max() / np.sqrt(np.mean(np.abs(w2) ** 2))
        note("split, part 2", dt, err)
        assert err <= BAR[dt], (c["name"], err)
        if dt == "c128":
            assert np.array_equal(g2, w2), c["name"]
        assert np.array_equal(E.to_host(), x)                             # E is only read
        # one shift for every row, from the host
        for sh in (0, int(c["shifts"][0]), fM + 1, -1):
            v1, v2 = ref.split(x, fM, fM1, c["powratio"], sh)
            hip_dsp.tdh_split_dev(E, fM, fM1, c["powratio"], p1, p2, sh)
            assert np.array_equal(p1.to_host(), v1.astype(x.dtype)), (c["name"], sh)
            assert np.abs(p2.to_host() - v2).max() <= BAR[dt] * np.sqrt(np.mean(np.abs(v2) ** 2)), (c["name"], sh)
    with pytest.raises(ValueError, match="must not be E"):
        hip_dsp.tdh_split_dev(E, fM, fM1, c["powratio"], _alias(E, p1.shape), p2, 0)


def _alias(E, shape):
    """A DeviceArray header of another shape on E's memory."""
    v = object.__new__(DeviceArray)
    v.shape, v.dtype, v.ptr, v._own = tuple(shape), E.dtype, E.ptr, False
    v.nbytes = int(np.prod(shape)) * E.dtype.itemsize
    return v


def run_metrics(c, shift):
    D = DeviceArray
    x = c["x"]
    sums = hip_dsp.tdh_metrics_dev(D.from_host(x), D.from_host(np.ascontiguousarray(c["idx_tx"], dtype=np.int32)), c["fM"], c["fM1"], c["powratio"],
                                   D.from_host(np.ascontiguousarray(c["coded1"], dtype=x.dtype)), D.from_host(np.ascontiguousarray(c["coded2"], dtype=x.dtype)),
                                   shift)
    return sums.to_host().reshape(x.shape[0], 2, 4)


def compare_metrics(c, got, dt, name):
    want, tie = ref.metrics(c["x"], c["idx_tx"], c["fM"], c["fM1"], c["powratio"], c["coded1"], c["coded2"], c["shifts"])
    assert tie >= ref.TIE_MARGIN, (name, tie)
    assert np.array_equal(got[:, :, :3], want[:, :, :3]), (name, got[:, :, :3], want[:, :, :3])
    err = np.abs(got[:, :, 3] / want[:, :, 3] - 1).max()
    note("squared-error sums", dt, err)
    assert err <= BAR[dt], (name, err)
    return want


@pytest.mark.parametrize("dt", DTS)
def test_hybrid_metrics(dt):
    for c in split_rows(dt):
        if c["name"].startswith("fM"):
            # (random rows: their samples are not kept clear of the boundaries - take the decisions' margin from the restatement and skip a close one)
            _, tie = ref.metrics(c["x"], c["idx_tx"], c["fM"], c["fM1"], c["powratio"], c["coded1"], c["coded2"], c["shifts"])
            if tie < ref.TIE_MARGIN:
                c = dict(c, idx_tx=mask_close(c))
        want = compare_metrics(c, run_metrics(c, DeviceArray.from_host(c["shifts"])), dt, c["name"])
        assert want[:, :, 2].sum() > 0
        if len(set(c["shifts"])) == 1:
            compare_metrics(c, run_metrics(c, int(c["shifts"][0])), dt, c["name"] + " host shift")


def mask_close(c):
    """The labels of ``c`` with -1 wherever the aligned sample is within TIE_MARGIN of a decision boundary (such a label is skipped)."""
    idx = np.array(c["idx_tx"], dtype=np.int32)
    p1, p2 = ref.split(c["x"], c["fM"], c["fM1"], c["powratio"], c["shifts"])
    i1, i2 = ref.positions(c["x"].shape[1], c["fM"], c["fM1"])
    for part, pos, coded in ((p1, i1, c["coded1"]), (p2, i2, c["coded2"])):
        for m in range(part.shape[0]):
            two = np.partition(ref._distances(part[m], coded), 1, axis=1)
            idx[m, pos[two[:, 1] - two[:, 0] < 2 * ref.TIE_MARGIN]] = -1
    return idx


@pytest.mark.parametrize("dt", DTS)
def test_labels_outside_the_alphabet_are_skipped(dt):
    s, x, labels, shifts = ref.received(ref.CASES[0], 3, dt)
    labels = labels.copy()
    rng = np.random.default_rng(5)
    gone = rng.random(labels.shape) < 0.3
    labels[gone] = rng.choice([-1, -7, 4, 16, 1000, 2 ** 31 - 1, -2 ** 31], size=int(gone.sum())).astype(np.int32)
    c = dict(s, x=x, idx_tx=labels, shifts=shifts)
    want = compare_metrics(c, run_metrics(c, DeviceArray.from_host(shifts)), dt, "skipped labels")
    assert 0 < want[:, :, 2].sum() < 0.85 * x.size                         # (a 4 is a label of format 1 and none of format 2)
    none = dict(c, idx_tx=np.full(labels.shape, -1, np.int32))
    assert not run_metrics(none, 0).any()


@pytest.mark.parametrize("dt", DTS)
def test_two_formats_of_one_order(dt):
    y = synthetic(4, 3, 1033, (16, 16), 2, dt, 16.0, (0, 0), seed=9)
    assert y["powratio"] == 1.0 and y["x"].shape[1] == 4132
    c = dict(y, shifts=np.zeros(2, np.int32))
    c["idx_tx"] = mask_close(c)
    want = compare_metrics(c, run_metrics(c, 0), dt, "M1 == M2")
    assert want[:, :, 0].min() > 0
    # M1 == M2 takes the reference's branch, format 2: on sums with a clear lead (two equal formats have none of their own)
    sums = DeviceArray.from_host(np.array([[1., 2., 3., 9.], [9., 1., 2., 3.]]))
    assert list(hip_dsp.tdh_align_dev(sums, 3, (16, 16)).to_host()) == [0, 1]


# ---- the classes
@pytest.mark.parametrize("dt", DTS)
def test_the_constructors_give_the_reference_arrays(dt):
    g = ref.gold()
    for k in range(4):
        M1, M2, N = (int(v) for v in g["tdh_cases"][k])
        for nm in (1, 2):
            s = ref.golden_signal("t%d_n%d_" % (k, nm), dt)
            sig = signals.TDHQAMSymbols((M1, M2), N, fr=float(g["tdh_fr"][k]), nmodes=nm, seed=int(g["tdh_seed"]) + k, dtype=ref.DT[dt])
            assert np.array_equal(np.asarray(sig), s["row"]) and sig.powratio == s["powratio"] and sig.M == (M1, M2)
            assert np.array_equal(np.asarray(sig.symbols_M1), s["part1"]) and np.array_equal(np.asarray(sig.symbols_M2), s["part2_scaled"])
    s = ref.golden_signal("tfs_", dt)
    p1 = signals.SignalQAMGrayCoded(16, 70, nmodes=2, seed=11, dtype=ref.DT[dt])
    p2 = signals.SignalQAMGrayCoded(4, 30, nmodes=2, seed=12, dtype=ref.DT[dt])
    assert np.array_equal(np.asarray(signals.TDHQAMSymbols.from_symbol_arrays(p1, p2, 0.3)), s["row"])
    s = ref.golden_signal("tpsk_", dt)
    sig = signals.TDHQAMSymbols((16, 4), 40, fr=0.25, M2class=signals.SignalPSKGrayCoded, nmodes=1, seed=5, dtype=ref.DT[dt])
    assert np.array_equal(np.asarray(sig), s["row"]) and isinstance(sig.symbols_M2, signals.SignalPSKGrayCoded) and sig.powratio == s["powratio"]
    for M in (2, 4, 8, 16):
        psk = signals.SignalPSKGrayCoded(M, 96, nmodes=2, seed=int(g["psk_seed"]), dtype=ref.DT[dt])
        coded = g["psk%d_%s_coded" % (M, dt)]
        assert np.array_equal(psk.coded_symbols, coded) and np.array_equal(np.asarray(psk), coded[g["psk%d_labels" % M]])
        assert np.array_equal(np.asarray(psk.bits), g["psk%d_bits" % M]) and np.array_equal(psk.modulate(psk.bits), np.asarray(psk))
        assert np.array_equal(psk.demodulate(np.asarray(psk)), g["psk%d_bits" % M])
        again = signals.SignalPSKGrayCoded.from_symbol_array(np.asarray(psk), M=M)
        assert np.array_equal(np.asarray(again), np.asarray(psk)) and np.array_equal(again.bits, g["psk%d_bits" % M])
        assert np.array_equal(psk.make_decision(np.asarray(psk) * 1.01), np.asarray(psk)) and not psk.cal_ser(synced=True).any()
    fb, fs, beta, taps = g["rs_params"]
    rs = signals.ResampledQAM(16, 128, fb=fb, fs=fs, resamplekwargs=dict(beta=beta, taps=int(taps)), nmodes=2, seed=int(g["rs_seed"]), dtype=ref.DT[dt])
    want = g["rs_%s_out" % dt]
    assert isinstance(rs, signals.ResampledQAM) and rs.shape == (2, 256) and rs.fs == fs and rs.fb == fb and rs.dtype == ref.DT[dt]
    assert np.array_equal(rs.symbols, g["rs_%s_coded" % dt][g["rs_labels"]])
    err = np.abs(np.asarray(rs) - want).max() / np.sqrt(np.mean(np.abs(want) ** 2))
    note("resampled row", dt, err)
    assert err <= BAR[dt], err
    back = signals.ResampledQAM.from_symbol_array(rs, fb, beta=beta, taps=int(taps))
    assert back.shape == (2, 128) and back.fs == fb


@pytest.mark.parametrize("dt", DTS)
def test_class_metrics_on_the_device_equal_the_host_path(dt):
    for case in ref.CASES:
        s, x, labels, shifts = ref.received(case, 2, dt)
        _, x0, labels0, zero = ref.received(case, 2, dt, rolled=False)
        p1 = signals.SignalQAM(s["part1"].copy(), s["M"][0], coded_symbols=s["coded1"], symbols=s["part1"].copy())
        p2 = signals.SignalQAM(s["part2"].copy(), s["M"][1], coded_symbols=s["coded2"], symbols=s["part2"].copy())
        sig = signals.TDHQAMSymbols.from_symbol_arrays(p1, p2, s["fM2"] / s["fM"])
        h1, h2, hs = sig.divide(x, method="hip", return_shifts=True)
        q1, q2, qs = sig.divide(x, method="pyt", return_shifts=True)
        assert list(hs) == list(qs) == list(shifts) and np.array_equal(h1, q1) and type(h1) is type(q1)
        assert np.abs(np.asarray(h2) - np.asarray(q2)).max() <= BAR[dt] * np.sqrt(np.mean(np.abs(np.asarray(q2)) ** 2))
        want = ref.rates(ref.metrics(x0, labels0, s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], zero)[0], s["M"])
        for key, fn in (("ser", sig.cal_ser), ("ber", sig.cal_ber), ("evm", sig.cal_evm)):
            dev, host = fn(x0, method="hip"), fn(x0, method="pyt")
            if key == "evm":
                assert np.abs(dev[0] / host[0] - 1).max() <= BAR[dt] and np.abs(dev[1] / host[1] - 1).max() <= BAR[dt]
                assert np.abs(dev[0] / want[key][0] - 1).max() <= BAR[dt]
            else:
                assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and np.array_equal(dev[0], want[key][0])
        # the rolled rows are a frame late: unsynchronised, every part finds its sequence again
        assert np.array_equal(sig.cal_ser(x, synced=False, method="hip")[0], want["ser"][0])
        # GMI per format: the existing pass on the split part
        snr = case["snr"]
        per, both = sig.cal_gmi(x0, snr=snr, method="hip")
        d1, d2 = sig.divide(x0, method="hip")
        mix = s["fM1"] / s["fM"] + s["fM2"] / s["fM"] / s["powratio"]
        g1 = d1.cal_gmi(synced=True, snr=snr - 10 * np.log10(mix))[0]
        g2 = d2.cal_gmi(synced=True, snr=snr - 10 * np.log10(mix * s["powratio"]))[0]
        assert np.array_equal(per[:, 0], g1) and np.array_equal(per[:, 1], g2)
        assert np.allclose(both, (g1 * s["fM1"] + g2 * s["fM2"]) / s["fM"], rtol=1e-15)
        assert np.all(per[:, 0] <= np.log2(s["M"][0])) and np.all(per[:, 1] <= np.log2(s["M"][1])) and np.all(per > 0.5 * np.log2(s["M"]))


def test_psk_row_through_viterbi_viterbi_and_its_ser():
    """8-PSK at 14 dB: 2^18 symbols, so that theory expects about 1760 symbol errors (at least 1000 asked).  The row's SER lies within five binomial
    sigma of ``theory.ser_vs_es_over_n0_psk``; the same row goes through ``phaserec.viterbiviterbi`` and ``cal_ser`` without error."""
    N, snr_db = 2 ** 18, 14.0
    sig = signals.SignalPSKGrayCoded(8, N, nmodes=1, seed=8, dtype=np.complex64)
    noisy = sig.recreate_from_np_array(ref.noisy_row(np.asarray(sig)[0], snr_db, 88)[None, :].astype(np.complex64))
    p = float(theory.ser_vs_es_over_n0_psk(10 ** (snr_db / 10), 8))
    assert p * N >= 1000
    ser = noisy.cal_ser(synced=True)
    sigma = np.sqrt(p * (1 - p) / N)
    print("8-PSK at 14 dB: SER %.6g, theory %.6g, %.2f sigma" % (ser[0], p, (ser[0] - p) / sigma))
    assert ser.shape == (1,) and abs(ser[0] - p) <= 5 * sigma, (ser, p, sigma)
    out, ph = phaserec.viterbiviterbi(noisy, 255)
    assert isinstance(out, signals.SignalPSKGrayCoded) and out.shape == noisy.shape and out.M == 8 and np.all(np.isfinite(ph))
    after = out.cal_ser(synced=True)
    assert after.shape == (1,) and 0 <= after[0] <= 1
    assert np.all(np.isfinite(out.cal_ber(synced=True))) and np.all(np.isfinite(out.cal_evm(synced=True)))


@pytest.mark.parametrize("dt", DTS)
def test_the_resident_source_is_the_class_with_prbs_bits(dt):
    d = synth.make_tdh_symbols_dev((16, 4), 4133, 0.3, nmodes=2, dtype=ref.DT[dt])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sig = signals.TDHQAMSymbols((16, 4), 4133, fr=0.3, nmodes=2, dtype=ref.DT[dt], bitclass=signals.PRBSBits)
    assert d["symbols"].shape == (2, 4130) and (d["f_M"], d["f_M1"], d["f_M2"], d["nframes"]) == (10, 7, 3, 413) and d["powratio"] == sig.powratio
    assert np.array_equal(d["symbols"].to_host(), np.asarray(sig))
    idx = d["idx_tx"].to_host()
    i1, i2 = ref.positions(4130, 10, 7)
    assert np.array_equal(idx[:, i1], d["idx_tx1"].to_host()) and np.array_equal(idx[:, i2], d["idx_tx2"].to_host())
    assert np.array_equal(d["alphabet1_host"][idx[:, i1]], np.asarray(sig.symbols_M1))


def test_resident_sweep_point_against_theory():
    """make_tdh_symbols_dev -> impair_pointwise_dev at 12 dB -> class sums, align -> tdh_metrics_dev: only the eight sums come back.  The combined
    BER over ``theory.hybrid_qam_ber_vs_esn0(12, 1 / powratio, 0.25, 16, 4)`` lies within 1 +- 5 / sqrt(expected errors) - about 16 700 errors,
    +- 3.9 %: the binomial spread, not a measurement.  Measured on an MI355X: a ratio of 0.9942 (BER 0.018174 against 0.018280, 16 772 errors expected)."""
    d = synth.make_tdh_symbols_dev((16, 4), 2 ** 18, 0.25, nmodes=1, dtype=np.complex64)
    E = d["symbols"]
    rx = DeviceArray(E.shape, E.dtype)
    hip_dsp.impair_pointwise_dev(E, rx, snr=(12.0, 1), seed=12)
    shift = hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(rx, d["f_M"]), d["f_M1"], d["M"])
    sums = hip_dsp.tdh_metrics_dev(rx, d["idx_tx"], d["f_M"], d["f_M1"], d["powratio"], d["alphabet1"], d["alphabet2"], shift)
    r = hip_dsp.tdh_rates(sums.to_host(), d["M"])
    assert list(shift.to_host()) == [0] and r["counts"][0, :, 2].tolist() == [3 * 2 ** 16, 2 ** 16]
    want = float(theory.hybrid_qam_ber_vs_esn0(12, 1 / d["powratio"], 0.25, 16, 4))
    expected = want * (3 * 2 ** 16 * 4 + 2 ** 16 * 2)
    ratio = r["ber"][1][0] / want
    print("resident sweep at 12 dB: BER %.6g, theory %.6g, ratio %.4f, expected errors %.0f" % (r["ber"][1][0], want, ratio, expected))
    assert 16000 < expected < 17500
    assert abs(ratio - 1) <= 5 / np.sqrt(expected), (ratio, expected)


def test_zz_report_measured_maxima():
    for (key, dt), v in sorted(SEEN.items()):
        print("measured max  %-22s %-5s %.3g" % (key, dt, v))
