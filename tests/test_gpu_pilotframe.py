"""Pilot frames on the GPU (csrc/pilot.hip): frames and splits against the reference's own (tests/golden/pilotframe.npz) bit for bit, the
pilot-aided estimates against the float64 restatement of tests/pilot_ref.py, the mirrored API against the reference's complex128 results, and
a chain that stays in HBM from the bit source to the metrics against the host path.

Inputs of the shared cases are multiples of 2^-12, so complex64 and complex128 hold the same values, and every case keeps its unwrap decisions
0.25 rad clear of a flip (tests/test_pilot_ref.py asserts it on the restatement alone): kernel and restatement then take the same decisions
and differ by rounding.  Bars, those of tests/test_gpu_cpr.py: 1e-5 (complex64) and 1e-11 (complex128); unwrapped phases, knots, traces and
fits as max-abs over max(1, max |ref|), fields as max-abs over the restatement's rms.  The mirrored API against the golden results: the larger
of 1e-11 and the bars of tests/test_pilot_ref.py, i.e. 1e-11.

Measured maxima on an MI355X over the shared cases and the long row:
                 phase     knots     trace     field     fit       constant phase   rotate_rows
    complex64    1.9e-16   4.1e-16   5.7e-8    2.6e-7    7.1e-14   1.5e-15          6.0e-8
    complex128   1.9e-16   4.1e-16   4.1e-16   6.2e-14   7.1e-14   1.5e-15          8.7e-14
(phases, knots and fits are formed in double in both precisions).  Mirrored API against the golden complex128 results: trace 1.5e-15, field
1.4e-14, fit 1.3e-16, constant phase 5.4e-19.  Resident chain, 64-QAM at 23 dB with phase noise, 3 frames: 19 and 28 symbol errors in 2 x 2520
payload symbols, on the device and on the host path alike.
"""
import os

import numpy as np
import pytest

import pilot_ref
from conftest import GOLDEN
from qampy_amd import _lib, phaserec, signals, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import ber_functions, hip_dsp, pilotbased_receiver

pytestmark = pytest.mark.gpu

DT =[np.complex64, np.complex128]
IDS = ["c64", "c128"]
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
BAR_GOLDEN = 1e-11
CASES = pilot_ref.cases()
SEED, ORDER = [0x1234, 0x4D2F0B], [15, 23]
_REF = {}
G = np.load(os.path.join(GOLDEN, "pilotframe.npz"))
GEOMS = [tuple(int(v) for v in row) for row in G["geoms"]]


def rel(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.result_type(ref.dtype, np.float64)) - ref)) / max(1.0, np.max(np.abs(ref))))


def rel_rms(a, ref):
    return float(np.max(np.abs(a.astype(np.complex128) - ref)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def ref_of(name, make):
    """The input and the restatement of a case, computed once and left unchanged."""
    if name not in _REF:
        a = make()
        N = a.pop("N")
        ph, margin, pos, K = pilot_ref.phase(**a)
        r = dict(args=a, N=N, phase=ph, margin=margin, pos=pos, K=K)
        if N is not None:
            r["knots"], r["kpos"] = pilot_ref.knots(ph, N, pos)
            r["field"], r["trace"], _ = pilot_ref.cpe(N=N, **a)
        rec, ref = a["E"][:, pos], a["sent"][:, np.arange(pos.size) % a["sent"].shape[1]]
        r["rec"], r["ref"] = np.ascontiguousarray(rec), np.ascontiguousarray(ref)
        r["const"] = pilot_ref.const_phase(rec, ref)[0]
        if pos.size >= 2:
            r["fit"] = pilot_ref.foe(rec, ref)[0]
        _REF[name] = r
    return _REF[name]


# ------------------------------------------------------------------------------------------------ frames
def make_signal(geom, dtype, **kw):
    M, F, S, R, nfr = geom
    return signals.SignalWithPilots(M, F, S, R, nfr, nmodes=2, Mpilots=4, dtype=dtype, bitclass=signals.PRBSBits, seed=SEED, order=ORDER, **kw)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_signal_with_pilots_is_the_reference_s(k, dtype):
    ref = pilot_ref.golden_frame(G, "f%d_%s_" % (k, IDS[DT.index(dtype)]))
    sig = make_signal(GEOMS[k], dtype)
    M, F, S, R, nfr = GEOMS[k]
    assert type(sig) is signals.SignalWithPilots and sig.dtype == dtype and sig.shape == (2, nfr * F)
    assert np.array_equal(np.asarray(sig), ref["frame"])
    assert np.array_equal(np.asarray(sig.pilots), ref["pilots"]) and np.array_equal(np.asarray(sig.symbols), ref["payload"])
    assert sig.pilots.dtype == ref["pilots"].dtype and sig.symbols.dtype == dtype
    assert (sig.frame_len, sig.nframes, sig.M, sig.Mpilots, sig.fb, sig.fs, sig.pilot_scale) == (F, nfr, M, 4, 1, 1, 1)
    assert np.array_equal(sig.pilot_seq, ref["pilots"][:, :S]) and np.array_equal(np.asarray(sig.coded_symbols), ref["pay_coded"])


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_every_frame_its_own_payload(dtype):
    ref = pilot_ref.golden_frame(G, "f0nr_%s_" % IDS[DT.index(dtype)])
    sig = make_signal(GEOMS[0], dtype, repeat_data=False)
    assert np.array_equal(np.asarray(sig), ref["frame"]) and np.array_equal(np.asarray(sig.symbols), ref["payload"])
    d = synth.make_pilot_frames_dev(*GEOMS[0][:4], nframes=3, seed=SEED, order=ORDER, dtype=dtype, repeat_data=False)
    assert np.array_equal(d["frame"].to_host(), ref["frame"]) and np.array_equal(d["payload"].to_host(), ref["payload"])
    assert np.array_equal(d["idx_tx"].to_host(), ref["payload_labels"])


def test_scaled_pilots_follow_numpy_s_promotion():
    ref = pilot_ref.golden_frame(G, "f0s_c64_")
    sig = make_signal(GEOMS[0], np.complex64, pilot_scale=1.5)
    assert sig.dtype == np.complex64 and sig.pilots.dtype == ref["pilots"].dtype and sig.pilot_scale == 1.5
    assert np.array_equal(np.asarray(sig), ref["frame"]) and np.array_equal(np.asarray(sig.pilots), ref["pilots"])
    wide = make_signal(GEOMS[3], np.complex64, pilot_scale=np.float64(1.1))          # a float64 scalar: numpy widens the pilots, the frame keeps its dtype
    plain = make_signal(GEOMS[3], np.complex64)
    assert wide.dtype == np.complex64 and wide.pilots.dtype == np.complex128
    want = np.asarray(plain).copy()
    want[:, np.asarray(plain.idx_pilots)] = np.asarray(plain.pilots) * np.float64(1.1)
    assert np.array_equal(np.asarray(wide), want)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_frames_made_in_hbm_are_the_reference_s(k, dtype):
    M, F, S, R, nfr = GEOMS[k]
    NP, ND = pilot_ref.counts(F, S, R)
    ref = pilot_ref.golden_frame(G, "f%d_%s_" % (k, IDS[DT.index(dtype)]))
    d = synth.make_pilot_frames_dev(M, F, S, R, nframes=nfr, seed=SEED, order=ORDER, dtype=dtype)
    assert all(isinstance(d[n], DeviceArray) for n in ("frame", "pilots", "payload", "idx_tx", "idx_frame", "alphabet", "pilot_alphabet"))
    assert (d["NP"], d["ND"], d["frame_len"], d["seq_len"], d["ins_rat"], d["nframes"]) == (NP, ND, F, S, R, nfr)
    assert np.array_equal(d["frame"].to_host(), ref["frame"])
    assert np.array_equal(d["pilots"].to_host(), ref["pilots"][:, :NP]) and np.array_equal(d["payload"].to_host(), ref["payload"][:, :ND])
    assert np.array_equal(d["alphabet"].to_host(), ref["pay_coded"])
    assert np.array_equal(d["idx_tx"].to_host(), ref["payload_labels"][:, :ND])
    idx = d["idx_frame"].to_host()
    pos_p, pos_d = pilot_ref.positions(F, S, R)
    for f in range(nfr):
        assert np.all(idx[:, f * F + pos_p] == -1) and np.array_equal(idx[:, f * F + pos_d], ref["payload_labels"][:, :ND])


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("k,frames", [(0, None), (0, [1]), (0, [0, 2]), (0, [2, 0]), (1, None), (1, [1]), (1, [1, 0]), (2, [1]), (3, None)])
def test_split_takes_an_assembled_frame_apart(k, frames, dtype):
    M, F, S, R, nfr = GEOMS[k]
    NP, ND = pilot_ref.counts(F, S, R)
    frame = pilot_ref.golden_frame(G, "f%d_%s_" % (k, IDS[DT.index(dtype)]))["frame"]
    # every frame its own content, so that a wrong frame number shows
    x = (frame * (1 + np.arange(nfr).repeat(F))).astype(dtype)
    want_pay, want_pil = pilot_ref.split(x, F, S, R, range(nfr) if frames is None else frames)
    E = DeviceArray.from_host(x)
    nf = nfr if frames is None else len(frames)
    pay, pil = DeviceArray((2, nf * ND), dtype), DeviceArray((2, nf * NP), dtype)
    assert hip_dsp.pilot_split_dev(E, F, S, R, frames, payload=pay, pilots=pil) == nf
    assert np.array_equal(pay.to_host(), want_pay) and np.array_equal(pil.to_host(), want_pil)
    only = DeviceArray((2, nf * ND), dtype, zero=True)
    hip_dsp.pilot_split_dev(E, F, S, R, frames, payload=only)
    assert np.array_equal(only.to_host(), want_pay)


def test_more_frame_lists_than_the_wrapper_keeps():
    """The device copies of the small tables are kept by content, a few of them: every list gives its own frames, before and after it has left."""
    F, S, R, nfr = 12, 2, 5, 6                              # NP = 4, ND = 8
    x = (np.arange(2 * nfr * F).reshape(2, -1) * (1 + 0.5j)).astype(np.complex64)
    E = DeviceArray.from_host(x)
    lists = [[a, b] for a in range(nfr) for b in range(nfr)][:2 * hip_dsp.PILOT_TABLES_KEPT + 3]
    for fr in lists + lists[:3]:
        pay, pil = DeviceArray((2, 16), np.complex64), DeviceArray((2, 8), np.complex64)
        hip_dsp.pilot_split_dev(E, F, S, R, fr, payload=pay, pilots=pil)
        want = pilot_ref.split(x, F, S, R, fr)
        assert np.array_equal(pay.to_host(), want[0]) and np.array_equal(pil.to_host(), want[1]), fr


@pytest.mark.parametrize("frames", [None, [1], [2, 0], [0, 1, 2]])
def test_the_signal_s_splits_equal_the_host_mask(frames):
    M, F, S, R, nfr = GEOMS[0]
    ref = pilot_ref.golden_frame(G, "f0_c128_")
    sig = signals.PilotSignal(G["est_x"], M, 1., 1., F, S, R, ref["pilots"], symbols=ref["payload"])
    for fn in (sig.get_data, sig.extract_pilots):
        host, dev = fn(frames), fn(frames, method="hip")
        assert dev.dtype == host.dtype and np.array_equal(dev, host)
    assert np.array_equal(sig.get_data(method="hip"), G["get_data"]) and np.array_equal(sig.extract_pilots(method="hip"), G["extract_pilots"])
    cut = signals.PilotSignal(G["est_x"][:, :2 * F + 300].astype(np.complex64), M, 1., 1., F, S, R, ref["pilots"])
    for fr in (None, [2], [1, 2]):                          # frame 2 is cut short: the host path answers
        assert np.array_equal(cut.get_data(fr, method="hip"), cut.get_data(fr)) and np.array_equal(cut.extract_pilots(fr, method="hip"), cut.extract_pilots(fr))


# ------------------------------------------------------------------------------------------------ estimates
def run_dev(r, dtype):
    """Every device form on one case: dict of host arrays."""
    a = r["args"]
    rt = np.zeros(1, dtype).real.dtype
    E, sent = DeviceArray.from_host(a["E"].astype(dtype)), DeviceArray.from_host(a["sent"].astype(dtype))
    nm, n = r["phase"].shape
    out = {}
    ph = DeviceArray((nm, n), np.float64)
    assert hip_dsp.pilot_phase_dev(E, a["where"], a["F"], a["nframes"], sent, ph, span=a["span"]) == n
    out["phase"] = ph.to_host()
    if r["N"] is not None:
        N = r["N"]
        span = r["trace"].shape[1]
        kph, kpos = DeviceArray((nm, n - N + 1), np.float64), DeviceArray((n - N + 1,), np.int64)
        hip_dsp.pilot_knots_dev(ph, N, kph, kpos, where=a["where"], F=a["F"])
        out["knots"], out["kpos"] = kph.to_host(), kpos.to_host()
        Eout, trace = DeviceArray((nm, span), dtype), DeviceArray((nm, span), rt)
        assert hip_dsp.pilot_cpe_dev(E, a["where"], a["F"], a["nframes"], sent, N, Eout, trace, span=a["span"]) == n
        out["field"], out["trace"] = Eout.to_host(), trace.to_host()
    rec, ref = DeviceArray.from_host(r["rec"].astype(dtype)), DeviceArray.from_host(r["ref"].astype(dtype))
    c = DeviceArray((nm,), np.float64)
    hip_dsp.pilot_const_phase_dev(rec, ref, c)
    out["const"] = c.to_host()
    if "fit" in r:
        fit, fo, fo_avg = DeviceArray((nm, 2), np.float64), DeviceArray((nm,), np.float64), DeviceArray((nm,), np.float64)
        hip_dsp.pilot_foe_dev(rec, ref, fit, fo)
        hip_dsp.pilot_foe_dev(rec, ref, fit, fo_avg, average=True)
        out["fit"], out["fo"], out["fo_avg"] = fit.to_host(), fo.to_host(), fo_avg.to_host()
    rot = DeviceArray(rec.shape, dtype)
    hip_dsp.rotate_rows_dev(rec, c, rot)
    out["rot"] = rot.to_host()
    return out


def compare(name, dtype, r, got):
    bar = BAR[dtype]
    rt = np.zeros(1, dtype).real.dtype
    errs = dict(phase=rel(got["phase"], r["phase"]), const=rel(got["const"], r["const"]))
    assert got["phase"].dtype == np.float64 and got["phase"].shape == r["phase"].shape
    if "trace" in got:
        assert got["trace"].dtype == rt and got["field"].dtype == dtype and got["trace"].shape == r["trace"].shape == got["field"].shape
        assert np.array_equal(got["kpos"], r["kpos"])
        errs.update(knots=rel(got["knots"], r["knots"]), trace=rel(got["trace"], r["trace"]), field=rel_rms(got["field"], r["field"]))
    if "fit" in got:
        errs["fit"] = rel(got["fit"], r["fit"])
        assert np.array_equal(got["fo"], got["fit"][:, 0]) and rel(got["fo_avg"], np.full(got["fo"].shape, np.mean(r["fit"][:, 0]))) <= bar
        assert np.all(got["fo_avg"] == got["fo_avg"][0])
    errs["rot"] = rel_rms(got["rot"], r["rec"] * np.exp(-1j * r["const"])[:, None])
    print("%s %s: %s" % (name, np.dtype(dtype).name, " ".join("%s %.3g" % kv for kv in sorted(errs.items()))))
    for what, e in errs.items():
        assert e <= bar, (name, what, e)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_against_the_restatement(case, dtype):
    r = ref_of(case["name"], case["make"])
    assert r["margin"] >= pilot_ref.MARGIN
    compare(case["name"], dtype, r, run_dev(r, dtype))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_the_wrap_ramp_wraps_at_the_chunk_seam(dtype):
    case = [c for c in CASES if c["name"] == "wrap-ramp"][0]
    r = ref_of(case["name"], case["make"])
    got = run_dev(r, dtype)
    theta = r["phase"] - 2 * np.pi * r["K"]
    K = np.rint((got["phase"] - theta) / (2 * np.pi)).astype(int)
    assert np.max(np.abs(got["phase"] - theta - 2 * np.pi * K)) < 1e-9
    assert list(np.diff(K[0])[pilot_ref.UW_CHUNK - 2:pilot_ref.UW_CHUNK + 1]) == [1, -1, 1] and np.array_equal(K, r["K"])


def test_a_row_of_more_than_1024_unwrap_chunks():
    r = ref_of("long-row", pilot_ref.long_row)
    assert r["margin"] >= pilot_ref.MARGIN and np.ptp(r["trace"]) > 20 and (r["phase"].shape[1] + pilot_ref.UW_CHUNK - 1) // pilot_ref.UW_CHUNK > 1024
    a, dtype = r["args"], np.complex64
    E, sent = DeviceArray.from_host(a["E"].astype(dtype)), DeviceArray.from_host(a["sent"].astype(dtype))
    n = r["phase"].shape[1]
    ph, Eout, trace = DeviceArray((1, n), np.float64), DeviceArray((1, n), dtype), DeviceArray((1, n), np.float32)
    assert hip_dsp.pilot_phase_dev(E, a["where"], a["F"], a["nframes"], sent, ph) == n
    assert hip_dsp.pilot_cpe_dev(E, a["where"], a["F"], a["nframes"], sent, r["N"], Eout, trace) == n
    errs = rel(ph.to_host(), r["phase"]), rel(trace.to_host(), r["trace"]), rel_rms(Eout.to_host(), r["field"])
    print("long row complex64: phase %.3g trace %.3g field %.3g" % errs)
    assert max(errs) <= BAR[dtype]


# ------------------------------------------------------------------------------------------------ mirrored API against the reference
def golden_signal():
    M, F, S, R, nfr = GEOMS[0]
    ref = pilot_ref.golden_frame(G, "f0_c128_")
    return signals.PilotSignal(G["est_x"], M, 1., 1., F, S, R, ref["pilots"], symbols=ref["payload"]), ref


@pytest.mark.parametrize("call", [0, 1, 2])
def test_pilot_cpe_on_the_device_matches_the_reference(call):
    name, kw, args = pilot_ref.golden_cpe_calls(G)[call]
    sig, ref = golden_signal()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (N = 4 becomes 5, with a warning, on both paths)
        out, tr = phaserec.pilot_cpe(sig, method="hip", **kw)
        host_out, host_tr = phaserec.pilot_cpe(sig, **kw)
    assert type(out) is type(host_out) and out.shape == host_out.shape and out.dtype == host_out.dtype
    assert tr.shape == host_tr.shape and tr.dtype == host_tr.dtype == np.complex128 and not np.any(tr.imag)
    e_t, e_f = rel(tr.real, G[name + "_ph"]), rel_rms(np.asarray(out), G[name + "_E"])
    print("%s: trace %.3g field %.3g" % (name, e_t, e_f))
    assert e_t <= BAR_GOLDEN and e_f <= BAR_GOLDEN
    # the core function, host arrays in and out
    S = GEOMS[0][2]
    pos = np.flatnonzero(sig._idx_pil)
    core = pilotbased_receiver.pilot_based_cpe_new(G["est_x"], ref["pilots"], pos, GEOMS[0][1], seq_len=S, num_average=5, method="hip")
    assert rel(core[1].real, G["cpe1_ph"]) <= BAR_GOLDEN and rel_rms(core[0], G["cpe1_E"]) <= BAR_GOLDEN


def test_offset_and_constant_phase_on_the_device_match_the_reference():
    sig, ref = golden_signal()
    S = GEOMS[0][2]
    rec, pil = G["est_x"][:, :S], ref["pilots"][:, :S]
    foe, modes, icpt = pilotbased_receiver.pilot_based_foe(rec, pil, method="hip")
    h_foe, h_modes, h_icpt = pilotbased_receiver.pilot_based_foe(rec, pil)
    assert modes.shape == h_modes.shape == (2, 1) and icpt.shape == h_icpt.shape and modes.dtype == h_modes.dtype and np.ndim(foe) == np.ndim(h_foe) == 0
    e = max(rel(modes, G["foe_modes"]), rel(icpt, G["foe_icpt"]), abs(float(foe) - float(G["foe_mean"])))
    c = phaserec.find_pilot_const_phase(G["const_rec"], G["const_ref"], method="hip")
    h_c = phaserec.find_pilot_const_phase(G["const_rec"], G["const_ref"])
    assert c.shape == h_c.shape == (2, 1) and c.dtype == h_c.dtype
    e_c = rel(c, G["const_ph"])
    print("fit %.3g constant phase %.3g" % (e, e_c))
    assert e <= BAR_GOLDEN and e_c <= BAR_GOLDEN
    one = phaserec.find_pilot_const_phase(G["const_rec"][0], G["const_ref"][0], method="hip")          # 1-d in, as on the host path
    assert one.shape == (1, 1) and one[0, 0] == c[0, 0]


# ------------------------------------------------------------------------------------------------ a chain that stays in HBM
CHAIN_SNR, CHAIN_LW, CHAIN_SEED, CHAIN_N = 23.0, 1e-5, 6, 5          # seed 6: the nearest boundary is 9.5e-4 away (of seeds 1 .. 24, 13 keep 1e-4)


def host_chain(x, d):
    """The host path on the impaired field: PilotSignal, phaserec.pilot_cpe, get_data, decisions.  ``(errors per mode, distance of the nearest
    payload sample to a decision boundary)``."""
    F, S, R, nfr = d["frame_len"], d["seq_len"], d["ins_rat"], d["nframes"]
    alphabet = d["alphabet_host"]
    sig = signals.PilotSignal(x, d["M"], 1., 1., F, S, R, d["pilots"].to_host(), symbols=d["payload"].to_host(), coded_symbols=alphabet)
    out, _ = phaserec.pilot_cpe(sig, N=CHAIN_N, use_seq=True, nframes=nfr)
    data = np.asarray(out.get_data())
    tx = np.tile(d["idx_tx"].to_host(), nfr)
    errors = [int(np.count_nonzero(synth.decide(r, alphabet) != t)) for r, t in zip(data, tx)]
    levels = np.unique(np.round(alphabet.real.astype(np.float64), 6))
    edges = (levels[1:] + levels[:-1]) / 2
    dist = min(float(np.min(np.abs(data.real[..., None] - edges))), float(np.min(np.abs(data.imag[..., None] - edges))))
    return errors, dist


def test_resident_chain_counts_the_host_path_s_errors():
    d = synth.make_pilot_frames_dev(64, 1024, 128, 16, nframes=3)
    F, S, R, nfr, NP, ND = d["frame_len"], d["seq_len"], d["ins_rat"], d["nframes"], d["NP"], d["ND"]
    dtype = np.complex64
    x = DeviceArray(d["frame"].shape, dtype)
    hip_dsp.impair_pointwise_dev(d["frame"], x, snr=(CHAIN_SNR, 1), phase=(CHAIN_LW, 1.0), seed=CHAIN_SEED)
    where = pilot_ref.positions(F, S, R)[0]
    Eout, trace = DeviceArray(x.shape, dtype), DeviceArray(x.shape, np.float32)
    hip_dsp.pilot_cpe_dev(x, where, F, nfr, d["pilots"], CHAIN_N, Eout, trace)
    frames = [DeviceArray((2, ND), dtype) for _ in range(nfr)]
    for f in range(nfr):
        hip_dsp.pilot_split_dev(Eout, F, S, R, [f], payload=frames[f])
    # nothing has been read back so far; the metrics of every frame against the one payload all frames repeat
    res = [ber_functions.cal_metrics_dev(frames[f], d["idx_tx"], d["alphabet"], sync="window") for f in range(nfr)]
    assert all(m["lag"] == 0 and m["rotation"] == 0 and m["compared"] == ND and m["tx_mode"] == r for fr in res for r, m in enumerate(fr))
    dev_errors = [sum(fr[r]["errors"] for fr in res) for r in range(2)]
    host_errors, dist = host_chain(x.to_host(), d)
    print("chain: errors per mode device %s host %s, nearest boundary %.3g" % (dev_errors, host_errors, dist))
    assert dist >= 1e-4, "choose other seeds: a payload sample of the host result lies %.3g from a decision boundary" % dist
    assert min(host_errors) > 0 and dev_errors == host_errors
