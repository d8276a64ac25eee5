"""The float64 restatement of the pilot-frame kernels (tests/pilot_ref.py) against the reference's own results (tests/golden/pilotframe.npz,
gen_golden_pilotframe.py), and the properties of the shared cases.  No GPU.

Frames and splits are copies: bit for bit.  The estimates differ from the reference in the order of a few roundings - the reference averages
by differences of a cumulative sum and fits with np.polyfit, the restatement (like the kernels) sums every window directly and fits from
centred sums.  Measured distance of the restatement to the golden complex128 results, max-abs over max(1, max|ref|) (the field: over its rms),
and the bar, four times that:

    trace   1.6e-15  ->  7e-15         field   1.4e-14  ->  6e-14
    fit     2.3e-16  ->  1e-15         constant phase   5.1e-18  ->  2.5e-17   (phases of about 1e-3 rad)
"""
import os

import numpy as np
import pytest

import pilot_ref
from conftest import GOLDEN

BAR_TRACE, BAR_FIELD, BAR_FIT, BAR_CONST = 7e-15, 6e-14, 1e-15, 2.5e-17


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "pilotframe.npz"))


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref))))


@pytest.mark.parametrize("F,S,R", [(1024, 128, 16), (1000, 40, 2), (515, 3, 0), (96, 0, 32), (12, 12, 0), (9, 0, 3), (7, 1, 2), (5, 0, 0)])
def test_the_maps_are_a_bijection_in_order(F, S, R):
    NP, ND = pilot_ref.counts(F, S, R)
    pil, dat = pilot_ref.positions(F, S, R)
    assert pil.size == NP and dat.size == ND and NP + ND == F
    assert [pilot_ref.kind(F, S, R, int(i)) for i in pil] == [(True, k) for k in range(NP)]
    assert [pilot_ref.kind(F, S, R, int(i)) for i in dat] == [(False, k) for k in range(ND)]


@pytest.mark.parametrize("dt", ["c64", "c128"])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_assemble_and_split_reproduce_the_reference_frames(g, k, dt):
    M, F, S, R, nfr = (int(v) for v in g["geoms"][k])
    NP, ND = pilot_ref.counts(F, S, R)
    ref = pilot_ref.golden_frame(g, "f%d_%s_" % (k, dt))
    assert ref["pilots"].shape == (2, nfr * NP) and ref["payload"].shape == (2, nfr * ND)
    frame, idx = pilot_ref.assemble(ref["pilots"][:, :NP], ref["payload"][:, :ND], F, S, R, nfr, labels=ref["payload_labels"][:, :ND])
    assert frame.dtype == ref["frame"].dtype and np.array_equal(frame, ref["frame"])
    pay, pil = pilot_ref.split(frame, F, S, R, range(nfr))
    assert np.array_equal(pay, ref["payload"]) and np.array_equal(pil, ref["pilots"])
    pos_p, pos_d = pilot_ref.positions(F, S, R)
    assert np.all(idx[:, pos_p] == -1) and np.array_equal(idx[:, F * (nfr - 1) + pos_d], ref["payload_labels"][:, :ND])


@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_every_frame_its_own_payload(g, dt):
    M, F, S, R, nfr = (int(v) for v in g["geoms"][0])
    NP, ND = pilot_ref.counts(F, S, R)
    ref = pilot_ref.golden_frame(g, "f0nr_%s_" % dt)
    assert ref["payload"].shape == (2, nfr * ND)
    frame = pilot_ref.assemble(ref["pilots"][:, :NP], ref["payload"], F, S, R, nfr, repeat_data=False)
    assert np.array_equal(frame, ref["frame"])
    assert not np.array_equal(ref["payload"][:, :ND], ref["payload"][:, ND:2 * ND])
    rep = pilot_ref.golden_frame(g, "f0_%s_" % dt)
    assert np.array_equal(rep["payload"][:, :ND], ref["payload"][:, :ND])           # the same source, longer


def test_the_splits_of_the_impaired_signal(g):
    M, F, S, R, nfr = (int(v) for v in g["geoms"][0])
    pay, pil = pilot_ref.split(g["est_x"], F, S, R, range(nfr))
    assert np.array_equal(pay, g["get_data"]) and np.array_equal(pil, g["extract_pilots"])
    pay, pil = pilot_ref.split(g["est_x"], F, S, R, [2, 0])
    NP, ND = pilot_ref.counts(F, S, R)
    assert np.array_equal(pay[:, :ND], g["get_data"][:, 2 * ND:]) and np.array_equal(pil[:, NP:], g["extract_pilots"][:, :NP])


@pytest.mark.parametrize("call", [0, 1, 2])
def test_carrier_phase_against_the_reference(g, call):
    name, _, args = pilot_ref.golden_cpe_calls(g)[call]
    field, trace, margin = pilot_ref.cpe(**args)
    assert margin >= (float(g["est_margin_cpe3"]) - 1e-12 if name == "cpe3" else pilot_ref.MARGIN)
    E, ph = g[name + "_E"], g[name + "_ph"]
    assert field.shape == E.shape and trace.shape == ph.shape
    d_trace, d_field = rel(trace, ph), float(np.max(np.abs(field - E)) / np.sqrt(np.mean(np.abs(E) ** 2)))
    print("%s: trace %.2e field %.2e" % (name, d_trace, d_field))
    assert d_trace <= BAR_TRACE and d_field <= BAR_FIELD


def test_offset_and_constant_phase_against_the_reference(g):
    M, F, S, R, nfr = (int(v) for v in g["geoms"][0])
    pil = pilot_ref.golden_frame(g, "f0_c128_")["pilots"]
    fit, margin = pilot_ref.foe(g["est_x"][:, :S], pil[:, :S])
    assert margin >= pilot_ref.MARGIN
    d_fit = max(rel(fit[:, 0], g["foe_modes"][:, 0]), rel(fit[:, 1], g["foe_icpt"][:, 0]))
    assert abs(np.mean(fit[:, 0]) - float(g["foe_mean"])) <= BAR_FIT
    assert abs(np.mean(fit[:, 0]) - float(g["est_fo"])) < 1e-4                       # and it is the offset that was put in
    c, margin = pilot_ref.const_phase(g["const_rec"], g["const_ref"])
    assert margin >= pilot_ref.MARGIN
    d_const = rel(c, g["const_ph"][:, 0])
    print("fit %.2e constant phase %.2e" % (d_fit, d_const))
    assert d_fit <= BAR_FIT and d_const <= BAR_CONST


def test_the_stored_margins_hold(g):
    assert float(g["est_margin"]) >= pilot_ref.MARGIN and float(g["est_margin_cpe3"]) >= 0.05


@pytest.mark.parametrize("case", pilot_ref.cases(), ids=lambda c: c["name"])
def test_every_case_keeps_its_unwrap_margin(case):
    a = case["make"]()
    N = a.pop("N")
    assert np.array_equal(a["E"] * 4096, np.round(a["E"] * 4096)) and np.array_equal(a["sent"] * 4096, np.round(a["sent"] * 4096))
    assert np.array_equal(a["E"].astype(np.complex64).astype(np.complex128), a["E"])
    ph, margin, pos, K = pilot_ref.phase(**a)
    assert margin >= pilot_ref.MARGIN
    if N is not None:
        assert 3 <= N <= pilot_ref.N_MAX and N % 2 == 1 and N <= ph.shape[1]
        kph, kpos = pilot_ref.knots(ph, N, pos)
        assert kph.shape == (ph.shape[0], ph.shape[1] - N + 1) and kpos.size == kph.shape[1] and np.all(np.diff(kpos) > 0)
    rec = a["E"][:, pos]
    ref = a["sent"][:, np.arange(pos.size) % a["sent"].shape[1]]
    assert np.allclose(pilot_ref.pair_phase(rec, ref)[0], ph, rtol=0, atol=1e-12)


def test_the_case_list_covers_what_the_kernels_tile_by():
    seen = {}
    for c in pilot_ref.cases():
        a = c["make"]()
        n = pilot_ref.used(a["where"], a["F"], a["nframes"], a["span"] or a["E"].shape[1]).size
        seen[c["name"]] = (n, a["N"], a["E"].shape[0], a["sent"].shape[1] != a["where"].size, a["span"] is not None)
    ns = {v[0] for v in seen.values()}
    assert {1, 2, 1023, 1024, 1025, 2049} <= ns and any(v[0] == v[1] for v in seen.values())
    assert {3, pilot_ref.N_MAX} <= {v[1] for v in seen.values()} and {1, 3} <= {v[2] for v in seen.values()}
    assert any(v[3] and v[0] > 6 for v in seen.values()) and any(v[4] for v in seen.values())


def test_the_wrap_ramp_wraps_where_it_was_built_to():
    E, sent, at = pilot_ref.wrap_ramp()
    ph, margin, pos, K = pilot_ref.phase(E, [0], 2, 2049, sent)
    assert margin >= pilot_ref.MARGIN and at == (pilot_ref.UW_CHUNK - 1, pilot_ref.UW_CHUNK, pilot_ref.UW_CHUNK + 1)
    assert list(np.diff(K[0])[at[0] - 1:at[2]]) == [1, -1, 1]
    assert np.count_nonzero(np.diff(K[0])) == 3                                      # and nowhere else


def test_the_long_row_is_long():
    a = pilot_ref.long_row()
    N = a.pop("N")
    field, trace, margin = pilot_ref.cpe(N=N, **a)
    assert margin >= pilot_ref.MARGIN and trace.shape == (1, 2 ** 20 + 1024) and np.ptp(trace) > 20
    assert (trace.shape[1] + pilot_ref.UW_CHUNK - 1) // pilot_ref.UW_CHUNK > 1024
