"""
Every instantiation of the segment trainer (train_seg_kernel, csrc/train_seg_*_{f32,f64,f32_ad}.hip) against the sequential recurrence.

The reference is exact: with the coarse correction off, no phase seeds and no acquisition, S passes of plain relaxation over S segments ARE the
sequential recurrence (the relaxation map is triangular: after pass p the segments 0 .. p - 1 are exact), so taps and the whole error trace are
compared element by element with the CPU oracle at the kernel's precision.  ``qh_pit_last_launch`` says which kernel took the passes: every case
states the (lanes per chain, taps per lane, padding taps, table size) it expects as literals - the tap counts come from an enumeration of
``seg_tpl`` (csrc/train_seg.h) done by hand, not from a copy of it - and a case that silently ran on another form fails.

Bars: those of test_lookahead_trainer_equals_direct_trainer (tests/test_gpu_parity.py) - complex128 rtol 1e-9 / atol 1e-11, complex64
rtol 2e-4 / atol 2e-5, five times the atol on the error trace.

Conditions on the inputs are assertions on the oracle alone (``_reference``, no GPU): phase-sensitive functions start from taps an oracle mcma
run converged; for the complex64 cases of the functions that take decisions (sbd, mddma, dd, rde, mrde) the oracle in complex64 and in
complex128 on the same values agree within a third of the complex64 bar - a near-tie that rounding flips in the REFERENCE must not be what a
kernel is measured against; cma2 (bounded only on short runs from converged taps) keeps its taps finite and within twice their start norm.
Alphabets above 16-QAM are generated at 40 dB SNR, where the distance of the equalised samples to a decision / partition boundary is
several standard deviations (28 dB: 1.5 sigma between the outer rings of 64-QAM rde).

The adaptive-step kernels (``*_f32_ad``) cannot be driven to the exact fixed point (the solver needs >= 16 segments and damps its corrections):
they get the check of test_adaptive_step_recipe_through_tier_b (tests/test_gpu_pit.py) with its bars, over the four tap layouts.
"""
import functools
import warnings

import numpy as np
import pytest

from oracle import oracle
from qampy_amd import synth, _lib
from qampy_amd._lib import DeviceArray
from qampy_amd.core.equalisation import hip_equalisation as hk
from qampy_amd.core.equalisation import equalisation as core_eq

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
RT = {"c64": np.float32, "c128": np.float64}
BAR = {"c128": dict(rtol=1e-9, atol=1e-11), "c64": dict(rtol=2e-4, atol=2e-5)}
ERR_ATOL = 5                                     # the error trace: atol x 5
DECIDING = ("sbd", "mddma", "dd", "rde", "mrde")
WARM = DECIDING + ("cma2",)                      # start from taps an oracle mcma run converged


def case(method, M, dn, ntaps, lanes, expect, nmodes=2, os_=2, S=4, blocks=5, extra=1, tail=37, niter=1, modes=None, ask=None, seed=99):
    """One row of the matrix.  ``lanes``: what seg_lanes is forced to; ``expect``: (lanes, taps per lane, padding taps, table size) the hook must
    report, or None for a shape the segment form must NOT take; the sweep has (S * blocks + extra) * 64 + tail steps; ``ask``: the segment
    count handed to the call when it differs from the S the report must show (a count the grid clips)."""
    return dict(method=method, M=M, dn=dn, ntaps=ntaps, lanes=lanes, expect=expect, nmodes=nmodes, os_=os_, S=S, blocks=blocks, extra=extra,
                tail=tail, niter=niter, modes=modes, ask=ask, seed=seed)


def _id(c):
    s = "%s%d-%s-%dtaps-l%d-m%d-os%d-S%d.%d.%d.%d-it%d" % (c["method"], c["M"], c["dn"], c["ntaps"], c["lanes"], c["nmodes"], c["os_"], c["S"],
                                                          c["blocks"], c["extra"], c["tail"], c["niter"])
    if c["modes"] is not None:
        s += "-sel" + "".join(str(m) for m in c["modes"])
    if c["ask"] is not None:
        s += "-ask%d" % c["ask"]
    return s


def _params(cases):
    return [pytest.param(c, id=_id(c)) for c in cases]


# ---------------------------------------------------------------------------------------------------------------- inputs and reference (CPU only)
@functools.lru_cache(maxsize=None)
def _capture(M, nmodes, os_, log2n, seed):
    snr = 28 if M <= 16 else 40
    sig = synth.make_capture(M, 2 ** log2n, nmodes=nmodes, os=os_, snr_db=snr, theta=np.pi / 5.6 if nmodes == 2 else None, dgd=30e-12, seed=seed,
                             dtype=np.complex128)
    return np.ascontiguousarray(np.asarray(sig)), np.asarray(sig.coded_symbols)


@functools.lru_cache(maxsize=None)
def _converged(M, nmodes, os_, log2n, seed, ntaps):
    """Start taps of the phase-sensitive functions: three mcma sweeps of the oracle (complex128) over the head of the capture."""
    E, _ = _capture(M, nmodes, os_, log2n, seed)
    tr = min(4096, (E.shape[1] - ntaps + 1) // os_)
    w0 = core_eq._init_taps(ntaps, nmodes, nmodes, np.complex128)
    s0 = np.ascontiguousarray(core_eq._reshape_symbols(None, "mcma", M, np.complex128, nmodes))
    _, w0, _ = oracle.train_equaliser(E, tr, 3, os_, 2e-3, w0, None, False, s0, "mcma")
    return w0


def _reference(c):
    """Arrays of a case at its precision, the oracle's result on them, and the conditions on the inputs (assertions on the oracle alone)."""
    method, M, dn, ntaps, nmodes, os_ = c["method"], c["M"], c["dn"], c["ntaps"], c["nmodes"], c["os_"]
    tr = (c["S"] * c["blocks"] + c["extra"]) * 64 + c["tail"]
    log2n = 13 if (tr - 1) * os_ + ntaps <= 2 ** 13 * os_ else 14
    E128, alphabet = _capture(M, nmodes, os_, log2n, c["seed"])
    assert (tr - 1) * os_ + ntaps <= E128.shape[1]
    ct, rt = CT[dn], RT[dn]
    E = np.ascontiguousarray(E128.astype(ct))
    w0 = _converged(M, nmodes, os_, log2n, c["seed"], ntaps) if method in WARM else core_eq._init_taps(ntaps, nmodes, nmodes, np.complex128)
    w0 = np.ascontiguousarray(w0.astype(ct))
    sy = np.ascontiguousarray(core_eq._reshape_symbols(alphabet if method in core_eq.DECISION_BASED else None, method, M, ct, nmodes))
    mu = rt(1e-4 if method == "cma2" else 3e-4)
    modes = None if c["modes"] is None else np.array(c["modes"], dtype=np.int64)
    eo, wo, _ = oracle.train_equaliser(E, tr, c["niter"], os_, mu, w0.copy(), modes, False, sy, method)
    assert np.all(np.isfinite(wo)) and np.all(np.isfinite(eo))
    if method == "cma2":
        assert c["S"] <= 3 and c["blocks"] <= 5, "cma2 stays bounded only on short runs from converged taps"
        assert np.linalg.norm(wo) <= 2 * np.linalg.norm(w0)
    if method in DECIDING and dn == "c64":
        # the reference's own rounding: complex64 against complex128 on the same values, within a third of the complex64 bar
        sy128 = np.ascontiguousarray(sy.astype(np.complex128))
        e2, w2, _ = oracle.train_equaliser(np.ascontiguousarray(E.astype(np.complex128)), tr, c["niter"], os_, np.float64(mu), w0.astype(np.complex128), modes,
                                           False, sy128, method)
        t = BAR["c64"]
        np.testing.assert_allclose(wo, w2, rtol=t["rtol"] / 3, atol=t["atol"] / 3)
        np.testing.assert_allclose(eo, e2, rtol=t["rtol"] / 3, atol=t["atol"] * ERR_ATOL / 3)
    return E, tr, w0, sy, mu, modes, eo, wo


def _run_pit(E, tr, niter, os_, mu, w0, sy, method, modes, pit):
    """The pit entry point on device arrays (in the manner of _run_pit of tests/test_gpu_pit.py): taps, error trace, report, launch record."""
    rt = np.float32 if E.dtype == np.complex64 else np.float64
    dE, dsy, dmu = DeviceArray.from_host(E), DeviceArray.from_host(sy), DeviceArray.from_host(np.array([mu], rt))
    dw, derr = DeviceArray.from_host(w0.copy()), DeviceArray((E.shape[0], tr * niter), E.dtype, zero=True)
    rep = hk.PitReportBuffer()
    hk.train_equaliser_dev(dE, tr, niter, os_, dmu, dw, modes, False, dsy, method, derr, pit=pit, report=rep)
    r = rep.read()
    return dw.to_host(), derr.to_host(), r, _lib.pit_last_launch()


def _check(c, forms):
    E, tr, w0, sy, mu, modes, eo, wo = _reference(c)              # (conditions on the inputs: before anything runs on the GPU)
    forms.set("pit_form", "segment")
    forms.set("seg_lanes", str(c["lanes"]))
    S, dn = c["S"], c["dn"]
    pit = dict(segments=c["ask"] if c["ask"] is not None else S, max_passes=S, tol=1e-14 if dn == "c128" else 1e-12, correction=0, phase_seed=0,
               acquire=0, exact_redo_off=1)
    w, e, rep, hook = _run_pit(E, tr, c["niter"], c["os_"], mu, w0, sy, c["method"], modes, pit)
    if c["expect"] is None:
        assert hook["form"] not in (0, 1), hook                   # a latency form took the passes - and says so
    else:
        lanes, tpl, rag, npart = c["expect"]
        assert hook == dict(form=1, lanes=lanes, tpl=tpl, rag=rag, npart=npart, adaptive=0), hook
    assert rep["segments"] == S and rep["passes"] == S, rep
    t = BAR[dn]
    sel = np.arange(c["nmodes"]) if modes is None else modes
    np.testing.assert_allclose(w[sel], wo[sel], **t)
    np.testing.assert_allclose(e, eo, rtol=t["rtol"], atol=t["atol"] * ERR_ATOL)
    rest = [m for m in range(c["nmodes"]) if m not in set(int(s) for s in sel)]
    assert not np.any(e[rest]), "rows of the error trace that belong to no selected mode stay zero"
    assert np.array_equal(w[rest], w0[rest])
    w2, e2, rep2, hook2 = _run_pit(E, tr, c["niter"], c["os_"], mu, w0, sy, c["method"], modes, pit)
    assert np.array_equal(w, w2) and np.array_equal(e, e2) and hook2 == hook, "a second identical call is bit-identical"


# ---------------------------------------------------------------------------------------------------------------- the matrix
# error function -> (alphabet, table size of the instantiation: partitions of rde / mrde, slicer levels of sbd / mddma / dd, 0 for the rest)
FUNCS = {"cma": (16, 0), "sgncma": (16, 0), "cma2": (16, 0), "mcma": (16, 0), "rde": (16, 2), "mrde": (64, 3), "sbd": (16, 3), "mddma": (64, 7), "dd": (16, 3)}
# 2 modes, 2 samples per symbol: taps -> (taps per lane, padding taps)
LAYOUT16 = {15: (2, 1), 21: (4, 3), 41: (6, 1), 37: (8, 3)}
LAYOUT8 = {21: (6, 3), 41: (11, 3)}


def _short(method):
    return dict(S=3, blocks=4, extra=1) if method == "cma2" else {}


def _function_by_precision():
    out = []
    for method, (M, npart) in FUNCS.items():
        for dn in ("c64", "c128"):
            for ntaps, (tpl, rag) in LAYOUT16.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart), **_short(method)))
        for ntaps, (tpl, rag) in LAYOUT8.items():
            out.append(case(method, M, "c64", ntaps, 8, (8, tpl, rag, npart), **_short(method)))
        out.append(case(method, M, "c128", 21, 8, (16, 4, 3, npart), **_short(method)))      # double precision has no 8-lane kernel: 16 lanes
    return out


@pytest.mark.parametrize("c", _params(_function_by_precision()))
def test_function_by_precision(c, forms):
    """Every error function in both precisions at one layout per taps-per-lane count (train_seg_<method>_{f32,f64}.hip)."""
    _check(c, forms)


def _layout_by_padding():
    out = []
    l16 = {16: (2, 0), 15: (2, 1), 20: (4, 0), 23: (4, 1), 22: (4, 2), 21: (4, 3), 36: (6, 0), 35: (6, 1), 46: (6, 2), 45: (6, 3), 38: (8, 2), 37: (8, 3)}
    l16_os1 = {56: (8, 0), 55: (8, 1)}
    l8 = {12: (6, 0), 23: (6, 1), 22: (6, 2), 21: (6, 3), 42: (11, 2), 41: (11, 3)}
    for method in ("mcma", "sbd", "mrde"):
        M, npart = FUNCS[method]
        for dn in ("c64", "c128"):
            for ntaps, (tpl, rag) in l16.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart)))
            for ntaps, (tpl, rag) in l16_os1.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart), os_=1))
        for ntaps, (tpl, rag) in l8.items():
            out.append(case(method, M, "c64", ntaps, 8, (8, tpl, rag, npart)))
        # 11 taps per lane without / with one padding tap: 2 modes would need 44 / 43 taps, which have no 16-lane layout (seg_supported asks for
        # one whatever the lane count) - four modes at 22 / 21 taps reach the same kernel
        out.append(case(method, M, "c64", 22, 8, (8, 11, 0, npart), nmodes=4, modes=(2, 0, 3, 1)))
        out.append(case(method, M, "c64", 21, 8, (8, 11, 1, npart), nmodes=4, modes=(2, 0, 3, 1)))
    return out


@pytest.mark.parametrize("c", _params(_layout_by_padding()))
def test_layout_by_padding(c, forms):
    """Every (taps per lane, padding taps) pair a filter can land on: the padding taps are the selects on a lane's last slots."""
    _check(c, forms)


def _mode_counts():
    out = []
    for method in ("mcma", "sbd"):
        M, npart = FUNCS[method]
        for dn in ("c64", "c128"):
            for ntaps, (tpl, rag) in {31: (2, 1), 48: (4, 0)}.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart), nmodes=1))
            for ntaps, (tpl, rag) in {96: (6, 0), 85: (8, 3)}.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart), nmodes=1, os_=1))
            for ntaps, (tpl, rag) in {8: (2, 0), 13: (4, 3), 22: (6, 2), 29: (8, 3)}.items():
                out.append(case(method, M, dn, ntaps, 16, (16, tpl, rag, npart), nmodes=4, modes=(2, 0, 3, 1)))
        for ntaps, (tpl, rag) in {12: (6, 0), 21: (11, 1)}.items():
            out.append(case(method, M, "c64", ntaps, 8, (8, tpl, rag, npart), nmodes=4, modes=(2, 0, 3, 1)))
    return out


@pytest.mark.parametrize("c", _params(_mode_counts()))
def test_mode_counts(c, forms):
    """1 mode (16 lanes of one input mode) and 4 modes, all four selected in a permuted order (4 / 2 lanes per input mode)."""
    _check(c, forms)


def _sampling_rates():
    out = []
    for method, (M, npart) in FUNCS.items():
        for os_ in (1, 2):
            out.append(case(method, M, "c64", 21, 16, (16, 4, 3, npart), os_=os_, **_short(method)))
    for method in ("mcma", "sbd"):
        M, npart = FUNCS[method]
        out.append(case(method, M, "c64", 15, 16, None, os_=3))               # 3 samples per symbol: a chunk does not fit the LDS row
        out.append(case(method, M, "c64", 43, 16, None))                      # 2 modes x 43 taps: no tap layout
        out.append(case(method, M, "c64", 43, 8, None))                       # ... whatever the lanes asked for (an 8-lane layout alone is not enough)
        out.append(case(method, M, "c64", 44, 8, None))
        out.append(case(method, M, "c64", 21, 16, None, modes=(1,)))          # one selected mode of two: a wave's chains span 4 segments = 8 rows
    return out


@pytest.mark.parametrize("c", _params(_sampling_rates()))
def test_sampling_rates_and_refused_shapes(c, forms):
    """Paired windows (2 samples per symbol) and the plain loop (any other rate) for every function; shapes the segment form cannot take
    must be reported as taken by another form - and still be the recurrence."""
    _check(c, forms)


# Which alphabet gives which table size (the hook confirms each):
#   rde   (rings: nsy = 2 n - 1 radii codes + partitions -> n - 1 partitions):  8-QAM 1, 16-QAM 2, 32-QAM (cross) 4, 64-QAM 8
#   mrde  (levels per axis):                                                    16-QAM 1, 32-QAM (cross) 2, 64-QAM 3, 128-QAM (cross) 5, 256-QAM 7
#   6 partitions: no alphabet; larger alphabets exceed the 8 partitions the kernels carry (128-QAM rde: 16, 1024-QAM mrde: 15)
#   sbd / mddma / dd (slicer thresholds per axis, square alphabets):            4-QAM 1, 16-QAM 3, 64-QAM 7, 256-QAM 15
PARTITIONS = {"rde": {8: 1, 16: 2, 32: 4, 64: 8}, "mrde": {16: 1, 32: 2, 64: 3, 128: 5, 256: 7}}
SLICERS = {4: 1, 16: 3, 64: 7, 256: 15}


def _tables():
    out = []
    for dn in ("c64", "c128"):
        for method, tab in PARTITIONS.items():
            for M, npart in tab.items():
                out.append(case(method, M, dn, 21, 16, (16, 4, 3, npart)))
        for method in ("sbd", "mddma", "dd"):
            for M, npart in SLICERS.items():
                out.append(case(method, M, dn, 21, 16, (16, 4, 3, npart)))
    return out


@pytest.mark.parametrize("c", _params(_tables()))
def test_table_sizes(c, forms):
    """Every partition count the host's alphabets produce for rde / mrde and every slicer size of the decision-directed functions."""
    _check(c, forms)


def _segment_grid():
    # (S, blocks per segment, segments with one block more, steps beyond the last block, sweeps)
    grid = [(2, 4, 0, 0, 1), (2, 5, 1, 1, 2), (3, 4, 2, 63, 1), (3, 8, 0, 1, 3), (5, 4, 0, 63, 1), (5, 5, 4, 0, 2), (8, 4, 7, 1, 1), (8, 8, 0, 63, 1),
            (24, 4, 0, 0, 1), (24, 5, 23, 63, 1), (24, 8, 0, 1, 1)]
    out = []
    for method in ("mcma", "sbd"):
        M, npart = FUNCS[method]
        for dn, lanes, lay in (("c64", 16, (16, 4, 3)), ("c64", 8, (8, 6, 3)), ("c128", 16, (16, 4, 3))):
            for S, blocks, extra, tail, niter in grid:
                out.append(case(method, M, dn, 21, lanes, lay + (npart,), S=S, blocks=blocks, extra=extra, tail=tail, niter=niter))
            # 12 segments asked of a sweep of 23 blocks: the grid holds 23 / 4 = 5 (4 blocks each, three of them 5), the report says so, and
            # 5 passes are the recurrence
            out.append(case(method, M, dn, 21, lanes, lay + (npart,), S=5, blocks=4, extra=3, tail=17, ask=12))
    return out


@pytest.mark.parametrize("c", _params(_segment_grid()))
def test_segment_grid(c, forms):
    """Segment counts 2 .. 24 (QH_PIT_MAXPASS: the most the fixed-point argument allows), segments of exactly 4 blocks (the minimum), 5 (ragged
    against the 128-step chunk of the long rows) and 8, none / all but one of them a block longer, tails of 0 / 1 / 63 steps, 1 - 3 sweeps, chain
    counts that do not fill the last wave (S = 3, 5: 6 and 10 chains for 4 or 8 chains per wave), a segment count the grid clips."""
    _check(c, forms)


# ---------------------------------------------------------------------------------------------------------------- adaptive-step units
@functools.lru_cache(maxsize=None)
def _adaptive_capture():
    sig = synth.make_capture(64, 2 ** 17, nmodes=2, snr_db=25, theta=np.pi / 3, dgd=30e-12, linewidth=0., seed=1000, dtype=np.complex64)
    return np.ascontiguousarray(np.asarray(sig)), np.asarray(sig.coded_symbols)


@pytest.mark.parametrize("ntaps,tpl,rag", [(13, 2, 1), (21, 4, 3), (41, 6, 1), (37, 8, 3)])
@pytest.mark.parametrize("method", ["cma", "mcma", "sbd", "mddma"])
def test_adaptive_step_units_through_tier_b(method, ntaps, tpl, rag):
    """train_seg_<method>_f32_ad.hip at 2 / 4 / 6 / 8 taps per lane: tier b against the exact entry point on the same 2^17-symbol 64-QAM capture,
    bars of test_adaptive_step_recipe_through_tier_b.  Blind functions start from centre-spike taps; decision functions run as the second
    stage behind mcma.  The last mode's solve must have run on the adaptive segment kernel with the stated layout and must not have been
    redone in the exact form."""
    E, alphabet = _adaptive_capture()
    mu = 1.9e-3
    blind = method in ("cma", "mcma")
    npart = 0 if blind else 7
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # nothing uncertified may come back
        if blind:
            kw = dict(Ntaps=ntaps, method=method, adaptive_stepsize=True)
            wa, ea = core_eq.equalise_signal(E, 2, mu, 64, **kw)
            wb, eb = core_eq.equalise_signal(E, 2, mu, 64, tier="b", **kw)
            ea, eb = [ea], [eb]
        else:
            kw = dict(Ntaps=ntaps, methods=("mcma", method), adaptive_stepsize=(True, True), symbols=alphabet, apply=False)
            wa, ea = core_eq.dual_mode_equalisation(E, 2, (mu, mu), 64, **kw)
            wb, eb = core_eq.dual_mode_equalisation(E, 2, (mu, mu), 64, tier="b", **kw)
    hook = _lib.pit_last_launch()
    reps = core_eq.last_pit_reports()
    assert len(reps) == len(ea) and all(r["converged"] for r in reps), reps
    for m in range(2):
        assert np.linalg.norm(wa[m] - wb[m]) / np.linalg.norm(wa[m]) < 3e-3
        for s, (a, b) in enumerate(zip(ea, eb)):
            assert np.sqrt(np.mean(np.abs(a[m] - b[m]) ** 2)) < (3e-3 if (blind or s == 0) else 5e-3)
    assert hook == dict(form=1, lanes=16, tpl=tpl, rag=rag, npart=npart, adaptive=1), hook
    assert not reps[-1]["per_mode"][-1]["exact_form"], reps[-1]
