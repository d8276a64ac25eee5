"""Digital pre-compensation on the GPU (csrc/precomp.hip): pattern numbers, the dyadic look-up tables and their counts bit for bit against the
float64 restatement of tests/precomp_ref.py and the reference's own results (tests/golden/precomp.npz); the noisy table, the applied table, the
arcsin and the DAC pre-emphasis against the restatement to the project's bars; a pre-distortion loop that stays in HBM; and the mirrored API
against the reference's complex128 results.

Inputs of the shared cases are multiples of 2^-10 with |tx - rx| <= 1, so complex64 and complex128 hold the same values and every sum is exact
in float32, in double and in the kernels' 64-bit fixed point (tests/test_precomp_ref.py asserts on the restatement alone that no sample sits
within 2^-11 of a decision boundary, but for the tie row).  Bars, those of tests/test_gpu_cpr.py and tests/test_gpu_pilotframe.py: 1e-5
(complex64) and 1e-11 (complex128); tables as max-abs over max(1, max |ref|), fields as max-abs over the reference's rms.

Measured maxima on an MI355X:
                 noisy table   applied field   arcsin    p_f       pre-emphasised field   loop, 2nd capture   loop, 1st rms
    complex64    0             5.0e-8          4.6e-8    4.9e-8    8.8e-7                 8.4e-8              1.5e-7
    complex128   2.0e-15       8.6e-18         1.7e-16   1.7e-15   2.6e-15                0                   0
(the table is complex128 and p_f is formed in double in both precisions).  Mirrored API against the golden complex128 results: arcsin
1.2e-16, p_f 1.7e-15, applied field 0, table from complex64 sent and complex128 received 0; tables and pattern numbers equal.
"""
import os

import numpy as np
import pytest

import precomp_ref as pr
from conftest import GOLDEN
from qampy_amd import _lib, synth
from qampy_amd._lib import DeviceArray
from qampy_amd.core import digital_pre_compensation as dpc
from qampy_amd.core import hip_dsp

pytestmark = pytest.mark.gpu

DT = [np.complex64, np.complex128]
IDS = ["c64", "c128"]
BAR = {np.complex64: 1e-5, np.complex128: 1e-11}
BAR_GOLDEN = 1e-11
G = np.load(os.path.join(GOLDEN, "precomp.npz"))
CASES = pr.cases()
_REF = {}


def rel(a, ref, floor=1.0):
    """max-abs over max(floor, max |ref|); ref is finite, and a NaN or an infinity in ``a`` makes the result NaN, which passes no bar"""
    assert np.all(np.isfinite(ref))
    return float(np.max(np.abs(np.asarray(a, dtype=np.result_type(ref.dtype, np.float64)) - ref)) / max(floor, np.max(np.abs(ref))))


def rel_where_finite(a, ref):
    """:func:`rel` over the entries where ref is finite (the NaN places themselves are compared by the caller)"""
    ok = np.isfinite(ref)
    return rel(a[ok], ref[ok])


def rel_rms(a, ref):
    return float(np.max(np.abs(a.astype(np.complex128) - ref)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def levels(kind):
    return hip_dsp.PatternLevels(*pr.levels_of(kind))


def table_size(kind, mem_len):
    lev_I, _, alphabet = pr.levels_of(kind)
    return (lev_I.size if alphabet is None else alphabet.size) ** mem_len


def ref_index(kind, mem_len, rows):
    """The restatement's index rows of an (nmodes, L) input, int32 as the device writes them"""
    both = [pr.pattern_index(x, *pr.levels_of(kind), mem_len) for x in rows]
    return np.array([b[0] for b in both], np.int32), np.array([b[1] for b in both], np.int32)


def lut_ref(name):
    """Index rows and, per mask, table and counts of a table case: computed once, left unchanged"""
    if name not in _REF:
        c = next(c for c in CASES["lut"] if c["name"] == name)
        a, b = pr.pattern_index(c["tx"], *pr.levels_of(c["kind"]), c["mem_len"])
        N = table_size(c["kind"], c["mem_len"])
        _REF[name] = dict(c, I=a, Q=b, N=N, tables={w: pr.lut(c["tx"], c["rx"], a, b, N, pr.mask_of(w, c["L"])) for w in pr.LUT_MASKS})
    return _REF[name]


# ------------------------------------------------------------------------------------------------ pattern index
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("i", range(len(pr.INDEX_CASES)), ids=["%s-m%d-L%d" % c[:3] for c in pr.INDEX_CASES])
def test_pattern_index_is_the_restatements(i, dt):
    c = CASES["index"][i]
    x = c["x"].reshape(1, -1)
    wI, wQ = ref_index(c["kind"], c["mem_len"], x)
    if "idx_%d_I" % i in G.files:
        assert np.array_equal(wI[0], G["idx_%d_I" % i]) and np.array_equal(wQ[0], G["idx_%d_Q" % i])
    iI, iQ = hip_dsp.pattern_index_dev(DeviceArray.from_host(x.astype(dt)), levels(c["kind"]), c["mem_len"])
    assert np.array_equal(iI.to_host(), wI) and np.array_equal(iQ.to_host(), wQ)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kind,mem_len,L", [("r8", 3, 1025), ("c16", 3, 257), ("r2", 7, 5)])
def test_pattern_index_of_three_modes(kind, mem_len, L, dt):
    x = np.array([pr.symbols(kind, L, 40 + m) for m in range(3)])
    wI, wQ = ref_index(kind, mem_len, x)
    E = DeviceArray.from_host(x.astype(dt))
    iI, iQ = hip_dsp.pattern_index_dev(E, levels(kind), mem_len)
    assert np.array_equal(iI.to_host(), wI) and np.array_equal(iQ.to_host(), wQ)
    only_Q = DeviceArray(E.shape, np.int32)
    assert hip_dsp.pattern_index_dev(E, levels(kind), mem_len, idx_Q=only_Q) == (None, only_Q) and np.array_equal(only_Q.to_host(), wQ)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("name", ["tie", "nan"])
def test_a_tie_goes_down_and_a_nan_to_level_0(name, dt):
    x = CASES[name].reshape(1, -1)
    iI, iQ = hip_dsp.pattern_index_dev(DeviceArray.from_host(x.astype(dt)), levels("r4"), 3)
    assert np.array_equal(iI.to_host()[0], G[name + "_I"]) and np.array_equal(iQ.to_host()[0], G[name + "_Q"])


def test_many_levels_are_searched_outside_lds():
    """more than 256 levels per rail: bisection in global memory; 1000 and 300 levels, a NaN and two infinities among the samples"""
    rng = np.random.default_rng(5)
    lev_I, lev_Q = np.cumsum(rng.integers(1, 5, 1000)) / 4.0, np.cumsum(rng.integers(1, 5, 300)) / 8.0
    x = (rng.integers(-8, 4 * int(lev_I[-1]) + 8, 2000) / 4.0 + 1 / 16) + 1j * (rng.integers(-8, 8 * int(lev_Q[-1]) + 8, 2000) / 8.0 + 1 / 32)
    x[3], x[4], x[5] = complex(np.nan, 1), complex(np.inf, -np.inf), complex(lev_I[500], lev_Q[10])
    wI, wQ = pr.pattern_index(x, lev_I, lev_Q, None, 2)
    iI, iQ = hip_dsp.pattern_index_dev(DeviceArray.from_host(x.reshape(1, -1)), hip_dsp.PatternLevels(lev_I, lev_Q), 2)
    assert np.array_equal(iI.to_host()[0], wI) and np.array_equal(iQ.to_host()[0], wQ)


# ------------------------------------------------------------------------------------------------ look-up table
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("which", pr.LUT_MASKS)
@pytest.mark.parametrize("name", [c[0] for c in pr.LUT_CASES])
def test_the_dyadic_table_is_the_references_bit_for_bit(name, which, dt):
    r = lut_ref(name)
    want, wnI, wnQ = r["tables"][which]
    at, val = pr.nonzero_table(want)
    assert np.array_equal(at, G["lut_%s_%s_at" % (name, which)]) and np.array_equal(val, G["lut_%s_%s_ea" % (name, which)])
    mask = pr.mask_of(which, r["L"])
    dmask = None if mask is None else DeviceArray.from_host(mask.astype(np.uint8))
    tx, rx = DeviceArray.from_host(r["tx"].astype(dt).reshape(1, -1)), DeviceArray.from_host(r["rx"].astype(dt).reshape(1, -1))
    ea, iI, iQ, nI, nQ = hip_dsp.cal_lut_dev(tx, rx, levels(r["kind"]), r["mem_len"], idx_data=dmask)
    got = ea.to_host()
    assert got.dtype == np.complex128 and got.shape == (1, r["N"])
    assert np.array_equal(iI.to_host()[0], r["I"]) and np.array_equal(iQ.to_host()[0], r["Q"])
    assert np.array_equal(nI.to_host()[0], wnI) and np.array_equal(nQ.to_host()[0], wnQ)
    assert np.array_equal(got[0], want)
    if which == "empty":
        assert not got.any()
    # a second call into other buffers: the same bits
    ea2, _, _, nI2, nQ2 = hip_dsp.cal_lut_dev(tx, rx, levels(r["kind"]), r["mem_len"], idx_data=dmask)
    assert np.array_equal(ea2.to_host().view(np.uint64), got.view(np.uint64)) and np.array_equal(nI2.to_host(), nI.to_host()) and np.array_equal(nQ2.to_host(), nQ.to_host())


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("name", ["lds", "mid"])
def test_the_table_of_three_modes_with_a_mask_per_mode(name, dt):
    """rows and masks differ per mode: the LDS path and the global path each keep the modes apart"""
    c = lut_ref(name)
    rows = [pr.capture(c["kind"], 1500, 60 + m) for m in range(3)]
    masks = np.array([np.arange(1500) % (m + 2) == 0 for m in range(3)])
    tx, rx = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    ea, iI, iQ, nI, nQ = hip_dsp.cal_lut_dev(DeviceArray.from_host(tx.astype(dt)), DeviceArray.from_host(rx.astype(dt)), levels(c["kind"]), c["mem_len"],
                                             idx_data=DeviceArray.from_host(masks.astype(np.uint8)))
    got, gI, gQ = ea.to_host(), nI.to_host(), nQ.to_host()
    for m in range(3):
        a, b = pr.pattern_index(tx[m], *pr.levels_of(c["kind"]), c["mem_len"])
        want, wnI, wnQ = pr.lut(tx[m], rx[m], a, b, c["N"], masks[m])
        assert np.array_equal(got[m], want) and np.array_equal(gI[m], wnI) and np.array_equal(gQ[m], wnQ), m


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kind,mem_len", [("r4", 3), ("r8", 5)])
def test_the_noisy_table(kind, mem_len, dt):
    """Gaussian errors, 4096 symbols: the fixed-point sums against the float64 restatement, and the same bits on a second call"""
    rng = np.random.default_rng(77)
    tx = pr.symbols(kind, 4096, 70).astype(dt)
    rx = (tx - 0.3 * (rng.standard_normal(4096) + 1j * rng.standard_normal(4096))).astype(dt)
    a, b = pr.pattern_index(tx, *pr.levels_of(kind), mem_len)
    N = table_size(kind, mem_len)
    want, wnI, wnQ = pr.lut(tx, rx, a, b, N)
    err = tx.astype(np.complex128) - rx.astype(np.complex128)
    dtx, drx = DeviceArray.from_host(tx.reshape(1, -1)), DeviceArray.from_host(rx.reshape(1, -1))
    ea, _, _, nI, nQ = hip_dsp.cal_lut_dev(dtx, drx, levels(kind), mem_len)
    got = ea.to_host()
    worst = float(np.max(np.abs(got[0] - want)) / max(1.0, np.abs(err.real).max(), np.abs(err.imag).max()))
    print("noisy table %s N=%d: %.3g" % (np.dtype(dt).name, N, worst))
    assert np.array_equal(nI.to_host()[0], wnI) and np.array_equal(nQ.to_host()[0], wnQ)
    assert worst <= BAR[dt]
    ea2 = hip_dsp.cal_lut_dev(dtx, drx, levels(kind), mem_len)[0]
    assert np.array_equal(ea2.to_host().view(np.uint64), got.view(np.uint64))


# ------------------------------------------------------------------------------------------------ apply and predistort
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("name,gain", [("lds", 1.0), ("mid", -0.75), ("cplx", 0.5)])
def test_apply_and_predistort(name, gain, dt):
    r = lut_ref(name)
    lv = levels(r["kind"])
    table = r["tables"]["full"][0] * (1 + 2.0 ** -7) + 3e-3                        # (values that do not sit on the input's grid)
    sig = np.array([r["tx"], r["tx"][::-1]]).astype(dt)
    tables = np.array([table, -table[::-1]])
    idx = [pr.pattern_index(s, *pr.levels_of(r["kind"]), r["mem_len"]) for s in sig]
    want = np.array([pr.apply_lut(s, t, a, b, gain) for s, t, (a, b) in zip(sig, tables, idx)])
    E, ea = DeviceArray.from_host(sig), DeviceArray.from_host(tables)
    iI, iQ = hip_dsp.pattern_index_dev(E, lv, r["mem_len"])
    out = hip_dsp.lut_apply_dev(E, ea, iI, iQ, DeviceArray(E.shape, dt), gain=gain).to_host()
    worst = rel_rms(out, want)
    print("applied field %s %s: %.3g" % (name, np.dtype(dt).name, worst))
    assert out.dtype == dt and worst <= BAR[dt]
    fused = hip_dsp.lut_predistort_dev(E, lv, r["mem_len"], ea, DeviceArray(E.shape, dt), gain=gain).to_host()
    assert np.array_equal(fused.view(out.real.dtype), out.view(out.real.dtype))                    # exactly index + apply
    assert np.array_equal(E.to_host(), sig)
    same = hip_dsp.lut_apply_dev(E, ea, iI, iQ, E, gain=gain)
    assert same is E and np.array_equal(E.to_host().view(out.real.dtype), out.view(out.real.dtype))      # in place


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_pointwise_kernels_on_odd_rows_and_row_views(dt):
    """Three rows of 257 samples - every row but the first starts on an odd sample - and row 1 of them as a view of its own (8-byte aligned
    only), read into another buffer and written in place: a row's result does not depend on where the row lies."""
    r = lut_ref("lds")
    x = np.array([r["tx"][:257], r["tx"][300:557], r["tx"][600:857]]).astype(dt)
    idx = [pr.pattern_index(s, *pr.levels_of("r4"), 3) for s in x]
    table = np.array([r["tables"]["full"][0] * (m + 1) + 1e-3 for m in range(3)])
    want = np.array([pr.apply_lut(s, t, a, b, 0.5) for s, t, (a, b) in zip(x, table, idx)])
    E, ea = DeviceArray.from_host(x), DeviceArray.from_host(table)
    iI, iQ = hip_dsp.pattern_index_dev(E, levels("r4"), 3)
    out = hip_dsp.lut_apply_dev(E, ea, iI, iQ, DeviceArray(E.shape, dt), gain=0.5).to_host()
    assert np.isfinite(out.view(out.real.dtype)).all() and rel_rms(out, want) <= BAR[dt]
    one = DeviceArray((1, 257), dt)
    got = hip_dsp.lut_apply_dev(_row_view(E, 1), _row_view(ea, 1), _row_view(iI, 1), _row_view(iQ, 1), one, gain=0.5).to_host()
    assert np.array_equal(got[0].view(out.real.dtype), out[1].view(out.real.dtype))
    y = (x / 4).astype(dt)
    S = DeviceArray.from_host(y)
    sin_all = hip_dsp.comp_mod_sin_dev(S, DeviceArray(S.shape, dt), vpi=1.2 + 0.9j).to_host()
    assert rel(sin_all.real, pr.comp_mod_sin(y, 1.2 + 0.9j).real) <= BAR[dt] and rel(sin_all.imag, pr.comp_mod_sin(y, 1.2 + 0.9j).imag) <= BAR[dt]
    row = _row_view(S, 1)
    hip_dsp.comp_mod_sin_dev(row, row, vpi=1.2 + 0.9j)                               # row 1 in place, rows 0 and 2 untouched
    after = S.to_host()
    assert np.array_equal(after[1].view(out.real.dtype), sin_all[1].view(out.real.dtype)) and np.array_equal(after[[0, 2]], y[[0, 2]])


def _row_view(a, i):
    """row i of a 2-d DeviceArray as a 2-d array of one row"""
    v = a.row(i)
    v.shape = (1,) + tuple(v.shape)
    return v


# ------------------------------------------------------------------------------------------------ arcsin
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("vpi", [1.14, 1.2 + 0.9j], ids=["real", "complex"])
@pytest.mark.parametrize("clip", [0, 1.0, 0.9])
def test_comp_mod_sin(clip, vpi, dt):
    x = pr.mod_sin_input()
    x = np.array([x, -x[::-1]]).astype(dt)
    want = pr.comp_mod_sin(x, vpi, clip)
    E = DeviceArray.from_host(x)
    got = hip_dsp.comp_mod_sin_dev(E, DeviceArray(E.shape, dt), vpi=vpi, clip=clip).to_host()
    assert got.dtype == dt
    assert np.array_equal(np.isnan(got.real), np.isnan(want.real)) and np.array_equal(np.isnan(got.imag), np.isnan(want.imag))
    if clip:
        assert not np.isnan(got.real).any() and not np.isnan(got.imag).any()
    else:
        assert np.isnan(got.imag).any() and not np.isnan(got.imag[np.abs(x.imag) <= 1]).any()
    worst = max(rel_where_finite(got.real, want.real), rel_where_finite(got.imag, want.imag))
    print("arcsin %s clip %s: %.3g" % (np.dtype(dt).name, clip, worst))
    assert worst <= BAR[dt]
    assert hip_dsp.comp_mod_sin_dev(E, E, vpi=vpi, clip=clip) is E and np.array_equal(E.to_host().view(got.real.dtype), got.view(got.real.dtype), equal_nan=True)


# ------------------------------------------------------------------------------------------------ DAC pre-emphasis
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", pr.DAC_CASES, ids=[c[0] for c in pr.DAC_CASES])
def test_comp_dac_resp_against_the_golden_table(case, dt):
    name, fb, n, beta, papr, prms, os_ = case
    want = G["dac_" + name]
    tab = hip_dsp.comp_dac_resp_dev(fb, n, beta, PAPR=papr, prms_dac=prms, os=os_, dtype=dt)
    got = tab.to_host()
    assert got.dtype == dt and got.shape == (n,)
    worst = rel(got, want)
    print("p_f %s %s: %.3g" % (name, np.dtype(dt).name, worst))
    assert np.isfinite(got).all() and worst <= BAR[dt]
    assert np.array_equal(got == 0, want == 0)                                     # the bins on the band edges fall as the reference's
    again = hip_dsp.comp_dac_resp_dev(fb, n, beta, PAPR=papr, prms_dac=prms, os=os_, dtype=dt, out=DeviceArray((n,), dt))
    assert np.array_equal(again.to_host().view(got.real.dtype), got.view(got.real.dtype))


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", [pr.DAC_CASES[0], pr.DAC_CASES[4]], ids=["d256", "d1000alt"])
def test_dac_preemphasis_is_the_filter(case, dt):
    name, fb, n, beta, papr, prms, os_ = case
    rng = np.random.default_rng(9)
    x = (rng.integers(-2048, 2049, (2, n)) / 1024 + 1j * rng.integers(-2048, 2049, (2, n)) / 1024).astype(dt)
    want = np.fft.ifft(G["dac_" + name] * np.fft.fft(x.astype(np.complex128), axis=-1), axis=-1)
    E = DeviceArray.from_host(x)
    got = hip_dsp.dac_preemphasis_dev(E, DeviceArray(E.shape, dt), fb, beta, PAPR=papr, prms_dac=prms, os=os_).to_host()
    worst = rel_rms(got, want)
    print("pre-emphasised field %s %s: %.3g" % (name, np.dtype(dt).name, worst))
    assert got.dtype == dt and worst <= BAR[dt]


# ------------------------------------------------------------------------------------------------ a loop that stays in HBM
@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_a_predistortion_loop_in_hbm(dt):
    """16-QAM from the device's bit source; the channel adds a fixed dyadic function of the 3-symbol rail pattern of the TRANSMITTED symbols (its
    index rows and table made on the host once, from the restatement).  One capture teaches the table, the pre-distorted second capture arrives
    clean."""
    nsym = 4096
    src = synth.make_symbols_dev(16, nsym, nmodes=2, dtype=dt)
    tx = src["symbols"]
    lv = hip_dsp.pattern_levels(src["alphabet_host"])
    assert lv.M == 4 and lv.N(3) == 64
    host = tx.to_host()
    idx = [pr.pattern_index(row, lv.lev_I, lv.lev_Q, None, 3) for row in host]
    rng = np.random.default_rng(3)
    D = (rng.integers(-64, 65, (2, 64)) + 1j * rng.integers(-64, 65, (2, 64))) / 1024.0       # |D| <= 1/16 per rail: no decision moves
    chI, chQ = DeviceArray.from_host(np.array([i[0] for i in idx], np.int32)), DeviceArray.from_host(np.array([i[1] for i in idx], np.int32))
    chD = DeviceArray.from_host(D)
    dist = np.array([D[m][idx[m][0]].real + 1j * D[m][idx[m][1]].imag for m in range(2)])

    def channel(s, out):
        return hip_dsp.lut_apply_dev(s, chD, chI, chQ, out)
    rx1 = channel(tx, DeviceArray(tx.shape, dt))
    ea, _, _, nI, nQ = hip_dsp.cal_lut_dev(tx, rx1, lv, 3)
    pre = hip_dsp.lut_predistort_dev(tx, lv, 3, ea, DeviceArray(tx.shape, dt))
    rx2 = channel(pre, DeviceArray(tx.shape, dt))
    ref = host.astype(np.complex128)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    e1, e2 = ref - rx1.to_host(), ref - rx2.to_host()
    first = abs(np.sqrt(np.mean(np.abs(e1) ** 2)) - np.sqrt(np.mean(np.abs(dist) ** 2))) / np.sqrt(np.mean(np.abs(dist) ** 2))
    second = float(np.max(np.abs(e2)) / rms)
    print("loop %s: 2nd capture %.3g, 1st rms %.3g" % (np.dtype(dt).name, second, first))
    assert nI.to_host().sum() == nQ.to_host().sum() == 2 * nsym
    assert first <= BAR[dt] and second <= BAR[dt]
    seen = nI.to_host() > 0
    table = ea.to_host()
    assert np.isfinite(table.view(np.float64)).all() and rel(table.real[seen], -D.real[seen]) <= BAR[dt] and rel(table.imag[nQ.to_host() > 0], -D.imag[nQ.to_host() > 0]) <= BAR[dt]


# ------------------------------------------------------------------------------------------------ mirrored API
def test_mirrored_api_against_the_golden_results():
    worst = {}
    for c in CASES["lut"]:
        ref_sym, real_ptrns = pr.ref_sym_of(c["kind"])
        for which in ("full", "third"):
            mask = pr.mask_of(which, c["L"])
            ea, iI, iQ = dpc.cal_lut(c["tx"], c["rx"], ref_sym, mem_len=c["mem_len"], idx_data=mask, real_ptrns=real_ptrns)
            sel = slice(None) if mask is None else np.flatnonzero(mask)
            assert ea.dtype == np.complex128 and ea.ndim == 1 and iI.dtype == iQ.dtype == np.int64
            at, val = pr.nonzero_table(ea)
            assert np.array_equal(at, G["lut_%s_%s_at" % (c["name"], which)]) and np.array_equal(val, G["lut_%s_%s_ea" % (c["name"], which)])
            assert np.array_equal(iI, G["lut_%s_I" % c["name"]][sel]) and np.array_equal(iQ, G["lut_%s_Q" % c["name"]][sel])
        ea32, _, _ = dpc.cal_lut(c["tx"].astype(np.complex64), c["rx"].astype(np.complex64), ref_sym, mem_len=c["mem_len"], real_ptrns=real_ptrns)
        assert ea32.dtype == np.complex128 and np.array_equal(pr.nonzero_table(ea32)[1], G["lut_%s_full_ea" % c["name"]])
    c = CASES["lut"][0]                     # complex64 sent, complex128 received: the error is formed in complex128, as numpy promotes
    rx_fine = c["rx"] + 2.0 ** -40
    ea_mixed = dpc.cal_lut(c["tx"].astype(np.complex64), rx_fine, pr.ref_sym_of(c["kind"])[0], mem_len=c["mem_len"])[0]
    want_mixed = pr.lut(c["tx"], rx_fine, *pr.pattern_index(c["tx"], *pr.levels_of(c["kind"]), c["mem_len"]), 64)[0]
    worst["mixed dtypes"] = rel(ea_mixed, want_mixed)
    assert np.abs(ea_mixed.real - G["lut_lds_full_ea"].real).max() > 2.0 ** -41          # (a cast of rx to complex64 would lose the 2^-40)
    for i, c in enumerate(CASES["index"]):
        if "idx_%d_I" % i not in G.files or c["L"] < 2:
            continue
        lev_I, lev_Q, alphabet = pr.levels_of(c["kind"])
        h = c["mem_len"] // 2
        if alphabet is None:
            got = dpc.find_sym_patterns(c["x"].real, lev_I, c["mem_len"])
        else:
            got = dpc.find_sym_patterns(c["x"], alphabet, c["mem_len"])
        assert got.dtype == np.int64 and np.array_equal(got, np.roll(G["idx_%d_I" % i], -h)), i
    x = CASES["index"][3]["x"]
    shuffled = np.array([1., -3., 3., -1.])                                          # a table that is not sorted keeps its own numbering
    got, ptrns = dpc.find_sym_patterns(x.real, shuffled, 2, ret_ptrns=True)
    lev = pr.decide(x.real, shuffled)
    assert np.array_equal(got, lev * 4 + np.roll(lev, -1)) and ptrns.shape == (16, 2) and np.array_equal(ptrns[got[0]], shuffled[[lev[0], lev[1]]])
    x = G["sin_x"]
    for key, vpi in (("sin_real", 1.14), ("sin_cplx", 1.2 + 0.9j)):
        got, want = dpc.comp_mod_sin(x, vpi), G[key]
        assert got.dtype == np.complex128 and np.array_equal(np.isnan(got.real), np.isnan(want.real)) and np.array_equal(np.isnan(got.imag), np.isnan(want.imag))
        worst["arcsin"] = max(worst.get("arcsin", 0), rel_where_finite(got.real, want.real), rel_where_finite(got.imag, want.imag))
    assert dpc.comp_mod_sin(x.astype(np.complex64)).dtype == np.complex64
    for name, fb, n, beta, papr, prms, os_ in pr.DAC_CASES:
        got = dpc.comp_dac_resp(fb, n, beta, PAPR=papr, prms_dac=prms, os=os_)
        assert got.dtype == np.complex128 and got.shape == (n,)
        worst["p_f"] = max(worst.get("p_f", 0), rel(got, G["dac_" + name]))
    r = lut_ref("lds")
    table = r["tables"]["full"][0]
    got = dpc.apply_lut(r["tx"], table, r["I"], r["Q"], gain=0.5)
    worst["apply"] = rel_rms(got, pr.apply_lut(r["tx"], table, r["I"], r["Q"], 0.5))
    assert got.shape == r["tx"].shape and got.dtype == np.complex128
    assert np.array_equal(dpc.clipper(np.array([2 - 3j, 0.5 + 0.25j]), 1.0), np.array([1 - 1j, 0.5 + 0.25j]))
    print("mirrored API: %s" % ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= BAR_GOLDEN
