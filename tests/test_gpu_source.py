"""The bit source and the Gray mapper on the MI355X (csrc/source.hip) against the reference's recorded outputs (tests/golden/source.npz) and
the numpy restatement (tests/source_ref.py).  Everything here is integer work or a table look-up: every comparison is exact."""
import functools
import hashlib
import warnings

import numpy as np
import pytest

import source_ref as ref
from qampy_amd import _lib, signals, synth
from qampy_amd.core import ber_functions, hip_dsp, prbs

pytestmark = pytest.mark.gpu

CT = {"c64": np.complex64, "c128": np.complex128}
ORDERS = (7, 15, 23, 31)
W = hip_dsp.PRBS_W                      # bits per workgroup of prbs_bits_dev
SYMS = hip_dsp.SOURCE_SYMS              # symbols per workgroup of the fused source
GUARD = 0xA5


@pytest.fixture(scope="module")
def fx(golden):
    return golden["source"]


def _dev(a):
    return _lib.DeviceArray.from_host(np.ascontiguousarray(a))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gen(order, n, seed=None, kind="ext", start=0, invert=False, lead=0):
    """``prbs_bits_dev`` into the middle of a guarded buffer, ``lead`` bytes past a 256-byte boundary: the bytes around it must stay."""
    total = _lib.DeviceArray((lead + n + 48,), np.uint8)
    total.set(np.full(lead + n + 48, GUARD, np.uint8))
    view = object.__new__(_lib.DeviceArray)                     # non-owning, as DeviceArray.row makes them
    view.shape, view.dtype, view.nbytes, view.ptr, view._own = (n,), np.dtype(np.uint8), n, total.ptr + lead, False
    hip_dsp.prbs_bits_dev(view, order, seed, kind=kind, start=start, invert=invert)
    got = total.to_host()
    assert np.all(got[:lead] == GUARD) and np.all(got[lead + n:] == GUARD), "wrote outside its row"
    return got[lead:lead + n]


@functools.lru_cache(maxsize=None)
def want(kind, order, seed=None, n=4 * W + 200):
    r = ref.prbs(kind, order, n, seed)
    r.setflags(write=False)
    return r


def gold_seed(fx, order, i):
    s = int(fx["seeds_%d" % order][i])
    return None if s < 0 else s


# ------------------------------------------------------------------------------------------------ bits against the fixture
@pytest.mark.parametrize("kind", ["ext", "int"])
@pytest.mark.parametrize("order", ORDERS)
def test_short_rows_are_the_references(fx, kind, order):
    n = int(fx["nshort"])
    for i in range(5):
        expect = np.unpackbits(fx["short_%s_%d_%d" % (kind, order, i)])[:n]
        assert np.array_equal(gen(order, n, gold_seed(fx, order, i), kind), expect), (kind, order, i)
    make = prbs.make_prbs_extXOR if kind == "ext" else prbs.make_prbs_intXOR
    host = make(order, 1000, gold_seed(fx, order, 3))
    assert host.dtype == bool and np.array_equal(host, np.unpackbits(fx["short_%s_%d_3" % (kind, order)])[:1000].astype(bool))
    bools = np.array([(gold_seed(fx, order, 3) >> p) & 1 for p in range(order)], bool)
    assert np.array_equal(make(order, 1000, bools), host)                        # a bool seed: element 0 is bit 0


@pytest.mark.parametrize("order", [23, 31])
def test_long_rows_windows_by_jump_ahead_and_the_whole_by_its_digest(fx, order):
    seed, n = int(fx["long_seed_%d" % order]), int(fx["long_n"])
    for off, win in zip(fx["long_offsets_%d" % order], fx["long_windows_%d" % order]):
        assert np.array_equal(gen(order, 256, seed, start=int(off), lead=int(off) % 16), np.unpackbits(win)), off
    whole = _lib.DeviceArray((n,), np.uint8)
    hip_dsp.prbs_bits_dev(whole, order, seed)
    assert hashlib.sha256(np.packbits(whole.to_host()).tobytes()).digest() == fx["long_sha256_%d" % order].tobytes()


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("order", ORDERS)
def test_lengths_and_starts_around_a_workgroup(order):
    full = want("ext", order)
    for n in (1, 2, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5):
        for start in (0, 1, order - 1, order, order + 1, W - 1, W + 1):
            assert np.array_equal(gen(order, n, start=start, lead=(start + n) % 16), full[start:start + n]), (n, start)
    galois = want("int", order)
    for n, start in ((1, 0), (65, order - 1), (W + 1, order), (3 * W + 5, W - 1)):
        assert np.array_equal(gen(order, n, kind="int", start=start, lead=3), galois[start:start + n]), (n, start)


@pytest.mark.parametrize("order", [7, 15, 23])
def test_a_row_that_crosses_the_period(order):
    period = 2 ** order - 1
    for kind in ("ext", "int"):
        full = ref.prbs(kind, order, period + 200, 0x35)
        assert np.array_equal(full[:200], full[period:period + 200])
        assert np.array_equal(gen(order, 300, 0x35, kind, start=period - 100), full[period - 100:period + 200])


@pytest.mark.parametrize("order", ORDERS)
def test_whole_periods_ahead_change_nothing(order):
    """start = s + m (2^o - 1), m up to 2^30 (order 31: past 2^61): reference-free, exact by periodicity."""
    period, s = 2 ** order - 1, 2 * W + 17
    for kind in ("ext", "int"):
        base = gen(order, 400, 0x4B, kind, start=s)
        assert np.array_equal(base, want(kind, order, 0x4B)[s:s + 400])
        for m in (1, 2 ** 10 + 1, 2 ** 30):
            assert s + m * period <= hip_dsp.PRBS_START_MAX
            assert np.array_equal(gen(order, 400, 0x4B, kind, start=s + m * period), base), (kind, m)


@pytest.mark.parametrize("order", ORDERS)
def test_split_invert_zero_seed_and_repeat(order):
    n, cut = 2 * W + 77, W + 4099
    one = gen(order, n, 0x11)
    assert np.array_equal(np.concatenate([gen(order, cut, 0x11), gen(order, n - cut, 0x11, start=cut, lead=cut % 16)]), one)
    assert np.array_equal(gen(order, n, 0x11, invert=True), 1 - one)
    assert _same(gen(order, n, 0x11), one)
    for kind in ("ext", "int"):
        assert not gen(order, n, 0, kind).any()
        assert gen(order, n, 0, kind, invert=True).all()
    assert set(np.unique(one)) == {0, 1}


# ------------------------------------------------------------------------------------------------ mapping
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", [4, 8, 16, 32, 64, 128, 256])
def test_mapping_against_the_fixture(fx, M, dn):
    nb, n = int(np.log2(M)), int(fx["sig_n"])
    bits = np.unpackbits(fx["sig_%d_bits" % M], axis=-1)[:, :n * nb]
    labels, coded = fx["sig_%d_labels" % M].astype(np.int32), fx["sig_%d_%s_coded" % (M, dn)]
    d_bits, d_al = _dev(bits), _dev(coded)
    d_lab, d_sym = _lib.DeviceArray((2, n), np.int32), _lib.DeviceArray((2, n), CT[dn])
    assert np.array_equal(hip_dsp.bits_to_labels_dev(d_bits, nb, d_lab).to_host(), labels)
    d_lab2 = _lib.DeviceArray((2, n), np.int32)
    assert _same(hip_dsp.modulate_bits_dev(d_bits, d_al, d_sym, d_lab2).to_host(), coded[labels])
    assert np.array_equal(d_lab2.to_host(), labels)
    assert _same(hip_dsp.modulate_bits_dev(_dev(bits.astype(bool)), d_al, _lib.DeviceArray((2, n), CT[dn])).to_host(), coded[labels])
    back = _lib.DeviceArray((2, n * nb), np.uint8)
    assert np.array_equal(hip_dsp.labels_to_bits_dev(d_lab, nb, back).to_host(), bits)
    dem, dem_lab = _lib.DeviceArray((2, n * nb), np.uint8), _lib.DeviceArray((2, n), np.int32)
    assert np.array_equal(hip_dsp.demodulate_dev(d_sym, d_al, dem, dem_lab).to_host(), bits)            # demodulate(modulate(bits)) = bits
    assert np.array_equal(dem_lab.to_host(), labels)
    assert np.array_equal(hip_dsp.demodulate_dev(d_sym.row(1), d_al, _lib.DeviceArray((n * nb,), np.uint8)).to_host(), bits[1])


def _straddle(nb):
    return W // nb + 1                  # for odd nb bit W lies inside a symbol


@pytest.mark.parametrize("nb", range(2, 11))
def test_fused_source_equals_the_three_steps(nb):
    """nsym: 1, 7, 4096, one past the fused form's workgroup, three of its workgroups and a bit, and a row whose bits straddle W."""
    rng = np.random.default_rng(nb)
    M = 2 ** nb
    for dn, order, kind in (("c64", 23, "ext"), ("c128", 15, "int")):
        alphabet = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(CT[dn])
        d_al = _dev(alphabet)
        for nsym in (1, 7, 4096, SYMS - 1, SYMS + 1, 3 * SYMS + 5, _straddle(nb)):
            start = 3 * nb + 1
            bits3 = _lib.DeviceArray((nsym * nb,), np.uint8)
            lab3, sym3 = _lib.DeviceArray((nsym,), np.int32), _lib.DeviceArray((nsym,), CT[dn])
            hip_dsp.prbs_bits_dev(bits3, order, 0x51, kind=kind, start=start)
            hip_dsp.bits_to_labels_dev(bits3, nb, lab3)
            hip_dsp.labels_to_symbols_dev(lab3, d_al, sym3)
            b3, l3, s3 = bits3.to_host(), lab3.to_host(), sym3.to_host()
            assert np.array_equal(b3, ref.prbs(kind, order, nsym * nb, 0x51, start)), (dn, nsym)
            assert np.array_equal(l3, ref.bits_to_labels(b3, nb)) and _same(s3, alphabet[l3]), (dn, nsym)
            sym, lab, bits = _lib.DeviceArray((nsym,), CT[dn]), _lib.DeviceArray((nsym,), np.int32), _lib.DeviceArray((nsym * nb,), np.uint8)
            hip_dsp.prbs_symbols_dev(sym, d_al, order, 0x51, kind=kind, start=start, labels=lab, bits=bits)
            assert _same(sym.to_host(), s3) and np.array_equal(lab.to_host(), l3) and np.array_equal(bits.to_host(), b3), (dn, nsym)
            alone = _lib.DeviceArray((nsym,), CT[dn])
            assert _same(hip_dsp.prbs_symbols_dev(alone, d_al, order, 0x51, kind=kind, start=start).to_host(), s3), (dn, nsym)
            lab_only = _lib.DeviceArray((nsym,), np.int32)
            hip_dsp.prbs_symbols_dev(alone, d_al, order, 0x51, kind=kind, start=start, labels=lab_only)
            assert np.array_equal(lab_only.to_host(), l3), (dn, nsym)


def test_fused_source_into_rows_of_a_stack_keeps_to_its_row():
    """Rows of odd length: the second row starts off the 16-byte grid; neighbours of every output stay untouched."""
    nsym, nb, M = SYMS + 3, 3, 8
    alphabet = np.arange(1, M + 1).astype(np.complex64) * (1 + 2j)
    sym, lab, bits = _lib.DeviceArray((3, nsym), np.complex64), _lib.DeviceArray((3, nsym), np.int32), _lib.DeviceArray((3, nsym * nb), np.uint8)
    sym.set(np.full((3, nsym), -7, np.complex64)), lab.set(np.full((3, nsym), -7, np.int32)), bits.set(np.full((3, nsym * nb), GUARD, np.uint8))
    hip_dsp.prbs_symbols_dev(sym.row(1), _dev(alphabet), 15, 9, labels=lab.row(1), bits=bits.row(1))
    b, l, s = bits.to_host(), lab.to_host(), sym.to_host()
    assert np.all(b[[0, 2]] == GUARD) and np.all(l[[0, 2]] == -7) and np.all(s[[0, 2]] == -7)
    assert np.array_equal(b[1], ref.prbs_ext(15, nsym * nb, 9)) and np.array_equal(l[1], ref.bits_to_labels(b[1], nb)) and _same(s[1], alphabet[l[1]])


def test_a_label_outside_the_alphabet_gives_zero():
    bits = ref.prbs_ext(15, 4 * 1000)
    labels = ref.bits_to_labels(bits, 4)
    assert labels.max() >= 12
    alphabet = (np.arange(12) + 1).astype(np.complex128) * (1 - 1j)
    out, lab = _lib.DeviceArray((1000,), np.complex128), _lib.DeviceArray((1000,), np.int32)
    got = hip_dsp.modulate_bits_dev(_dev(bits), _dev(alphabet), out, lab, nb=4).to_host()
    assert np.array_equal(lab.to_host(), labels)
    assert _same(got, np.where(labels < 12, alphabet[np.minimum(labels, 11)], 0))


# ------------------------------------------------------------------------------------------------ objects
@pytest.mark.parametrize("dn", CT)
@pytest.mark.parametrize("M", [4, 8, 16, 32, 64, 128, 256])
def test_gray_coded_signal_from_prbs_is_the_references(fx, M, dn):
    nb, n = int(np.log2(M)), int(fx["sig_n"])
    sig = signals.SignalQAMGrayCoded(M, n, nmodes=2, bitclass=signals.PRBSBits, dtype=CT[dn], seed=[int(s) for s in fx["sig_seed"]],
                                     order=[int(o) for o in fx["sig_order"]])
    coded, labels = fx["sig_%d_%s_coded" % (M, dn)], fx["sig_%d_labels" % M]
    assert isinstance(sig, signals.SignalQAMGrayCoded) and isinstance(sig.bits, signals.PRBSBits) and sig.bits.dtype == bool
    assert _same(np.asarray(sig.coded_symbols), coded) and _same(np.asarray(sig), coded[labels]) and _same(sig.symbols, coded[labels])
    assert np.array_equal(np.asarray(sig.bits), np.unpackbits(fx["sig_%d_bits" % M], axis=-1)[:, :n * nb].astype(bool))
    assert (sig.M, sig.fb, sig.fs, sig.os, sig.Nbits) == (M, 1, 1, 1, nb)
    assert _same(sig.modulate(sig.bits), coded[labels]) and np.array_equal(sig.demodulate(np.asarray(sig)), np.asarray(sig.bits))
    assert np.array_equal(sig[:, 5:50].bits, sig.bits) and sig.recreate_from_np_array(np.asarray(sig) * 2).bits is sig.bits


def test_from_bit_array_truncates_and_warns(fx):
    n = int(fx["fba_nbits"])
    bits = np.unpackbits(fx["fba_bits"], axis=-1)[:, :n].astype(bool)
    with pytest.warns(UserWarning, match="not divisible by log2"):
        sig = signals.SignalQAMGrayCoded.from_bit_array(bits, 16, dtype=np.complex64)
    assert sig.shape == (2, n // 4) and _same(np.asarray(sig), fx["fba_coded"][fx["fba_labels"]]) and _same(np.asarray(sig.coded_symbols), fx["fba_coded"])
    assert np.array_equal(sig.bits, bits[:, :n // 4 * 4])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        whole = signals.SignalQAMGrayCoded.from_bit_array(bits[0, :1000], 16, dtype=np.complex64)
    assert _same(np.asarray(whole), np.asarray(sig)[:1])


def test_from_symbol_array_is_the_references(fx):
    with pytest.warns(UserWarning, match="not normalized"):
        sig = signals.SignalQAMGrayCoded.from_symbol_array(fx["fsa_in"], M=64)
    assert sig.dtype == np.complex128 and _same(np.asarray(sig.coded_symbols), fx["fsa_coded"])
    assert _same(np.asarray(sig), fx["fsa_coded"][fx["fsa_labels"]])
    assert np.array_equal(sig.bits[-1], np.unpackbits(fx["fsa_bits_last_mode"])[:256 * 6].astype(bool))      # the reference keeps the last mode's
    assert np.array_equal(sig.bits, ref.labels_to_bits(fx["fsa_labels"], 6).astype(bool))


# ------------------------------------------------------------------------------------------------ resident loop
def test_make_symbols_dev_feeds_the_metrics():
    n = 2 ** 14
    cap = synth.make_symbols_dev(16, n, keep_bits=True)
    sig = signals.SignalQAMGrayCoded(16, n, nmodes=2, bitclass=signals.PRBSBits, dtype=np.complex64)
    assert set(cap) == {"symbols", "idx_tx", "alphabet", "alphabet_host", "M", "bits"} and cap["M"] == 16
    assert np.array_equal(cap["idx_tx"].to_host(), ref.bits_to_labels(np.asarray(sig.bits), 4))
    assert _same(cap["symbols"].to_host(), np.asarray(sig)) and np.array_equal(cap["bits"].to_host().view(bool), np.asarray(sig.bits))
    assert _same(cap["alphabet_host"], np.asarray(sig.coded_symbols)) and "bits" not in synth.make_symbols_dev(16, 64)
    for res in ber_functions.cal_metrics_dev(cap["symbols"], cap["idx_tx"], cap["alphabet"], snr_db=20):
        assert (res["errors"], res["bit_errors"], res["compared"]) == (0, 0, n)
