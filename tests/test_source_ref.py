"""tests/source_ref.py (the numpy restatement of the bit source and the Gray mapper) against the reference's outputs stored in
tests/golden/source.npz (tests/golden/gen_golden_source.py).  Every comparison is exact.  No GPU, no reference."""
import hashlib
import os

import numpy as np
import pytest

import source_ref as ref

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "source.npz"))
NSHORT, NLONG = int(GOLD["nshort"]), int(GOLD["long_n"])


def gold_seed(order, i):
    s = int(GOLD["seeds_%d" % order][i])
    return None if s < 0 else s


@pytest.mark.parametrize("kind", ["ext", "int"])
@pytest.mark.parametrize("order", [7, 15, 23, 31])
def test_short_sequences(kind, order):
    for i in range(5):
        want = np.unpackbits(GOLD["short_%s_%d_%d" % (kind, order, i)])[:NSHORT]
        got = ref.prbs(kind, order, NSHORT, gold_seed(order, i))
        assert np.array_equal(got, want), (kind, order, i)
        assert np.array_equal(ref.prbs(kind, order, 300, gold_seed(order, i), start=1234), want[1234:1534])
    assert not np.unpackbits(GOLD["short_%s_%d_4" % (kind, order)]).any()                     # seed 0: all zeros


def test_the_galois_form_is_the_register_for_its_first_bits_and_the_recurrence_after():
    for order in (7, 15, 23, 31):
        for i in range(4):
            want = np.unpackbits(GOLD["short_int_%d_%d" % (order, i)])[:2000]
            assert np.array_equal(ref.galois_steps(order, 2000, gold_seed(order, i)), want)


def test_a_bool_seed_is_read_with_element_zero_as_bit_zero():
    assert ref.seed_int(7, [1, 0, 0, 0, 0, 0, 0]) == 1 and ref.seed_int(7, np.array([0, 0, 0, 0, 0, 0, 1], bool)) == 64
    assert ref.seed_int(15) == 2 ** 15 - 1 and ref.seed_int(23, 5) == 5


@pytest.mark.parametrize("order", [23, 31])
def test_long_sequences(order):
    bits = ref.prbs_ext(order, NLONG, int(GOLD["long_seed_%d" % order]))
    for off, win in zip(GOLD["long_offsets_%d" % order], GOLD["long_windows_%d" % order]):
        assert np.array_equal(bits[off:off + 256], np.unpackbits(win)), off
    assert hashlib.sha256(np.packbits(bits).tobytes()).digest() == GOLD["long_sha256_%d" % order].tobytes()


def test_period_of_order_15():
    bits = ref.prbs_ext(15, 3 * (2 ** 15 - 1), 0x2A5F)
    assert np.array_equal(bits[:2 ** 15 - 1], bits[2 ** 15 - 1:2 * (2 ** 15 - 1)])


@pytest.mark.parametrize("M", [4, 8, 16, 32, 64, 128, 256])
def test_signal_bits_and_labels(M):
    nb, n = int(np.log2(M)), int(GOLD["sig_n"])
    bits = np.unpackbits(GOLD["sig_%d_bits" % M], axis=-1)[:, :n * nb]
    for m in range(2):
        assert np.array_equal(bits[m], ref.prbs_ext(int(GOLD["sig_order"][m]), n * nb, int(GOLD["sig_seed"][m])))
    assert np.array_equal(ref.bits_to_labels(bits, nb), GOLD["sig_%d_labels" % M])
    assert np.array_equal(ref.labels_to_bits(GOLD["sig_%d_labels" % M], nb), bits)


def test_from_bit_array_and_from_symbol_array_cases():
    bits = np.unpackbits(GOLD["fba_bits"], axis=-1)[:, :int(GOLD["fba_nbits"])]
    assert np.array_equal(ref.bits_to_labels(bits[:, :1000], 4), GOLD["fba_labels"])
    assert np.array_equal(ref.labels_to_bits(GOLD["fsa_labels"], 6)[-1], np.unpackbits(GOLD["fsa_bits_last_mode"])[:256 * 6])
    near = np.argmin(np.abs(GOLD["fsa_in"][..., None] - GOLD["fsa_coded"]), axis=-1)
    assert np.array_equal(near, GOLD["fsa_labels"])
