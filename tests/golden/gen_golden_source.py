#!/usr/bin/env python3
"""
Generate tests/golden/source.npz - the reference's bit sources and Gray mapper - by IMPORTING THE REFERENCE (this container only).

Run from the repo root like gen_golden_sync.py, with the reference's source tree on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python3 -O tests/golden/gen_golden_source.py

Only data is written: seeds, offsets and the reference's outputs.  Bit rows are stored with ``np.packbits`` (numpy's default bit order).

``orders``, ``nshort``; per order ``seeds_<o>`` (5 values, -1 standing for None: all ones; 1; 2^(o-1); an arbitrary one; 0) and per kind
(``ext``: ``make_prbs_extXOR``; ``int``: ``pythran_dsp.prbs_int(seed, mask, o, N)`` with ``make_prbs_intXOR``'s masks - that function itself
raises TypeError in the reference) and seed number ``i`` the first ``nshort`` = 2^16 + 77 bits, ``short_<kind>_<o>_<i>``.

``long_n`` = 2^22; per order 23 and 31 (external form): ``long_seed_<o>``, ``long_offsets_<o>``, ``long_windows_<o>`` (one packed 256-bit
window per offset) and ``long_sha256_<o>`` (the digest of the packed 2^22 bits, as bytes).

``sig_M``, ``sig_seed``, ``sig_order``, ``sig_n``: per M ``SignalQAMGrayCoded(M, 4096, nmodes=2, bitclass=PRBSBits, seed=..., order=[15, 23])``:
``sig_<M>_bits`` (packed rows), ``sig_<M>_labels`` (uint16) and per dtype ``sig_<M>_<c64|c128>_coded``; the signal itself is
``coded[labels]`` (asserted here).

``fba_*``: ``from_bit_array`` of ``RandomBits(1003, nmodes=2, seed=3)`` at M = 16, complex64 (1003 is no multiple of 4): the bits, the
labels of the result and the alphabet.  ``fsa_*``: ``from_symbol_array`` of 2 x 256 noisy 64-QAM symbols (``fsa_in``), M = 64: the alphabet,
the labels of the result and the reference's ``bits`` (it keeps those of the LAST mode only, one row).  ``rb_*``: ``RandomBits(257, 2, 12345)``.
"""
import hashlib
import os

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import signals as ref_signals                                    # noqa: E402
from qampy.core import prbs as ref_prbs                                     # noqa: E402
from qampy.core.pythran_dsp import prbs_int as ref_prbs_int                 # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ORDERS = (7, 15, 23, 31)
TAPS = {7: 6, 15: 14, 23: 18, 31: 28}
NSHORT = 2 ** 16 + 77
NLONG = 2 ** 22
ARBITRARY = {7: 0x55, 15: 0x2A5F, 23: 0x5A3C19, 31: 0x4D2F0B71}
SIG_M = (4, 8, 16, 32, 64, 128, 256)
SIG_SEED, SIG_ORDER, SIG_N = [0x1234, 0x4D2F0B], [15, 23], 4096


def labels_of(sig, coded):
    idx = np.argmin(np.abs(np.asarray(sig)[..., None] - coded), axis=-1)
    assert np.array_equal(coded[idx], np.asarray(sig))
    return idx.astype(np.uint16)


def main():
    arr = {"orders": np.array(ORDERS), "nshort": np.int64(NSHORT), "long_n": np.int64(NLONG)}
    for o in ORDERS:
        seeds = [None, 1, 2 ** (o - 1), ARBITRARY[o], 0]
        arr["seeds_%d" % o] = np.array([-1 if s is None else s for s in seeds], dtype=np.int64)
        for i, s in enumerate(seeds):
            arr["short_ext_%d_%d" % (o, i)] = np.packbits(ref_prbs.make_prbs_extXOR(o, NSHORT, s))
            si = 2 ** o - 1 if s is None else s
            arr["short_int_%d_%d" % (o, i)] = np.packbits(ref_prbs_int(si, 2 ** o + 2 ** TAPS[o] + 1, o, NSHORT).astype(bool))
    for o in (23, 31):
        seed = ARBITRARY[o] ^ 0x1F
        bits = ref_prbs.make_prbs_extXOR(o, NLONG, seed)
        offsets = np.array([0, o - 1, o, o + 1, 2 ** 16 - 3, 2 ** 16, 2 ** 16 + 1, 1000003, 2 ** 21 - 128, 2 ** 21 + 1, 3 * 2 ** 20 + 77, NLONG - 256],
                           dtype=np.int64)
        arr["long_seed_%d" % o], arr["long_offsets_%d" % o] = np.int64(seed), offsets
        arr["long_windows_%d" % o] = np.array([np.packbits(bits[a:a + 256]) for a in offsets])
        arr["long_sha256_%d" % o] = np.frombuffer(hashlib.sha256(np.packbits(bits).tobytes()).digest(), dtype=np.uint8)

    arr["sig_M"], arr["sig_seed"], arr["sig_order"], arr["sig_n"] = np.array(SIG_M), np.array(SIG_SEED), np.array(SIG_ORDER), np.int64(SIG_N)
    for M in SIG_M:
        for dn, ct in (("c64", np.complex64), ("c128", np.complex128)):
            sig = ref_signals.SignalQAMGrayCoded(M, SIG_N, nmodes=2, bitclass=ref_signals.PRBSBits, dtype=ct, seed=list(SIG_SEED), order=list(SIG_ORDER))
            coded = np.asarray(sig.coded_symbols)
            assert sig.dtype == ct and coded.dtype == ct
            labels, bits = labels_of(sig, coded), np.packbits(np.asarray(sig.bits), axis=-1)
            for key, val in (("sig_%d_labels" % M, labels), ("sig_%d_bits" % M, bits)):
                assert key not in arr or np.array_equal(arr[key], val)
                arr[key] = val
            arr["sig_%d_%s_coded" % (M, dn)] = coded

    rb = ref_signals.RandomBits(1003, nmodes=2, seed=3)
    sig = ref_signals.SignalQAMGrayCoded.from_bit_array(rb, 16, dtype=np.complex64)
    arr["fba_bits"], arr["fba_nbits"], arr["fba_coded"] = np.packbits(np.asarray(rb), axis=-1), np.int64(1003), np.asarray(sig.coded_symbols)
    arr["fba_labels"] = labels_of(sig, np.asarray(sig.coded_symbols))
    assert sig.shape == (2, 250)

    rng = np.random.default_rng(17)
    clean = ref_signals.SignalQAMGrayCoded(64, 256, nmodes=2, seed=5)
    noisy = np.asarray(clean) + 0.05 * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape))
    sig = ref_signals.SignalQAMGrayCoded.from_symbol_array(noisy, M=64)
    arr["fsa_in"], arr["fsa_coded"] = noisy, np.asarray(sig.coded_symbols)
    arr["fsa_labels"] = labels_of(sig, np.asarray(sig.coded_symbols))
    arr["fsa_bits_last_mode"] = np.packbits(np.asarray(sig.bits))
    assert np.asarray(sig.bits).shape == (256 * 6,)

    arr["rb_bits"], arr["rb_args"] = np.packbits(np.asarray(ref_signals.RandomBits(257, nmodes=2, seed=12345)), axis=-1), np.array([257, 2, 12345])
    path = os.path.join(OUT, "source.npz")
    np.savez_compressed(path, **arr)
    print("wrote source.npz (%d arrays, %.1f KiB)" % (len(arr), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
