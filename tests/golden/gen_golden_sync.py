#!/usr/bin/env python3
"""
Generate tests/golden/sync.npz - the reference's sequence synchronisation - by IMPORTING THE REFERENCE (this container only).

Run from the repo root like gen_golden.py, with the reference's source tree and this repository on PYTHONPATH (reference first):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_sync.py

Inputs come from tests/sync_ref.py (``case``: a 16-QAM pattern made periodic, started ``shift`` samples in, turned and with a little
noise), rounded to multiples of 1 / scale (2^-10) so that complex64 and complex128 hold the same values, and stored as int16
(re, im) * scale, as gen_golden_metrics.py stores its rows.  Only data is written: these inputs and the reference's outputs.

Per case ``c<k>`` (``cases``: ntx, nrx, shift, turns): ``_txq`` / ``_rxq``; per ``adjust`` in tx / rx the reference's
``find_sequence_offset_complex`` of the pair as ``sync_and_adjust`` calls it (``_<adjust>_offset``, ``_turns``, ``_peak``, and
``_runner_up``: the largest |cc| outside the peak's index relative to the peak's) and ``sync_and_adjust``'s aligned rows
(``_<adjust>_txq`` / ``_<adjust>_rxq``: rotated copies of the inputs, so int16 holds them exactly).

``qam_*``: two modes of 4096 16-QAM symbols (``qam_tx_label``, uint8 into ``qam_coded``), received with noise (``qam_rxq``), the
transmitted pattern rolled by 3000 symbols, turned a quarter turn and its modes swapped (``qam_pattern_label``); the reference's
``SignalQAM._sync_and_adjust`` (aligned pattern as labels), ``cal_ser`` and ``cal_ber`` with ``synced=False``.
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import signals as ref_signals                                    # noqa: E402
from qampy.core import ber_functions as ref_ber                             # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import sync_ref                                                             # noqa: E402

SCALE = 1024
CASES = [(100, 100, 75, 1), (100, 100, 0, 0), (257, 100, 37, 3), (100, 257, 99, 2), (100, 300, 1, 1), (1000, 3500, 750, 2), (3500, 1000, 2625, 3),
         (128, 129, 96, 0)]


def rounded(v):
    return np.round(v * SCALE) / SCALE


def quantised(v):
    """int16 (..., 2) holding re, im * SCALE exactly."""
    q = np.stack([v.real, v.imag], axis=-1) * SCALE
    assert np.all(np.abs(q) < 2 ** 15) and np.array_equal(q, np.round(q))
    return q.astype(np.int16)


def runner_up(cc):
    a = np.abs(cc)
    k = int(np.argmax(a))
    return float(np.delete(a, k).max() / a[k])


def main():
    arr = {"scale": np.float64(SCALE), "cases": np.array(CASES, dtype=np.int64)}
    for k, (ntx, nrx, shift, turns) in enumerate(CASES):
        tx, rx = (rounded(v) for v in sync_ref.case(ntx, nrx, shift, turns))
        pre = "c%d_" % k
        arr[pre + "txq"], arr[pre + "rxq"] = quantised(tx), quantised(rx)
        for adjust in ("tx", "rx"):
            x, y = (rx, tx) if adjust == "tx" else (tx, rx)
            offset, _, nturns, peak = ref_ber.find_sequence_offset_complex(x, y)
            _, cc = ref_ber.find_sequence_offset(x, y, show_cc=True)
            (atx, arx), peak2 = ref_ber.sync_and_adjust(tx, rx, adjust=adjust)
            assert peak2 == peak
            p = pre + adjust + "_"
            arr[p + "offset"], arr[p + "turns"], arr[p + "peak"] = np.int64(offset), np.int64(nturns), np.float64(peak)
            arr[p + "runner_up"] = np.float64(runner_up(cc))
            arr[p + "txq"], arr[p + "rxq"] = quantised(atx), quantised(arx)

    # 16-QAM, two modes of 4096 symbols: the pattern handed to the metrics is rolled by 3000, turned a quarter turn, its modes swapped
    n = 4096
    sym = [sync_ref.qam16(n, 11 + m) for m in range(2)]
    coded = sym[0][1]
    tx = np.array([s[0] for s in sym])
    rng = np.random.default_rng(5)
    rx = rounded(tx + 0.07 * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape)))
    pattern = np.roll(tx[::-1] * 1j, 3000, axis=-1)
    label = lambda v: np.argmin(np.abs(np.asarray(v)[..., None] - coded), axis=-1).astype(np.uint8)      # noqa: E731
    assert np.allclose(coded[label(pattern)], pattern, atol=1e-12)
    pattern = coded[label(pattern)]
    arr["qam_coded"], arr["qam_tx_label"], arr["qam_pattern_label"], arr["qam_rxq"] = coded, label(tx), label(pattern), quantised(rx)
    for dn, ct in (("c64", np.complex64), ("c128", np.complex128)):
        sig = ref_signals.SignalQAMGrayCoded.from_symbol_array(pattern.astype(ct), M=16, dtype=ct)
        assert np.allclose(np.sort_complex(np.asarray(sig.coded_symbols)), np.sort_complex(coded.astype(ct)))
        arr["qam_%s_coded" % dn] = np.asarray(sig.coded_symbols)
        arr["qam_%s_pattern_label" % dn] = np.argmin(np.abs(pattern[..., None] - np.asarray(sig.coded_symbols)), axis=-1).astype(np.uint8)
        rsig = sig.recreate_from_np_array(rx.astype(ct))
        t_al, r_al = sig._sync_and_adjust(sig.symbols, np.asarray(rsig))
        arr["qam_%s_aligned_label" % dn] = np.argmin(np.abs(np.asarray(t_al)[..., None] - np.asarray(sig.coded_symbols)), axis=-1).astype(np.uint8)
        assert np.array_equal(np.asarray(r_al), rx.astype(ct))
        arr["qam_%s_ser" % dn], arr["qam_%s_ber" % dn] = rsig.cal_ser(), rsig.cal_ber()
    path = os.path.join(OUT, "sync.npz")
    np.savez_compressed(path, **arr)
    print("wrote sync.npz (%d arrays, %.1f KiB)" % (len(arr), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
