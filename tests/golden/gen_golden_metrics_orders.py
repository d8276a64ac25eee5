#!/usr/bin/env python3
"""
Generate tests/golden/metrics_orders.npz - the reference's signal-quality metrics for the orders metrics.npz lacks (8-, 512- and
1024-QAM) - by IMPORTING THE REFERENCE (this container only).  Run from the repo root like gen_golden_metrics.py:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_metrics_orders.py

Same recipe and storage as gen_golden_metrics.py (its helpers are reused), except that rows are 2^14 symbols long - at 2^12 a
1024-QAM class can be empty and the reference's own SNR estimate is NaN - and labels are stored as uint16.  Only data is written.
"""
import os
import sys
import time

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_metrics as g                                              # noqa: E402

from qampy.core import pythran_dsp as ref_dsp                               # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NSYM = 2 ** 14
SNRS = {8: (11., 17.), 512: (28., 34.), 1024: (31., 37.)}


def main():
    g.NSYM = NSYM                                                           # received() draws rows of g.NSYM symbols
    t0 = time.time()
    arr = {"Ms": np.array(sorted(SNRS)), "nsym": np.int64(NSYM), "nllr": np.int64(g.NLLR), "rx_scale": np.float64(g.SCALE)}
    for M, snrs in sorted(SNRS.items()):
        nb = int(np.log2(M))
        slow_n = max(8, 2 ** 16 // (M * M))
        arr["M%d_snr_db" % M] = np.array(snrs)
        arr["M%d_mi_slow_n" % M] = np.int64(slow_n)
        for j, snr_db in enumerate(snrs):
            tx, rx = g.received(M, snr_db, seed=100 * M + j)
            for dn, ct in g.CT.items():
                sig, rsig = g.ref_signal(tx, rx, M, ct)
                if j == 0:
                    arr["M%d_%s_coded" % (M, dn)] = sig.coded_symbols
                    arr["M%d_%s_bitmap_sig" % (M, dn)] = sig._bitmap_mtx
                lab = _labels16(sig, sig.symbols)
                if dn == "c64":
                    arr["M%d_s%d_tx_label" % (M, j)] = lab
                assert np.array_equal(arr["M%d_s%d_tx_label" % (M, j)], lab)
                pre = "M%d_s%d_%s_" % (M, j, dn)
                if dn == "c128":
                    base = np.round(np.asarray(sig.coded_symbols)[lab] * g.SCALE)
                    arr["M%d_s%d_rxd" % (M, j)] = (g.quantised(rx) - np.stack([base.real, base.imag], axis=-1)).astype(np.int16)
                snr = g.metrics(arr, pre, sig, rsig, M, slow_n if j == 0 else 0)
                r0 = np.ascontiguousarray(np.asarray(rsig)[0, :g.NLLR])
                ft = np.float32 if dn == "c64" else np.float64
                arr[pre + "llr"] = ref_dsp.soft_l_value_demapper(r0, nb, snr[0], sig._bitmap_mtx).astype(ft)
                arr[pre + "llr_minmax"] = ref_dsp.soft_l_value_demapper_minmax(r0, nb, snr[0], sig._bitmap_mtx).astype(ft)
                print("M=%d s%d %s done (%.1f s)" % (M, j, dn, time.time() - t0), flush=True)
    path = os.path.join(OUT, "metrics_orders.npz")
    np.savez_compressed(path, **arr)
    print("wrote metrics_orders.npz (%d arrays, %.1f KiB) in %.1f s" % (len(arr), os.path.getsize(path) / 1024, time.time() - t0))


def _labels16(sig, symbols):
    """gen_golden_metrics.labels as uint16 (labels up to 1023), row by row."""
    coded = np.asarray(sig.coded_symbols)
    symbols = np.asarray(symbols)
    lab = np.stack([np.argmax(row[:, None] == coded, axis=-1) for row in symbols])
    assert np.array_equal(coded[lab], symbols)
    return lab.astype(np.uint16)


if __name__ == "__main__":
    main()
