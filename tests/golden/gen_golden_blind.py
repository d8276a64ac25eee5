#!/usr/bin/env python3
"""
Generate tests/golden/blind.npz - the reference's blind signal-quality estimates - by IMPORTING THE REFERENCE (where its source tree is at hand only).

Run from the repo root like gen_golden_metrics.py, with the reference's source tree on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python3 -O tests/golden/gen_golden_blind.py

Only data is written.  Per case c = (M, snr dB) of ``cases``: ``c<c>_idx`` (uint16), the labels of 2**14 random symbols of the reference's unit-power
alphabet ``alphabet_<M>``, and ``c<c>_rx`` (int16 (N, 2)), the symbols scaled by 1.7 plus white noise, re and im times ``rx_scale`` = 2048 rounded:
the received row is ``rx / 2048`` and the known row ``round(2048 alphabet[idx]) / 2048``, the same values in complex64 and complex128.  Per case
and dtype d in (c64, c128): ``c<c>_<d>_mom`` = (mean |E|^2, mean |E|^4) as numpy forms them in that type, ``_S`` = (S1, S2) by the reference's
expressions, ``_snr`` = cal_snr_qam, ``_s0`` = cal_s0, ``_evm`` = cal_evm blind, ``_evmk`` = cal_evm against the known row and, for M = 4, ``_qpsk`` =
cal_snr_blind_qpsk.  ``c<c>_<d>_bsnr`` / ``_bs0`` (16,): the same two per block of 1024 samples for the cases of ``block_cases``.  ``gamma_M`` /
``gamma``: _cal_gamma for M = 4 .. 1024.

Tolerances, measured here against the reference alone; every block of a block case counts like a case of its own:
- ``tol_c128``: 10 x the largest relative deviation, over the cases and quantities compared, between the reference's complex128 value and the
  restatement tests/blind_ref.py with every mean an exactly rounded math.fsum - the spread two summation orders give;
- ``tol_c64_<q>``, q in (snr, s0, evm, evmk, qpsk): 2 x the largest |ref(complex64) - ref(the complex64 samples as complex128)| relative: what the
  reference's own float32 arithmetic contributes, which a device that sums in double does not follow.

Two conditions of the inputs are required (a case takes the first seed 1000 + c + 100 j that meets them): every case whose SNR is compared has a
condition number |gamma k / (gamma k - 1)| <= 200 and every block a finite positive SNR; no 4-QAM sample lies within 5e-4 rad of an axis, the
branch cut of the fourth root.
"""
import os
import sys
import time

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import theory as ref_theory                                         # noqa: E402
from qampy.core import signal_quality as ref_sq                                # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import blind_ref                                                               # noqa: E402

N, SCALE, GAIN, BLOCK = 2 ** 14, 2048., 1.7, 1024
CASES = [(4, 8.), (4, 15.), (4, 25.), (16, 12.), (16, 20.), (64, 18.), (256, 32.), (32, 20.)]
BLOCK_CASES = [1, 3]
NO_SNR = (256,)                     # ill-conditioned by nature: moments, S1, S2 and the blind EVM only
DTYPES = (("c64", np.complex64), ("c128", np.complex128))


def quantised(x):
    q = np.rint(np.stack([x.real, x.imag], axis=-1) * SCALE)
    require(np.abs(q).max() < 2 ** 15, "a sample leaves the int16 grid")
    return q.astype(np.int16)


def require(cond, what):
    """(an assert statement is compiled away under -O)"""
    if not cond:
        raise SystemExit("gen_golden_blind: %s" % (what,))


def draw(c, M, db, al, gamma):
    """Labels, received grid values and the condition number of case c: the first seed 1000 + c + 100 j whose row meets the two conditions."""
    for j in range(20):
        rng = np.random.default_rng(1000 + c + 100 * j)
        idx = rng.integers(0, M, N)
        noise = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5 * 10 ** (-db / 10))
        q = quantised(GAIN * (al[idx] + noise))
        rx = (q[:, 0] + 1j * q[:, 1]) / SCALE
        k = blind_ref.moments(rx)
        cond = abs(gamma * k[0] ** 2 / k[1] / (gamma * k[0] ** 2 / k[1] - 1))
        ang = np.angle(rx)
        near = np.min(abs(ang[:, None] - np.array([-np.pi, -np.pi / 2, 0, np.pi / 2, np.pi])), axis=1).min()
        if (M in NO_SNR or cond <= 200) and (M != 4 or near > 5e-4):
            return idx, q, rx, cond, near
    raise SystemExit("gen_golden_blind: no seed meets the conditions of case %d" % c)


def rel(a, b):
    return abs(a - b) / abs(b)


def main():
    t0 = time.time()
    arr = {"cases": np.array(CASES), "block_cases": np.array(BLOCK_CASES), "block": np.int64(BLOCK), "rx_scale": np.float64(SCALE),
           "no_snr_M": np.array(NO_SNR), "gamma_M": 2 ** np.arange(2, 11)}
    arr["gamma"] = np.array([ref_sq._cal_gamma(int(M)) for M in arr["gamma_M"]])
    dev128, dev64 = 0., {q: 0. for q in ("snr", "s0", "evm", "evmk", "qpsk")}
    table, closest = [], np.inf
    for c, (M, db) in enumerate(CASES):
        al = ref_theory.cal_symbols_qam(M) / np.sqrt(ref_theory.cal_scaling_factor_qam(M))
        arr["alphabet_%d" % M] = np.asarray(al, dtype=np.complex128)
        gamma = ref_sq._cal_gamma(M)
        ideal = ref_theory.cal_symbols_qam(M).flatten()
        idx, q, rx, cond, near = draw(c, M, db, al, gamma)
        arr["c%d_idx" % c], arr["c%d_rx" % c] = idx.astype(np.uint16), q
        kq = quantised(al[idx])
        known = (kq[:, 0] + 1j * kq[:, 1]) / SCALE
        closest = min(closest, near) if M == 4 else closest
        vals = {}
        for name, ct in DTYPES:
            E, K = rx.astype(ct), known.astype(ct)
            require(np.all(E.astype(np.complex128) == rx) and np.all(K.astype(np.complex128) == known), "the grid values are not exact in %s" % name)
            r2, r4 = np.mean(abs(E) ** 2), np.mean(abs(E) ** 4)
            S1 = 1 - 2 * r2 ** 2 / r4 - np.sqrt((2 - gamma) * (2 * r2 ** 4 / r4 ** 2 - r2 ** 2 / r4))
            S2 = gamma * r2 ** 2 / r4 - 1
            v = dict(mom=np.array([r2, r4], dtype=np.float64), S=np.array([S1, S2], dtype=np.float64), snr=ref_sq.cal_snr_qam(E, M), s0=ref_sq.cal_s0(E, M),
                     evm=ref_sq.cal_evm(E, M), evmk=ref_sq.cal_evm(E, M, known=K))
            if M == 4:
                v["qpsk"] = ref_sq.cal_snr_blind_qpsk(E)
            if c in BLOCK_CASES:
                blocks = E[:N // BLOCK * BLOCK].reshape(-1, BLOCK)
                v["bsnr"] = np.array([ref_sq.cal_snr_qam(b, M) for b in blocks], dtype=np.float64)
                v["bs0"] = np.array([ref_sq.cal_s0(b, M) for b in blocks], dtype=np.float64)
                require(np.all(np.isfinite(v["bsnr"]) & (v["bsnr"] > 0)), "a block of case %d has no finite positive SNR" % c)
            for key, x in v.items():
                arr["c%d_%s_%s" % (c, name, key)] = np.asarray(x, dtype=np.float64)
            vals[name] = v
        # complex128: the reference against the restatement under another summation order
        st = blind_ref.row_stats(rx, gamma, fsum=True)
        other = dict(snr=st[4], s0=st[5], evm=blind_ref.evm(rx, ideal, gamma, fsum=True), evmk=blind_ref.evm(rx, ideal, gamma, known=known, fsum=True))
        if M == 4:
            other["qpsk"] = blind_ref.qpsk_snr(rx, fsum=True)[2]
        row = [M, db, cond]
        for key in ("snr", "s0", "evm", "evmk", "qpsk"):
            if key not in other or (M in NO_SNR and key != "evm"):
                row += [np.nan, np.nan]
                continue
            d128 = rel(other[key], vals["c128"][key])
            up = {"snr": ref_sq.cal_snr_qam, "s0": ref_sq.cal_s0}.get(key)
            E64 = rx.astype(np.complex64).astype(np.complex128)
            K64 = known.astype(np.complex64).astype(np.complex128)
            if key in ("snr", "s0"):
                wide = up(E64, M)
            elif key == "evm":
                wide = ref_sq.cal_evm(E64, M)
            elif key == "evmk":
                wide = ref_sq.cal_evm(E64, M, known=K64)
            else:
                wide = ref_sq.cal_snr_blind_qpsk(E64)
            d64 = rel(vals["c64"][key], wide)
            if c in BLOCK_CASES and key in ("snr", "s0"):         # the blocks of the two block cases count like cases of their own
                for b in range(N // BLOCK):
                    sl = slice(b * BLOCK, (b + 1) * BLOCK)
                    d128 = max(d128, rel(blind_ref.row_stats(rx[sl], gamma, fsum=True)[4 if key == "snr" else 5], vals["c128"]["b" + key][b]))
                    d64 = max(d64, rel(vals["c64"]["b" + key][b], up(E64[sl], M)))
            dev128, dev64[key] = max(dev128, d128), max(dev64[key], d64)
            row += [d128, d64]
        table.append(row)
    arr["tol_c128"] = np.float64(10 * dev128)
    for key, d in dev64.items():
        arr["tol_c64_%s" % key] = np.float64(2 * d)
    arr["tol_table"] = np.array(table, dtype=np.float64)
    path = os.path.join(OUT, "blind.npz")
    np.savez_compressed(path, **arr)
    print("cases: M, snr dB, condition, then per quantity (snr, s0, evm, evmk, qpsk) the complex128 and complex64 deviations")
    for row in table:
        print("  %4d %5.1f %7.1f  " % tuple(row[:3]) + " ".join("%8.1e" % x for x in row[3:]))
    print("closest 4-QAM sample to an axis: %.1e rad" % closest)
    print("tol_c128 = %.2e; " % arr["tol_c128"] + ", ".join("tol_c64_%s = %.2e" % (k, arr["tol_c64_%s" % k]) for k in dev64))
    print("wrote %s (%.0f kB) in %.1f s" % (path, os.path.getsize(path) / 1e3, time.time() - t0))


if __name__ == "__main__":
    main()
