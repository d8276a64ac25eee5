#!/usr/bin/env python3
"""
Generate tests/golden/pilotframe.npz - the reference's pilot frames and pilot-aided estimates - by IMPORTING THE REFERENCE.

Run from the repo root with the reference's source tree on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python3 -O tests/golden/gen_golden_pilotframe.py

Only data is written.

Frames: ``SignalWithPilots(M, F, S, R, nframes, nmodes=2, Mpilots=4, dtype=..., bitclass=PRBSBits, seed=SEED, order=ORDER)`` for the rows of
``geoms`` (M, F, S, R, nframes), both dtypes.  Per geometry ``k`` and dtype ``dt`` (c64, c128), prefix ``f<k>_<dt>_``:
    pil_coded, pay_coded   the alphabets of ``sig.pilots`` (scaled) and ``sig.symbols``
    pilots, payload        ``sig.pilots`` (nmodes, nframes NP) and ``sig.symbols`` (nmodes, nframes ND) as uint16 labels into them
    frame                  the signal as uint16 labels into ``concatenate([pil_coded, pay_coded])``
(every label array is asserted to give back the reference's values bit for bit).  ``f0nr_<dt>_``: geometry 0 with ``repeat_data=False``;
``f0s_c64_``: geometry 0, complex64, ``pilot_scale=1.5`` (a Python float: numpy keeps complex64).

Estimates, complex128, on geometry 0's frame under a carrier offset of ``est_fo`` = 1e-3 cycles/symbol, a random-walk phase of ``est_sigma`` rad
per symbol and AWGN at 25 dB, from the seed ``est_seed`` - the first seed from 0 on for which no unwrap decision of cpe1, cpe2, the offset
estimate and the constant phase below is closer than 0.25 rad to a flip (measured with tests/pilot_ref.py on the pilots each call uses,
checked here; ``est_margin`` is the smallest) and none of cpe3 closer than 0.05 rad (``est_margin_cpe3``).  cpe3 cannot keep 0.25: in its second
frame the reference pairs the received pilots with ``np.tile(...)[:, :n]`` of the references, which are not the pilots that were sent there, so
the raw phase steps between neighbours are multiples of pi / 2 plus the 0.2 rad that the carrier offset adds over 32 symbols, and a dozen of
them are +-pi + 0.2 rad with 0.08 rad of noise on top.  0.05 rad is still 10^13 roundings of a double-precision angle.
    est_x                               the impaired signal (2, 3072)
    cpe1_E, cpe1_ph                     phaserec.pilot_cpe(sig, N=5, use_seq=True): field (2, 1024) complex128, trace (its real part) float64
    cpe2_E, cpe2_ph                     pilot_cpe(sig, N=3, use_seq=False)
    cpe3_E, cpe3_ph                     pilot_cpe(sig, N=4, pilot_rat=2, max_blocks=40, nframes=2)   ((2, 2048); N becomes 5)
    foe_mean, foe_modes, foe_icpt       pilot_based_foe(x[:, :S], sig.pilot_seq)
    const_rec, const_ref, const_ph      find_pilot_const_phase(extract_pilots() of cpe1's field - one frame -, that frame's sig.pilots)
    get_data, extract_pilots            sig.get_data() and sig.extract_pilots() of the impaired signal
"""
import os
import sys
import warnings

import numpy as np

assert not __debug__, "run with python3 -O (see gen_golden.py)"

from qampy import phaserec as ref_phaserec                                   # noqa: E402
from qampy import signals as ref_signals                                     # noqa: E402
from qampy.core import pilotbased_receiver as ref_pr                         # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pilot_ref                                                             # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED, ORDER = [0x1234, 0x4D2F0B], [15, 23]
GEOMS = ((64, 1024, 128, 16, 3), (16, 1000, 40, 2, 2), (256, 515, 3, 0, 2), (4, 96, 0, 32, 1))
DT = {"c64": np.complex64, "c128": np.complex128}
EST_FO, EST_SIGMA, EST_SNR = 1e-3, 4e-3, 25.
MARGIN_CPE3 = 0.05                       # rad: see the module docstring


def labels_of(x, coded):
    x = np.asarray(x)
    idx = np.argmin(np.abs(x[..., None] - coded), axis=-1)
    assert np.array_equal(coded[idx], x)
    return idx.astype(np.uint16)


def frame_keys(arr, prefix, sig):
    pil_coded = np.unique(np.asarray(sig.pilots))
    pay_coded = np.asarray(sig.symbols.coded_symbols)
    arr[prefix + "pil_coded"], arr[prefix + "pay_coded"] = pil_coded, pay_coded
    arr[prefix + "pilots"] = labels_of(sig.pilots, pil_coded)
    arr[prefix + "payload"] = labels_of(sig.symbols, pay_coded)
    arr[prefix + "frame"] = labels_of(sig, np.concatenate([pil_coded, pay_coded]))


def make(geom, dtype, **kw):
    M, F, S, R, nframes = geom
    return ref_signals.SignalWithPilots(M, F, S, R, nframes, nmodes=2, Mpilots=4, dtype=dtype, bitclass=ref_signals.PRBSBits, seed=SEED, order=ORDER, **kw)


def impair(sig, seed):
    rng = np.random.default_rng(seed)
    nm, L = sig.shape
    ph = 2 * np.pi * EST_FO * np.arange(L) + np.cumsum(EST_SIGMA * rng.standard_normal((nm, L)), axis=1)
    sd = 10 ** (-EST_SNR / 20) / np.sqrt(2)
    return np.asarray(sig) * np.exp(1j * ph) + sd * (rng.standard_normal((nm, L)) + 1j * rng.standard_normal((nm, L)))


def margins(sig, x):
    """The unwrap margin of every estimate below, on the pilots it uses (the selection of pilot_based_cpe_new, restated)."""
    F, S = sig.frame_len, sig._pilot_seq_len
    pos = np.flatnonzero(sig._idx_pil)
    pil, ph = np.asarray(sig.pilots), np.asarray(sig.ph_pilots)
    m = [pilot_ref.phase(x, pos, F, 1, pil)[1],
         pilot_ref.phase(x, pos[S:], F, 1, ph)[1],
         pilot_ref.phase(x, pos[S:][:40:2], F, 2, ph[:, ::2])[1],
         pilot_ref.pair_phase(x[:, :S], pil[:, :S])[1]]
    return m


def main():
    warnings.simplefilter("ignore")
    arr = {"geoms": np.array(GEOMS, dtype=np.int64), "seed": np.array(SEED, dtype=np.int64), "order": np.array(ORDER, dtype=np.int64)}
    for k, geom in enumerate(GEOMS):
        for dt, dtype in DT.items():
            frame_keys(arr, "f%d_%s_" % (k, dt), make(geom, dtype))
    for dt, dtype in DT.items():
        frame_keys(arr, "f0nr_%s_" % dt, make(GEOMS[0], dtype, repeat_data=False))
    frame_keys(arr, "f0s_c64_", make(GEOMS[0], np.complex64, pilot_scale=1.5))

    sig = make(GEOMS[0], np.complex128)
    S = sig._pilot_seq_len
    for seed in range(1000):
        x = impair(sig, seed)
        m = margins(sig, x)
        if min(m[0], m[1], m[3]) >= pilot_ref.MARGIN and m[2] >= MARGIN_CPE3:
            break
    if not (min(m[0], m[1], m[3]) >= pilot_ref.MARGIN and m[2] >= MARGIN_CPE3):          # (no assert: this script runs under -O)
        raise RuntimeError("no seed keeps the unwrap decisions away from a flip: %s" % (m,))
    rx = sig.recreate_from_np_array(x)
    arr.update(est_seed=np.int64(seed), est_fo=np.float64(EST_FO), est_sigma=np.float64(EST_SIGMA), est_snr=np.float64(EST_SNR),
               est_margin=np.float64(min(m[0], m[1], m[3])), est_margin_cpe3=np.float64(m[2]), est_x=x)
    for name, kw in (("cpe1", dict(N=5, use_seq=True)), ("cpe2", dict(N=3, use_seq=False)), ("cpe3", dict(N=4, pilot_rat=2, max_blocks=40, nframes=2))):
        out, ph = ref_phaserec.pilot_cpe(rx, **kw)
        assert np.all(np.asarray(ph).imag == 0)
        arr[name + "_E"], arr[name + "_ph"] = np.asarray(out), np.asarray(ph).real.copy()
        if name == "cpe1":
            out1 = out
    foe, foe_modes, icpt = ref_pr.pilot_based_foe(np.asarray(rx)[:, :S], np.asarray(sig.pilot_seq))
    arr.update(foe_mean=np.float64(foe), foe_modes=np.asarray(foe_modes), foe_icpt=np.asarray(icpt))
    rec = np.asarray(out1.extract_pilots())                                  # (nframes=1: cpe1's field is one frame long)
    ref = np.asarray(sig.pilots)[:, :rec.shape[1]]
    if not pilot_ref.pair_phase(rec, ref)[1] >= pilot_ref.MARGIN:
        raise RuntimeError("the constant-phase input has an unwrap decision close to a flip")
    arr.update(const_rec=rec, const_ref=ref, const_ph=np.asarray(ref_phaserec.find_pilot_const_phase(rec, ref)))
    arr.update(get_data=np.asarray(rx.get_data()), extract_pilots=np.asarray(rx.extract_pilots()))
    path = os.path.join(OUT, "pilotframe.npz")
    np.savez_compressed(path, **arr)
    print("wrote %s (%d bytes), seed %d, margins %s" % (path, os.path.getsize(path), seed, m))


if __name__ == "__main__":
    main()
