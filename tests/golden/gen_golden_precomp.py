#!/usr/bin/env python3
"""
Generate tests/golden/precomp.npz - the reference's digital pre-compensation (qampy/core/digital_pre_compensation.py) - by IMPORTING THE
REFERENCE.

Run from the repo root with the reference's source tree and this repository on PYTHONPATH (reference first), and WITH ``-O``:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree>:. python3 -O tests/golden/gen_golden_precomp.py

``-O`` is not optional here.  The reference's table average, ``pythran_dsp.cal_lut_avg``, asserts ``idx_I.shape[0] > L`` while ``cal_lut`` hands
it index arrays of exactly length ``L``: uncompiled and under plain ``python`` every ``cal_lut`` call raises AssertionError.  Compiled, the
assert is gone; ``-O`` removes it from the pure-Python module in the same way.

Inputs are those of tests/precomp_ref.py ``cases()`` (multiples of 2^-10, |tx - rx| <= 1, at most 4099 samples per row), made anew from
their seeds and stored here as well, as integers (value * 1024).  Outputs are the reference's results on the complex128 inputs.  This script
asserts that the reference gives the same table for the complex64 copy of every input (always complex128: it divides by an integer array),
and that the restatement agrees with the reference on every case before anything is written.

Keys:
    idx_{i}_x, idx_{i}_I, idx_{i}_Q      index case i of precomp_ref.INDEX_CASES with L >= mem_len (the reference's rolling window cannot wrap
                                         twice): input (L, 2) int32, and find_sym_patterns as cal_lut centres it, int32
    tie_x, tie_I, tie_Q, nan_x, nan_I, nan_Q
                                         the tie row and the NaN row (r4, mem_len 3); nan_x is float64 (L, 2), not scaled
    lut_{name}_tx, lut_{name}_rx         table case of precomp_ref.LUT_CASES: inputs (L, 2) int32
    lut_{name}_I, lut_{name}_Q           cal_lut's index arrays under the full mask, int32
    lut_{name}_{mask}_at, lut_{name}_{mask}_ea
                                         positions (int64) and values (complex128) of the entries of ea that are not 0, per mask of LUT_MASKS
    sin_x, sin_real, sin_cplx            comp_mod_sin(mod_sin_input(), 1.14) and (..., 1.2 + 0.9j)
    dac_{name}                           comp_dac_resp of precomp_ref.DAC_CASES, complex128; the roll-off goes in as np.float64 - with the Python
                                         float 0.0 the reference's raised cosine raises ZeroDivisionError before it finds the roll-off band empty
"""
import os
import sys

import numpy as np

assert not __debug__, "run with python3 -O: cal_lut_avg's assert fails on what cal_lut hands it"

from qampy.core import digital_pre_compensation as ref                         # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import precomp_ref as pr                                                      # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def check(ok, what):
    """(an assert would be compiled out under -O)"""
    if not ok:
        raise RuntimeError("the restatement and the reference disagree: %s" % (what,))


def scaled(x):
    v = np.stack([x.real, x.imag], axis=-1) * pr.Q
    check(np.array_equal(v, np.rint(v)), "input not on the grid")
    return v.astype(np.int32)


def ref_index(x, kind, mem_len):
    """find_sym_patterns per rail (or on the complex alphabet) as cal_lut calls and centres it"""
    lev_I, lev_Q, alphabet = pr.levels_of(kind)
    at = np.arange(x.size) - mem_len // 2
    if alphabet is None:
        return ref.find_sym_patterns(x.real, lev_I, mem_len)[at], ref.find_sym_patterns(x.imag, lev_Q, mem_len)[at]
    p = ref.find_sym_patterns(x, alphabet, mem_len)[at]
    return p, p


def main():
    cs = pr.cases()
    out = {}
    for i, c in enumerate(cs["index"]):
        if c["L"] < c["mem_len"]:
            continue
        a, b = ref_index(c["x"], c["kind"], c["mem_len"])
        ra, rb = pr.pattern_index(c["x"], *pr.levels_of(c["kind"]), c["mem_len"])
        check(np.array_equal(a, ra) and np.array_equal(b, rb), i)
        out["idx_%d_x" % i], out["idx_%d_I" % i], out["idx_%d_Q" % i] = scaled(c["x"]), a.astype(np.int32), b.astype(np.int32)
    for name in ("tie", "nan"):
        x = cs[name]
        a, b = ref_index(x, "r4", 3)
        ra, rb = pr.pattern_index(x, *pr.levels_of("r4"), 3)
        check(np.array_equal(a, ra) and np.array_equal(b, rb), name)
        out[name + "_x"] = scaled(x) if name == "tie" else np.stack([x.real, x.imag], axis=-1)
        out[name + "_I"], out[name + "_Q"] = a.astype(np.int32), b.astype(np.int32)
    for c in cs["lut"]:
        name, tx, rx = c["name"], c["tx"], c["rx"]
        ref_sym, real_ptrns = pr.ref_sym_of(c["kind"])
        out["lut_%s_tx" % name], out["lut_%s_rx" % name] = scaled(tx), scaled(rx)
        for which in pr.LUT_MASKS:
            mask = pr.mask_of(which, c["L"])
            ea, iI, iQ = ref.cal_lut(tx, rx, ref_sym, mem_len=c["mem_len"], idx_data=mask, real_ptrns=real_ptrns)
            ea32, _, _ = ref.cal_lut(tx.astype(np.complex64), rx.astype(np.complex64), ref_sym, mem_len=c["mem_len"], idx_data=mask, real_ptrns=real_ptrns)
            check(ea.dtype == ea32.dtype == np.complex128 and np.array_equal(ea, ea32), (name, which, "complex64"))
            rI, rQ = pr.pattern_index(tx, *pr.levels_of(c["kind"]), c["mem_len"])
            rea, _, _ = pr.lut(tx, rx, rI, rQ, ea.size, mask)
            sel = slice(None) if mask is None else np.flatnonzero(mask)
            check(np.array_equal(rea, ea) and np.array_equal(rI[sel], iI) and np.array_equal(rQ[sel], iQ), (name, which))
            if which == "full":
                out["lut_%s_I" % name], out["lut_%s_Q" % name] = iI.astype(np.int32), iQ.astype(np.int32)
            out["lut_%s_%s_at" % (name, which)], out["lut_%s_%s_ea" % (name, which)] = pr.nonzero_table(ea)
    x = pr.mod_sin_input()
    out["sin_x"] = x
    with np.errstate(invalid="ignore"):
        out["sin_real"], out["sin_cplx"] = ref.comp_mod_sin(x, 1.14), ref.comp_mod_sin(x, 1.2 + 0.9j)
    for name, fb, n, beta, papr, prms, os_ in pr.DAC_CASES:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["dac_" + name] = ref.comp_dac_resp(fb, n, np.float64(beta), PAPR=papr, prms_dac=prms, os=os_)
        mine = pr.comp_dac_resp(fb, n, beta, PAPR=papr, prms_dac=prms, os=os_)
        check(np.abs(mine - out["dac_" + name]).max() <= 1e-11 * np.abs(out["dac_" + name]).max(), name)
    np.savez_compressed(os.path.join(OUT, "precomp.npz"), **out)
    print("wrote precomp.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(OUT, "precomp.npz"))))


if __name__ == "__main__":
    main()
