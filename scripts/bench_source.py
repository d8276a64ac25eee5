#!/usr/bin/env python3
"""Time the bit source and the Gray mapper (csrc/source.hip) at a C3-size payload - 2 modes x 2^22 64-QAM symbols, complex64, PRBS-15 / 23 -
each figure the median of warm runs between HIP events, two launches (one per mode) where a stage works row by row:

    prbs_bits        prbs_bits_dev of both rows (2 x 25 M bits, one byte each)
    three_step       prbs_bits_dev -> bits_to_labels_dev -> labels_to_symbols_dev
    fused_symbols    prbs_symbols_dev, symbols only
    fused_all        prbs_symbols_dev with labels and bits

against two floors taken in the same run: a device fill (qh_memset) of as many bytes as the stage writes - the traffic floor - and the
reference's make_prbs_extXOR + SignalQAMGrayCoded._modulate on the CPU for 2^18 bits, scaled linearly to the payload (the reference is
pure Python where its pythran module is not compiled, and it is not installed beside this package: its figure is taken by a run of this
script with --reference-tree on a machine that has it, kept in a JSON file and merged with --reference-json).

    python3 scripts/bench_source.py [--reps 20] [--log2-nsym 22] [--out-dir profiles] [--reference-json FILE]
    python3 scripts/bench_source.py --reference-tree DIR --reference-only --out-dir DIR2        (CPU only: writes source_reference_cpu.json)

Writes <out-dir>/source_bench.json and <out-dir>/source_timings.md and prints the JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def reference_cpu(tree, nbits=2 ** 18, M=64):
    """Seconds of the reference's bit generation and mapping for ``nbits`` bits on this CPU (best of 3)."""
    sys.path.insert(0, tree)
    from qampy.core import prbs as rp
    from qampy import signals as rs, theory as rt
    coded = rs.SignalQAMGrayCoded._generate_mapping(M, np.sqrt(rt.cal_scaling_factor_qam(M)), dtype=np.complex64)[0]
    t_bits, t_mod = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        bits = rp.make_prbs_extXOR(23, nbits)
        t1 = time.perf_counter()
        rs.SignalQAMGrayCoded._modulate(bits[:nbits // 6 * 6], None, coded, dtype=np.complex64)
        t2 = time.perf_counter()
        t_bits.append(t1 - t0), t_mod.append(t2 - t1)
    import qampy.core.pythran_dsp as pd
    return dict(nbits=nbits, prbs_s=min(t_bits), modulate_s=min(t_mod), pythran_compiled=not pd.__file__.endswith(".py"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2-nsym", type=int, default=22)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reference-tree")
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--reference-json")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    cpu = reference_cpu(a.reference_tree) if a.reference_tree else None
    if a.reference_only:
        with open(os.path.join(a.out_dir, "source_reference_cpu.json"), "w") as f:
            json.dump(cpu, f)
        print(json.dumps(cpu))
        return
    if cpu is None and a.reference_json:
        with open(a.reference_json) as f:
            cpu = json.load(f)

    from qampy_amd import _lib, theory
    from qampy_amd._lib import DeviceArray
    from qampy_amd.core import hip_dsp

    def median_ms(fn):
        fn()
        _lib.sync()
        ts = []
        for _ in range(a.reps):
            s, e = _lib.Event(), _lib.Event()
            s.record()
            fn()
            e.record()
            _lib.sync()
            ts.append(e.elapsed_ms(s))
        return float(np.median(ts))

    _lib.init(0)
    M, nb, nm, nsym = 64, 6, 2, 2 ** a.log2_nsym
    orders = (15, 23)
    al = DeviceArray.from_host(np.ascontiguousarray(theory.coded_symbols_qam(M, dtype=np.complex64)))
    bits, lab, sym = DeviceArray((nm, nsym * nb), np.uint8), DeviceArray((nm, nsym), np.int32), DeviceArray((nm, nsym), np.complex64)
    b_bits, b_lab, b_sym = bits.nbytes, lab.nbytes, sym.nbytes

    def prbs_bits():
        for m in range(nm):
            hip_dsp.prbs_bits_dev(bits.row(m), orders[m])

    def three_step():
        prbs_bits()
        hip_dsp.bits_to_labels_dev(bits, nb, lab)
        hip_dsp.labels_to_symbols_dev(lab, al, sym)

    def fused(all_outputs):
        for m in range(nm):
            hip_dsp.prbs_symbols_dev(sym.row(m), al, orders[m], labels=lab.row(m) if all_outputs else None, bits=bits.row(m) if all_outputs else None)

    fill = DeviceArray((b_bits + b_lab + b_sym,), np.uint8)

    def fill_ms(nbytes):
        return median_ms(lambda: _lib.call("qh_memset", fill.ptr, 1, nbytes))

    stages = [("prbs_bits", prbs_bits, b_bits), ("three_step", three_step, b_bits + b_lab + b_sym),
              ("fused_symbols", lambda: fused(False), b_sym), ("fused_all", lambda: fused(True), b_bits + b_lab + b_sym)]
    res = {"device": _lib.device_name(), "reps": a.reps, "dtype": "complex64", "M": M, "nmodes": nm, "nsym": nsym, "orders": list(orders),
           "bits_per_workgroup": hip_dsp.PRBS_W, "symbols_per_workgroup": hip_dsp.SOURCE_SYMS}
    for name, fn, written in stages:
        ms, floor = median_ms(fn), fill_ms(written)
        res[name] = {"ms": ms, "bytes_written": written, "fill_ms": floor, "over_fill": ms / floor, "written_GBps": written / ms / 1e6}
    if cpu:
        scale = nm * nsym * nb / cpu["nbits"]
        res["reference_cpu"] = dict(cpu, scaled_to_bits=nm * nsym * nb, scaled_prbs_s=cpu["prbs_s"] * scale, scaled_modulate_s=cpu["modulate_s"] * scale)
    with open(os.path.join(a.out_dir, "source_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Bit source and Gray mapper: timings", "",
             "%s, %d x 2^%d %d-QAM symbols (PRBS-%d / PRBS-%d), complex64, median of %d warm runs between HIP events (scripts/bench_source.py)." % (
                 res["device"], nm, a.log2_nsym, M, orders[0], orders[1], a.reps),
             "The fill is `qh_memset` of as many bytes as the stage writes, timed in the same run: the traffic floor.", "",
             "| stage | ms | bytes written | fill ms | multiple of the fill | GB/s written |", "|---|---|---|---|---|---|"]
    for name, _, _ in stages:
        r = res[name]
        lines.append("| %s | %.4f | %d | %.4f | %.2f | %.0f |" % (name, r["ms"], r["bytes_written"], r["fill_ms"], r["over_fill"], r["written_GBps"]))
    lines.append("")
    if cpu:
        rc = res["reference_cpu"]
        lines.append("Reference on the CPU (%s): make_prbs_extXOR %.3f s and _modulate %.4f s for 2^%d bits; SCALED linearly to the %d bits of this payload: "
                     "%.1f s and %.2f s." % ("pythran module compiled" if rc["pythran_compiled"] else "its pythran module runs uncompiled, as plain Python",
                                             rc["prbs_s"], rc["modulate_s"], int(np.log2(rc["nbits"])), rc["scaled_to_bits"], rc["scaled_prbs_s"],
                                             rc["scaled_modulate_s"]))
    else:
        lines.append("Reference on the CPU: not measured in this run.")
    with open(os.path.join(a.out_dir, "source_timings.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
