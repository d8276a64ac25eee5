#!/usr/bin/env python3
"""
bench.py - equalised MSym/s of the adaptive-equaliser + carrier-recovery hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3|ns|c2|c1|c5] [--tier b|a] [--tol T] [--full] [--no-cpu-baseline] ...

One "step" = one pass of the hot path (dual-mode tap training -> filter application -> blind phase search, unwrap and
de-rotation of every mode) over one synthetic dual-polarisation 2 SPS capture that is already resident in HBM.
With N GPUs every rank processes its own independent channel (seed 1000 + rank, BASELINE.json config 4): weak scaling, no
collective on the data path; the process group (qampy_amd/comm.py: RCCL through ctypes on the library's HIP stream, no PyTorch)
carries only the barriers, the max-over-ranks of the elapsed time, the sum of the symbol-error counters and the count of ranks.
`--gpus N` with N > 1 starts the N ranks itself unless it already runs inside a launcher's environment (RANK / WORLD_SIZE, e.g.
under torch.distributed.run as the driver starts it).  `--split-capture` (N > 1, informational) is the other sharding: ONE capture,
the tier-b segments spread over the ranks with an all-reduce of their end taps per pass ("scaling": "strong").

Trainer tiers.  Tier "a" is the exact sequential recurrence (the reference's order of evaluation).  Tier "b"
solves the SAME recurrence from the SAME start taps in parallel in time (concurrently trained segments + waveform relaxation +
linearised coarse correction) and stops when its device-side estimate of the rms deviation of the equaliser output from the
sequential recurrence is below `tol` (default 1e-3, relative).  The timed pipeline uses tier b, and its number is the headline
`value` only if it certifies itself in this very run: every stage converged by that estimate AND, measured against the exact
path run beside it on the same capture, the recovered output is within tol (relative rms), the taps within 3 tol (relative) and
the symbol errors within +-3 per mode.  Otherwise, or with `--tier a`, the headline is the exact path's.  Both are always in
the line (`tier_a`, `tier_b`, `headline_tier`); with `--full`, `speedup_vs_cpu` is keyed to the tier that produced `value`.

PLAIN AND FULL RUNS.  A plain run does what its headline needs and no more: it sets up, warms up, times the K steps, certifies tier b against
the exact path as above (the certificate decides which tier is the headline), writes `--dump-outputs` if asked and prints the line.  `--full`
adds everything else the benchmark measures or checks: timing runs of their own for the roofline and the one-capture / one-receiver figures,
the other shapes and tolerances listed below, the reference's own benchmark definitions, the CPU baselines and the channel bank.  What the
timed steps compute and how they are timed is the same in both.

OUTPUT.  stdout carries ONE compact JSON line (`headline_line`: a whitelist, <= 6 KB enforced before it is printed) with the contract's keys
(metric, value, unit, n_gpus, steps, warmup, ms_per_step, higher_is_better, scaling, vs_baseline, dtype, data, config), the certificate
(`tier_b.checks`, `tier_b.elementwise_summary`), `ser`, `ms_per_step_per_rank`, `comm_backend`, and with `--full` also `roofline`, `cpu_baseline`,
`tier_b_tight` and `parity_vs_cpu`.  The whole result is written to `--detail-out`; round 5 printed it all as one 30 KB line, which the driver
could not parse.  The certificate at tol = 1e-4 includes the ELEMENT-WISE bar of the exact path (rtol = atol = 1e-4 on every tap and every
equaliser-output sample).

`--dump-outputs DIR` writes what the headline path returned for its last timed step (rank 0: taps, error traces, equaliser output, phase,
recovered output, test-angle indices, step sizes) as DIR/<name>.npy, float32 / float64, at most 64 MB (`dump_files`).  The captures depend on
the arguments only, so two builds run with the same arguments can be compared file by file.

A --full run (N = 1, workload c3) additionally carries
  tier_b_loose  the same solver held to tol = 1e-2 (the SER-equivalent tier), informational
  cert_24dB     the same shape at 24 dB SNR, where both paths make thousands of symbol errors: counts within 3 sigma per mode
  ns, c2        the north star's 10^7-symbol shape and BASELINE configs[1]: tier b + exact path + certificate
  roofline      dominant kernel of the step (largest total kernel time): for the relaxation passes and the phase search the bound is
                VALU issue (achieved / peak in wave instructions per second, instruction count from the PMC profile of the same
                kernel sources when there is one), with the HBM view (algorithmic bytes / 8 TB/s) and the flop view beside it
  cpu_baseline  the oracle's reference-flag OpenMP build ("port" of the pythran loops, exact recurrence) on the GPU host's cores:
                the whole capture with all threads (3 runs) and with one thread, CPU model, H2D / D2H times
  parity_vs_cpu, channel_bank (+ its own CPU leg), stages_ms, ser
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# SURVEY.md §8d / BASELINE.md configs.  Step sizes / linewidth of c3 and ns: MRDE is phase sensitive and false-locks when the
# CMA stage leaves a rotated constellation (its phase diffuses ~ mu^2 * N); mu = (2e-4, 2e-4) with a 100 Hz source
# converges on both modes over 2^22 symbols (verified with the CPU oracle, seeds 1000-1001).  c3 is the 2^22-symbol variant of
# the north-star configuration (64-QAM, 41 taps, CMA -> MRDE, 64-angle BPS) and the largest single-GPU configuration in
# BASELINE.json's `configs`.
WORKLOADS = {
    # configs[0]: the reference's own CPU-runnable plumbing case (Scripts/cma_equaliser.py): a parity-test case, not a bench line
    "c1": dict(M=4, nsym=2 ** 16, nmodes=1, ntaps=11, methods=("cma",), mu=(1e-3,), niter=(1,), adaptive=(False,), A=None, Nbps=0,
               snr_db=14, linewidth=0., label="QPSK 1-pol 2 SPS 2^16 sym, 11-tap CMA (no carrier recovery)"),
    "c2": dict(M=16, nsym=2 ** 20, ntaps=21, methods=("mcma",), mu=(1e-3,), niter=(1,), adaptive=(False,), A=32, Nbps=20,
               snr_db=25, linewidth=50e3, label="16-QAM 2-pol 2 SPS 2^20 sym, 21-tap MCMA + 32-angle BPS"),
    "c3": dict(M=64, nsym=2 ** 22, ntaps=41, methods=("cma", "mrde"), mu=(2e-4, 2e-4), niter=(1, 1), adaptive=(False, False),
               A=64, Nbps=20, snr_db=30, linewidth=100.,
               label="64-QAM 2-pol 2 SPS 2^22 sym, 41-tap dual-mode CMA->MRDE + 64-angle BPS"),
    "ns": dict(M=64, nsym=10 ** 7, ntaps=41, methods=("cma", "mrde"), mu=(2e-4, 2e-4), niter=(1, 1), adaptive=(False, False),
               A=64, Nbps=20, snr_db=30, linewidth=100.,
               label="64-QAM 2-pol 2 SPS 10^7 sym, 41-tap dual-mode CMA->MRDE + 64-angle BPS (north star)"),
}
WORKLOADS["c5"] = dict(M=256, nsym=2 ** 16, ntaps=45, methods=("cma", "sbd_data"), mu=(1e-3, 1e-3), niter=(30, 30), adaptive=(True, True), A=None, Nbps=0,
                       snr_db=35, linewidth=10e3,
                       label="pilot-based 256-QAM 2-pol 2 SPS, 2^16-symbol frames: frame sync + data-aided pilot equaliser + filter + pilot phase recovery")
VALU_PEAK_TFLOPS = 157.3        # fp32 vector (packed FMA), MI355X_MICROARCH.md
VALU_PEAK_GINSTR = 614.4        # wave64 fp32 instructions per second, nominal: 1024 SIMDs x 2.4 GHz / 4 cycles (measured, clock-throttled ceilings: 697 plain v_fma, 537 v_pk_fma - profiles/r02_ubench_issue.txt)
SEG_INSTR_PER_WAVE_STEP = {16: 51, 8: 82}    # train_seg_kernel main loop per wave and step by lanes per chain (ISA count incl. s_nop / s_waitcnt / ds_read at 41 taps x 2 modes, cma, DESIGN.md 3.2.2: 43 VALU + 5 s_nop + 2 ds_read + 0.6 s_waitcnt at 16 lanes since round 5; the counters of profiles/pmc_instr_*.json replace it when they belong to these sources)
HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FUSED_BYTES_PER_SYM = 88   # read E once, write err1, err2, out, ph (complex64, 2 modes, 2 samples/symbol)
SER_TOL_ERRORS = 3         # decisions: tier b's symbol errors per mode within this many of the exact path's (ONE of the checks; see run_pair)


# ------------------------------------------------------------------------------------------------------------ launcher
def self_launch(argv, gpus):
    """`python bench.py --gpus N` outside a launcher's environment: start the N ranks (one per GPU) and relay their exit code
    (qampy_amd.comm.launch: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT, as torch.distributed.run sets them)."""
    from qampy_amd import comm
    return comm.launch(os.path.abspath(__file__), argv, gpus)


# ------------------------------------------------------------------------------------------------------------ workload
def make_input(cfg, nsym, seed, host=False):
    """The capture of this rank: synthesised on the GPU (csrc/synth.hip, ~1 ms) and copied to the host once for the CPU legs;
    --host-synth uses the numpy generator instead (same impairments, frequency-domain filters, ~10 s at 2^22 symbols)."""
    from qampy_amd import synth
    from qampy_amd.signals import SignalQAM
    nm = cfg.get("nmodes", 2)
    if not host:
        d = synth.make_capture_dev(cfg["M"], nsym, nmodes=nm, os=2, snr_db=cfg["snr_db"], theta=np.pi / 5.6 if nm == 2 else None, dgd=30e-12,
                                   linewidth=cfg["linewidth"], fb=20e9, beta=0.1, seed=seed)
        return SignalQAM(d["E"].to_host(), cfg["M"], fb=d["fb"], fs=d["fs"], symbols=d["symbols"].to_host(), coded_symbols=d["alphabet_host"])
    return synth.make_capture(cfg["M"], nsym, nmodes=nm, os=2, snr_db=cfg["snr_db"], theta=np.pi / 5.6 if nm == 2 else None, dgd=30e-12,
                              linewidth=cfg["linewidth"], fb=20e9, beta=0.1, seed=seed, dtype=np.complex64)


def make_receiver(cfg, sig, tier="a", pit=None):
    from qampy_amd.pipeline import ResidentReceiver
    return ResidentReceiver(sig.shape[0], sig.shape[1], 2, cfg["M"], cfg["ntaps"], cfg["mu"], methods=cfg["methods"], Niter=cfg["niter"],
                            adaptive_stepsize=cfg["adaptive"], TrSyms=(None,) * len(cfg["methods"]), Mtestangles=cfg["A"],
                            Nbps=cfg["Nbps"], dtype=np.complex64, alphabet=sig.coded_symbols, tier=tier, pit=pit)


def make_group(n, cfg, sig, pit=None):
    from qampy_amd.pipeline import ReceiverGroup
    return ReceiverGroup(n, sig.shape[0], sig.shape[1], 2, cfg["M"], cfg["ntaps"], cfg["mu"], methods=cfg["methods"], Niter=cfg["niter"],
                         adaptive_stepsize=cfg["adaptive"], TrSyms=(None,) * len(cfg["methods"]), Mtestangles=cfg["A"],
                         Nbps=cfg["Nbps"], dtype=np.complex64, alphabet=sig.coded_symbols, tier="b", pit=pit)


class DryReceiver:
    """--dry-run: stands in for the ResidentReceiver where there is no GPU, so that the launcher, the rank bookkeeping and
    the reductions of the N > 1 path can be exercised on CPU (tests/test_distributed.py).  Kernels are replaced by a sleep."""

    def __init__(self, cfg, nsym, tier):
        self.nstage, self.tier, self.nmodes = len(cfg["methods"]), tier, cfg.get("nmodes", 2)
        self.Mtestangles = cfg["A"]
        self.N = nsym

    def run(self):
        time.sleep(0.002)

    def ser(self, *a, **k):
        return [dict(errors=0, compared=self.N) for _ in range(self.nmodes)]


def stage_list(rx):
    names = ["gram"] + ["train%d:%s" % (s + 1, m) for s, m in enumerate(rx.methods)] + ["apply"] + (["bps_recover"] if rx.Mtestangles else [])
    fns = [rx.build_gram] + [lambda s=s: rx.train(s) for s in range(rx.nstage)] + [rx.apply] + ([rx.recover] if rx.Mtestangles else [])
    return names, fns


def timed_steps(rx, steps, warmup, barrier_sync, overlap=False, pool=None, after=None):
    """W warm-up passes, then exactly K passes bracketed by barrier + device sync; HIP events between the stages.  Returns
    (elapsed s, mean stage ms, per-step pass kernel ms of tier b).  after(rx): called right behind the timed region, while the receiver still
    holds the results of the last timed pass.

    overlap: consecutive passes as ResidentReceiver.run(overlap=True) enqueues them - the phase search of pass k on stream 2 beside the
    training of pass k + 1 (the last one flushed inside the timed region).  The stage times are then event pairs on the stream the stage
    ran on; their sum exceeds the step time by what ran side by side."""
    from qampy_amd import _lib
    names, fns = stage_list(rx)
    pass_ms = [[] for _ in range(rx.nstage)]
    acq_ms = [[] for _ in range(rx.nstage)]
    if overlap:
        order = ["start", "gram"] + ["train%d" % s for s in range(rx.nstage)] + ["apply"]
        fed = [0]

        def feed():
            # consecutive captures that DIFFER: the next member of the resident pool goes into the receiver's second input buffer (a reference, no
            # copy); run() prepares it beside this capture's cold stage and swaps the buffers when it is done with the current one
            if pool:
                fed[0] += 1
                rx.E_next = pool[fed[0] % len(pool)]
                rx._next_loaded = True
        if pool:
            rx.E = pool[0]
            rx.invalidate() if getattr(rx, "_prep", None) is not None else None
        for _ in range(warmup):
            feed()
            rx.run(overlap=True, prefetch=True)
        rx.wait_post()
        evpool = [_lib.Event() for _ in range(steps * (len(order) + 2) + 2)]
        marks = [dict() for _ in range(steps + 1)]

        def marker(k):
            def mark(name):
                e = evpool.pop()
                e.record()
                marks[k][name] = e
                if name.startswith("train"):
                    s = int(name[5:])
                    p, a = rx.pit_timing[s]
                    pass_ms[s].append(list(p))
                    acq_ms[s].append(a)
            return mark
        barrier_sync()
        t0 = time.perf_counter()
        for k in range(steps):
            feed()
            rx.run(overlap=True, mark=marker(k), prefetch=True)      # (prefetch: the next capture's acquisition + eigenbasis beside this capture's cold stage)
        rx.wait_post(marker(steps))
        barrier_sync()
        elapsed = time.perf_counter() - t0
        if after:
            after(rx)
        if pool:
            # back to the pool's first capture (the one the exact path, the CPU legs and the SER harness work on): one untimed pass, so that the results,
            # reports and deviations read after this call belong to it
            rx.E = pool[0]
            rx._next_loaded = False
            rx.invalidate()
            rx.run(overlap=True)
            rx.wait_post()
        stage_ms = [float(np.mean([marks[k][order[j + 1]].elapsed_ms(marks[k][order[j]]) for k in range(steps)])) for j in range(len(order) - 1)]
        if rx.Mtestangles:
            stage_ms.append(float(np.mean([mk["post_end"].elapsed_ms(mk["post_begin"]) for mk in marks if "post_end" in mk])))
        return elapsed, stage_ms, pass_ms, acq_ms
    for _ in range(warmup):
        rx.run()
    ev = [[_lib.Event() for _ in range(len(fns) + 1)] for _ in range(steps)]
    barrier_sync()
    t0 = time.perf_counter()
    for k in range(steps):
        rx.reset()
        ev[k][0].record()
        for j, fn in enumerate(fns):
            fn()
            ev[k][j + 1].record()
            if rx.tier == "b" and 1 <= j <= rx.nstage:
                p, a = rx.pit_timing[j - 1]
                pass_ms[j - 1].append(list(p))
                acq_ms[j - 1].append(a)
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if after:
        after(rx)
    stage_ms = [float(np.mean([ev[k][j + 1].elapsed_ms(ev[k][j]) for k in range(steps)])) for j in range(len(fns))]
    return elapsed, stage_ms, pass_ms, acq_ms


def timed_group(group, steps, warmup, barrier_sync, overlap=True, pool=None, after=None):
    """timed_steps for a pipeline.ReceiverGroup: exactly K passes in total, dealt round robin to the receivers (each on its own host thread and
    library streams), bracketed by barrier + device sync; HIP events on the stream every stage ran on, from all receivers.
    after(rx): as in timed_steps, on the thread of the receiver that ran the last timed pass.
    pool: resident captures rotated through the receivers (pass k of receiver i is capture (i + k n) mod len(pool) of the pool: consecutive passes of
    the job are consecutive, DIFFERENT captures), handed over as references like timed_steps does."""
    from qampy_amd import _lib
    n = len(group.rx)
    rx0 = group.rx[0]
    pass_ms = [[] for _ in range(rx0.nstage)]
    acq_ms = [[] for _ in range(rx0.nstage)]
    order = ["start", "gram"] + ["train%d" % s for s in range(rx0.nstage)] + ["apply"]
    fed = [0] * n
    keep = [r.E for r in group.rx]                 # (the receivers' own input buffers stay alive: a dropped DeviceArray synchronises the device)

    def feed(i, k, rx):
        fed[i] += 1
        rx.E_next = pool[(i + fed[i] * n) % len(pool)]
        rx._next_loaded = True

    def to_first(rx):                              # back to (a receiver's copy of) the pool's first capture: results / reports read afterwards belong to it
        i = group.rx.index(rx)
        rx.E = keep[i]
        rx._next_loaded = False
        rx.invalidate()
        rx.run(overlap=True)
        rx.wait_post()
        _lib.sync()
    feed = feed if pool else None
    if pool:
        group.map(lambda rx: rx.invalidate() if getattr(rx, "_prep", None) is not None else None)
    group.run(warmup * n, overlap=overlap, prefetch=overlap, feed=feed)
    pools = [[_lib.Event() for _ in range((steps // n + 2) * (len(order) + 3) + 4)] for _ in range(n)]
    marks = {}

    def mark(i, k):
        d = marks.setdefault((i, k), {})

        def m(name):
            e = pools[i].pop()
            e.record()
            d[name] = e
            if name.startswith("train"):
                st = int(name[5:])
                p, a = group.rx[i].pit_timing[st]
                pass_ms[st].append(list(p))
                acq_ms[st].append(a)
        return m
    barrier_sync()
    t0 = time.perf_counter()
    group.run(steps, overlap=overlap, mark=mark, prefetch=overlap, feed=feed)
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if after:
        group.map(after, which=[(steps - 1) % n])
    if pool:
        group.map(to_first)
    full = [d for d in marks.values() if "apply" in d]
    stage_ms = [float(np.mean([d[order[j + 1]].elapsed_ms(d[order[j]]) for d in full])) for j in range(len(order) - 1)]
    if rx0.Mtestangles:
        bps = [d["post_end"].elapsed_ms(d["post_begin"]) for d in marks.values() if "post_end" in d] + [d["bps"].elapsed_ms(d["apply"]) for d in full if "bps" in d]
        stage_ms.append(float(np.mean(bps)))
    return elapsed, stage_ms, pass_ms, acq_ms


def channel_bank_run(cfg, sig, nch, steps, barrier_sync, trainer="iterative"):
    """Informational: `nch` independent captures of the workload resident on ONE GPU, all stages for all channels per step,
    exact trainers (one workgroup per channel and mode).  Every channel is an independent capture generated on the device
    (seed 2000 + c).  NOT the headline `value` (BASELINE configs are single captures)."""
    from qampy_amd import _lib
    from qampy_amd.core import ber_functions as ber
    from qampy_amd.pipeline import ChannelBank
    E = np.asarray(sig)
    bank = ChannelBank(nch, E.shape[0], E.shape[1], 2, cfg["M"], cfg["ntaps"], cfg["mu"], methods=cfg["methods"], Niter=cfg["niter"],
                       adaptive_stepsize=cfg["adaptive"], TrSyms=(None,) * len(cfg["methods"]), Mtestangles=cfg["A"], Nbps=cfg["Nbps"],
                       dtype=np.complex64, alphabet=sig.coded_symbols, trainer=trainer)
    from qampy_amd import synth
    nsym_c = E.shape[1] // 2
    idx_tx = []
    for c in range(nch):
        d = synth.make_capture_dev(cfg["M"], nsym_c, nmodes=E.shape[0], os=2, snr_db=cfg["snr_db"], theta=np.pi / 5.6 if E.shape[0] == 2 else None,
                                   dgd=30e-12, linewidth=cfg["linewidth"], fb=20e9, beta=0.1, seed=2000 + c, E=bank.E.row(c))
        idx_tx.append(d["idx_tx"])
    bank.run()
    ev0, ev1 = _lib.Event(), _lib.Event()
    barrier_sync()
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        bank.run()
    ev1.record()
    barrier_sync()
    el = time.perf_counter() - t0
    nsym = E.shape[1] // 2
    sers = {}
    worst = 0.
    for c in range(nch):
        rows = ber.cal_ser_dev((bank.out if cfg["A"] else bank.eq).row(c), idx_tx[c], bank.rx.alphabet, 256, 8192, 2000) if cfg["A"] else []
        ser_c = [r["errors"] / max(r["compared"], 1) for r in rows]
        worst = max([worst] + ser_c)
        if c in (0, nch // 2, nch - 1):
            sers[str(c)] = ser_c
    return dict(channels=nch, trainer=trainer, value=round(nch * nsym * steps / el / 1e6, 3), unit="MSym/s", steps=steps, ms_per_step=round(el / steps * 1e3, 2),
                ms_per_step_events=round(ev1.elapsed_ms(ev0) / steps, 2), ser_of_channels=sers, worst_ser=worst,
                note="informational: %d independent captures of this workload processed together on one GPU (exact trainers: one "
                     "workgroup per channel and mode in a single launch per stage); not the headline value" % nch)


def symbol_errors(out, sig, trim=2000):
    """(errors, compared) per mode of a recovered signal (host arrays); alignment on a prefix, decisions over the whole run."""
    from qampy_amd import synth
    from qampy_amd.core.equalisation import hip_equalisation as hk
    res = []
    npre = min(out.shape[1], 1 << 16)
    tx_idx = [hk.make_decision(np.ascontiguousarray(t), sig.coded_symbols)[2] for t in sig.symbols]
    for r in out:
        _, _, m, rot, lag = synth.count_symbol_errors(r[:npre], sig.symbols[:, :npre + 512], sig.coded_symbols, trim=min(trim, npre // 8))
        lag += min(trim, npre // 8)                                   # lag was measured on the trimmed prefix
        rx_idx = hk.make_decision(np.ascontiguousarray(r * np.complex64(np.exp(1j * rot * np.pi / 2))), sig.coded_symbols)[2]
        i0, i1 = trim, r.size - trim
        a = rx_idx[i0:i1]
        b = tx_idx[m][i0 - lag:i1 - lag]
        n = min(a.size, b.size)
        res.append((int(np.count_nonzero(a[:n] != b[:n])), int(n)))
    return res


# ------------------------------------------------------------------------------------------------------------ CPU legs
def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _omp_threads(n):
    """Set the OpenMP team size of the already loaded oracle (libgomp), returns the previous maximum."""
    import ctypes
    g = ctypes.CDLL("libgomp.so.1")
    prev = g.omp_get_max_threads()
    g.omp_set_num_threads(int(n))
    return prev


def cpu_pipeline(cfg, E, coded_symbols):
    """One pass of the hot path through the oracle (reference-flag OpenMP build) on host arrays; returns times + results."""
    from oracle import oracle
    from qampy_amd.core.equalisation import equalisation as host
    ntaps = cfg["ntaps"]
    nm = E.shape[0]
    w = host._init_taps(ntaps, nm, nm, np.complex64)
    tr = host._cal_training_symbol_len(2, ntaps, E.shape[1])
    syms = [host._reshape_symbols(coded_symbols if m in host.DECISION_BASED else None, m, cfg["M"], np.complex64, nm) for m in cfg["methods"]]
    angles = np.linspace(-np.pi / 4, np.pi / 4, cfg["A"] or 1, endpoint=False, dtype=np.float32).reshape(1, -1)
    t0 = time.perf_counter()
    for s, m in enumerate(cfg["methods"]):
        _, w, _ = oracle.train_equaliser(E, tr, cfg["niter"][s], 2, np.float32(cfg["mu"][s]), w, None, cfg["adaptive"][s], syms[s], m, fast=True)
    t1 = time.perf_counter()
    eq = oracle.apply_filter_to_signal(E, 2, w, fast=True)
    t2 = time.perf_counter()
    N = cfg["Nbps"]
    if cfg["A"]:
        ph = np.array([oracle.select_angles(angles, oracle.bps(eq[m], angles, coded_symbols, N, fast=True)) for m in range(nm)])
        ph[:, N:-N] = np.unwrap(ph[:, N:-N] * 4) / 4
        out = eq * np.exp(1j * ph)
    else:
        out = eq
    t3 = time.perf_counter()
    return dict(seconds=t3 - t0, train_s=t1 - t0, apply_s=t2 - t1, bps_s=t3 - t2, wxy=w, out=out.astype(np.complex64))


def cpu_baseline(cfg, sig, nsym, sample_1t, runs=3):
    """the whole capture with all host threads (`runs` runs -> spread) and a bounded sample with ONE thread."""
    from oracle import oracle
    try:
        oracle.build(fast_native=True)       # -march=native for THIS host
    except Exception as e:                   # fall back to the prebuilt library
        print("cpu_baseline: native rebuild failed (%s), using the prebuilt oracle" % e, file=sys.stderr)
    E = np.ascontiguousarray(np.asarray(sig)[:, :2 * nsym])
    ncores = os.cpu_count()
    res = [cpu_pipeline(cfg, E, sig.coded_symbols) for _ in range(runs)]
    secs = [r["seconds"] for r in res]
    best = res[int(np.argmin(secs))]
    prev = _omp_threads(1)
    try:
        one = cpu_pipeline(cfg, np.ascontiguousarray(E[:, :2 * sample_1t]), sig.coded_symbols)
    finally:
        _omp_threads(prev)
    return dict(all=dict(value=nsym / min(secs) / 1e6, runs_s=[round(s, 3) for s in secs], cores=ncores,
                         stages_s=dict(train=round(best["train_s"], 3), apply=round(best["apply_s"], 3), bps=round(best["bps_s"], 3))),
                one=dict(value=sample_1t / one["seconds"] / 1e6, sample=sample_1t, seconds=round(one["seconds"], 3),
                         stages_s=dict(train=round(one["train_s"], 3), apply=round(one["apply_s"], 3), bps=round(one["bps_s"], 3))),
                result=best)


CPU_BANK_WORKER = r"""
import sys, time, json, numpy as np
sys.path.insert(0, %(root)r)
import bench
cfg = dict(bench.WORKLOADS[%(workload)r])
d = np.load(%(path)r)
E, coded = d["E"], d["coded"]
bench.cpu_pipeline(cfg, np.ascontiguousarray(E[:, :8192]), coded)            # load + warm the library
t0 = time.perf_counter()
for _ in range(%(reps)d):
    bench.cpu_pipeline(cfg, E, coded)
print(json.dumps(dict(seconds=time.perf_counter() - t0)))
"""


def cpu_channel_bank(cfg, workload, sig, sample, workers, reps=1):
    """CPU counterpart of the channel bank: `workers` independent captures processed concurrently, one single-threaded
    oracle pipeline per capture (one process each, OMP_NUM_THREADS=1) - how a many-core host would run a WDM bank."""
    import tempfile
    path = os.path.join(tempfile.gettempdir(), "qampy_cpu_bank_%d.npz" % os.getpid())
    np.savez(path, E=np.ascontiguousarray(np.asarray(sig)[:, :2 * sample]), coded=np.asarray(sig.coded_symbols))
    code = CPU_BANK_WORKER % dict(root=ROOT, workload=workload, path=path, reps=reps)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    t0 = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, text=True) for _ in range(workers)]
    secs, last_err = [], ""
    for p in procs:
        out, err = p.communicate(timeout=600)
        try:
            secs.append(json.loads(out.strip().splitlines()[-1])["seconds"])
        except (ValueError, IndexError):
            last_err = err[-300:]
    wall = time.perf_counter() - t0
    try:
        os.remove(path)
    except OSError:
        pass
    if not secs:
        return dict(error="no worker finished: " + last_err)
    return dict(value=round(len(secs) * sample * reps / max(secs) / 1e6, 3), unit="MSym/s", workers=len(secs), threads_per_worker=1, sample=sample,
                reps=reps, slowest_worker_s=round(max(secs), 2), wall_s_incl_startup=round(wall, 1),
                note="aggregate of %d concurrent single-threaded oracle pipelines, each on its own copy of a %d-symbol capture" % (len(secs), sample))


def transfer_times(sig, rx):
    """Host <-> HBM copies the host-array entry points pay per capture (not part of `value`)."""
    from qampy_amd import _lib
    E = np.array(np.asarray(sig), copy=True, order="C")              # a FRESH pageable array: what a caller who just read a capture from disk hands over
    _lib.sync()
    t0 = time.perf_counter(); rx.E.set(E); _lib.sync(); h2d = time.perf_counter() - t0
    # ... and the same array again: the runtime pins the pages of a pageable source for the DMA and keeps the mapping, so a caller who re-uses its
    # input buffer pays the pinning once (round 5's line showed the first figure without saying so: 4.8 GB/s against round 4's 54 GB/s of a repeat)
    t0 = time.perf_counter(); rx.E.set(E); _lib.sync(); h2d_again = time.perf_counter() - t0
    t0 = time.perf_counter()
    o = (rx.out if rx.Mtestangles else rx.eq).to_host(); w = rx.wxy.to_host(); e = [x.to_host() for x in rx.err]
    d2h = time.perf_counter() - t0
    nb = o.nbytes + w.nbytes + sum(x.nbytes for x in e)
    return dict(h2d_ms=round(h2d * 1e3, 2), h2d_GBps=round(E.nbytes / h2d / 1e9, 1), h2d_same_array_again_ms=round(h2d_again * 1e3, 2),
                h2d_same_array_again_GBps=round(E.nbytes / h2d_again / 1e9, 1), d2h_ms=round(d2h * 1e3, 2), d2h_GBps=round(nb / d2h / 1e9, 1),
                bytes_in=int(E.nbytes), bytes_out=int(nb), note="pageable numpy arrays through hipMemcpy (h2d: first copy from a fresh array, pinning included; then the same array again); outputs = recovered signal + taps + both error traces into fresh pageable arrays")


# ------------------------------------------------------------------------------------------------------------ config 5
def pilot_chain(cap, dtype=np.complex64, frames=None, keep=False):
    """BASELINE config 5 through the basic API (host arrays in and out): sync2frame -> corr_foe -> pilot_equaliser_nframes (data-aided
    second stage, filter over every frame; from the second frame on the frames' pilot-aided sweeps train together: one launch per stage
    over all (frame, mode) chains) -> pilot_cpe over all frames; returns stage times and results (keep: with the arrays the calls returned)."""
    from qampy_amd import equalisation, phaserec
    from qampy_amd.signals import PilotSignal
    sig = PilotSignal(cap["E"].astype(dtype), cap["M"], cap["fb"], cap["fs"], cap["frame_len"], cap["seq_len"], cap["ins_rat"], cap["pilots"],
                      symbols=cap["payload"], coded_symbols=cap["alphabet"])
    t = [time.perf_counter()]
    ok = sig.sync2frame()
    t.append(time.perf_counter())
    sig.corr_foe()
    t.append(time.perf_counter())
    if frames is None:
        frames = np.arange((sig.shape[-1] - int(np.max(sig.shiftfctrs))) // (sig.os * sig.frame_len))
        while len(frames) > 1 and sig.shape[-1] - (int(np.max(sig.shiftfctrs)) + int(frames[-1]) * sig.os * sig.frame_len) <= sig.os * sig.frame_len + 64:
            frames = frames[:-1]
    taps, eq, _ = equalisation.pilot_equaliser_nframes(sig, (1e-3, 1e-3), 45, foe_comp=False, frames=list(frames), methods=("cma", "sbd_data"))
    t.append(time.perf_counter())
    out, ph = phaserec.pilot_cpe(eq, N=5, use_seq=False, nframes=len(frames))
    t.append(time.perf_counter())
    d = np.diff(t)
    res = dict(ok=bool(ok), seconds=t[-1] - t[0], frames=len(frames),
               stages_ms=dict(frame_sync=d[0] * 1e3, foe=d[1] * 1e3, pilot_equaliser_and_filter=d[2] * 1e3, pilot_cpe=d[3] * 1e3),
               ser=[float(v) for v in out.cal_ser(frames=np.arange(len(frames)))], taps=np.array(taps))
    if keep:
        res["arrays"] = dict(taps=np.array(taps), eq=np.asarray(eq), out=np.asarray(out), ph=np.asarray(ph))
    return res


class _OracleKernels:
    """cpu_baseline leg of config 5: the same host layer on the oracle's kernels (reference-flag build)."""

    def __enter__(self):
        from oracle import oracle
        from qampy_amd.core.equalisation import equalisation as core_eq
        k = core_eq._kernels
        self.k, self.saved = k, {n: getattr(k, n) for n in ("ResidentField", "ResidentJobs", "train_equaliser", "apply_filter_to_signal", "train_equaliser_windows_search")}

        class OracleField:
            def __init__(self, E, defer=False):
                self.E = E

            def finish(self):
                pass

            def train(self, *a):
                return oracle.train_equaliser(self.E, *a, fast=True)

            def apply(self, os_, wx, modes=None):
                return oracle.apply_filter_to_signal(self.E, os_, np.ascontiguousarray(wx), modes, fast=True)

        class OracleJobs:
            def __init__(self, slices, job_modes):
                self.slices, self.job_modes = [np.ascontiguousarray(x) for x in slices], [int(m) for m in job_modes]

            def train(self, TrSyms, Niter, os_, mu, wx, adaptive, symbols, method):
                for E, m in zip(self.slices, self.job_modes):
                    _, wx, _ = oracle.train_equaliser(E, TrSyms, Niter, os_, mu, wx, np.array([m]), adaptive, symbols, method, fast=True)
                return wx

            def train_bank(self, TrSyms, Niter, os_, mu, bank, adaptive, symbols, method):
                res = np.array(bank, copy=True)
                for j, (E, m) in enumerate(zip(self.slices, self.job_modes)):
                    _, w, _ = oracle.train_equaliser(E, TrSyms, Niter, os_, mu, np.ascontiguousarray(res[j]), np.array([m]), adaptive, symbols, method, fast=True)
                    res[j] = w
                return res

            def apply(self, os_, wx):
                return np.array([oracle.apply_filter_to_signal(E, os_, np.ascontiguousarray(wx), np.array([m]), fast=True)[0] for E, m in zip(self.slices, self.job_modes)])

        def search(E, starts, win_len, TrSyms, Niter, os_, mu, wx0, modes, adaptive, symbols, method):
            res = [oracle.train_equaliser(np.ascontiguousarray(E[:, s0:s0 + win_len]), TrSyms, Niter, os_, mu, wx0.copy(), modes, adaptive, symbols, method, fast=True)
                   for s0 in np.asarray(starts)]
            var = np.array([np.var(r[0], axis=-1) for r in res]).T
            best = np.argmin(var, axis=-1)
            return var, best, np.array([res[b][1] for b in best])

        k.ResidentField = OracleField
        k.ResidentJobs = OracleJobs
        k.train_equaliser = lambda *a: oracle.train_equaliser(*a, fast=True)
        k.apply_filter_to_signal = lambda *a, **kw: oracle.apply_filter_to_signal(*a, fast=True, **kw)
        k.train_equaliser_windows_search = search
        from qampy_amd.core import phaserecovery
        self.dsp, self.cfo = phaserecovery._dsp, phaserecovery._dsp.comp_freq_offset
        t_exp = lambda E, fo, os_=1: (E * np.exp(-2j * np.pi * np.arange(1, E.shape[1] + 1, dtype=float) * np.asarray(fo, dtype=float).reshape(-1, 1) / os_)).astype(E.dtype)
        self.dsp.comp_freq_offset = t_exp
        self.trace = self.dsp.pilot_phase_trace

        def t_trace(E, knots, kph):
            tr = np.array([np.interp(np.arange(E.shape[1]), knots, p) for p in kph]).astype(E.dtype)
            return E * np.exp(-1j * tr), tr
        self.dsp.pilot_phase_trace = t_trace
        return self

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            setattr(self.k, n, v)
        self.dsp.comp_freq_offset = self.cfo
        self.dsp.pilot_phase_trace = self.trace


def run_c5(args, cfg):
    """`--workload c5`: the pilot receiver is a CALLER of the hot path; single GPU, host arrays in and out
    (so `value` includes the PCIe copies of the basic API - noted in the line).  A capture of `--c5-frames` frames (default 9: eight whole
    frames after the synchronisation) is recovered per step: frame sync once per capture, the frames' pilot trainings batched."""
    from qampy_amd import synth, _lib
    _lib.init(0)
    cap = synth.make_pilot_capture(M=cfg["M"], frame_len=cfg["nsym"], nframes=args.c5_frames)
    for _ in range(max(args.warmup, 1)):
        pilot_chain(cap)
    runs = [pilot_chain(cap, keep=bool(args.dump_outputs) and k == args.steps - 1) for k in range(args.steps)]
    el = sum(r["seconds"] for r in runs)
    best = runs[-1]
    nfr = best["frames"]
    if args.dump_outputs:
        write_dump(dump_files(best.pop("arrays")), args.dump_outputs)
    # the sequential heart of a frame: Niter sweeps x 3 stages x seq_len steps of the exact recurrence with the adaptive step, two modes side by side
    steps_per_frame = 3 * 30 * 1024
    out = dict(metric="equalised MSym/s (2-pol, 2 SPS; a step recovers %d frames of one capture)" % nfr, value=round(cfg["nsym"] * nfr * args.steps / el / 1e6, 4), unit="MSym/s", n_gpus=1,
               ranks_seen=1, steps=args.steps,
               warmup=args.warmup, ms_per_step=round(el / args.steps * 1e3, 3), ms_per_frame=round(el / args.steps / nfr * 1e3, 3), higher_is_better=True, scaling="weak",
               vs_baseline=None, dtype="f32", data="synthetic",
               config=dict(workload=cfg["label"], key="c5", frame_len=cfg["nsym"], frames_captured=args.c5_frames, frames_recovered=nfr, ntaps=[17, 45],
                           methods=list(cfg["methods"]), niter=[10, 30], boundary="basic API: host arrays in and out (PCIe inside the timed region)",
                           batching="frame sync once per capture; pre-convergence stages frame after frame (the reference hands the taps on in place), the 2 x 30 "
                                    "pilot-aided sweeps of frames 1.. together: one launch per stage over all (frame, mode) chains"),
               stages_ms={k: round(float(np.mean([r["stages_ms"][k] for r in runs])), 3) for k in best["stages_ms"]},
               ser=dict(payload_per_mode=best["ser"], sync_ok=best["ok"]), device=_lib.device_name(),
               roofline=dict(bound="latency (dependent instruction issue)", kernel="pilot-sequence training (exact recurrence, adaptive step: 3 x 30 sweeps of 1024 steps per frame)",
                             achieved=round(steps_per_frame * nfr / (best["stages_ms"]["pilot_equaliser_and_filter"] * 1e-3) / 1e6, 3), peak=None, unit="M sequential steps/s",
                             frac=None, traffic=None,
                             note="sequential chains of 1024 steps x 30 sweeps: neither HBM nor MFMA bounds them - one dependent step costs ~130 ns on a lone "
                                  "wavefront (DESIGN.md 3.1); what the batching buys is that the chains of all frames and modes run side by side"))
    if args.full:
        one = pilot_chain(cap, frames=[0])                      # the same capture, first frame only (what rounds 1-3 timed)
        out["single_frame"] = dict(ms=round(one["seconds"] * 1e3, 3), stages_ms={k: round(v, 3) for k, v in one["stages_ms"].items()})
    if args.full and not args.no_cpu_baseline:
        from oracle import oracle
        try:
            oracle.build(fast_native=True)
        except Exception:
            pass
        with _OracleKernels():
            pilot_chain(cap, np.complex64, frames=[0])
            cpu = pilot_chain(cap, np.complex64)
        out["cpu_baseline"] = dict(value=round(cfg["nsym"] * cpu["frames"] / cpu["seconds"] / 1e6, 4), unit="MSym/s", cores=os.cpu_count(), kind="port",
                                   sample="the same capture (%d frames) through the same host layer on the oracle's kernels (one run)" % cpu["frames"], cpu_model=cpu_model(),
                                   stages_ms={k: round(v, 2) for k, v in cpu["stages_ms"].items()})
        out["parity_vs_cpu"] = dict(ser_gpu=best["ser"], ser_cpu=cpu["ser"], max_abs_tap_diff=float(np.max(np.abs(best["taps"] - cpu["taps"]))))
        out["speedup_vs_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 2)
    emit(out, args.detail_out)


# ------------------------------------------------------------------------------------------------------------ tiers
ELEMENTWISE_RTOL = ELEMENTWISE_ATOL = 1e-4        # the bar the EXACT path is held to against the golden vectors (tests/conftest.py, SURVEY.md 8c: complex64)


def elementwise(ref, got, rtol=ELEMENTWISE_RTOL, atol=ELEMENTWISE_ATOL):
    """np.testing.assert_allclose's criterion as a measurement: share of elements with |got - ref| <= atol + rtol |ref|, and the largest deviation."""
    d = np.abs(np.asarray(got) - np.asarray(ref))
    ok = d <= atol + rtol * np.abs(ref)
    return dict(share_within=float(np.mean(ok)) if d.size else 1.0, max_abs=float(d.max()) if d.size else 0.0, outside=int(d.size - np.count_nonzero(ok)))


def deviation_vs_exact(rx, rxa, cfg):
    """How far tier b's results are from the exact path's on the same capture (host copies): recovered output, taps and the error
    trace of every stage, per output mode, modulo a common quarter turn per mode (symmetry of the error functions)."""
    wa, wb = rxa.wxy.to_host(), rx.wxy.to_host()
    ea = (rxa.out if cfg["A"] else rxa.eq).to_host()
    eb = (rx.out if cfg["A"] else rx.eq).to_host()
    out_rms, out_max, tap_rel, tap_max, g_m = [], [], [], [], []
    ew = dict(rtol=ELEMENTWISE_RTOL, atol=ELEMENTWISE_ATOL, taps=[], equaliser_out=[], err_traces=[])
    for m in range(wa.shape[0]):
        g = 1j ** int(np.rint(np.angle(np.vdot(wb[m].ravel(), wa[m].ravel())) / (np.pi / 2)))
        g_m.append(g)
        ew["taps"].append(elementwise(wa[m], g * wb[m]))
        tap_rel.append(float(np.linalg.norm(wa[m] - g * wb[m]) / np.linalg.norm(wa[m])))
        tap_max.append(float(np.max(np.abs(wa[m] - g * wb[m]))))
        dd = np.abs(ea[m] - g * eb[m])
        out_rms.append(float(np.sqrt(np.mean(dd ** 2)) / np.sqrt(np.mean(np.abs(ea[m]) ** 2))))
        out_max.append(float(dd.max()))
    del ea, eb
    extra = {}
    if cfg["A"]:
        # the same for the equaliser output BEFORE the phase search, and how often the search picked another test angle: the search is an
        # arg-min over A angles per symbol - a near-tie flips with any perturbation (the reference's own float32 / float64 runs differ
        # there too) and turns a window of symbols by one angle step (pi / 2 / A rad); `out_rms_dev_same_angle` leaves those symbols out
        qa, qb = rxa.eq.to_host(), rx.eq.to_host()
        ia, ib = rxa.idx.to_host(), rx.idx.to_host()
        oa, ob = rxa.out.to_host(), rx.out.to_host()
        eq_rms, flip, same = [], [], []
        for m in range(wa.shape[0]):
            g = g_m[m]
            eq_rms.append(float(np.sqrt(np.mean(np.abs(qa[m] - g * qb[m]) ** 2)) / np.sqrt(np.mean(np.abs(qa[m]) ** 2))))
            ew["equaliser_out"].append(elementwise(qa[m], g * qb[m]))
            k = int(np.rint(np.angle(g) / (np.pi / 2)))              # a quarter turn of the taps shifts the selected angle by a whole period
            keep = ((ia[m] - ib[m]) % cfg["A"]) == 0 if k == 0 else None
            if keep is None:                                          # (compare through the phases instead)
                pa_, pb_ = rxa.ph.to_host()[m], rx.ph.to_host()[m]
                keep = np.abs(np.angle(np.exp(1j * (pa_ - pb_)) * np.conj(g))) < 0.25 * (np.pi / 2 / cfg["A"])
            flip.append(float(1.0 - np.mean(keep)))
            dd = np.abs(oa[m] - g * ob[m])[keep]
            same.append(float(np.sqrt(np.mean(dd ** 2)) / np.sqrt(np.mean(np.abs(oa[m]) ** 2))) if dd.size else 0.0)
        extra = dict(eq_rms_dev_vs_exact=eq_rms, bps_angle_mismatch_fraction=flip, out_rms_dev_same_angle=same)
        del qa, qb, ia, ib, oa, ob
    else:
        qa, qb = rxa.eq.to_host(), rx.eq.to_host()
        ew["equaliser_out"] = [elementwise(qa[m], g_m[m] * qb[m]) for m in range(wa.shape[0])]
        del qa, qb
    err_rms = []
    for s_ in range(rx.nstage):                                   # error traces: rms of the difference, in units of the signal rms (unit power)
        xa, xb = rxa.err[s_].to_host(), rx.err[s_].to_host()
        row, ewrow = [], []
        for m in range(xa.shape[0]):
            c = np.vdot(xb[m], xa[m])
            g = 1j ** int(np.rint(np.angle(c) / (np.pi / 2))) if abs(c) > 0 else 1.0
            row.append(float(np.sqrt(np.mean(np.abs(xa[m] - g * xb[m]) ** 2))))
            ewrow.append(elementwise(xa[m], g * xb[m]))
        err_rms.append(row)
        ew["err_traces"].append(ewrow)
        del xa, xb
    return dict(out_rms_dev_vs_exact=out_rms, out_max_dev_vs_exact=out_max, tap_rel_dev_vs_exact=tap_rel, max_abs_tap_dev_vs_exact=tap_max,
                err_trace_rms_dev_vs_exact=err_rms, elementwise=ew, **extra)


def tier_b_block(cfg, rx, stage_names, pass_ms, acq_ms, reports, value, ms, errs, nsym):
    kern = []
    for s in range(rx.nstage):
        flat = [p for step in pass_ms[s] for p in step]
        kern.append(dict(mean_ms=float(np.mean(flat)) if flat else 0., acquisition_ms=float(np.mean(acq_ms[s])) if acq_ms[s] else 0.))
    return dict(method="parallel in time: %s; segments trained concurrently by the exact kernels, waveform relaxation + linearised coarse "
                       "correction; segment 0 starts from the caller's taps (fixed point = the sequential recurrence); stopped by the device-side "
                       "estimate of the output deviation from the sequential recurrence < tol" % " -> ".join(cfg["methods"]),
                value=round(value, 4), unit="MSym/s", ms_per_step=round(ms, 3),
                stages=[dict(stage=stage_names[1 + s], S=r["segments"], seg_len=r["seg_len"], P=r["passes"], converged=r["converged"], exact_form=bool(r.get("exact_form", False)), tol=r["tol"],
                             defect=[float("%.3g" % d) for d in r["defect"]],
                             est_deviation_rms=[float("%.3g" % d) for d in r.get("deviation_rms", [])],
                             est_deviation_worst=[float("%.3g" % d) for d in r.get("deviation", [])],
                             est_deviation_taps=[float("%.3g" % d) for d in r.get("deviation_taps", [])],
                             est_deviation_taps_worst=[float("%.3g" % d) for d in r.get("deviation_taps_worst", [])],
                             result_change=[float("%.3g" % d) for d in r.get("result_change", [])],
                             acquisition=dict(steps=r["acquisition"]["steps"], mu=r["acquisition"]["mu"], diverged=r["acquisition"]["diverged"]),
                             coarse_correction=r["correction"], gain=round(r["gain"], 4),
                             pass_ms=round(kern[s]["mean_ms"], 3), acquisition_ms=round(kern[s]["acquisition_ms"], 3))
                        for s, r in enumerate(reports)],
                errors=[e for e, _ in errs], converged=bool(all(r["converged"] for r in reports)),
                limits=dict(max_segments=65536, coarse_correction_max_nmodes_x_ntaps=128, segment_kernel_max_taps="(64+4)*os + ntaps + 8 <= 192",
                            max_passes_default=16, max_passes_cap=24),
                pipeline_hbm=dict(achieved=round(FUSED_BYTES_PER_SYM * nsym / (ms * 1e-3) / 1e9, 2), peak=HBM_PEAK_GBS, unit="GB/s",
                                  frac=round(FUSED_BYTES_PER_SYM * nsym / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 6),
                                  note="whole step against the fully fused lower bound of 88 B per symbol period"))


def make_pool(cfg, nsym, rx, first_seed, ncap):
    """`ncap` resident captures for one receiver: its own (already loaded: seed `first_seed`) and ncap - 1 more synthesised on the device, seeds
    1000 + ((first_seed - 1000 + j) mod ncap) - the ranks of an N-GPU run rotate through the SAME captures, each starting at its own."""
    from qampy_amd import synth
    pool = [rx.E]
    for j in range(1, ncap):
        seed = 1000 + ((first_seed - 1000 + j) % ncap)
        pool.append(synth.make_capture_dev(cfg["M"], nsym, nmodes=cfg.get("nmodes", 2), os=2, snr_db=cfg["snr_db"], theta=np.pi / 5.6 if cfg.get("nmodes", 2) == 2 else None,
                                           dgd=30e-12, linewidth=cfg["linewidth"], fb=20e9, beta=0.1, seed=seed)["E"])
    return pool


def run_pair(cfg, sig, nsym, steps, warmup, barrier_sync, pit, exact_steps, tol_check, overlap=False, in_flight=1, pool_n=1, first_seed=1000, after=None,
             full=True):
    """Tier b (timed, `steps` passes) and the exact path beside it on the same resident capture: both blocks, the measured
    deviation and the certificate.  Returns (tier_b, tier_a, extras for the roofline).  after: timed_steps' hook, for tier b's timed passes.

    overlap: the timed passes are consecutive captures of a running receiver (ResidentReceiver.run(overlap=True): phase search of pass k
    beside the training of pass k + 1); the same receiver is then timed one capture at a time as well (`one_capture_at_a_time`).
    full: also the timing runs of their own that only the roofline and the informational figures read (every pass event-timed,
    one capture at a time, one receiver of a group); the certificate does not depend on them."""
    overlap = bool(overlap and cfg["A"])
    group, pool = None, None
    if in_flight > 1 and overlap:
        # `in_flight` captures on the GPU at a time (pipeline.ReceiverGroup): the timed K passes are dealt round robin to that many receivers
        group = make_group(in_flight, cfg, sig, pit)
        group.load(sig)
        rx = group.rx[0]
        names, _ = stage_list(rx)
        pool = make_pool(cfg, nsym, rx, first_seed, pool_n) if pool_n > 1 else None
        elapsed, stage_ms, pass_ms, acq_ms = timed_group(group, steps, warmup, barrier_sync, overlap=True, pool=pool, after=after)
    else:
        rx = make_receiver(cfg, sig, tier="b", pit=pit)
        rx.load(sig)
        names, _ = stage_list(rx)
        pool = make_pool(cfg, nsym, rx, first_seed, pool_n) if (overlap and pool_n > 1) else None
        elapsed, stage_ms, pass_ms, acq_ms = timed_steps(rx, steps, warmup, barrier_sync, overlap=overlap, pool=pool, after=after)
    reports = rx.pit_reports()
    pass_all = None
    if full and group is None and not getattr(rx, "exchanges", None):
        # every relaxation pass timed (an event pair per pass: ~11 us of idle stream per pass - a run of its own, after the timed region, in the same
        # mode): the dominant kernel's AVERAGE launch duration for the roofline (the timed region itself times one pass per sweep, pass 1)
        from qampy_amd import _lib as _l
        _l.call("qh_set_pit_timing", 2)
        try:
            _, _, pass_all, _ = timed_steps(rx, max(2, min(steps, 16)), 1, barrier_sync, overlap=overlap, pool=pool)      # (two rounds of the capture pool: a 5-step sample let one disturbed pass move the average by 10 %)
        finally:
            _l.call("qh_set_pit_timing", 1)
    ser_rows = rx.ser(sig.symbols, maxlag=256, window=8192, trim=2000) if cfg["A"] else []
    errs = [(d["errors"], d["compared"]) for d in ser_rows]
    tb = tier_b_block(cfg, rx, names, pass_ms, acq_ms, reports, nsym * steps / elapsed / 1e6, elapsed / steps * 1e3, errs, nsym)
    tb["stages_ms"] = {n: round(t, 3) for n, t in zip(names, stage_ms)}
    if pool:
        tb["capture_pool"] = dict(captures=len(pool), seeds=[first_seed] + [1000 + ((first_seed - 1000 + j) % len(pool)) for j in range(1, len(pool))],
                                  what="the K timed captures are DIFFERENT captures: a pool of resident captures rotated through the receiver's two input buffers (references, no "
                                       "copies); stages / passes / deviations / symbol errors in this block belong to the pool's first capture (seed %d), processed once more "
                                       "after the timed region" % first_seed)
    if pass_all is not None:
        for s_, st in enumerate(tb["stages"]):
            flat = [p for step in pass_all[s_] for p in step]
            per_pass = [float(np.mean([step[q] for step in pass_all[s_] if len(step) > q])) for q in range(max((len(step) for step in pass_all[s_]), default=0))]
            st["pass_ms_all_launches"] = round(float(np.mean(flat)), 4) if flat else None
            st["pass_ms_by_pass"] = [round(x, 4) for x in per_pass]
    if group is not None:
        # every receiver of the group: certified by the device, and bit for bit the result of receiver 0
        others = [g.fetch() for g in group.rx[1:]]
        mine = rx.fetch()
        same = all(np.array_equal(o[k], mine[k]) for o in others for k in ("wxy", "eq", "out"))
        conv = all(r["converged"] for rp in group.pit_reports() for r in rp)
        del others, mine
        from qampy_amd import _lib as _l
        tb["in_flight"] = dict(receivers=in_flight, all_receivers_identical=bool(same), all_receivers_converged=bool(conv),
                               what="%d captures on the GPU at a time, one host thread and one set of library streams per receiver (pipeline.ReceiverGroup); "
                                    "pass_ms / stages_ms are means over all receivers inside the timed region" % in_flight)
        if full:
            k0 = max(2, min(steps, 10))
            el0, ms0, _, _ = group.map(lambda r: timed_steps(r, k0, 1, _l.sync, overlap=True), which=[0])[0]      # on the receiver's own thread (its streams, its scratch)
            tb["in_flight"]["one_receiver"] = dict(value=round(nsym * k0 / el0 / 1e6, 4), ms_per_step=round(el0 / k0 * 1e3, 3), steps=k0,
                                                   stages_ms={n: round(t, 3) for n, t in zip(names, ms0)})
        tb["converged"] = bool(tb["converged"] and same and conv)
    if overlap:
        tb["pipelining"] = dict(
            what="consecutive captures: the phase search of pass k runs on stream 2 beside the training of pass k + 1 (same kernels, same results bit for bit); "
                 "stages_ms are event pairs on the stream each stage ran on, so their sum exceeds ms_per_step by what ran side by side")
        if full:
            k1 = max(2, min(steps, 5))
            if group is not None:
                el1, ms1, _, _ = group.map(lambda r: timed_steps(r, k1, 1, _l.sync), which=[0])[0]
            else:
                el1, ms1, _, _ = timed_steps(rx, k1, 1, barrier_sync)
            tb["pipelining"]["one_capture_at_a_time"] = dict(value=round(nsym * k1 / el1 / 1e6, 4), ms_per_step=round(el1 / k1 * 1e3, 3), steps=k1,
                                                             stages_ms={n: round(t, 3) for n, t in zip(names, ms1)})
    ta = None
    if exact_steps > 0:
        rxa = make_receiver(cfg, sig, tier="a")
        rxa.load(sig)
        el_a, ms_a, _, _ = timed_steps(rxa, exact_steps, 1, barrier_sync)
        errs_a = [d["errors"] for d in rxa.ser(sig.symbols, maxlag=256, window=8192, trim=2000)] if cfg["A"] else []
        ta = dict(method="exact sequential recurrence (reference order of evaluation)", value=round(nsym * exact_steps / el_a / 1e6, 4), unit="MSym/s",
                  steps=exact_steps, ms_per_step=round(el_a / exact_steps * 1e3, 3), stages_ms={n: round(t, 3) for n, t in zip(names, ms_a)},
                  errors=errs_a,
                  train_cycles_per_step={names[1 + s2]: round(ms_a[1 + s2] * 1e-3 * 2.4e9 / (rxa.TrSyms[s2] * rxa.Niter[s2]), 1) for s2 in range(rxa.nstage)})
        dev = deviation_vs_exact(rx, rxa, cfg)
        tb.update(dev)
        tb["errors_exact"] = errs_a
        tb["speedup_vs_exact"] = round(tb["value"] / ta["value"], 2)
        # the certificate of this run: the device's own (every stage's estimated deviation below tol) AND the measurement against
        # the exact path: recovered output within tol (relative rms), taps within 3 tol (relative norm; the device holds its rms-over-segments
        # estimate to 2 tol, the final taps sit at the worst segment of it), decisions: identical error counts +-3
        # (with a phase search behind the equaliser the tolerance is held by the equaliser output and by the recovered output on the
        # symbols where both searches chose the same test angle; where a near-tie of the arg-min fell the other way the recovered output
        # differs by one angle step whatever the tolerance - the fraction of such symbols and the all-symbol figure are in the line too)
        ok_eq = all(d <= tol_check for d in dev.get("eq_rms_dev_vs_exact", dev["out_rms_dev_vs_exact"]))
        ok_same = all(d <= tol_check for d in dev.get("out_rms_dev_same_angle", dev["out_rms_dev_vs_exact"]))
        ok_tap = all(d <= 3 * tol_check for d in dev["tap_rel_dev_vs_exact"])
        ok_ser = all(abs(a - b) <= SER_TOL_ERRORS for a, b in zip(errs_a, [e for e, _ in errs]))
        ok_err = all(d <= 3 * tol_check for row in dev["err_trace_rms_dev_vs_exact"] for d in row)
        # every entry of `checks` is part of the certificate (all must hold); figures that are reported but not held to the tolerance
        # are under `info` - the recovered output over ALL symbols includes the windows in which a near-tie of the phase search's arg-min
        # fell the other way (one test-angle step, whatever the tolerance; the reference's own float32 / float64 runs differ there too)
        tb["checks"] = dict(converged=tb["converged"], equaliser_out_rms_dev_le_tol=bool(ok_eq), recovered_out_rms_dev_on_same_angle_symbols_le_tol=bool(ok_same),
                            tap_rel_dev_le_3tol=bool(ok_tap), err_trace_rms_dev_le_3tol=bool(ok_err), errors_within_3=bool(ok_ser), tol=tol_check)
        # ELEMENT by element (round 6): the bar the exact path is held to against the golden vectors (assert_allclose, rtol = atol = 1e-4) - at the
        # tolerance 1e-4 every tap and every sample of the equaliser output has to be inside it (part of the certificate); the error traces are
        # measured and reported (an earlier stage is certified at 2 tol and its error function turns an output deviation into 1.3 - 5 x as much
        # trace deviation on the outer symbols): `elementwise_summary`
        ew = dev["elementwise"]
        tb["elementwise_summary"] = dict(
            rtol=ew["rtol"], atol=ew["atol"],
            taps_share_within=min(r["share_within"] for r in ew["taps"]), taps_max_abs=max(r["max_abs"] for r in ew["taps"]),
            equaliser_out_share_within=min(r["share_within"] for r in ew["equaliser_out"]), equaliser_out_max_abs=max(r["max_abs"] for r in ew["equaliser_out"]),
            err_traces_share_within=[min(r["share_within"] for r in row) for row in ew["err_traces"]],
            err_traces_max_abs=[max(r["max_abs"] for r in row) for row in ew["err_traces"]])
        if tol_check <= ELEMENTWISE_RTOL * (1 + 1e-9):
            tb["checks"]["taps_every_element_within_rtol_atol_1e-4"] = bool(tb["elementwise_summary"]["taps_share_within"] == 1.0)
            tb["checks"]["equaliser_out_every_element_within_rtol_atol_1e-4"] = bool(tb["elementwise_summary"]["equaliser_out_share_within"] == 1.0)
        tb["info"] = dict(recovered_out_rms_dev_all_symbols=dev["out_rms_dev_vs_exact"], other_angle_symbol_fraction=dev.get("bps_angle_mismatch_fraction"),
                          exact_form_stages=[st["stage"] for st in tb["stages"] if st.get("exact_form")])
        tb["certified"] = bool(all(v for k, v in tb["checks"].items() if k != "tol"))
        del rxa
    else:
        tb["certified"] = tb["converged"]
    if group is not None:
        group.close()
    return tb, ta, dict(rx=rx, names=names, stage_ms=stage_ms, elapsed=elapsed, errs=errs, reports=reports)


def api_end_to_end_block(cfg, sig, nsym, tol, rx_ref, reps=3):
    """What a drop-in user gets, PCIe included: numpy arrays in -> ``qampy_amd.equalisation.dual_mode_equalisation`` (or equalise_signal for a
    one-stage recipe) with the process-wide default tier set to b (``qampy_amd.set_default_tier("b", tol)`` - no ``tier=`` keyword at the call,
    exactly what the reference's callers write, qampy/equalisation.py:194-264) -> ``qampy_amd.phaserec.bps`` (qampy/phaserec.py:62-92) -> numpy
    arrays out (taps, both error traces, equalised signal, recovered signal, phase).  Checked against the resident receiver's results on the
    same capture (same solver, same tolerance: identical)."""
    import qampy_amd
    from qampy_amd import equalisation as api_eq, phaserec as api_ph, _lib
    was = qampy_amd.get_default_tier()
    qampy_amd.set_default_tier("b", tol)
    try:
        def once(sig=sig):
            if len(cfg["methods"]) == 2:
                out, wxy, errs = api_eq.dual_mode_equalisation(sig, cfg["mu"], cfg["ntaps"], Niter=cfg["niter"], methods=cfg["methods"],
                                                               adaptive_stepsize=cfg["adaptive"])
            else:
                out, wxy, e1 = api_eq.equalise_signal(sig, cfg["mu"][0], Ntaps=cfg["ntaps"], Niter=cfg["niter"][0], method=cfg["methods"][0],
                                                      adaptive_stepsize=cfg["adaptive"][0], apply=True)
                errs = (e1,)
            rec, ph = api_ph.bps(out, cfg["A"], cfg["Nbps"])
            return out, wxy, errs, rec, ph
        res = once()                                            # warm-up (pools, scratch)
        _lib.sync()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = once()
            t.append(time.perf_counter() - t0)
        # the same chain on a FRESH input array (a capture just read from disk: the runtime pins its pages for the DMA on first use - `transfers`)
        fresh = sig.recreate_from_np_array(np.array(np.asarray(sig), copy=True, order="C"))
        _lib.sync()
        t0 = time.perf_counter()
        once(fresh)
        t_fresh = time.perf_counter() - t0
        del fresh
        out, wxy, errs, rec, ph = res
        nbytes_in = np.asarray(sig).nbytes + np.asarray(out).nbytes
        nbytes_out = sum(np.asarray(e).nbytes for e in errs) + np.asarray(out).nbytes + np.asarray(rec).nbytes + np.asarray(ph).nbytes
        ref = rx_ref.fetch()
        same = dict(taps=bool(np.array_equal(np.asarray(wxy), ref["wxy"])), equalised=bool(np.array_equal(np.asarray(out), ref["eq"])),
                    recovered=bool(np.array_equal(np.asarray(rec), ref["out"])),
                    taps_max_abs_dev=float(np.max(np.abs(np.asarray(wxy) - ref["wxy"]))),
                    recovered_rel_rms_dev=float(np.sqrt(np.mean(np.abs(np.asarray(rec) - ref["out"]) ** 2) / np.mean(np.abs(ref["out"]) ** 2))))
        best = min(t)
        return dict(value=round(nsym / best / 1e6, 3), unit="MSym/s", ms_per_capture=round(best * 1e3, 3), runs_ms=[round(x * 1e3, 3) for x in t], tol=tol,
                    fresh_input_array=dict(ms_per_capture=round(t_fresh * 1e3, 3), value=round(nsym / t_fresh / 1e6, 3),
                                           note="one call on an input array the runtime has not seen (its pages are pinned for the DMA on first use); `value` "
                                                "above is the steady state of a caller that re-uses its input buffer"),
                    host_bytes_in=int(nbytes_in), host_bytes_out=int(nbytes_out),
                    pcie_floor_ms=round((nbytes_in / 54.5e9 + nbytes_out / 55e9) * 1e3, 2),
                    same_as_resident_receiver=same,
                    what="numpy in -> qampy_amd.equalisation.dual_mode_equalisation -> qampy_amd.phaserec.bps -> numpy out; default tier b set process-wide "
                         "(qampy_amd.set_default_tier), results on pooled pinned memory, stage 1's error trace copied back while stage 2 trains, the rows of "
                         "the phase search pipelined over both PCIe directions; pcie_floor_ms = the bytes that cross at ~55 GB/s one after the other")
    finally:
        qampy_amd.set_default_tier(*was)


def ref_benchmarks_block(tol, cpu=True):
    """The reference's OWN benchmark definitions (/root/reference/test/test_benchmarks.py: test_equalisation_prec :57-80, test_bps :38-47,
    test_apply_filter_benchmark :128-150, test_quantize_precision :22-30, test_select_angles_benchmark :152-176) through the same call
    surface - host arrays in and out, PCIe included - on captures of the same shape from this repository's generator: best of 3 wall times of
    the call the reference hands to pytest-benchmark; beside each, the oracle's reference-flag build on the same arrays (all host threads)."""
    from qampy_amd import synth, equalisation as api_eq, phaserec as api_ph, theory
    from qampy_amd.core import hip_dsp
    from qampy_amd.core.equalisation import equalisation as host, hip_equalisation as hk
    from oracle import oracle

    def best(fn, n=3):
        fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter(); r = fn(); t.append(time.perf_counter() - t0)
        return round(min(t) * 1e3, 3), r
    import ctypes as C

    def cpu_best(fn):
        """the CPU port at its best thread count out of {all, 16, 1} (an OpenMP team of hundreds of threads costs a small call more than it gives)"""
        try:
            gomp = C.CDLL("libgomp.so.1")
        except OSError:
            return best(fn)[0], os.cpu_count()
        res = []
        for nt in (os.cpu_count(), 16, 1):
            gomp.omp_set_num_threads(int(nt))
            res.append((best(fn)[0], nt))
        gomp.omp_set_num_threads(int(os.cpu_count()))
        return min(res)
    rows = []
    # ---- test_equalisation_prec: QPSK, 10^5 symbols, 2 modes, 2 samples / symbol, 40 taps, mu = 4e-4, adaptive step, 14 dB, PMD
    for dt in (np.complex64, np.complex128):
        sig = synth.make_capture(4, 10 ** 5, nmodes=2, os=2, snr_db=14, theta=np.pi / 5.45, dgd=75e-12, linewidth=0., fb=40e9, beta=0.1, seed=7, dtype=dt)
        E = np.ascontiguousarray(np.asarray(sig))
        for method in ("cma", "mcma", "sbd", "mddma", "dd"):
            row = dict(bench="equalise_signal", method=method, dtype=np.dtype(dt).name, nsym=10 ** 5, ntaps=40, adaptive_stepsize=True)
            row["tier_a_ms"], (w_a, e_a) = best(lambda: api_eq.equalise_signal(sig, 4e-4, Ntaps=40, method=method, adaptive_stepsize=True, tier="a"))
            row["tier_b_ms"], (w_b, e_b) = best(lambda: api_eq.equalise_signal(sig, 4e-4, Ntaps=40, method=method, adaptive_stepsize=True, tier="b", pit=dict(tol=tol)))
            rep = host.last_pit_reports()
            row["tier_b_exact_form"] = bool(rep and rep[0].get("exact_form"))
            row["tier_b_tap_rel_dev"] = float(np.linalg.norm(w_a - w_b) / np.linalg.norm(w_a))
            if cpu:
                tr = host._cal_training_symbol_len(2, 40, E.shape[1])
                sy = host._reshape_symbols(sig.coded_symbols if method in host.DECISION_BASED else None, method, 4, dt, 2)
                rt = np.float32 if dt is np.complex64 else np.float64
                row["cpu_port_ms"], row["cpu_port_threads"] = cpu_best(lambda: oracle.train_equaliser(E, tr, 1, 2, rt(4e-4), host._init_taps(40, 2, 2, dt), None, True, sy, method, fast=True))
            rows.append(row)
    # ---- test_bps: 64-QAM, 2^12 symbols (x 2 modes here), 64 test angles, N = 11
    for dt in (np.complex64, np.complex128):
        s1 = synth.make_capture(64, 2 ** 12, nmodes=2, os=1, snr_db=35, linewidth=0., seed=8, dtype=dt) * np.exp(1j * np.pi / 5.1)
        row = dict(bench="bps", dtype=np.dtype(dt).name, nsym=2 ** 12, test_angles=64, N=11)
        row["hip_ms"], _ = best(lambda: api_ph.bps(s1, 64, 11))
        if cpu:
            rt = np.float32 if dt is np.complex64 else np.float64
            ang = np.linspace(-np.pi / 4, np.pi / 4, 64, endpoint=False, dtype=rt).reshape(1, -1)
            a1 = np.ascontiguousarray(np.asarray(s1))
            row["cpu_port_ms"], row["cpu_port_threads"] = cpu_best(lambda: [oracle.bps(a1[m], ang, s1.coded_symbols.astype(dt), 11, fast=True) for m in range(2)])
        rows.append(row)
    # ---- test_apply_filter_benchmark: 2^17 symbols, 2 modes, 40 taps
    for dt in (np.complex64, np.complex128):
        sig = synth.make_capture(4, 2 ** 17, nmodes=2, os=2, snr_db=14, linewidth=0., fb=40e9, seed=9, dtype=dt)
        wxy, _ = api_eq.equalise_signal(sig, 4e-4, Ntaps=40, method="mcma")
        row = dict(bench="apply_filter", dtype=np.dtype(dt).name, nsym=2 ** 17, ntaps=40)
        row["hip_ms"], _ = best(lambda: api_eq.apply_filter(sig, wxy))
        if cpu:
            E = np.ascontiguousarray(np.asarray(sig))
            row["cpu_port_ms"], row["cpu_port_threads"] = cpu_best(lambda: oracle.apply_filter_to_signal(E, 2, wxy, fast=True))
        rows.append(row)
    # ---- test_quantize_precision: make_decision on 2^20 symbols of 128-QAM; test_select_angles_benchmark: 2^17 indices into a 64-angle grid
    for dt in (np.complex64, np.complex128):
        al = np.ascontiguousarray(theory.coded_symbols_qam(128, dtype=dt))
        x = np.ascontiguousarray(al[np.random.default_rng(3).integers(0, 128, 2 ** 20)])
        row = dict(bench="make_decision", dtype=np.dtype(dt).name, nsym=2 ** 20, M=128)
        row["hip_ms"], _ = best(lambda: hk.make_decision(x, al))
        if cpu:
            row["cpu_port_ms"], row["cpu_port_threads"] = cpu_best(lambda: oracle.make_decision(x, al, fast=True))
        rows.append(row)
        rt = np.float32 if dt is np.complex64 else np.float64
        ang = np.linspace(-np.pi / 4, np.pi / 4, 64, endpoint=False, dtype=rt).reshape(1, -1)
        idx = np.random.default_rng(4).integers(0, 64, 2 ** 17).astype(np.int32)
        row = dict(bench="select_angles", dtype=np.dtype(rt).name, n=2 ** 17, test_angles=64)
        row["hip_ms"], _ = best(lambda: hip_dsp.select_angles(ang, idx))
        if cpu:
            row["cpu_port_ms"], row["cpu_port_threads"] = cpu_best(lambda: oracle.select_angles(ang, idx))
        rows.append(row)
    return dict(rows=rows, note="the reference's pytest-benchmark shapes (test/test_benchmarks.py) through the mirrored call surface, host arrays in and out (PCIe, allocation "
                                "and launch latency included: at 10^5 symbols the exact recurrence IS the call - 2 chains of 10^5 dependent steps - and tier b has too few "
                                "segments to fill the chip); cpu_port_ms = the oracle's reference-flag build on the same arrays at the best of {all, 16, 1} OpenMP threads (cpu_port_threads)")


def capture_pool_block(cfg, nsym, tol, barrier_sync, ncap=8, rounds=3):
    """Informational: K consecutive captures that are DIFFERENT captures - a pool of `ncap` resident captures (seeds 1000 .. 1000 + ncap - 1: the captures the
    ranks of an `ncap`-GPU run get) rotated through one running receiver (overlap + prefetch through its second input buffer, no copies).  The headline
    feeds the same resident capture K times; the number of passes a capture needs depends on the capture (profiles/r05_seed_sweep.txt), so this is the
    receiver's AVERAGE throughput over captures, and the spread is what an N-GPU line with one fixed capture per rank shows as inefficiency."""
    from qampy_amd import synth, _lib
    caps = [synth.make_capture_dev(cfg["M"], nsym, nmodes=2, os=2, snr_db=cfg["snr_db"], theta=np.pi / 5.6, dgd=30e-12, linewidth=cfg["linewidth"], fb=20e9, beta=0.1, seed=1000 + j)
            for j in range(ncap)]
    class _S:                                       # (make_receiver only reads shape and alphabet)
        shape = (2, 2 * nsym); coded_symbols = caps[0]["alphabet_host"]
    rx = make_receiver(cfg, _S, tier="b", pit=dict(tol=tol))
    rx.load(caps[0]["E"].to_host())                 # (derives the acquisition chunk on the host)
    pool = [c["E"] for c in caps]
    rx.E = pool[0]

    def feed(k):
        rx.E_next = pool[(k + 1) % ncap]
        rx._next_loaded = True
    per_cap = []
    for k in range(ncap):                           # warm-up round: every capture once, its report read
        feed(k)
        rx.run(overlap=True, prefetch=True)
        rx.wait_post()
        per_cap.append([(r["passes"], bool(r["converged"]), bool(r["exact_form"])) for r in rx.pit_reports()])
    barrier_sync()
    t0 = time.perf_counter()
    for k in range(rounds * ncap):
        feed(k)
        rx.run(overlap=True, prefetch=True)
    rx.wait_post()
    barrier_sync()
    el = time.perf_counter() - t0
    n = rounds * ncap
    return dict(captures=ncap, steps=n, value=round(nsym * n / el / 1e6, 3), unit="MSym/s", ms_per_step=round(el / n * 1e3, 3), tol=tol,
                passes_per_capture=[[p for p, _, _ in row] for row in per_cap], all_certified_by_the_device=bool(all(c and not x for row in per_cap for _, c, x in row)),
                note="informational: consecutive captures that differ (seeds 1000 .. %d, the captures of an %d-GPU run), rotated through one receiver" % (1000 + ncap - 1, ncap))


def survey_recipe_block(barrier_sync, tol):
    """SURVEY.md 8d's LITERAL C3 recipe - mu = (1e-3, 5e-4), linewidth 5 kHz - and what is closest to it that the reference's own recurrence converges on
    at 2^22 symbols.  Measured with the exact path (profiles/r05_survey_recipe_exact_path.txt: three seeds x linewidths 0 / 1 / 5 kHz x 2^16 .. 2^22): at
    these step sizes the cma -> mrde chain converges on every capture of <= 2^18 symbols and FAILS on at least one mode of every 2^22-symbol capture, at
    every linewidth including 0 (the constant-modulus stage's misadjustment at mu = 1e-3 lets a mode slip within 4 million steps); at half the step sizes
    it converges at 0 and 1 kHz.  Rows: the literal recipe at 2^18 (converges) and at 2^22 (the exact path's symbol errors; tier b then returns the exact
    form for the stage whose trajectory is not a contraction), and (5e-4, 2.5e-4) at 1 kHz and 2^22."""
    rows = []
    for name, mu, lw, lg in (("literal, 2^18", (1e-3, 5e-4), 5e3, 18), ("literal, 2^22", (1e-3, 5e-4), 5e3, 22), ("half steps, 1 kHz, 2^22", (5e-4, 2.5e-4), 1e3, 22)):
        cfg = dict(WORKLOADS["c3"], mu=mu, linewidth=lw, nsym=2 ** lg, label="64-QAM 2-pol 2 SPS 2^%d sym, 41-tap CMA->MRDE mu %s, %g Hz" % (lg, mu, lw))
        sig = make_input(cfg, cfg["nsym"], 1000)
        tb, ta, ex = run_pair(cfg, sig, cfg["nsym"], 3, 1, barrier_sync, dict(tol=tol), 1, tol, overlap=False)
        rows.append(dict(recipe=name, mu=list(mu), linewidth_hz=lw, nsym=cfg["nsym"], errors_exact=ta["errors"], errors_tier_b=tb["errors"],
                         exact_path_converges=bool(max(ta["errors"]) < 0.01 * cfg["nsym"]), tier_b_ms=tb["ms_per_step"], tier_b_MSym_s=tb["value"],
                         exact_ms=ta["ms_per_step"], certified=tb["certified"], checks=tb.get("checks"),
                         stages=[dict(stage=st["stage"], S=st["S"], seg_len=st["seg_len"], P=st["P"], exact_form=st.get("exact_form", False),
                                      est_deviation_rms=st["est_deviation_rms"][-1:]) for st in tb["stages"]],
                         eq_rms_dev_vs_exact=tb.get("eq_rms_dev_vs_exact"), tap_rel_dev_vs_exact=tb.get("tap_rel_dev_vs_exact")))
        del ex, sig
    return dict(tol=tol, rows=rows, note="one capture at a time (no overlap), 3 timed passes each; see the docstring of bench.survey_recipe_block and DESIGN.md 6")


def in_flight_block(cfg, sig, nsym, n, steps, barrier_sync, pit):
    """Informational: `n` captures on the GPU at a time (pipeline.ReceiverGroup, one host thread + library stream set per receiver), `steps` passes in
    total, no events inside the timed region; every receiver certified by the device and bit-identical to receiver 0."""
    g = make_group(n, cfg, sig, pit)
    try:
        g.load(sig)
        g.run(2 * n, prefetch=True)
        barrier_sync()
        t0 = time.perf_counter()
        g.run(steps, prefetch=True)
        barrier_sync()
        el = time.perf_counter() - t0
        res = [r.fetch() for r in g.rx]
        same = all(np.array_equal(o[k], res[0][k]) for o in res[1:] for k in ("wxy", "eq", "out"))
        reps = g.pit_reports()
        return dict(receivers=n, value=round(nsym * steps / el / 1e6, 4), unit="MSym/s", ms_per_step=round(el / steps * 1e3, 3), steps=steps,
                    all_receivers_identical=bool(same), all_receivers_converged=bool(all(r["converged"] for rp in reps for r in rp)),
                    passes=[[r["passes"] for r in rp] for rp in reps],
                    note="informational, never the headline: %d receivers side by side, each the overlapped single receiver of the headline; what one capture leaves "
                         "idle (control path between the relaxation passes, acquisition, eigen-solver) the other uses" % n)
    finally:
        g.close()


def cert_snr_block(cfg, snr_db, nsym, seed, barrier_sync, pit, overlap=False):
    """Certification capture WITH symbol errors (the default capture makes none on either path, so its error count cannot fail):
    same shape at a lower SNR; tier b's error counts against the exact path's, per mode, within 3 standard deviations of the count."""
    c2 = dict(cfg, snr_db=snr_db)
    sig = make_input(c2, nsym, seed)
    tb, ta, ex = run_pair(c2, sig, nsym, 2, 1, barrier_sync, pit, 1, pit.get("tol", TOL_DEFAULT) if pit else TOL_DEFAULT, overlap=overlap)
    ea, eb = ta["errors"], tb["errors"]
    sig3 = [3.0 * float(np.sqrt(max(a, 1))) for a in ea]
    ok = all(abs(a - b) <= s3 for a, b, s3 in zip(ea, eb, sig3)) and min(ea) > 100
    del ex
    return dict(snr_db=snr_db, nsym=nsym, seed=seed, errors_exact=ea, errors_tier_b=eb, allowed_difference_3sigma=[round(x, 1) for x in sig3],
                exact_path_has_errors=bool(min(ea) > 100), within_3sigma=bool(ok), converged=tb["converged"], passes=[st["P"] for st in tb["stages"]],
                out_rms_dev_vs_exact=tb["out_rms_dev_vs_exact"], tap_rel_dev_vs_exact=tb["tap_rel_dev_vs_exact"],
                tier_b_MSym_s=tb["value"], tier_a_MSym_s=ta["value"])


def adaptive_block(log2n=20, seed=1000):
    """Informational: the reference script's adaptive-step recipe (Scripts/64_qam_equalisation.py:26-32: 64-QAM, 25 dB, 13 taps, mu = 1.9e-3,
    mcma -> mddma, adaptive_stepsize=(True, True), the shared step size carried from mode to mode) through tier b against the exact path,
    stage by stage on one capture (each stage from the exact taps of the one before; kernels only, arrays resident; second call timed)."""
    from qampy_amd import synth, _lib
    from qampy_amd.core.equalisation import equalisation as eq, hip_equalisation as hk
    from qampy_amd._lib import DeviceArray
    nsym, ntaps, mu0 = 1 << log2n, 13, 1.9e-3
    sig = synth.make_capture(64, nsym, nmodes=2, snr_db=25, theta=np.pi / 3, dgd=30e-12, linewidth=0., seed=seed, dtype=np.complex64)
    E = np.ascontiguousarray(np.asarray(sig))
    tr = eq._cal_training_symbol_len(2, ntaps, E.shape[1])
    dE = DeviceArray.from_host(E)
    w0 = eq._init_taps(ntaps, 2, 2, np.complex64)
    stages = []
    for method in ("mcma", "mddma"):
        sy = eq._reshape_symbols(sig.coded_symbols if method == "mddma" else None, method, 64, np.complex64, 2)
        dsy = DeviceArray.from_host(np.ascontiguousarray(sy))
        res = {}
        for tier in ("a", "b"):
            dw, derr, dmu = DeviceArray.from_host(w0.copy()), DeviceArray((2, tr), np.complex64), DeviceArray.from_host(np.array([mu0], np.float32))
            rep = hk.PitReportBuffer() if tier == "b" else None
            kw = dict(pit={}, report=rep) if tier == "b" else {}
            for _ in range(2):
                dw.set(w0.copy()); dmu.set(np.array([mu0], np.float32)); _lib.sync()
                t0 = time.perf_counter()
                hk.train_equaliser_dev(dE, tr, 1, 2, dmu, dw, None, True, dsy, method, derr, zero_err=True, **kw)
                _lib.sync(); dt = time.perf_counter() - t0
            res[tier] = dict(w=dw.to_host(), err=derr.to_host(), mu=float(dmu.to_host()[0]), ms=dt * 1e3, rep=rep.read() if rep is not None else None)
        a, b = res["a"], res["b"]
        r = b["rep"]
        stages.append(dict(stage=method, ms_exact=round(a["ms"], 2), ms_tier_b=round(b["ms"], 2), speedup=round(a["ms"] / b["ms"], 2),
                           tap_rel_dev_vs_exact=[float(np.linalg.norm(a["w"][m] - b["w"][m]) / np.linalg.norm(a["w"][m])) for m in range(2)],
                           err_trace_rms_dev_vs_exact=[float(np.sqrt(np.mean(np.abs(a["err"][m] - b["err"][m]) ** 2))) for m in range(2)],
                           final_mu_rel_dev=abs(a["mu"] - b["mu"]) / a["mu"], final_mu_exact=a["mu"],
                           last_mode=dict(segments=r["segments"], seg_len=r["seg_len"], passes=r["passes"], converged=r["converged"], exact_form=r.get("exact_form", False),
                                          est_deviation_rms=[float("%.3g" % d) for d in r["deviation_rms"]])))
        w0 = a["w"]
    return dict(workload="64-QAM 2-pol 2 SPS 2^%d sym, 13-tap MCMA -> MDDMA, adaptive step (the reference script's recipe)" % log2n, nsym=nsym, stages=stages,
                note="tier b with adapt_step: modes solved in turn (shared step size), exact head of 16384 steps, r = 1/mu and the previous error as boundary "
                     "states, corrections damped (0.7), tolerance / 3; a sweep that is not certified within 24 passes is redone in the exact form inside the call "
                     "(exact_form = true for the last mode, deviations exactly 0 for such a mode)")


def shape_block(key, barrier_sync, pit, steps, overlap=False):
    """Another BASELINE shape in the same line (ns: the north star's 10^7 symbols; c2: configs[1]): tier b, the exact path, SER, certificate."""
    cfg = dict(WORKLOADS[key])
    nsym = cfg["nsym"]
    sig = make_input(cfg, nsym, 1000)
    tb, ta, ex = run_pair(cfg, sig, nsym, steps, 1, barrier_sync, pit, 1, pit.get("tol", TOL_DEFAULT) if pit else TOL_DEFAULT, overlap=overlap)
    del ex
    return dict(workload=cfg["label"], nsym=nsym, tier_b=dict(value=tb["value"], ms_per_step=tb["ms_per_step"], one_capture_at_a_time=(tb.get("pipelining") or {}).get("one_capture_at_a_time"),
                                                               certified=tb["certified"], checks=tb.get("checks"), info=tb.get("info"),
                                                               stages=[dict(stage=st["stage"], S=st["S"], seg_len=st["seg_len"], P=st["P"], converged=st["converged"], exact_form=st.get("exact_form", False),
                                                                            est_deviation_rms=st["est_deviation_rms"][-1:] , pass_ms=st["pass_ms"]) for st in tb["stages"]],
                                                               out_rms_dev_vs_exact=tb["out_rms_dev_vs_exact"], tap_rel_dev_vs_exact=tb["tap_rel_dev_vs_exact"],
                                                               eq_rms_dev_vs_exact=tb.get("eq_rms_dev_vs_exact"), out_rms_dev_same_angle=tb.get("out_rms_dev_same_angle"),
                                                               bps_angle_mismatch_fraction=tb.get("bps_angle_mismatch_fraction"),
                                                               err_trace_rms_dev_vs_exact=tb["err_trace_rms_dev_vs_exact"], errors=tb["errors"], stages_ms=tb["stages_ms"],
                                                               elementwise=tb.get("elementwise"), elementwise_summary=tb.get("elementwise_summary")),
                tier_a=dict(value=ta["value"], ms_per_step=ta["ms_per_step"], errors=ta["errors"]), speedup_vs_exact=tb["speedup_vs_exact"])


def pmc_json(name, workload):
    """profiles/<name>_<workload>.json from the PMC passes of the same workload (scripts/gpu_pmc*.sh), only while the kernel sources
    are the ones that were profiled."""
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", "%s_%s.json" % (name, workload))))
        return pmc if pmc.get("kernel_sources_sha") == kernel_sources_sha() else None
    except (OSError, ValueError):
        return None


TOL_DEFAULT = 1e-3         # library default of tier b: estimated relative rms deviation of the equaliser output from the sequential recurrence
TOL_TIGHT = 1e-4           # SURVEY.md 8c's complex64 bar (rtol 1e-4 taps, atol 1e-4 output / error): what the headline is held to since round 5


# ------------------------------------------------------------------------------------------------------------ main
# ---------------------------------------------------------------------------------------------------------------------------------------------
# The line the driver parses.  Everything informational (other shapes, tolerances, recipes, per-pass arrays, prose) goes to --detail-out and is
# NOT on stdout: round 5's 30 KB line could not be parsed by the driver.  `headline_line` is a whitelist, every string is
# cut to LINE_STR_MAX characters and the result is checked against LINE_MAX_BYTES before it is printed.
LINE_MAX_BYTES = 6000
LINE_STR_MAX = 160


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def _short(v, nd=6):
    """Floats to `nd` significant digits, strings cut, containers walked."""
    if isinstance(v, bool) or v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        return float("%.*g" % (nd, v))
    if isinstance(v, str):
        return v if len(v) <= LINE_STR_MAX else v[:LINE_STR_MAX - 3] + "..."
    if isinstance(v, dict):
        return {k: _short(x, nd) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_short(x, nd) for x in v]
    return _short(float(v), nd) if hasattr(v, "__float__") else str(v)


def headline_line(out, detail_path=None):
    """The ONE JSON line of the bench contract, from the full result `out` (which is written to `detail_path`)."""
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling"))
    line["vs_baseline"] = out.get("vs_baseline")
    line.update(_pick(out, ("dtype", "data", "dry_run", "headline_tier", "note", "error", "comm_backend", "comm_degraded", "ms_per_step_per_rank", "device")))
    cfg = out.get("config") or {}
    c = _pick(cfg, ("workload", "key", "nsym_per_channel", "channels", "ntaps", "methods", "niter", "mu", "test_angles", "bps_N", "complex_dtype", "tol",
                    "train_mode", "parallelism"))
    line["config"] = c
    if out.get("stages_ms"):
        line["stages_ms"] = out["stages_ms"]
    r = out.get("roofline")
    if r:
        rl = {k: r.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic")}
        rl.update(_pick(r, ("algorithmic_bytes", "algorithmic_flops", "launch_ms", "launches_per_step", "issue_frac", "traffic_vs_fused", "useful_flops_frac",
                            "chains", "lanes_per_chain", "steps_per_chain", "traffic_note")))
        if isinstance(r.get("hbm"), dict):
            rl["hbm"] = _pick(r["hbm"], ("achieved", "peak", "unit", "frac"))
        if isinstance(r.get("step"), dict):
            rl["passes"] = r["step"].get("passes")
        line["roofline"] = rl
    cb = out.get("cpu_baseline")
    if cb:
        c2 = _pick(cb, ("value", "unit", "cores", "kind", "sample", "cpu_model"))
        if isinstance(cb.get("one_thread"), dict):
            c2["one_thread"] = _pick(cb["one_thread"], ("value", "sample"))
        line["cpu_baseline"] = c2
    line.update(_pick(out, ("speedup_vs_cpu", "speedup_vs_cpu_tier")))
    tb = out.get("tier_b")
    if tb:
        t = _pick(tb, ("value", "ms_per_step", "certified", "converged", "errors", "speedup_vs_cpu"))
        if tb.get("stages"):
            t["passes"] = [st.get("P") for st in tb["stages"]]
        for k in ("elementwise_summary", "checks"):
            if tb.get(k):
                t[k] = tb[k]
        line["tier_b"] = t
    if out.get("tier_a"):
        line["tier_a"] = _pick(out["tier_a"], ("value", "ms_per_step", "steps", "errors", "speedup_vs_cpu"))
    if out.get("one_capture_at_a_time"):
        line["one_capture_at_a_time"] = _pick(out["one_capture_at_a_time"], ("value", "ms_per_step"))
    tt = out.get("tier_b_tight")
    if tt:
        line["tier_b_tight"] = dict(tol=tt.get("tol"), certified=tt.get("certified"),
                                    **{k: dict(_pick(tt[k], ("value", "certified", "passes")),
                                               **({"taps_eq_all_elements_within_1e-4": bool(tt[k]["elementwise_summary"]["taps_share_within"] == 1.0
                                                                                            and tt[k]["elementwise_summary"]["equaliser_out_share_within"] == 1.0)}
                                                  if isinstance(tt[k].get("elementwise_summary"), dict) else {}))
                                       for k in ("c3", "ns", "c2") if isinstance(tt.get(k), dict)})
    if out.get("parity_vs_cpu"):
        line["parity_vs_cpu"] = _pick(out["parity_vs_cpu"], ("sample", "errors_gpu", "errors_cpu", "errors_gpu_exact", "ser_gpu", "ser_cpu", "max_abs_tap_diff"))
    if out.get("ser"):
        line["ser"] = out["ser"]
    if out.get("api_end_to_end"):
        line["api_end_to_end"] = _pick(out["api_end_to_end"], ("value", "unit", "ms_per_capture"))
    for k in ("extra_shapes_error",):
        if out.get(k):
            line[k] = out[k]
    if detail_path:
        line["detail"] = detail_path
    line = _short(line)
    txt = json.dumps(line, separators=(",", ":"))
    if len(txt) > LINE_MAX_BYTES:                    # never print a line the driver cannot hold: drop the optional blocks, largest first
        for k in ("stages_ms", "tier_a", "one_capture_at_a_time", "api_end_to_end", "parity_vs_cpu", "tier_b_tight", "tier_b", "ser"):
            line.pop(k, None)
            txt = json.dumps(line, separators=(",", ":"))
            if len(txt) <= LINE_MAX_BYTES:
                break
    return txt


def emit(out, detail_path):
    """Write the full result to `detail_path` (and nothing of it to stdout), print the headline line."""
    written = None
    if detail_path:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(detail_path)), exist_ok=True)
            with open(detail_path, "w") as f:
                json.dump(out, f, indent=1, default=lambda o: float(o) if hasattr(o, "__float__") else str(o))
            written = detail_path
        except OSError as e:
            sys.stderr.write("bench.py: detail file %s not written (%s)\n" % (detail_path, e))
    print(headline_line(out, written))
    sys.stdout.flush()


# ------------------------------------------------------------------------------------------------------------ output dump
DUMP_MAX_BYTES = 64 << 20          # --dump-outputs: all files together
DUMP_SAMPLE = 1 << 18              # positions kept along the last axis of a longer array (halved until the files fit)
DUMP_SEED = 1000                   # the sample of an axis of length n: np.random.default_rng([DUMP_SEED, n]) - the same in every run and build


def _real_view(a):
    """float32 / float64 copy of an output array: complex -> trailing axis (real, imaginary); integers -> float64 (exact)."""
    if np.iscomplexobj(a):
        return np.stack([a.real, a.imag], axis=-1).astype(np.float64 if a.dtype == np.complex128 else np.float32)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def dump_files(res):
    """The arrays a caller of the timed path receives (a dict as ResidentReceiver.fetch() returns it; tuples of per-stage arrays become
    <name>1, <name>2, ..., tuples of scalars one array) as {file name: float array} within DUMP_MAX_BYTES: an array longer than the sample along
    its last axis is kept at a fixed, seeded, sorted sample of positions, stored beside it as <name>_sample_index."""
    arrays = {}
    for k, v in res.items():
        if isinstance(v, (tuple, list)) and not all(np.ndim(x) == 0 for x in v):
            arrays.update(("%s%d" % (k, i + 1), np.asarray(x)) for i, x in enumerate(v))
        else:
            arrays[k] = np.asarray(v)
    sample = DUMP_SAMPLE
    while sample >= 1024:
        files = {}
        for name, a in sorted(arrays.items()):
            if a.ndim and a.shape[-1] > sample:
                pos = np.sort(np.random.default_rng([DUMP_SEED, a.shape[-1]]).choice(a.shape[-1], sample, replace=False))
                files[name] = _real_view(a[..., pos])
                files[name + "_sample_index"] = pos.astype(np.float64)
            else:
                files[name] = _real_view(a)
        if sum(f.nbytes for f in files.values()) <= DUMP_MAX_BYTES:
            return files
        sample //= 2
    raise ValueError("outputs do not fit into %d bytes" % DUMP_MAX_BYTES)


def write_dump(files, path):
    os.makedirs(path, exist_ok=True)
    for name, a in files.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--nsym", type=int, default=None, help="override the number of symbol periods per capture")
    ap.add_argument("--tier", default="b", choices=["a", "b"],
                    help="trainer of the timed pipeline: b = parallel-in-time solver of the recurrence held to --tol (headline only if it certifies "
                         "itself in this run, device estimate AND measurement against the exact path); a = the exact sequential recurrence")
    ap.add_argument("--tol", type=float, default=0., help="tier b: accepted relative rms deviation of the equaliser output from the sequential recurrence (0 = library default 1e-3)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU legs")
    ap.add_argument("--cpu-sample", type=int, default=None, help="--full: symbol periods the all-thread CPU baseline processes (default: the whole capture)")
    ap.add_argument("--cpu-sample-1t", type=int, default=None, help="--full: symbol periods of the one-thread CPU run (default: the whole capture)")
    ap.add_argument("--exact-steps", type=int, default=2, help="timed passes of the exact path beside tier b (N = 1)")
    ap.add_argument("--host-synth", action="store_true", help="generate the capture with the host (numpy) generator instead of on the GPU")
    ap.add_argument("--bank-trainer", default="iterative", choices=["auto", "iterative"])
    ap.add_argument("--bank", type=int, default=128, help="--full: channels of the informational channel-bank run at N=1 (0 = skip)")
    ap.add_argument("--cpu-bank-workers", type=int, default=-1, help="--full: concurrent single-threaded CPU pipelines of the bank's CPU leg (-1: min(cores, 128), 0: skip)")
    ap.add_argument("--pool", type=int, default=8, help="tier b, consecutive captures: resident captures rotated through the receiver (seeds 1000 + ((rank + j) mod pool)); 1 = the same "
                                                       "capture every step (rounds 1-4)")
    ap.add_argument("--in-flight", type=int, default=1, help="tier b: captures on the GPU at a time (pipeline.ReceiverGroup, one host thread per receiver); 1 = one receiver")
    ap.add_argument("--no-overlap", action="store_true", help="tier b: time one capture at a time only (default: consecutive captures, the phase search of "
                                                              "pass k on stream 2 beside the training of pass k + 1)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: timing runs of their own for the roofline and the one-capture / one-receiver "
                         "figures, the other shapes and tolerances, the reference's benchmark definitions, the CPU baselines and the channel bank.  Without it a run "
                         "sets up, warms up, times the K steps, certifies tier b against the exact path and prints the line")
    ap.add_argument("--no-extra-shapes", action="store_true", help="--full: skip the ns / c2 / 24 dB / loose-tolerance blocks")
    ap.add_argument("--split-capture", action="store_true",
                    help="N > 1: ONE capture, the segments of the tier-b trainer spread over the ranks with an all-reduce of their end taps per pass "
                         "(qampy_amd.distributed; strong scaling, informational - the default is one independent capture per GPU)")
    ap.add_argument("--c5-frames", type=int, default=9, help="workload c5: frames in the synthetic capture (the first and the last are cut by the frame offset)")
    ap.add_argument("--require-rccl", action="store_true",
                    help="N > 1 with one GPU per rank: refuse to run (exit 3) when the process group could not be built on RCCL.  Default since round 5: go on with the socket "
                         "backend - the data path has no collective (one independent capture per rank; the group only carries barriers, the max of the elapsed time and error "
                         "counters) - and flag it: comm_backend = 'tcp', comm_degraded = true, the reason in config.comm_note")
    ap.add_argument("--allow-tcp", action="store_true", help="(kept for older command lines: the default since round 5, see --require-rccl)")
    ap.add_argument("--detail-out", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="file the FULL result goes to (other shapes and tolerances, recipes, per-pass arrays, notes); stdout carries the compact headline line only; '' = no file")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: kernels replaced by a sleep, socket collectives - exercises launcher + reductions")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps: what the headline path returned for its LAST timed step (rank 0), as DIR/<name>.npy in float32 / float64 "
                         "(complex: trailing axis real, imaginary; long arrays at a fixed seeded sample of positions, <name>_sample_index.npy), <= 64 MB in all")
    args = ap.parse_args()
    if args.dump_outputs and args.dry_run:
        ap.error("--dump-outputs: a dry run computes nothing")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    from qampy_amd import sharding
    from qampy_amd.comm import Comm
    rank, local_rank, world = sharding.rank_info()
    if world != args.gpus:
        if rank == 0:
            print(json.dumps(dict(error="launched with WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))))
        sys.exit(2)
    cfg = dict(WORKLOADS[args.workload])
    nsym = args.nsym or cfg["nsym"]
    if args.workload == "c5":
        if world > 1 or args.dry_run:
            print(json.dumps(dict(error="workload c5 runs on one GPU")))
            sys.exit(2)
        return run_c5(args, cfg)

    # ---- process group: RCCL through ctypes (one rank per GPU); sockets where there is no GPU or RCCL cannot start
    if args.dry_run:
        dev, _lib = None, None
    else:
        from qampy_amd import _lib
        ndev = max(_lib.device_count(), 1)
        dev = local_rank % ndev                      # a launcher may expose a single device per rank
        _lib.init(dev)
    backend = "tcp" if args.dry_run else os.environ.get("QAMPY_BENCH_BACKEND", "auto")
    cm = Comm(device=dev, backend=backend)
    ranks_seen = int(round(sharding.reduce_sum_counts([[1.0]], cm)[0, 0]))
    comm_degraded = bool(world > 1 and not args.dry_run and cm.backend != "rccl" and ndev >= world)
    if comm_degraded and args.require_rccl:
        # every rank has its own GPU and the group is still not RCCL: refuse (all ranks agreed on the backend, so all of them leave here)
        if rank == 0:
            print(json.dumps(dict(error="N = %d ranks on %d visible GPUs but the process group is '%s', not RCCL (%s); without --require-rccl the run goes on with host-side collectives and says so"
                                        % (world, ndev, cm.backend, cm.note or "no reason recorded"), n_gpus=world, ranks_seen=ranks_seen, comm_backend=cm.backend)))
        cm.close()
        sys.stdout.flush()
        if getattr(cm, "stuck", False):
            os._exit(3)
        sys.exit(3)

    def barrier_sync():
        if not args.dry_run:
            _lib.sync()
        cm.barrier()

    # Headline tolerance: the TIGHTEST of (1e-4, 1e-3) at which tier b certifies itself in this run (--tol fixes one).  1e-4 is SURVEY.md 8c's
    # bar for complex64 (the exact path is held to it against the golden vectors); 1e-3 was the headline tolerance of rounds 2-4.
    tol_ladder = [args.tol] if args.tol > 0 else [TOL_TIGHT, TOL_DEFAULT]
    pit = dict(tol=tol_ladder[0])
    overlap = args.tier == "b" and not args.no_overlap and not args.dry_run
    tol_check = tol_ladder[0]
    if args.dry_run:
        rx = DryReceiver(cfg, nsym, args.tier)
        for _ in range(args.warmup):
            rx.run()
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            rx.run()
        barrier_sync()
        own = time.perf_counter() - t0
        per_rank = np.zeros((1, world)); per_rank[0, rank] = own / args.steps * 1e3
        per_rank_ms = [round(float(x), 3) for x in sharding.reduce_sum_counts(per_rank, cm)[0]]
        elapsed = sharding.reduce_max_time(own, cm)
        counts_all = sharding.reduce_sum_counts([[d["errors"], d["compared"]] for d in rx.ser()], cm)
        if rank == 0:
            emit(dict(metric="equalised MSym/s (2-pol, 2 SPS)", value=round(sharding.aggregate_throughput(nsym, world, args.steps, elapsed), 4),
                      unit="MSym/s", n_gpus=world, ranks_seen=ranks_seen, steps=args.steps, warmup=args.warmup,
                      ms_per_step=round(elapsed / args.steps * 1e3, 3), higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f32",
                      data="synthetic", dry_run=True, comm_backend=cm.backend, ms_per_step_per_rank=per_rank_ms,
                      config=dict(workload=cfg["label"], key=args.workload, nsym_per_channel=nsym, channels=world, ntaps=cfg["ntaps"], methods=list(cfg["methods"]),
                                  mu=list(cfg["mu"]), test_angles=cfg["A"], parallelism="1 independent channel per GPU, no collective on the data path"),
                      ser=dict(errors_all=int(counts_all[:, 0].sum()), symbols_all=int(counts_all[:, 1].sum()))), args.detail_out)
        cm.close()
        return

    # ---- independent channel per rank (seed 1000 + channel), synthesised on the GPU (or the host), then made resident
    split = args.split_capture and world > 1 and args.tier == "b"
    dumped = {}                                      # --dump-outputs: the last timed pass's results, reduced to the files at once (dump_files)
    keep_last = (lambda r: dumped.update(files=dump_files(r.fetch()))) if (args.dump_outputs and rank == 0) else None
    sig = make_input(cfg, nsym, sharding.channel_seed(0 if split else rank), host=args.host_synth)
    tier_a = tier_b = None
    if split:                                        # every rank holds the same capture
        from qampy_amd.distributed import SplitCaptureReceiver
        rx = SplitCaptureReceiver(sig.shape[0], sig.shape[1], 2, cfg["M"], cfg["ntaps"], cfg["mu"], methods=cfg["methods"], Niter=cfg["niter"],
                                  adaptive_stepsize=cfg["adaptive"], TrSyms=(None,) * len(cfg["methods"]), Mtestangles=cfg["A"], Nbps=cfg["Nbps"],
                                  dtype=np.complex64, alphabet=sig.coded_symbols, pit=pit, comm=cm)
        rx.load(sig)
        stage_names, _ = stage_list(rx)
        elapsed, stage_ms, pass_ms, acq_ms = timed_steps(rx, args.steps, args.warmup, barrier_sync, after=keep_last)
        reports = rx.pit_reports()
        errs = [(d["errors"], d["compared"]) for d in rx.ser(sig.symbols, maxlag=256, window=8192, trim=2000)]
        tier_b = tier_b_block(cfg, rx, stage_names, pass_ms, acq_ms, reports, nsym * args.steps / elapsed / 1e6, elapsed / args.steps * 1e3, errs, nsym)
        tier_b["certified"] = tier_b["converged"]
    elif args.tier == "b":
        tried = []
        for t_ in tol_ladder:
            pit, tol_check = dict(tol=t_), t_
            tier_b, tier_a, ex = run_pair(cfg, sig, nsym, args.steps, args.warmup, barrier_sync, pit, args.exact_steps if world == 1 else 0, tol_check, overlap=overlap, in_flight=args.in_flight,
                                          pool_n=max(1, args.pool), first_seed=sharding.channel_seed(rank), after=keep_last, full=args.full)
            if tier_b["certified"] or world > 1:         # (N > 1: every rank must take the same rung - the tightest; its certificate is all-reduced below)
                break
            tried.append(dict(tol=t_, certified=False, checks=tier_b.get("checks"), passes=[st["P"] for st in tier_b["stages"]], value=tier_b["value"],
                              out_rms_dev_vs_exact=tier_b.get("out_rms_dev_vs_exact"), tap_rel_dev_vs_exact=tier_b.get("tap_rel_dev_vs_exact")))
            del ex
        rx, stage_names, stage_ms, elapsed, errs, reports = ex["rx"], ex["names"], ex["stage_ms"], ex["elapsed"], ex["errs"], ex["reports"]
        if tried:
            tier_b["tighter_tolerances_not_certified"] = tried
    else:
        rx = make_receiver(cfg, sig, tier="a")
        rx.load(sig)
        stage_names, _ = stage_list(rx)
        elapsed, stage_ms, _, _ = timed_steps(rx, args.steps, args.warmup, barrier_sync, after=keep_last)
        reports = None
        errs = [(d["errors"], d["compared"]) for d in rx.ser(sig.symbols, maxlag=256, window=8192, trim=2000)] if cfg["A"] else []
        tier_a = dict(method="exact sequential recurrence (reference order of evaluation)", value=round(nsym * args.steps / elapsed / 1e6, 4), unit="MSym/s",
                      steps=args.steps, ms_per_step=round(elapsed / args.steps * 1e3, 3), stages_ms={n: round(t, 3) for n, t in zip(stage_names, stage_ms)},
                      errors=[e for e, _ in errs])
    per_rank = np.zeros((1, world)); per_rank[0, rank] = elapsed / args.steps * 1e3
    per_rank_ms = [round(float(x), 3) for x in sharding.reduce_sum_counts(per_rank, cm)[0]]          # every rank's own ms per step
    elapsed = sharding.reduce_max_time(elapsed, cm)
    certified_local = 1.0 if (args.tier == "a" or tier_b["certified"]) else 0.0
    certified_all = int(round(sharding.reduce_sum_counts([[certified_local]], cm)[0, 0])) == world
    counts_all = sharding.reduce_sum_counts([[e, n] for e, n in errs], cm) if errs else np.zeros((1, 2))
    comm_backend, comm_note = cm.backend, cm.note
    if not split:
        cm.close()                                   # the other ranks are done; rank 0 goes on alone (CPU legs, extra shapes)
    if rank != 0:
        if split:
            cm.close()
        if getattr(cm, "stuck", False):
            sys.stdout.flush()
            os._exit(0)
        return

    value_timed = sharding.aggregate_throughput(nsym, 1 if split else world, args.steps, elapsed)
    ms_timed = elapsed / args.steps * 1e3
    nsel = rx.modes.size
    # ---- algorithmic bytes per launch of every stage / kernel (SURVEY.md 8d general formula)
    bps_b = rx.bytes_per_symbol()
    train_bytes = [rx.TrSyms[s] * 8 * (rx.nmodes * 2 + nsel) for s in range(rx.nstage)]          # one sweep = one relaxation pass
    stage_bytes = [rx.TrSyms[0] * (8 * 2 * rx.nmodes + 64 * 16)] + [rx.Niter[s] * train_bytes[s] for s in range(rx.nstage)]
    stage_bytes += [rx.N * bps_b["apply"]] + ([rx.N * bps_b["bps"]] if cfg["A"] else [])

    out = dict(metric="equalised MSym/s (2-pol, 2 SPS)", value=round(value_timed, 4), unit="MSym/s", n_gpus=world, ranks_seen=ranks_seen,
               steps=args.steps, warmup=args.warmup, ms_per_step=round(ms_timed, 3), higher_is_better=True, scaling="strong" if split else "weak", vs_baseline=None,
               dtype="f32", data="synthetic",
               config=dict(workload=cfg["label"], key=args.workload, nsym_per_channel=nsym, channels=1 if split else world, ntaps=cfg["ntaps"],
                           methods=list(cfg["methods"]), niter=list(cfg["niter"]), mu=list(cfg["mu"]), test_angles=cfg["A"], bps_N=cfg["Nbps"],
                           complex_dtype="complex64", train_mode=None, comm_backend=comm_backend,
                           parallelism=("ONE capture: tier-b segments over %d ranks, all-reduce of the segments' end taps per pass (%d exchanges, %.1f MiB per step)"
                                        % (world, rx.exchanges // max(args.steps + args.warmup, 1), rx.exchanged_bytes / max(args.steps + args.warmup, 1) / 2 ** 20))
                           if split else "1 independent channel per GPU, no collective on the data path"),
               stages_ms={n: round(t, 3) for n, t in zip(stage_names, stage_ms)},
               ser=dict(per_mode_rank0=[e / max(n, 1) for e, n in errs], errors_rank0=[e for e, _ in errs], errors_all=int(counts_all[:, 0].sum()),
                        symbols_all=int(counts_all[:, 1].sum())),
               device=_lib.device_name(), comm_backend=comm_backend, comm_degraded=comm_degraded, ms_per_step_per_rank=per_rank_ms)
    if comm_note:
        out["config"]["comm_note"] = comm_note
    if split:
        cm.close()
    if tier_b is not None:
        if world > 1:
            tier_b["certified"] = bool(certified_all)
        out["tier_b"] = tier_b
        if tier_b.get("pipelining"):
            # value / ms_per_step: K consecutive captures through one running receiver (step time = K passes / elapsed); the figure for a single
            # capture handed over and waited for is beside it
            out["config"]["pipelining"] = ("consecutive captures; phase search of capture k (stream 2) and acquisition + eigenbasis of capture k + 2 (stream 1) beside the training of "
                                           "capture k + 1 (stream 0); --no-overlap for one at a time")
            if tier_b.get("capture_pool"):
                out["config"]["capture_pool"] = ("%d different resident captures per GPU (seeds %s), rotated: consecutive captures differ; --pool 1 feeds the same capture every step"
                                                 % (tier_b["capture_pool"]["captures"], tier_b["capture_pool"]["seeds"]))
            if tier_b["pipelining"].get("one_capture_at_a_time"):
                out["one_capture_at_a_time"] = tier_b["pipelining"]["one_capture_at_a_time"]
        if tier_b.get("in_flight"):
            out["config"]["in_flight"] = "%d captures on the GPU at a time (ReceiverGroup: one host thread + stream set per receiver); --in-flight 1 for one receiver" % tier_b["in_flight"]["receivers"]
            if tier_b["in_flight"].get("one_receiver"):
                out["one_receiver"] = tier_b["in_flight"]["one_receiver"]
    if tier_a is not None:
        out["tier_a"] = tier_a

    # ---- headline: tier b only with its certificate; else the exact path
    use_b = args.tier == "b" and tier_b is not None and tier_b["certified"]
    uncertified_b = args.tier == "b" and not use_b and tier_a is None       # N > 1 (no exact run beside it) and a stage that did not converge
    head_ms = stage_ms
    if args.tier == "b" and not use_b and tier_a is not None:
        # the exact path takes the headline: timed on its own with this run's --steps / --warmup (the block beside tier b ran --exact-steps passes)
        rxh = make_receiver(cfg, sig, tier="a")
        rxh.load(sig)
        el_h, ms_h, _, _ = timed_steps(rxh, args.steps, args.warmup, _lib.sync, after=keep_last)
        del rxh
        out["value"] = round(nsym * args.steps / el_h / 1e6, 4)
        out["ms_per_step"] = round(el_h / args.steps * 1e3, 3)
        out["stages_ms"] = {n: round(t, 3) for n, t in zip(stage_names, ms_h)}
        out["note"] = "tier b did not certify itself in this run: headline = exact path"
        head_ms = ms_h
    if uncertified_b:
        out["note"] = "tier b did NOT certify itself on every rank and no exact path ran beside it (N > 1): value is tier b's, uncertified"
    out["headline_tier"] = "b" if (use_b or uncertified_b) else "a"
    if dumped:
        write_dump(dumped.pop("files"), args.dump_outputs)
    out["config"]["tol"] = tol_check if args.tier == "b" else None
    out["config"]["train_mode_detail"] = (
        ("parallel-in-time solver of the reference's recurrence (tier b, tol %g), certified in-run.  Device: estimated rms deviation of the equaliser output from the "
         "sequential recurrence < tol on every stage (a stage that is not certified is redone in the exact form inside the call)" % tol_check
         + ("; measured against the exact path on the same capture, two levels: (1) equaliser output <= tol (relative rms), taps <= 3 tol (relative norm), error traces <= 3 tol (rms) - every symbol; "
            "(2) recovered output (after the phase search) <= tol on the symbols where both searches chose the same test angle; the other symbols (fraction f = %s per mode: "
            "near-ties of the arg-min over the test angles, one angle step apart whatever the tolerance) are reported, not held to tol; symbol-error counts within +-%d"
            % (["%.2g" % v for v in (tier_b.get("bps_angle_mismatch_fraction") or [])], SER_TOL_ERRORS)
            if world == 1 else " on every rank")) if use_b else
        ("parallel-in-time (tier b), NOT certified" if uncertified_b else "exact sequential recurrence (tier a)"))

    out["config"]["train_mode"] = (("parallel-in-time solver of the reference's recurrence (tier b), certified in-run against the exact path at tol %g" % tol_check) if use_b else
                                   ("parallel-in-time (tier b), NOT certified" if uncertified_b else "exact sequential recurrence (tier a)"))

    if args.full:
        # ---- roofline of the dominant kernel (largest total kernel time per step); --full only: the launch times it rests on come from
        # run_pair's timing runs of their own (every pass event-timed, the phase search one capture at a time)
        if use_b or uncertified_b:
            # launch duration of a pass kernel: the average over ALL its launches (every pass event-timed in a run of its own, run_pair), else pass 1's
            def _pms(st_):
                return st_.get("pass_ms_all_launches") or st_["pass_ms"]
            cands = [(_pms(tier_b["stages"][s]) * tier_b["stages"][s]["P"], "train%d:%s relaxation pass" % (s + 1, cfg["methods"][s]),
                      train_bytes[s], _pms(tier_b["stages"][s])) for s in range(rx.nstage)]
            cands.append((stage_ms[0], "gram", stage_bytes[0], stage_ms[0]))
            if cfg["A"]:
                # the phase search enqueued in parts between the next capture's passes (pipeline.py): the stage's event pair then spans most of a step;
                # its kernel time is what the same kernels took one capture at a time
                one = ((tier_b.get("pipelining") or {}).get("one_capture_at_a_time") or {}).get("stages_ms") or {}
                bps_ms = one.get("bps_recover", stage_ms[-1]) if (overlap and int(getattr(rx, "post_parts", 0)) != 1) else stage_ms[-1]
                cands.append((bps_ms, "bps_recover", stage_bytes[-1], bps_ms))
            tot, kname, kbytes, kms = max(cands)
            hbm = dict(achieved=round(kbytes / (kms * 1e-3) / 1e9, 3), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(kbytes / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 6),
                       algorithmic_bytes=int(kbytes))
            roofline = dict(bound="hbm", kernel=kname, achieved=hbm["achieved"], peak=HBM_PEAK_GBS, unit="GB/s", frac=hbm["frac"], traffic=None,
                            algorithmic_bytes=int(kbytes), launch_ms=round(kms, 3), launches_per_step=None, pipeline=tier_b["pipeline_hbm"])
            instr = pmc_json("pmc_instr", args.workload)
            if kname == "bps_recover" and rx.ct == np.complex64 and cfg["A"] <= 64:
                # streaming phase search: lane <-> test angle, VALU instructions per distance row and wave
                NL = max(1, int(round(np.sqrt(cfg["M"]))) // 2)
                per_sym, src = 20.0 + 2 * NL, "ISA count of bps_stream_kernel (20 + 2 levels per axis)"
                hit = [v for k, v in (instr or {}).get("kernels", {}).items() if k.startswith("qh::bps_stream_kernel")]
                C_, W = 1024, 2 * cfg["Nbps"]
                rows = -(-nsym // C_) * (-(-(C_ + W - 1) // 16) * 16) * rx.modes.size          # distance rows incl. the 2N-1 halo of every chunk
                if hit and hit[0].get("SQ_INSTS_VALU"):
                    per_sym, src = float(hit[0]["SQ_INSTS_VALU"]) / rows, "SQ_INSTS_VALU / distance rows (profiles/pmc_instr_%s.json)" % args.workload
                winstr = rows * per_sym
                sflops = nsym * rx.modes.size * cfg["A"] * 25.0                         # slicer search ~ A x 25 flop per symbol and mode
                roofline.update(bound="valu-fp32", achieved=round(sflops / (kms * 1e-3) / 1e12, 3), peak=VALU_PEAK_TFLOPS, unit="TFLOP/s",
                                frac=round(sflops / (kms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 4), algorithmic_flops=int(sflops),
                                issue_frac=round(winstr / (kms * 1e-3) / 1e9 / VALU_PEAK_GINSTR, 4),
                                issue=dict(achieved=round(winstr / (kms * 1e-3) / 1e9, 1), peak=VALU_PEAK_GINSTR, unit="G wave-instr/s"),
                                hbm=hbm, valu_instr_per_symbol=round(per_sym, 2), valu_instr_source=src,
                                note="lane <-> test angle, one wave per 1024 symbols; the stage time also holds alphabet analysis, unwrap scan and de-rotation")
            if "relaxation pass" in kname:
                # what bounds the pass kernel: instruction issue of the fp32 vector units, not HBM
                st = tier_b["stages"][int(kname[5]) - 1]
                chains = st["S"] * rx.modes.size
                ntot = rx.nmodes * rx.Ntaps
                flops = chains * st["seg_len"] * (2 * ntot) * 8.0           # filter + update: 2 x ntot complex multiply-adds per chain and step
                tpl8 = 11 if rx.nmodes * -(-rx.Ntaps // 11) <= 8 and 11 * -(-rx.Ntaps // 11) - rx.Ntaps <= 3 else (6 if rx.nmodes * -(-rx.Ntaps // 6) <= 8 and 6 * -(-rx.Ntaps // 6) - rx.Ntaps <= 3 else 0)
                lpc = 8 if chains > 4096 and tpl8 else 16                   # seg_lanes (train_seg.h)
                waves = -(-chains // (64 // lpc))
                ipw, src = float(SEG_INSTR_PER_WAVE_STEP[lpc]), "ISA count of the main loop incl. s_nop / s_waitcnt (DESIGN.md 3.2.2)"
                mid = _lib.METHOD_ID[cfg["methods"][int(kname[5]) - 1]]
                hit = [v for k, v in (instr or {}).get("kernels", {}).items() if k.startswith("qh::train_seg_kernel<float, %d," % mid)]
                if hit and hit[0].get("SQ_INSTS_VALU") and hit[0].get("SQ_WAVES"):
                    ipw = float(hit[0]["SQ_INSTS_VALU"]) / (float(hit[0]["SQ_WAVES"]) * st["seg_len"])
                    src = "SQ_INSTS_VALU / (SQ_WAVES x steps per chain) of the same kernel sources (profiles/pmc_instr_%s.json)" % args.workload
                winstr = waves * st["seg_len"] * ipw
                # The roofline of this kernel is the packed-fp32 VECTOR peak (intensity 54 flop/B against a machine balance of ~20: the compute
                # side binds; no GEMM shape at 2 output modes, so not MFMA): `achieved` = ALGORITHMIC flops of one launch (filter +
                # update = 2 x nmodes x ntaps complex multiply-adds x 8 flop per chain and step) / the event-timed launch duration, `frac` = that over
                # 157.3 TFLOP/s.  `issue_frac` beside it is the utilisation view (all vector instructions the kernel issues - DPP adds, selects,
                # error function included - against 1024 SIMDs x 2.4 GHz / 4 cycles): how busy the issue ports are, not how much of it is useful.
                roofline.update(bound="valu-fp32", achieved=round(flops / (kms * 1e-3) / 1e12, 3), peak=VALU_PEAK_TFLOPS, unit="TFLOP/s",
                                frac=round(flops / (kms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 4), algorithmic_flops=int(flops), hbm=hbm, launches_per_step=st["P"],
                                issue_frac=round(winstr / (kms * 1e-3) / 1e9 / VALU_PEAK_GINSTR, 4),
                                issue=dict(achieved=round(winstr / (kms * 1e-3) / 1e9, 1), peak=VALU_PEAK_GINSTR, unit="G wave-instr/s", valu_instr_per_wave_step=round(ipw, 1),
                                           irreducible_pk_fma_per_wave_step=round((64 // lpc) * 2 * ntot * 4 / 2 / 64.0, 1), valu_instr_source=src),
                                chains=int(chains), lanes_per_chain=lpc, waves=int(waves), waves_per_simd=round(waves / 1024.0, 2), steps_per_chain=int(st["seg_len"]),
                                launch_ms_by_pass=st.get("pass_ms_by_pass"), launch_ms_pass1_in_timed_region=st["pass_ms"],
                                launch_ms_source="average over ALL launches of the kernel, every pass event-timed on the library stream in a run of its own right after the timed region "
                                                 "(same receiver, same mode: consecutive captures, phase search and next capture's preparation beside the passes); "
                                                 "the first pass of a sweep shares the chip with them (launch_ms_by_pass)" if st.get("pass_ms_all_launches") else "pass 1 of every sweep, event-timed inside the timed region",
                                note="one launch trains all segments of the sweep (%d lanes per chain, %d chains per wave64, one wave per SIMD); frac = algorithmic flops of the "
                                     "recurrence / packed-fp32 vector peak; issue_frac = vector instructions issued / nominal issue rate; `hbm`: algorithmic bytes of one sweep "
                                     "(read E, write err) against 8 TB/s" % (lpc, 64 // lpc))
            # ---- whole step: useful arithmetic and traffic against the fused bound - what the NUMBER of passes costs
            ntot_ = rx.nmodes * rx.Ntaps
            useful = sum(rx.Niter[s2] * rx.TrSyms[s2] * nsel * 2 * ntot_ * 8.0 for s2 in range(rx.nstage)) + rx.N * nsel * ntot_ * 8.0 \
                + (rx.N * nsel * cfg["A"] * 25.0 if cfg["A"] else 0.0)
            moved = sum(tier_b["stages"][s2]["P"] * train_bytes[s2] for s2 in range(rx.nstage)) + stage_bytes[-2 if cfg["A"] else -1] + (stage_bytes[-1] if cfg["A"] else 0)
            roofline["step"] = dict(useful_flops=int(useful), useful_flops_frac=round(useful / (ms_timed * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 4),
                                    passes=[st_["P"] for st_ in tier_b["stages"]], sweeps_of_the_recurrence=[int(n) for n in rx.Niter],
                                    algorithmic_bytes_moved=int(moved), fused_bound_bytes=int(FUSED_BYTES_PER_SYM * nsym),
                                    traffic_vs_fused=round(moved / float(FUSED_BYTES_PER_SYM * nsym), 2),
                                    note="useful flops = the sweeps of the recurrence themselves (once each) + filter + slicer phase search (SURVEY.md 8d); bytes moved = "
                                         "every pass re-reads the capture and re-writes the error trace: passes x 48 B + filter 48 B + search 40 B per symbol against the fused 88 B")
            roofline["useful_flops_frac"] = roofline["step"]["useful_flops_frac"]
            roofline["traffic_vs_fused"] = roofline["step"]["traffic_vs_fused"]
        else:
            dom = int(np.argmax(head_ms))
            achieved = stage_bytes[dom] / (head_ms[dom] * 1e-3) / 1e9
            roofline = dict(bound="latency (dependent instruction issue)" if 1 <= dom <= rx.nstage else "hbm", kernel=stage_names[dom], achieved=round(achieved, 3), peak=HBM_PEAK_GBS,
                            unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 6), traffic=None, algorithmic_bytes=int(stage_bytes[dom]),
                            note="exact sequential LMS recurrence: dependent-issue bound, one workgroup per output mode (DESIGN.md 3.1); HBM figure for reference")
        # measured HBM traffic of the dominant kernel: from the PMC passes of the same workload (scripts/gpu_pmc.sh ->
        # profiles/pmc_traffic_<workload>.json), quoted only while the kernel sources are the ones that were profiled
        pmc = pmc_json("pmc_traffic", args.workload)
        if pmc:
            kern = roofline["kernel"]
            pat = None
            if "relaxation pass" in kern:
                pat = "qh::train_seg_kernel<float, %d," % _lib.METHOD_ID[cfg["methods"][int(kern[5]) - 1]]
            elif kern.startswith("train"):
                mid = _lib.METHOD_ID[cfg["methods"][int(kern[5]) - 1]]
                pat = ("qh::train_la_kernel<float, %d," % mid, "qh::train_bi_kernel<float, %d," % mid)
            elif kern == "bps_recover":
                pat = ("qh::bps_stream_kernel", "qh::bps_kernel<float>")
            elif kern == "gram":
                pat = "qh::gram_slide_kernel<float"
            hit = [v for k, v in pmc["kernels"].items() if pat and k.startswith(pat)]
            if hit:
                roofline["traffic"] = hit[0]["hbm_bytes"]
        else:
            roofline["traffic_note"] = "no PMC traffic profile of these kernel sources under profiles/: not quoted"
        out["roofline"] = roofline
        # ---- the phase search beside it (detail file): slicer flops of SURVEY.md 8d (2 A 25 per symbol period) / the fused recovery
        # stage one capture at a time (search + unwrap + de-rotation, event pair on its stream); the search kernel's own duration and its instruction
        # counters are in profiles/r06_bps_profile.txt (rocprofv3)
        if cfg["A"] and tier_b is not None:
            one = ((tier_b.get("pipelining") or {}).get("one_capture_at_a_time") or {}).get("stages_ms") or {}
            ms_b = one.get("bps_recover")
            if ms_b and ms_b > 0:
                fl = nsym * nsel * cfg["A"] * 25.0
                by = rx.N * bps_b["bps"]
                out["roofline_phase_search"] = dict(bound="valu-fp32", kernel="bps_recover (analysis + search + unwrap + de-rotation, all modes)", launch_ms=round(ms_b, 3),
                                                    algorithmic_flops=int(fl), achieved=round(fl / (ms_b * 1e-3) / 1e12, 3), peak=VALU_PEAK_TFLOPS, unit="TFLOP/s",
                                                    frac=round(fl / (ms_b * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 4), algorithmic_bytes=int(by),
                                                    hbm=dict(achieved=round(by / (ms_b * 1e-3) / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(by / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)),
                                                    note="whole stage one capture at a time; the search kernel alone: profiles/r06_bps_profile.txt (358 us at C3: 0.24 of the peak)")

    # ---- the other shapes and tolerances of a --full run (N = 1): loose tolerance, a capture with symbol errors, ns, c2
    if args.full and world == 1 and args.tier == "b" and not args.no_extra_shapes and not split:
        try:
            ksteps = max(2, min(args.steps, 10))
            tb2, _, ex2 = run_pair(cfg, sig, nsym, ksteps, 1, barrier_sync, dict(pit, tol=1e-2), 0, 1e-2, overlap=overlap)
            rx2 = ex2["rx"]
            rxa = make_receiver(cfg, sig, tier="a"); rxa.load(sig); rxa.run(); _lib.sync()
            dv = deviation_vs_exact(rx2, rxa, cfg)
            out["tier_b_loose"] = dict(tol=1e-2, value=tb2["value"], ms_per_step=tb2["ms_per_step"], converged=tb2["converged"], errors=tb2["errors"],
                                       passes=[st["P"] for st in tb2["stages"]], est_deviation_rms=[st["est_deviation_rms"][-1:] for st in tb2["stages"]],
                                       out_rms_dev_vs_exact=dv["out_rms_dev_vs_exact"], tap_rel_dev_vs_exact=dv["tap_rel_dev_vs_exact"],
                                       err_trace_rms_dev_vs_exact=dv["err_trace_rms_dev_vs_exact"],
                                       note="informational: the same solver held to a 10 x looser deviation (SER-equivalent tier of SURVEY 7.3-1(b)); never the headline")
            del rx2, rxa, ex2
            if abs(tol_check - TOL_DEFAULT) > 1e-12:
                # the library's default tolerance (the headline of rounds 2-4) beside the headline's, with its own certificate against the exact path
                tb3, _, ex3 = run_pair(cfg, sig, nsym, ksteps, 1, barrier_sync, dict(pit, tol=TOL_DEFAULT), 1, TOL_DEFAULT, overlap=overlap)
                out["tier_b_tol_1e-3"] = dict(tol=TOL_DEFAULT, value=tb3["value"], ms_per_step=tb3["ms_per_step"], one_capture_at_a_time=(tb3.get("pipelining") or {}).get("one_capture_at_a_time"),
                                              certified=tb3["certified"], checks=tb3.get("checks"), info=tb3.get("info"), errors=tb3["errors"],
                                              passes=[st["P"] for st in tb3["stages"]], est_deviation_rms=[st["est_deviation_rms"][-1:] for st in tb3["stages"]],
                                              eq_rms_dev_vs_exact=tb3.get("eq_rms_dev_vs_exact"), out_rms_dev_same_angle=tb3.get("out_rms_dev_same_angle"),
                                              out_rms_dev_vs_exact=tb3["out_rms_dev_vs_exact"], tap_rel_dev_vs_exact=tb3["tap_rel_dev_vs_exact"],
                                              err_trace_rms_dev_vs_exact=tb3["err_trace_rms_dev_vs_exact"],
                                              note="informational: the same solver at the library's default tolerance 1e-3 (the headline tolerance of rounds 2-4)")
                del ex3
            if cfg["A"]:
                rxe = make_receiver(cfg, sig, tier="b", pit=pit); rxe.load(sig); rxe.run(); _lib.sync()
                out["api_end_to_end"] = api_end_to_end_block(cfg, sig, nsym, tol_check, rxe)
                del rxe
            if overlap and args.in_flight == 1:
                out["three_in_flight"] = in_flight_block(cfg, sig, nsym, 3, 3 * max(4, min(args.steps, 20)), barrier_sync, pit)
            if args.workload == "c3":
                out["cert_24dB"] = cert_snr_block(cfg, 24.0, min(nsym, 1 << 21), 1001, barrier_sync, pit, overlap=overlap)
                for key in ("ns", "c2"):
                    out[key] = shape_block(key, barrier_sync, pit, 10, overlap=overlap)
                out["adaptive_step"] = adaptive_block()
                out["survey_recipe"] = survey_recipe_block(barrier_sync, tol_check)
                if args.pool > 1 and overlap:
                    tb1, _, ex1 = run_pair(cfg, sig, nsym, ksteps, 1, barrier_sync, pit, 0, tol_check, overlap=overlap)
                    out["same_capture_every_step"] = dict(value=tb1["value"], ms_per_step=tb1["ms_per_step"], passes=[st["P"] for st in tb1["stages"]],
                                                          note="informational: the workload of rounds 1-4 - the SAME resident capture (seed 1000) K times; the headline rotates %d different captures" % args.pool)
                    del ex1
                else:
                    out["capture_pool"] = capture_pool_block(cfg, nsym, tol_check, barrier_sync)
                out["ref_benchmarks"] = ref_benchmarks_block(tol_check, cpu=not args.no_cpu_baseline)
                # SURVEY.md 8c's tolerance on the three BASELINE shapes, each with the in-run certificate against the exact path
                rows = dict(c3=dict(value=tier_b["value"], certified=tier_b["certified"], checks=tier_b.get("checks"), passes=[st["P"] for st in tier_b["stages"]],
                                    eq_rms_dev_vs_exact=tier_b.get("eq_rms_dev_vs_exact"), tap_rel_dev_vs_exact=tier_b.get("tap_rel_dev_vs_exact"),
                                    err_trace_rms_dev_vs_exact=tier_b.get("err_trace_rms_dev_vs_exact"), out_rms_dev_same_angle=tier_b.get("out_rms_dev_same_angle"),
                                    other_angle_symbol_fraction=tier_b.get("bps_angle_mismatch_fraction"), elementwise_summary=tier_b.get("elementwise_summary")))
                for key in ("ns", "c2"):
                    b_ = out[key]["tier_b"]
                    rows[key] = dict(value=b_["value"], certified=b_["certified"], checks=b_["checks"], passes=[st["P"] for st in b_["stages"]],
                                     eq_rms_dev_vs_exact=b_["eq_rms_dev_vs_exact"], tap_rel_dev_vs_exact=b_["tap_rel_dev_vs_exact"],
                                     err_trace_rms_dev_vs_exact=b_["err_trace_rms_dev_vs_exact"], out_rms_dev_same_angle=b_["out_rms_dev_same_angle"],
                                     other_angle_symbol_fraction=b_["bps_angle_mismatch_fraction"], elementwise_summary=b_.get("elementwise_summary"))
                out["tier_b_tight"] = dict(tol=tol_check, certified=bool(all(r["certified"] for r in rows.values())), **rows,
                                           held="equaliser output <= tol (relative rms, every symbol), taps <= 3 tol (relative norm), error traces <= 3 tol (rms, signal units), "
                                                "recovered output <= tol on every symbol whose test angle agrees with the exact path's (the share of the others is reported), "
                                                "symbol errors within +-%d, every stage certified by the device's own estimate; element by element (rtol = atol = 1e-4, the exact "
                                                "path's own bar): every tap and every equaliser-output sample inside, the error traces' share reported" % SER_TOL_ERRORS)
            _lib.call("qh_release_scratch")
        except Exception as e:                    # informational blocks never take the headline down
            out["extra_shapes_error"] = "%s: %s" % (type(e).__name__, e)

    if args.full and world == 1 and not args.no_cpu_baseline:
        sample = min(nsym, args.cpu_sample or nsym)
        cb = cpu_baseline(cfg, sig, sample, min(sample, args.cpu_sample_1t or sample))
        r_cpu = cb["result"]
        sig_s = sig.recreate_from_np_array(np.asarray(sig)[:, :2 * sample])
        sig_s._symbols = sig.symbols[:, :sample]
        e_cpu = symbol_errors(r_cpu["out"], sig_s)
        out["cpu_baseline"] = dict(value=round(cb["all"]["value"], 4), unit="MSym/s", cores=cb["all"]["cores"], kind="port",
                                   algorithm="exact sequential recurrence (the reference's loops and OpenMP placement)",
                                   sample="%s symbol periods of the same capture, all stages, %d OpenMP threads (placement as in the reference: "
                                          "modes-parallel train, collapse(2) apply, L-parallel BPS distances)" % ("all %d" % sample if sample == nsym else "first %d" % sample, cb["all"]["cores"]),
                                   runs_s=cb["all"]["runs_s"], stages_s=cb["all"]["stages_s"], cpu_model=cpu_model(),
                                   one_thread=dict(value=round(cb["one"]["value"], 4), sample=cb["one"]["sample"], seconds=cb["one"]["seconds"], stages_s=cb["one"]["stages_s"]),
                                   transfers=transfer_times(sig, rx))
        # GPU vs CPU on the identical sample: SER / taps
        if sample == nsym:
            e_gpu = errs
            w_gpu = rx.wxy.to_host()
        else:
            rx2 = make_receiver(cfg, sig_s, tier=args.tier, pit=pit)
            rx2.load(np.asarray(sig)[:, :2 * sample])
            rx2.run()
            r2 = rx2.fetch()
            e_gpu = symbol_errors(r2["out"] if cfg["A"] else r2["eq"], sig_s)
            w_gpu = r2["wxy"]
        tapd = []
        for m in range(w_gpu.shape[0]):
            g = 1j ** int(np.rint(np.angle(np.vdot(w_gpu[m].ravel(), r_cpu["wxy"][m].ravel())) / (np.pi / 2)))
            tapd.append(float(np.max(np.abs(r_cpu["wxy"][m] - g * w_gpu[m]))))
        out["parity_vs_cpu"] = dict(sample=sample, errors_gpu=[e for e, _ in e_gpu], errors_cpu=[e for e, _ in e_cpu],
                                    errors_gpu_exact=tier_a["errors"] if (tier_a and sample == nsym) else None,
                                    ser_gpu=[e / max(n, 1) for e, n in e_gpu] if sample != nsym else out["ser"]["per_mode_rank0"],
                                    ser_cpu=[e / n for e, n in e_cpu], max_abs_tap_diff=tapd)
        # The ratio is keyed to the tier that produced `value`.  The CPU leg runs the exact recurrence; tier b solves the SAME recurrence
        # from the same start taps in another order of evaluation, to the stated tolerance (measured above) - tier a's own ratio beside it.
        out["speedup_vs_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 2)
        out["speedup_vs_cpu_tier"] = out["headline_tier"]
        if tier_a:
            tier_a["speedup_vs_cpu"] = round(tier_a["value"] / out["cpu_baseline"]["value"], 2)
        if tier_b:
            tier_b["speedup_vs_cpu"] = round(tier_b["value"] / out["cpu_baseline"]["value"], 2)

    if args.full and world == 1 and args.bank > 1:
        del rx
        try:
            # channels x symbol periods bounded to what 128 captures of 2^22 periods take (bank buffers + block-iterative scratch)
            nbank = max(2, min(args.bank, (args.bank << 22) // max(nsym, 1)))
            out["channel_bank"] = channel_bank_run(cfg, sig, nbank, max(1, min(args.steps, 2)), barrier_sync, args.bank_trainer)
            _lib.call("qh_release_scratch")
            workers = min(os.cpu_count() or 1, 128) if args.cpu_bank_workers < 0 else args.cpu_bank_workers
            if workers > 0 and not args.no_cpu_baseline:
                out["channel_bank"]["cpu_baseline"] = cpu_channel_bank(cfg, args.workload, sig, min(nsym, 1 << 17), workers)
                if "value" in out["channel_bank"]["cpu_baseline"]:
                    out["channel_bank"]["speedup_vs_cpu_bank"] = round(out["channel_bank"]["value"] / out["channel_bank"]["cpu_baseline"]["value"], 2)
        except Exception as e:                    # informational only: never take the headline line down with it
            out["channel_bank"] = dict(channels=args.bank, error="%s: %s" % (type(e).__name__, e))

    emit(out, args.detail_out)
    if getattr(cm, "stuck", False):                  # a helper thread is still inside RCCL's bootstrap: do not wait for it at interpreter exit
        os._exit(0)


def kernel_sources_sha():
    """Fingerprint of the kernel sources a PMC profile belongs to (profiles/pmc_traffic_*.json carry it)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "qampy_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


if __name__ == "__main__":
    main()
