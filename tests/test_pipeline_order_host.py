"""
The stream choreography of ``pipeline.ResidentReceiver`` checked without a GPU: the library is replaced by a recorder that keeps the
enqueue order on the three library streams, drives the tier-b hooks the way the library does, and runs a happens-before check over
every buffer an entry point reads or writes.  A hazard is two accesses to one buffer, at least one of them a write, that no stream
order, event or host synchronisation puts one after the other.
"""
import bisect
import ctypes as C
import re

import numpy as np
import pytest

from qampy_amd import _lib, pipeline
from qampy_amd.core.equalisation import hip_equalisation as _k

BASE = 1 << 60                  # fake device addresses: far above anything the host allocator hands out
NPASS = 4                       # simulated relaxation passes of a tier-b training call
_vp = C.c_void_p

# entry point -> (argument positions read, argument positions written); the positions are checked against _lib.SIGNATURES below
_TRAIN_RW = ((0, 6, 7, 12), (6, 7, 15))          # E, mu, taps, symbols in; mu (adaptive step), taps, error trace out
_PIT_RW = ((0, 6, 7, 11, 16), (6, 7, 14, 18))    # ... symbols, Gram table in; ... error trace, report out (+ basis, prepared from the options)
_RECOVER_RW = ((0, 3, 5), (8, 9, 10))
ACCESS = {
    "qh_memcpy_d2d": ((1,), (0,)), "qh_memset": ((), (0,)), "qh_memcpy_h2d": ((), (0,)), "qh_memcpy_d2h": ((1,), ()),
    "qh_memcpy_h2d_async": ((), (0,)), "qh_memcpy_d2h_async": ((1,), ()),
    "qh_train_equaliser_c64_dev": _TRAIN_RW, "qh_train_equaliser_c64_gram_dev": ((0, 6, 7, 12, 17), (6, 7, 15)),
    "qh_train_equaliser_c64_pit_dev": _PIT_RW,
    "qh_gram_build_c64_dev": ((0,), ()), "qh_gram_build_c64_batch_dev": ((0,), ()),      # (+ the library's own table, see _gram_build)
    "qh_train_equaliser_c64_batch_dev": ((0, 7, 8, 13, 18), (7, 8, 16)),
    "qh_pit_basis_c64_dev": ((0,), (6,)), "qh_pit_prepare_c64_dev": ((0, 5, 6, 10), (14,)),
    "qh_apply_filter_c64_dev": ((0, 4), (8,)),
    "qh_bps_recover_c64_dev": _RECOVER_RW, "qh_bps_recover_part_c64_dev": _RECOVER_RW,
    "qh_bps_twostage_recover_c64_dev": ((0, 3, 6), (9, 10, 11, 12)),
    "qh_vv_recover_c64_dev": ((0,), (5, 6)), "qh_partition16_recover_c64_dev": ((0,), (4, 5)),
    "qh_find_freq_offset_c64_dev": ((0,), (7, 8, 9)), "qh_comp_freq_offset_c64_dev": ((0, 3), (5,)),
    "qh_impair_pointwise_c64_dev": ((0,), (10, 11)), "qh_apply_pmd_c64_dev": ((0,), (5,)),
    "qh_iq_moments_c64_dev": ((0,), (4,)), "qh_iq_coeffs_dev": ((0,), (5,)), "qh_iq_affine_c64_dev": ((0, 3), (4,)),
    "qh_cd_filter_c64_dev": ((0,), (8,)),
    "qh_resample_c64_dev": ((0,), (9,)), "qh_row_moments_c64_dev": ((0,), (3,)), "qh_center_scale_c64_dev": ((0, 3), (4,)),
}
for _name, (_r, _w) in ACCESS.items():
    assert all(_lib.SIGNATURES[_name][i] is _vp for i in _r + _w), _name
# calls that move no data: recorded, never a buffer access
PLAIN = {"qh_use_stream", "qh_stream_wait_event", "qh_event_record", "qh_sync", "qh_malloc", "qh_free", "qh_event_create", "qh_event_destroy",
         "qh_pit_auto_segments", "qh_pit_basis_bytes", "qh_pit_prepare_bytes", "qh_pit_last_timing", "qh_get_gram_budget_gb", "qh_get_form", "qh_set_trainer"}


class FakeLibrary:
    """Stands in for ``_lib.call``.  ``log``: every call as (stream, entry point, arguments); ``hazards``: what the happens-before check found."""

    def __init__(self):
        self.next, self.starts, self.ends = BASE, [], []
        self.cur = 0
        self.clock = {s: {} for s in (0, 1, 2)}        # vector clock of a stream: stream -> sequence number it has seen
        self.host = {}                                  # what the host has waited for: ordered before everything enqueued later
        self.seq = {0: 0, 1: 0, 2: 0}
        self.events = {}
        self.accesses = {}                              # allocation -> [(stream, seq, is_write, entry point)]
        self.log, self.hazards = [], []
        self.gram = None

    # -------------------------------------------------------------------------------------------- the recorder
    def call(self, name, *a):
        if name not in ACCESS and name not in PLAIN:
            raise AssertionError("%s: not in the access table of tests/test_pipeline_order_host.py" % name)
        if name not in ("qh_free", "qh_event_destroy"):           # (these come from the garbage collector)
            self.log.append((self.cur, name, a))
        handler = getattr(self, "_" + name, None)
        if handler is not None:
            handler(*a)
        elif name in ACCESS:
            self.op(name, a)

    def alloc(self, nbytes):
        p = self.next
        self.next += (max(int(nbytes), 1) + 255) // 256 * 256
        self.starts.append(p)
        self.ends.append(self.next)
        return p

    def base(self, p):
        """The allocation a device pointer lies in (rows and offsets count as the whole array); None for host memory."""
        if p is None or p < BASE:
            return None
        i = bisect.bisect_right(self.starts, p) - 1
        assert i >= 0 and p < self.ends[i], "a device pointer outside every allocation"
        return self.starts[i]

    def op(self, name, a, reads=(), writes=(), tag=""):
        """One unit of device work on the current stream: stamp it, check it against every earlier access of the buffers it touches."""
        s = self.cur
        for k, v in self.host.items():
            self.clock[s][k] = max(self.clock[s].get(k, 0), v)
        self.seq[s] += 1
        self.clock[s][s] = self.seq[s]
        r, w = ACCESS.get(name, ((), ()))
        touched = [(self.base(a[i]), False) for i in r] + [(self.base(p), False) for p in reads]
        touched += [(self.base(a[i]), True) for i in w] + [(self.base(p), True) for p in writes]
        for buf, is_write in touched:
            if buf is None:
                continue
            for (s0, q0, w0, n0) in self.accesses.setdefault(buf, []):
                if (is_write or w0) and self.clock[s].get(s0, 0) < q0:
                    self.hazards.append((buf, n0, s0, name + tag, s))
            self.accesses[buf].append((s, self.seq[s], is_write, name + tag))

    def publish(self, streams):
        for s in streams:
            for k, v in self.clock[s].items():
                self.host[k] = max(self.host.get(k, 0), v)

    # -------------------------------------------------------------------------------------------- entry points with a behaviour of their own
    def _qh_malloc(self, ref, nbytes):
        ref._obj.value = self.alloc(nbytes)

    def _qh_event_create(self, ref):
        ref._obj.value = self.alloc(1)

    def _qh_use_stream(self, idx):
        assert idx in (0, 1, 2)
        self.cur = idx

    def _qh_event_record(self, ev):
        self.events[ev] = dict(self.clock[self.cur])

    def _qh_stream_wait_event(self, ev):
        for k, v in self.events.get(ev, {}).items():              # (an event never recorded: the wait returns at once, as in HIP)
            self.clock[self.cur][k] = max(self.clock[self.cur].get(k, 0), v)

    def _qh_sync(self):
        self.publish((0, 1, 2))

    def _qh_memcpy_h2d(self, *a):
        self.op("qh_memcpy_h2d", a)
        self.publish((self.cur,))

    def _qh_memcpy_d2h(self, dst, src, n):
        C.memset(dst, 0, n)
        self.op("qh_memcpy_d2h", (dst, src, n))
        self.publish((self.cur,))

    def _qh_pit_auto_segments(self, TrSyms, mu, nsel, cold, ref):
        ref._obj.value = 8

    def _qh_pit_basis_bytes(self, ntot, ref):
        ref._obj.value = 4096

    def _qh_pit_prepare_bytes(self, nmodes, ntaps, steps, itemsize, ref):
        ref._obj.value = 8192

    def _qh_pit_last_timing(self, buf, nmax, n, acq):
        n._obj.value, acq._obj.value = 0, 0.

    def _qh_get_gram_budget_gb(self, ref):
        ref._obj.value = 8.

    def _qh_get_form(self, key, ref):
        ref._obj.value = 0

    def _gram_build(self, name, a):
        if self.gram is None:
            self.gram = self.alloc(1 << 20)                      # library-owned, reused by every build
        self.op(name, a, writes=(self.gram,))
        a[-1]._obj.value = self.gram

    def _qh_gram_build_c64_dev(self, *a):
        self._gram_build("qh_gram_build_c64_dev", a)

    def _qh_gram_build_c64_batch_dev(self, *a):
        self._gram_build("qh_gram_build_c64_batch_dev", a)

    def _qh_train_equaliser_c64_pit_dev(self, *a):
        """The options behind the byref argument: the basis and the prepared acquisition are read at the start and in every pass; ``on_pass`` runs
        before each pass's trainer launch, ``on_pass0`` once after the first."""
        name, o, s = "qh_train_equaliser_c64_pit_dev", a[17]._obj, self.cur
        self.op(name, a, reads=(o.basis, o.prepared))
        for p in range(NPASS):
            if o.on_pass:
                _lib.PIT_PASS_HOOK(o.on_pass)(o.on_pass_user, 0, p)
            assert self.cur == s, "a hook left another stream current"
            self.op(name, a, reads=(o.basis, o.prepared), tag=":pass%d" % p)
            if p == 0 and o.on_pass0:
                _lib.PIT_HOOK(o.on_pass0)(o.on_pass0_user)
            assert self.cur == s, "a hook left another stream current"


class FakeArray(_lib.DeviceArray):
    def free(self):                 # (nothing of the fake address space ever reaches the real library)
        pass


class FakeEvent(_lib.Event):
    def __del__(self):
        pass


class FakeReport(_k.PitReportBuffer):
    def free(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLibrary()

    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", lib.call)
    monkeypatch.setattr(_lib, "DeviceArray", FakeArray)
    monkeypatch.setattr(_lib, "Event", FakeEvent)
    monkeypatch.setattr(pipeline, "DeviceArray", FakeArray)
    monkeypatch.setattr(_k, "DeviceArray", FakeArray)
    monkeypatch.setattr(_k, "PitReportBuffer", FakeReport)
    monkeypatch.delenv("QAMPY_POST_PARTS", raising=False)
    return lib


def sequence(lib, start=0):
    """The recorded calls from ``start`` on as (stream, entry point, arguments) with every device pointer, event and option pointer replaced by
    the order of its first appearance: two runs made the same calls on the same buffers in the same order iff their sequences are equal."""
    seen = {}

    def label(p):
        if p is None or p < BASE:
            return None if p is None else "host"
        return seen.setdefault(lib.base(p), "dev%d" % len(seen))
    out = []
    for s, name, a in lib.log[start:]:
        sig, row = _lib.SIGNATURES[name], []
        for t, v in zip(sig, a):
            if hasattr(v, "_obj"):                                # a byref argument: the options of a tier-b call, else an output
                o = v._obj
                if isinstance(o, _lib.PitOpts):
                    v = tuple((f, label(getattr(o, f)) if f in ("basis", "prepared") else bool(getattr(o, f)) if f.startswith("on_") else getattr(o, f))
                              for f, _ in o._fields_ if getattr(o, f))
                else:
                    v = "ref"
            elif t is _vp:
                v = label(v)
            elif not isinstance(v, (int, float, bytes, str)):
                v = "ref"
            row.append(v)
        out.append((s, name, tuple(row)))
    return out


# ------------------------------------------------------------------------------------------------ scenarios
L = 1024
CAPTURE = (np.arange(2 * L).reshape(2, L) % 7 + 1j).astype(np.complex64)


def receiver(tier="b", M=64, **kw):
    al = np.exp(2j * np.pi * np.arange(M) / M).astype(np.complex64)
    return pipeline.ResidentReceiver(2, L, 2, M, 5, (1e-3, 1e-3), methods=("cma", "cma"), Mtestangles=16, Nbps=8, alphabet=al, tier=tier, **kw)


def _foe(rx):
    rx.compensate_foe(fft_size=256)


def _impair(rx):
    rx.impair(2., snr=20.)


def _hand_write(rx):
    rx.input_free()
    rx.E.copy_from(rx.hand_source)


def _hand_write_unordered(rx):
    rx.E.copy_from(rx.hand_source)


SCENARIOS = {
    "a": dict(tier="a", overlap=False), "a-overlap": dict(tier="a"), "a-overlap-hand-write": dict(tier="a", between=_hand_write),
    "b": dict(overlap=False), "b-overlap-parts0": dict(parts=0), "b-overlap-parts1": dict(parts=1), "b-overlap-parts3": dict(parts=3),
    "b-overlap-parts16": dict(parts=16),
    "b-prefetch-resident": dict(prefetch=True), "b-prefetch-fed": dict(prefetch=True, feed=True), "b-prefetch-fed-parts1": dict(prefetch=True, feed=True, parts=1),
    "b-serial-prefetch-fed": dict(overlap=False, prefetch=True, feed=True),
    "b-twostage": dict(Bbps=4), "b-twostage-parts1": dict(Bbps=4, parts=1), "b-vv": dict(carrier="vv", M=4),
    "b-foe-between": dict(between=_foe), "b-impair-between": dict(between=_impair, parts=3), "b-hand-write": dict(between=_hand_write),
    "b-hand-write-parts1": dict(between=_hand_write, parts=1),
}


def play(lib, tier="b", overlap=True, parts=0, prefetch=False, feed=False, between=None, **kw):
    """Four consecutive runs, then wait_post(); ``between``: called before every run but the first.  The receiver comes back with the names
    it had after ``__init__`` as ``declared``."""
    rx = receiver(tier, **kw)
    declared = set(vars(rx))
    rx.declared, rx.hand_source = declared, _lib.DeviceArray((2, L), np.complex64)
    rx.post_parts = parts
    rx.load(CAPTURE)
    for k in range(4):
        if feed:
            rx.load_next(CAPTURE + k)
        if between is not None and k:
            between(rx)
        rx.run(overlap=overlap, prefetch=prefetch)
    rx.wait_post()
    return rx


def names(rx):
    """Allocation -> the receiver's name for it."""
    out = {}

    def put(name, v):
        if isinstance(v, _lib.DeviceArray) and v.ptr:
            out.setdefault(v.ptr, name)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                put("%s[%d]" % (name, i), x)
    for k, v in vars(rx).items():
        put(k, v)
    return out


def described(lib, rx):
    nm = names(rx)
    return sorted({(nm.get(buf, hex(buf)), "%s on stream %d" % (n0, s0), "%s on stream %d" % (n1, s1)) for buf, n0, s0, n1, s1 in lib.hazards})


@pytest.mark.parametrize("case", sorted(SCENARIOS))
def test_no_buffer_is_touched_out_of_order(fake, case):
    rx = play(fake, **SCENARIOS[case])
    assert described(fake, rx) == []
    assert set(vars(rx)) - {"declared", "hand_source"} == rx.declared, "an attribute was created after __init__"
    want = {0} | ({1} if SCENARIOS[case].get("prefetch") else set()) | ({2} if SCENARIOS[case].get("overlap", True) else set())
    assert {s for s, _, _ in fake.log} == want, "the scenario did not run what it is named after"


@pytest.mark.parametrize("tier", ["a", "b"])
def test_the_check_sees_a_hand_write_that_nothing_orders(fake, tier):
    """The control: ``rx.E.copy_from(...)`` right after ``run(overlap=True)`` without ``input_free()``.  Tier b: the copy overwrites the capture
    the filter on stream 2 is still reading.  Tier a: the filter ran on stream 0, nothing to find."""
    rx = play(fake, tier=tier, between=_hand_write_unordered)
    found = described(fake, rx)
    if tier == "a":
        assert found == []
    else:
        assert found and all(h == ("E", "qh_apply_filter_c64_dev on stream 2", "qh_memcpy_d2d on stream 0") for h in found), found


def test_the_hooks_are_driven_and_the_search_goes_in_parts(fake):
    """The fake drives ``on_pass`` / ``on_pass0`` like the library: with ``post_parts = 3`` the pending search is three part launches on stream 2,
    with 16 (more parts than passes) the passes take four and the rest follows the training."""
    for parts, want in ((3, 3), (16, 16)):
        del fake.log[:]
        play(fake, parts=parts)
        got = [(s, a[-2], a[-1]) for s, n, a in fake.log if n == "qh_bps_recover_part_c64_dev"]
        assert got == [(2, i, want) for i in range(want)] * 3 and not fake.hazards


def test_every_attribute_is_declared_in_init(fake):
    """One receiver through every loading and conditioning stage and both kinds of run: no name appears that ``__init__`` did not set."""
    rx = receiver("b")
    declared = set(vars(rx))
    rx.load(CAPTURE)
    rx.load_next(CAPTURE)
    rx.load_resampled(np.concatenate([CAPTURE, CAPTURE], axis=1), 4., fs=2.)
    rx.load_resampled(np.concatenate([CAPTURE, CAPTURE], axis=1), 4., fs=2., next_capture=True)
    rx.compensate_cd(2., 17e-6, 1e3)
    rx.frontend()
    rx.compensate_foe(fft_size=256)
    rx.impair(2., snr=20., dgd=1e-12)
    for overlap, prefetch in ((False, False), (True, False), (True, True), (True, True)):
        rx.run(overlap=overlap, prefetch=prefetch)
    rx.impair(2., snr=20., next_capture=True)
    rx.wait_post()
    rx.apply()
    rx.recover()
    rx.release_thread_state()
    assert set(vars(rx)) == declared and not fake.hazards
    src = open(pipeline.__file__.replace(".pyc", ".py")).read()
    assert not re.search(r"getattr\(self, \"", src)
    bank = pipeline.ChannelBank(2, 2, L, 2, 64, 5, (1e-3, 1e-3), methods=("cma", "cma"), Mtestangles=16, Nbps=8, alphabet=rx.alphabet_host)
    declared = set(vars(bank))
    bank.load(0, CAPTURE)
    bank.run()
    bank.run_pipelined(3)
    assert set(vars(bank)) == declared


def test_conditioning_a_capture_that_was_placed_by_hand(fake):
    """Tier b, the capture copied into ``rx.E`` on the device and never through ``load()``: ``impair(snr=...)`` and ``frontend()`` complete, and
    ``impair`` makes the calls it makes after a ``load()``."""
    seqs = []
    for loaded in (True, False):
        rx = receiver("b")
        if loaded:
            rx.load(CAPTURE)
        else:
            rx.E.copy_from(_lib.DeviceArray((2, L), np.complex64))
        start = len(fake.log)
        rx.impair(2., snr=20., power=1.0)
        seqs.append(sequence(fake, start))
        assert rx.pit[0]["acq_chunk"] == rx._acq_chunk_rule(1.0 * (1 + 2 * 10 ** -2.), 1e-3, rx.pit[0]) and rx._acq_asked[0]
    assert seqs[0] == seqs[1] and [n for _, n, _ in seqs[0]] == ["qh_impair_pointwise_c64_dev"]
    rx = receiver("b")
    rx.E.copy_from(_lib.DeviceArray((2, L), np.complex64))
    rx.frontend()
    assert rx._acq_asked[0] and rx._load_power == 0.


def test_on_stream_restores_stream_0(fake):
    with _lib.on_stream(2):
        assert fake.cur == 2
    assert fake.cur == 0
    with pytest.raises(ZeroDivisionError):
        with _lib.on_stream(1):
            1 // 0
    assert fake.cur == 0 and [a for _, n, a in fake.log if n == "qh_use_stream"] == [(2,), (0,), (1,), (0,)]
