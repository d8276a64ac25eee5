"""
Signal objects: the part of qampy/signals.py (1952 lines) the hot path and a transmitter need.

The hot-path wrappers only touch ``sig.os, sig.M, sig.fb, sig.fs, sig.coded_symbols, sig.symbols`` and
``sig.recreate_from_np_array(arr, fs=...)`` (qampy/equalisation.py:246-259, qampy/phaserec.py:92, qampy/signals.py:179-181, :209-220,
:872-878): :class:`SignalQAM` is one duck-typed ndarray subclass carrying exactly these around data somebody else produced.  Any object
exposing the same attributes - including a real ``qampy.signals.SignalQAMGrayCoded`` - works with ``qampy_amd.equalisation`` /
``qampy_amd.phaserec``.  :class:`PilotSignal` does the same for the pilot receiver (the attributes of ``SignalWithPilots`` the receiver reads).

The source of a signal is here too, with the reference's call surface (qampy/signals.py:53-137, :611-905): :class:`RandomBits`,
:class:`PRBSBits` (the generator runs on the device, csrc/source.hip) and :class:`SignalQAMGrayCoded` - bits to Gray-mapped symbols on the
device, ``from_bit_array``, ``from_symbol_array``, ``modulate``, ``bits`` - and :class:`SignalWithPilots` (:1430-1645), which lays pilots and
payload out as frames on the device (csrc/pilot.hip) - :class:`SignalPSKGrayCoded`, :class:`ResampledQAM` and :class:`TDHQAMSymbols` (:932-947,
:1142-1427), time-domain hybrid QAM, whose split and metrics the reference left unfinished and csrc/hybrid.hip runs on the device.
``QPSKfromBERT`` and ``SymbolOnlySignal`` stay out of scope.
"""
import warnings

import numpy as np

from . import theory
from .core import ber_functions

_ATTRS = ("_M", "_fb", "_fs", "_coded_symbols", "_symbols")


class SignalQAM(np.ndarray):
    """
    2-D complex array ``(nmodes, nsamples)`` with QAM metadata.

    Parameters
    ----------
    data : array_like (nmodes, N) complex
    M : QAM order
    fb : symbol rate, fs : sampling rate (``os = int(fs/fb)`` as in signals.py:179-181)
    symbols : transmitted symbol sequence (nmodes, nsym) the capture is based on (used by data-aided methods / SER)
    coded_symbols : alphabet in Gray-label order; generated from ``M`` when omitted
    """

    def __new__(cls, data, M, fb=1., fs=None, symbols=None, coded_symbols=None):
        obj = np.atleast_2d(np.asarray(data)).view(cls)
        if not np.iscomplexobj(obj):
            raise ValueError("SignalQAM needs a complex array")
        obj._M = int(M)
        obj._fb = fb
        obj._fs = fb if fs is None else fs
        if coded_symbols is None:
            coded_symbols = theory.coded_symbols_qam(M, dtype=obj.dtype)
        obj._coded_symbols = np.asarray(coded_symbols)
        obj._symbols = None if symbols is None else np.atleast_2d(np.asarray(symbols))
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        for a in _ATTRS:
            setattr(self, a, getattr(obj, a, None))

    # ---- the attributes the wrappers read
    @property
    def M(self):
        return self._M

    @property
    def fb(self):
        return self._fb

    @property
    def fs(self):
        return self._fs

    @property
    def os(self):
        return int(self.fs / self.fb)

    @property
    def coded_symbols(self):
        return self._coded_symbols

    @property
    def symbols(self):
        return self._symbols

    def recreate_from_np_array(self, arr, **kwargs):
        """Re-wrap a plain array with this signal's metadata (behaviour of signals.py:209-220)."""
        out = np.asarray(arr).view(type(self))
        for a in _ATTRS:
            setattr(out, a, getattr(self, a))
        if "fb" in kwargs and "fs" not in kwargs:
            kwargs["fs"] = self.os * kwargs["fb"]
        for k, v in kwargs.items():
            if "_" + k in _ATTRS:
                k = "_" + k
            setattr(out, k, v)
        return out

    def resample(self, fnew, **kwargs):
        """Resample every mode to the rate ``fnew`` with a root-raised-cosine filter of symbol period ``Ts`` (default ``1 / fb``) on the GPU:
        :func:`qampy_amd.core.resample.rrcos_resample` with this signal's ``fs`` (behaviour of qampy/signals.py:223-243).  Keyword arguments
        are those of ``rrcos_resample`` (``beta``, ``taps``, ``renormalise``, ``fftconv``).  The symbols, the metadata and the class are
        kept and ``fs`` becomes ``fnew``; a ratio close to 1 returns a copy."""
        from .core import resample as _rs
        if np.isclose(fnew / self.fs, 1):
            out = self.recreate_from_np_array(np.array(self))
        else:
            Ts = kwargs.pop("Ts", 1 / self.fb)
            arr = _rs.rrcos_resample(np.asarray(self), self.fs, fnew, Ts=Ts, **kwargs)
            out = self.recreate_from_np_array(arr.astype(self.dtype, copy=False), fs=fnew)
        if self._symbols is not None:
            out._symbols = self._symbols.copy()
        return out

    # ---- signal-quality metrics (qampy/signals.py:245-560); rows of ``signal_rx`` are modes, results are per mode.  ``sync_method``: where
    # the alignment of an unsynchronised capture runs - "pyt": scipy on the host (the reference's), "hip": csrc/sync.hip on the device
    @property
    def Nbits(self):
        """Bits per symbol."""
        return int(np.log2(self.M))

    def _signal_present(self, signal):
        return np.atleast_2d(np.asarray(self if signal is None else signal))

    def _sync_and_adjust(self, tx, rx, synced=False, sync_method="pyt"):
        """Transmitted and received rows brought together (signals.py:245-266): unless ``synced``, every received mode takes
        the still unassigned transmitted mode with the largest correlation peak, rotated and rolled onto it
        (``ber_functions.sync_and_adjust``, on the host or - ``sync_method="hip"`` - on the device); ``synced``: only the lengths
        are adjusted."""
        if sync_method not in ("pyt", "hip"):
            raise ValueError("sync_method must be 'pyt' (host) or 'hip' (device), not %r" % (sync_method,))
        if tx is None:
            raise ValueError("no transmitted symbols attached")
        tx, rx = np.atleast_2d(tx), np.atleast_2d(rx)
        if synced:
            return self._adjust_only(tx, rx)
        free = list(range(max(tx.shape[0], rx.shape[0])))
        tx_out, rx_out = [], []
        for j in range(rx.shape[0]):
            best, pick = -100., None
            for i in free:
                pair, peak = ber_functions.sync_and_adjust(tx[i], rx[j], method=sync_method)
                if peak > best:
                    best, pick, chosen = peak, i, pair
            free.remove(pick)
            tx_out.append(chosen[0])
            rx_out.append(chosen[1])
        return np.array(tx_out), np.array(rx_out)

    @staticmethod
    def _adjust_only(tx, rx):
        """Lengths only (signals.py:268-292): modes beyond the received ones are dropped, tx cut or repeated to rx's length."""
        if tx.shape[0] > rx.shape[0]:
            tx = tx[:rx.shape[0]]
        if tx.shape == rx.shape:
            return tx, rx
        method = "truncate" if tx.shape[1] > rx.shape[1] else "extend"
        pairs = [ber_functions.adjust_data_length(t, r, method) for t, r in zip(tx, rx)]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])

    def make_decision(self, signal=None, verbose=False):
        """Nearest alphabet point per sample (signals.py:847-870); ``verbose``: also the distances and indices."""
        from .core.equalisation import hip_equalisation as hk
        signal = self._signal_present(signal)
        alphabet = np.ascontiguousarray(self.coded_symbols, dtype=signal.dtype)
        out = [hk.make_decision(np.ascontiguousarray(row), alphabet) for row in signal]
        det, dist, idx = (np.array([o[n] for o in out]) for n in range(3))
        return (det, dist, idx) if verbose else det

    def demodulate(self, symbols):
        """Bits ``(nmodes, N * Nbits)`` (MSB first per symbol) of integer labels or of the decisions of complex symbols."""
        symbols = np.atleast_2d(symbols)
        idx = symbols if np.issubdtype(symbols.dtype, np.integer) else self.make_decision(symbols, verbose=True)[2]
        shifts = np.arange(self.Nbits - 1, -1, -1)
        return ((idx[..., None].astype(np.int64) >> shifts) & 1).astype(bool).reshape(idx.shape[0], -1)

    def cal_ser(self, signal_rx=None, synced=False, verbose=False, sync_method="pyt"):
        """Symbol error rate per mode (signals.py:295-333); ``verbose``: also the error vector and the synchronised tx."""
        tx, rx = self._sync_and_adjust(self.symbols, self._signal_present(signal_rx), synced, sync_method)
        errs = self.make_decision(rx) - tx
        ser = np.count_nonzero(errs, axis=-1) / rx.shape[1]
        return (ser, errs, tx) if verbose else ser

    def cal_ber(self, signal_rx=None, synced=False, verbose=False, sync_method="pyt"):
        """Bit error rate per mode (signals.py:335-374); ``verbose``: also the bit errors and the synchronised tx bits."""
        tx, rx = self._sync_and_adjust(self.symbols, self._signal_present(signal_rx), synced, sync_method)
        rx_bits, tx_bits = self.demodulate(rx), self.demodulate(tx)
        errs = tx_bits ^ rx_bits
        ber = np.count_nonzero(errs, axis=-1) / rx_bits.shape[1]
        return (ber, errs, tx_bits) if verbose else ber

    def cal_evm(self, signal_rx=None, synced=False, blind=False, sync_method="pyt"):
        """RMS error vector magnitude per mode against the known symbols, or (``blind``) against the decisions
        (signals.py:376-421)."""
        rx = self._signal_present(signal_rx)
        if blind:
            tx = self.make_decision(rx)
        else:
            tx, rx = self._sync_and_adjust(self.symbols, rx, synced, sync_method)
        d = tx - rx
        return np.asarray(np.sqrt(np.mean(d.real ** 2 + d.imag ** 2, axis=-1)))

    def est_snr(self, signal_rx=None, synced=False, symbols_tx=None, verbose=False, sync_method="pyt"):
        """Linear SNR per mode from the known symbols (signals.py:423-455); ``verbose``: ``(snr, S0, N0)``."""
        from .core import hip_dsp
        tx, rx = self._sync_and_adjust(self.symbols if symbols_tx is None else symbols_tx, self._signal_present(signal_rx), synced, sync_method)
        est = np.array([hip_dsp.estimate_snr(np.ascontiguousarray(r), np.ascontiguousarray(t, dtype=r.dtype),
                                             np.ascontiguousarray(self.coded_symbols, dtype=r.dtype)) for r, t in zip(rx, tx)], dtype=np.float64)
        est = est.reshape(-1, 3)
        return (est[:, 0], est[:, 1], est[:, 2]) if verbose else est[:, 0]

    def normalize_and_center(self, symbol_based=False, synced=False):
        """Every mode minus its mean and scaled to unit power, in place (signals.py:549-568).  Plain: the mean power of the centred row, on the
        device (``row_moments_dev`` + ``center_scale_dev``).  ``symbol_based``: the signal power ``est_snr`` finds from the attached symbols
        (``synced`` as there) - what low SNRs need, where the mean power is mostly noise."""
        if not symbol_based:
            from . import _lib
            from .core import resample as _rs
            rows = np.atleast_2d(np.asarray(self))
            E = _lib.DeviceArray.from_host(rows if rows.dtype == np.complex64 else rows.astype(np.complex128))
            _rs.center_scale_dev(E, _rs.row_moments_dev(E), power=1.0)
            self[...] = E.to_host().reshape(self.shape)
        else:
            self -= np.asarray(self).mean(axis=-1)[:, None]
            p = self.est_snr(synced=synced, verbose=True)[1]
            for i in range(self.shape[0]):
                self[i] /= np.sqrt(p[i])

    def _snr_linear(self, snr, tx, rx):
        """Per-mode linear SNR: estimated on the aligned rows when ``snr`` is None, else ``snr`` in dB (one value or one per mode)."""
        if snr is None:
            return self.est_snr(rx, synced=True, symbols_tx=tx)
        snr = np.atleast_1d(snr)
        return np.ones(rx.shape[0]) * 10 ** (snr / 10) if snr.size != rx.shape[0] else 10 ** (snr / 10)

    def cal_gmi(self, signal_rx=None, synced=False, snr=None, llr_minmax=False, sync_method="pyt"):
        """``(GMI, GMI_per_bit)`` per mode from soft-decision LLRs (signals.py:457-508); ``snr`` in dB, estimated when None.
        One fused device pass per mode (``qh_metrics_*_dev``): the LLRs are never stored."""
        from . import _lib
        tx, rx = self._sync_and_adjust(self.symbols, self._signal_present(signal_rx), synced, sync_method)
        snr = self._snr_linear(snr, tx, rx)
        ct = rx.dtype
        alphabet = _lib.DeviceArray.from_host(np.ascontiguousarray(self.coded_symbols, dtype=ct))
        labels = self.make_decision(tx, verbose=True)[2].astype(np.int32)
        nb = self.Nbits
        per_bit = np.zeros((rx.shape[0], nb), dtype=np.float64)
        for m in range(rx.shape[0]):
            row = _lib.DeviceArray.from_host(np.ascontiguousarray(rx[m]))
            lab = _lib.DeviceArray.from_host(np.ascontiguousarray(labels[m]))
            counts, sums = np.zeros(3, np.int64), np.zeros(2 + nb, np.float64)
            _lib.call("qh_metrics_%s_dev" % ("c64" if ct == np.complex64 else "c128"), row.ptr, rx.shape[1], lab.ptr, rx.shape[1],
                      alphabet.ptr, alphabet.shape[0], 0, 0, 0, float(snr[m]), int(bool(llr_minmax)), _lib.ptr(counts), _lib.ptr(sums))
            per_bit[m] = 1 - sums[2:] / max(int(counts[2]), 1)
        return np.sum(per_bit, axis=-1), per_bit

    def cal_mi(self, signal_rx=None, synced=False, snr=None, fast=True, sync_method="pyt"):
        """Mutual information per mode (signals.py:510-548); ``snr`` in dB, estimated when None (then ``N0 = 1 / snr``)."""
        from .core import signal_quality
        tx, rx = self._sync_and_adjust(self.symbols, self._signal_present(signal_rx), synced, sync_method)
        N0 = 1 / self._snr_linear(snr, tx, rx)
        alphabet = np.ascontiguousarray(self.coded_symbols, dtype=rx.dtype)
        return np.array([signal_quality.cal_mi(np.ascontiguousarray(rx[m]), np.ascontiguousarray(tx[m], dtype=rx.dtype), alphabet, N0[m], fast)
                         for m in range(rx.shape[0])], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ bit sources and the Gray-coded signal
class RandomBits(np.ndarray):
    """
    ``RandomBits(N, nmodes=1, seed=None)``: bool array ``(nmodes, N)`` of ``np.random.RandomState(seed).randint(0, 2, (nmodes, N))`` - the
    reference's values (qampy/signals.py:53-86), drawn on the host (a Mersenne Twister is not worth a kernel).
    """

    def __new__(cls, N, nmodes=1, seed=None):
        state = np.random.RandomState(seed)
        obj = state.randint(0, high=2, size=(nmodes, N)).astype(bool).view(cls)
        obj._rand_state, obj._seed = state, seed
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        self._seed = getattr(obj, "_seed", None)
        self._rand_state = getattr(obj, "_rand_state", None)


class PRBSBits(np.ndarray):
    """
    ``PRBSBits(N, nmodes=1, seed=[None, None], order=[15, 23])``: bool array ``(nmodes, N)``, row ``i`` the external-XOR PRBS of ``order[i]``
    started from ``seed[i]`` (None: all ones) - qampy/signals.py:89-142 - generated on the device (``hip_dsp.prbs_bits_dev``).  When ``order``
    has fewer entries than ``nmodes`` a warning is given and the modes without an entry take a random order out of 15 and 23 and a random seed.
    """

    def __new__(cls, N, nmodes=1, seed=[None, None], order=[15, 23]):
        from . import _lib
        from .core import hip_dsp
        order, seed = list(order), list(seed)
        if len(order) < nmodes:
            warnings.warn("PRBSorder is not given for all dimensions, picking random orders and seeds")
            given = min(len(order), len(seed))
            order, seed = order[:given], seed[:given]
            for _ in range(given, nmodes):
                o = int(np.random.choice([15, 23]))
                order.append(o)
                seed.append(int(np.random.randint(0, 2 ** o)))
        N = int(N)
        d = _lib.DeviceArray((nmodes, N), np.uint8)
        for i in range(nmodes):
            hip_dsp.prbs_bits_dev(d.row(i), order[i], seed[i], kind="ext")
        obj = d.to_host().view(bool).view(cls)
        obj._order, obj._seed = order, seed
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        self._seed = getattr(obj, "_seed", None)
        self._order = getattr(obj, "_order", None)


def _check_dtype(dtype):
    assert dtype in [np.complex128, np.complex64], "only np.complex128 and np.complex64  or None dtypes are supported"


def _gray_alphabet(M, scale, dtype):
    """The constellation over ``scale`` in Gray-label order (``_generate_mapping``, qampy/signals.py:831-845)."""
    points = theory.cal_symbols_qam(M).astype(dtype)
    points /= scale
    code = theory.gray_code_qam(M)
    place = np.zeros_like(code)
    place[code] = np.arange(code.size)
    return points[place]


class SignalQAMGrayCoded(SignalQAM):
    """
    ``SignalQAMGrayCoded(M, N, nmodes=1, fb=1, bitclass=RandomBits, dtype=np.complex128, **kwargs)``: ``N`` Gray-coded M-QAM symbols per mode at
    one sample per symbol, made from the bits of ``bitclass(N * log2(M), nmodes=nmodes, **kwargs)`` (qampy/signals.py:611-675).  The mapping
    bits -> labels (MSB first) -> ``coded_symbols[label]`` runs on the device (``hip_dsp.modulate_bits_dev``); the values are the reference's.
    ``bits`` holds the bit array, ``symbols`` a copy of the signal; everything :class:`SignalQAM` offers is inherited.
    """

    def __new__(cls, M, N, nmodes=1, fb=1, bitclass=RandomBits, dtype=np.complex128, **kwargs):
        _check_dtype(dtype)
        coded = cls._alphabet(M, dtype)
        bits = bitclass(int(N * np.log2(M)), nmodes=nmodes, **kwargs)
        return cls._wrap(cls._modulate(bits, coded), M, fb, coded, bits)

    @classmethod
    def _alphabet(cls, M, dtype, power=None):
        """``coded_symbols`` of the class: the M-QAM constellation of mean power ``power`` (None: 1) in Gray-label order (``_generate_mapping``)."""
        scale = np.sqrt(theory.cal_scaling_factor_qam(M))
        return _gray_alphabet(M, scale if power is None else scale / np.sqrt(power), dtype)

    @classmethod
    def _wrap(cls, data, M, fb, coded, bits):
        obj = SignalQAM.__new__(cls, data, M, fb=fb, coded_symbols=coded)
        obj._bits = bits
        obj._symbols = np.array(obj)
        return obj

    def __array_finalize__(self, obj):
        super().__array_finalize__(obj)
        if obj is not None:
            self._bits = getattr(obj, "_bits", None)

    def recreate_from_np_array(self, arr, **kwargs):
        out = super().recreate_from_np_array(arr, **kwargs)
        out._bits = self._bits
        return out

    @staticmethod
    def _modulate(data, coded_symbols):
        """Rows of bits to rows of ``coded_symbols``, on the device; bits beyond the last whole symbol are left out (signals.py:705-731)."""
        from . import _lib
        from .core import hip_dsp
        data = np.atleast_2d(np.asarray(data))
        nb = int(np.log2(coded_symbols.shape[0]))
        nsym = data.shape[1] // nb
        if nsym < 1 or data.shape[0] < 1:
            return np.empty((data.shape[0], nsym), dtype=coded_symbols.dtype)
        if nb == 1:                          # two points (BPSK): a bit is its own label, and the device mapper starts at two bits per symbol
            return coded_symbols[(data != 0).astype(np.intp)]
        bits = _lib.DeviceArray.from_host(np.ascontiguousarray(data[:, :nsym * nb] != 0).view(np.uint8))
        out = _lib.DeviceArray((data.shape[0], nsym), coded_symbols.dtype)
        hip_dsp.modulate_bits_dev(bits, _lib.DeviceArray.from_host(np.ascontiguousarray(coded_symbols)), out)
        return out.to_host()

    @property
    def bits(self):
        return self._bits

    def modulate(self, data):
        """Modulate rows of bits into this signal's alphabet (a plain ``(nmodes, len // Nbits)`` array of the signal's dtype)."""
        return self._modulate(data, np.ascontiguousarray(self.coded_symbols, dtype=self.dtype))

    @classmethod
    def from_bit_array(cls, bits, M, fb=1, dtype=np.complex128):
        """A signal from a given 1-d or 2-d bit array (qampy/signals.py:784-829); a length that is no multiple of ``log2(M)`` is cut to one
        with a warning, and ``bits`` holds the bits that were modulated."""
        _check_dtype(dtype)
        arr = np.atleast_2d(bits)
        nb = int(np.log2(M))
        if arr.shape[1] % nb > 0:
            warnings.warn("Length of bits not divisible by log2(M) truncating")
            arr = arr[:, :arr.shape[1] // nb * nb]
        coded = cls._alphabet(M, dtype)
        return cls._wrap(cls._modulate(arr, coded), M, fb, coded, arr)

    @classmethod
    def from_symbol_array(cls, symbs, M=None, fb=1, dtype=None):
        """A signal from given symbols (qampy/signals.py:733-782): the alphabet scaled to the power of the distinct values of ``symbs``,
        decisions on it, then the decisions' bits - both on the device (what ``hip_dsp.demodulate_dev`` does, the decided symbols kept as
        the signal).  ``bits`` holds every mode's bits,
        ``(nmodes, N * log2(M))``."""
        from . import _lib
        from .core import hip_dsp
        from .core.equalisation import hip_equalisation as hk
        if dtype is not None:
            _check_dtype(dtype)
        symbs = np.atleast_2d(symbs)
        if M is None:
            warnings.warn("no M given, estimating how mnay unique symbols are in array, this can cause errors")
            M = np.unique(symbs).shape[0]
        if dtype is None:
            dtype = symbs.dtype
        P = (abs(np.unique(symbs)) ** 2).mean()
        if not np.isclose(P, 1):
            warnings.warn("Power of symbols is not normalized to 1, this might cause issues later")
        coded = cls._alphabet(M, dtype, power=(abs(np.unique(symbs)) ** 2).mean())
        nb = int(np.log2(M))
        E = _lib.DeviceArray.from_host(np.ascontiguousarray(symbs, dtype=dtype))
        alphabet = _lib.DeviceArray.from_host(np.ascontiguousarray(coded))
        det, labels = _lib.DeviceArray(E.shape, dtype), _lib.DeviceArray(E.shape, np.int32)
        bits = _lib.DeviceArray((E.shape[0], E.shape[1] * nb), np.uint8)
        hk.make_decision_dev(E, alphabet, det, None, labels)
        if nb == 1:                          # (a label of two points is its bit)
            return cls._wrap(det.to_host(), M, fb, coded, labels.to_host().astype(bool))
        hip_dsp.labels_to_bits_dev(labels, nb, bits)
        return cls._wrap(det.to_host(), M, fb, coded, bits.to_host().view(bool))


class SignalPSKGrayCoded(SignalQAMGrayCoded):
    """
    ``SignalPSKGrayCoded(M, N, nmodes=1, fb=1, bitclass=RandomBits, dtype=np.complex128, **kwargs)``: Gray-coded M-PSK symbols
    (qampy/signals.py:932-947).  ``coded_symbols[g]`` is the point of ``theory.cal_symbols_psk(M)`` whose binary-reflected Gray label is ``g``, so
    neighbours on the circle differ in one bit; bits map to labels MSB first, as in the QAM class, on the device.  Decisions and the ``cal_*``
    metrics run through the same nearest-point kernels: they take any alphabet.
    """

    @classmethod
    def _alphabet(cls, M, dtype, power=None):
        """The unit circle's points in Gray-label order; like the reference's mapping it ignores the power asked for."""
        points = theory.cal_symbols_psk(M).astype(dtype)
        n = np.arange(M)
        place = np.zeros(M, dtype=np.intp)
        place[n ^ (n >> 1)] = n
        return points[place]


class ResampledQAM(SignalQAMGrayCoded):
    """
    ``ResampledQAM(M, N, fb=1, fs=1, resamplekwargs={"beta": 0.1}, **kwargs)``: a :class:`SignalQAMGrayCoded` made at the symbol rate ``fb`` and
    resampled to ``fs`` with a root-raised-cosine filter (qampy/signals.py:1142-1178) - :meth:`SignalQAM.resample` with ``resamplekwargs`` on the
    GPU.  ``**kwargs`` go to :class:`SignalQAMGrayCoded`.  The default ``resamplekwargs`` leave the filter length to ``rrcos_resample``; its
    whole-row spectral form (``taps=None``) is not implemented.
    """

    def __new__(cls, M, N, fb=1, fs=1, resamplekwargs={"beta": 0.1}, **kwargs):
        return super().__new__(cls, M, N, fb=fb, **kwargs).resample(fs, **resamplekwargs)

    @classmethod
    def from_symbol_array(cls, array, fs, **kwargs):
        """``array`` (a signal object) resampled to ``fs``; ``**kwargs`` are those of ``rrcos_resample``.  The result keeps ``array``'s class."""
        return array.resample(fs, **kwargs)


# ------------------------------------------------------------------------------------------------ time-domain hybrid QAM
_TATTRS = ("_symbols_M1", "_symbols_M2", "_fr", "_powratio", "_power_method", "_fb", "_fs")


def _nearest(rows, alphabet):
    """Labels of the nearest point of ``alphabet`` per sample of the host rows, by squared distance in double, the first on a tie."""
    rows = np.atleast_2d(np.asarray(rows)).astype(np.complex128)
    a = np.asarray(alphabet).astype(np.complex128)
    out = np.empty(rows.shape, dtype=np.int32)
    for m, row in enumerate(rows):
        for lo in range(0, row.size, 1 << 14):
            d = row[lo:lo + (1 << 14), None] - a[None, :]
            out[m, lo:lo + (1 << 14)] = np.argmin(d.real ** 2 + d.imag ** 2, axis=1)
    return out


class TDHQAMSymbols(np.ndarray):
    """
    ``TDHQAMSymbols(M, N, fr=0.5, power_method="dist", M1class=SignalQAMGrayCoded, M2class=SignalQAMGrayCoded, **kwargs)``: time-domain hybrid
    QAM ``(nmodes, N)`` at one sample per symbol - two formats ``M = (M1, M2)`` interleaved in a fixed frame (qampy/signals.py:1182-1427).  With
    ``f_M, f_M1, f_M2`` of ``Fraction(fr).limit_denominator()``, position ``n`` carries format 1 when ``n % f_M < f_M1``, else format 2, whose
    symbols are divided by ``sqrt(powratio)`` so that both alphabets keep the same spacing (``power_method="dist"``).  ``N`` is cut to whole
    frames with a warning; ``**kwargs`` go to both part classes, as in the reference (two PRBS sources then start from the same bits).

    ``symbols_M1`` and ``symbols_M2`` are the parts as signal objects (``symbols_M2`` holds the scaled values, as the reference's does; its own
    ``symbols`` the unit-power ones).  The array values are the reference's, bit for bit.

    The reference stops there: its split and every ``cal_*`` raise.  Here :meth:`divide` aligns a received signal to the frame and takes it
    apart, and :meth:`cal_ser`, :meth:`cal_ber`, :meth:`cal_evm` and :meth:`cal_gmi` measure it per format and combined - ``method="pyt"`` in
    numpy, ``"hip"`` through csrc/hybrid.hip (DESIGN.md 3.21 has the semantics).
    """

    def __new__(cls, M, N, fr=0.5, power_method="dist", M1class=SignalQAMGrayCoded, M2class=SignalQAMGrayCoded, **kwargs):
        fM, fM1, fM2 = cls._cal_fractions(fr)
        frames = int(N) // fM
        if N % fM > 0:
            warnings.warn("length of overall pattern not divisable by number of frames, truncating to %d symbols" % (fM * frames))
        return cls._interleave(M1class(M[0], frames * fM1, **kwargs), M2class(M[1], frames * fM2, **kwargs), fr, power_method)

    @classmethod
    def _interleave(cls, syms1, syms2, fr, power_method):
        """The hybrid signal of two whole-frame parts; ``syms2`` is divided by ``sqrt(powratio)`` in place."""
        fM, fM1, fM2 = cls._cal_fractions(fr)
        scale = cls.calculate_power_ratio(syms1.coded_symbols, syms2.coded_symbols, power_method)
        syms2 /= np.sqrt(scale)
        N = syms1.shape[1] + syms2.shape[1]
        out = np.zeros((syms1.shape[0], N), dtype=syms1.dtype)
        _, idx1, idx2 = cls._cal_symbol_idx(N, fM, fM1)
        out[:, idx1] = syms1
        out[:, idx2] = syms2
        obj = out.view(cls)
        obj._symbols_M1, obj._symbols_M2, obj._powratio, obj._fr, obj._power_method = syms1, syms2, scale, fr, power_method
        obj._fb = obj._fs = syms1.fb
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        for a in _TATTRS:
            setattr(self, a, getattr(obj, a, None))

    @staticmethod
    def _cal_fractions(fr):
        from .core import hip_dsp
        return hip_dsp.tdh_geometry(fr)

    @staticmethod
    def _cal_symbol_idx(N, f_M, f_M1):
        idx = np.arange(N)
        return idx, idx % f_M < f_M1, idx % f_M >= f_M1

    @staticmethod
    def calculate_power_ratio(M1symbols, M2symbols, method="dist"):
        """Power ratio of two alphabets at equal spacing (``hip_dsp.tdh_power_ratio``); only ``"dist"`` exists."""
        from .core import hip_dsp
        return hip_dsp.tdh_power_ratio(M1symbols, M2symbols, method)

    powratio = property(lambda self: self._powratio)
    f_M = property(lambda self: self._cal_fractions(self.fr)[0])
    f_M1 = property(lambda self: self._cal_fractions(self.fr)[1])
    f_M2 = property(lambda self: self._cal_fractions(self.fr)[2])
    M = property(lambda self: (self._symbols_M1.M, self._symbols_M2.M))
    symbols_M1 = property(lambda self: self._symbols_M1)
    symbols_M2 = property(lambda self: self._symbols_M2)
    fr = property(lambda self: self._fr)
    fb = property(lambda self: self._fb)
    fs = property(lambda self: self._fs)
    os = property(lambda self: int(self.fs / self.fb))

    @classmethod
    def from_symbol_arrays(cls, syms_M1, syms_M2, fr, power_method="dist"):
        """A hybrid signal from two signal objects of one dtype and one number of modes (qampy/signals.py:1318-1366).  When the parts do not
        fill whole frames at the ratio ``fr`` a warning is given and each is cut to ``nframes * f_M1`` / ``nframes * f_M2`` symbols (the
        reference then fails on a shape mismatch).  The parts are copied: ``syms_M2`` itself is left unscaled."""
        assert syms_M1.ndim == 2 and syms_M2.ndim == 2, "input needs to have two dimensions"
        assert syms_M1.dtype == syms_M2.dtype, "both input symbol arrays need to have the same dtype"
        assert syms_M1.shape[0] == syms_M2.shape[0], "Number of modes must be the same"
        fM, fM1, fM2 = cls._cal_fractions(fr)
        N1, N2 = syms_M1.shape[1], syms_M2.shape[1]
        nframes = (N1 + N2) // fM
        if nframes * fM1 > N1 or nframes * fM2 > N2:
            warnings.warn("Need to truncate input arrays as ratio is not possible otherwise")
            nframes = min(N1 // fM1, N2 // fM2)
        return cls._interleave(cls._cut(syms_M1, nframes * fM1), cls._cut(syms_M2, nframes * fM2), fr, power_method)

    @staticmethod
    def _cut(sig, n):
        """A copy of the first ``n`` symbols of a part with its metadata (its ``symbols`` cut alike)."""
        out = sig.recreate_from_np_array(np.array(sig)[:, :n])
        if getattr(sig, "_symbols", None) is not None:
            out._symbols = np.array(sig._symbols)[:, :n]
        return out

    def recreate_from_np_array(self, arr, **kwargs):
        """Re-wrap a plain array with this signal's class and attributes."""
        out = np.atleast_2d(np.asarray(arr)).view(type(self))
        for a in _TATTRS:
            setattr(out, a, getattr(self, a))
        if "fb" in kwargs and "fs" not in kwargs:
            kwargs["fs"] = self.os * kwargs["fb"]
        for k, v in kwargs.items():
            setattr(out, "_" + k if "_" + k in _TATTRS else k, v)
        return out

    def _demodulate(self):
        raise NotImplementedError("Use demodulation of subclasses")

    def _modulate(self):
        raise NotImplementedError("Use modulation of subclasses")

    # ---- what the reference left unfinished (its _divide_signal_frame and every cal_* raise): DESIGN.md 3.21
    def _received(self, signal):
        rx = np.atleast_2d(np.asarray(self if signal is None else signal))
        if rx.shape[1] % self.f_M:
            raise ValueError("a row of %d symbols does not hold whole frames of %d" % (rx.shape[1], self.f_M))
        return rx

    def divide(self, signal=None, method="pyt", return_shifts=False):
        """``(part1, part2)`` of ``signal`` (default: this signal), as objects of the parts' classes carrying the transmitted parts as
        ``symbols``: every row is aligned to the frame - the cyclic shift at which the positions of the higher-order format have the largest
        mean magnitude - and split, part 2 times ``sqrt(powratio)``, back on its unit-power alphabet.  The split aligns the format, not the
        sequence.  ``method="hip"``: on the device (``hip_dsp.tdh_divide``); ``return_shifts``: also the shift per row."""
        from .core import hip_dsp
        p1, p2, shifts = hip_dsp.tdh_divide(self._received(signal), self.fr, self.M, self.powratio, method=method)
        parts = (self._symbols_M1.recreate_from_np_array(p1), self._symbols_M2.recreate_from_np_array(p2))
        return parts + (shifts,) if return_shifts else parts

    def _tx_labels(self, n1, n2):
        """Transmitted labels of the two parts, repeated or cut to ``n1`` / ``n2`` symbols."""
        out = []
        for part, n in ((self._symbols_M1, n1), (self._symbols_M2, n2)):
            lab = _nearest(part.symbols, part.coded_symbols)
            out.append(np.ascontiguousarray(np.tile(lab, (1, -(-n // lab.shape[1])))[:, :n]))
        return out

    def _hard_sums(self, signal_rx, synced, method):
        """The eight sums per mode, ``(nmodes, 2, 4)``: symbol errors, bit errors, compared, squared error of either format."""
        from . import _lib
        from .core import ber_functions as bf, hip_dsp
        if method not in ("pyt", "hip"):
            raise ValueError("method must be 'pyt' (host) or 'hip' (device), not %r" % (method,))
        rx = self._received(signal_rx)
        nm, L = rx.shape
        fM, fM1, fM2 = self._cal_fractions(self.fr)
        coded = [np.asarray(self._symbols_M1.coded_symbols), np.asarray(self._symbols_M2.coded_symbols)]
        if synced and method == "hip":
            ct = _lib.suffix(rx.dtype)[2]
            lab1, lab2 = self._tx_labels(L // fM * fM1, L // fM * fM2)
            idx = np.empty((nm, L), dtype=np.int32)
            _, i1, i2 = self._cal_symbol_idx(L, fM, fM1)
            idx[:, i1], idx[:, i2] = lab1[:nm], lab2[:nm]
            D = _lib.DeviceArray
            E = D.from_host(np.ascontiguousarray(rx, dtype=ct))
            shift = hip_dsp.tdh_align_dev(hip_dsp.tdh_class_sums_dev(E, fM), fM1, self.M)
            sums = hip_dsp.tdh_metrics_dev(E, D.from_host(idx), fM, fM1, self.powratio, D.from_host(np.ascontiguousarray(coded[0], dtype=ct)),
                                           D.from_host(np.ascontiguousarray(coded[1], dtype=ct)), shift)
            return sums.to_host().reshape(nm, 2, 4)
        parts = hip_dsp.tdh_divide(rx, self.fr, self.M, self.powratio, method=method)[:2]
        sums = np.zeros((nm, 2, 4))
        for k, (part, tx_part) in enumerate(zip(parts, (self._symbols_M1, self._symbols_M2))):
            a = coded[k].astype(np.complex128)
            tx_all = np.atleast_2d(np.asarray(tx_part.symbols))
            for m in range(nm):
                r = part[m]
                if synced:
                    t = np.tile(tx_all[m], -(-r.size // tx_all.shape[1]))[:r.size]
                else:
                    (t, r), _ = bf.sync_and_adjust(tx_all[m], r, method=method)
                lt, lr = _nearest(t, a)[0], _nearest(r, a)[0]
                d = r.astype(np.complex128) - a[lt]
                bit_errors = int(np.unpackbits((lt ^ lr).astype(">u4").view(np.uint8)).sum())
                sums[m, k] = (np.count_nonzero(lt != lr), bit_errors, r.size, np.sum(d.real ** 2 + d.imag ** 2))
        return sums

    def _rates(self, key, signal_rx, synced, method):
        from .core import hip_dsp
        return hip_dsp.tdh_rates(self._hard_sums(signal_rx, synced, method), self.M)[key]

    def make_decision(self, signal=None, method="pyt"):
        """The decisions of ``signal`` (default: this signal) in the hybrid layout: the rows aligned and split (:meth:`divide`), every part
        decided on its own alphabet, and the decisions interleaved again, format 2 over ``sqrt(powratio)``."""
        p1, p2 = self.divide(signal, method=method)
        d1 = np.asarray(p1.coded_symbols)[_nearest(p1, p1.coded_symbols)].astype(p1.dtype)
        d2 = (np.asarray(p2.coded_symbols)[_nearest(p2, p2.coded_symbols)] * (1 / np.sqrt(self.powratio))).astype(p2.dtype)
        out = np.empty((d1.shape[0], d1.shape[1] + d2.shape[1]), dtype=d1.dtype)
        _, i1, i2 = self._cal_symbol_idx(out.shape[1], self.f_M, self.f_M1)
        out[:, i1], out[:, i2] = d1, d2
        return out

    def cal_ser(self, signal_rx=None, synced=True, method="pyt"):
        """Symbol error rate ``(per format (nmodes, 2), combined (nmodes,))`` of ``signal_rx`` (default: this signal) against the transmitted
        parts.  The rows are aligned to the frame first; ``synced=False``: every part is then synchronised to its transmitted part
        (``ber_functions.sync_and_adjust``).  ``method="hip"``: alignment and the fused metrics pass on the device, eight sums come back;
        with ``synced=False`` the split and the synchronisation run on the device and the synchronised parts are counted on the host."""
        return self._rates("ser", signal_rx, synced, method)

    def cal_ber(self, signal_rx=None, synced=True, method="pyt"):
        """Bit error rate, as :meth:`cal_ser`; the combined rate is weighted by bits, ``(b1 + b2) / (n1 log2 M1 + n2 log2 M2)``."""
        return self._rates("ber", signal_rx, synced, method)

    def cal_evm(self, signal_rx=None, synced=True, method="pyt"):
        """RMS error vector magnitude against the transmitted symbols, as :meth:`cal_ser`; format 2 after its rescale to unit power."""
        return self._rates("evm", signal_rx, synced, method)

    def cal_gmi(self, signal_rx=None, synced=True, snr=None, method="pyt"):
        """Generalised mutual information ``(per format (nmodes, 2), combined (nmodes,))`` in bits per symbol: the signal is split and every
        part goes through its class's ``cal_gmi`` (one fused device pass per mode); the combined value weights the formats by their share of
        the frame.  ``snr``: Es / N0 of the hybrid signal in dB, turned into each format's own - format 1 has the power ``1 / mix`` of the mean,
        format 2 after its rescale ``1 / (powratio mix)``, ``mix = f_M1 / f_M + f_M2 / (f_M powratio)`` - or None: estimated per part."""
        p1, p2 = self.divide(signal_rx, method=method)
        fM, fM1, fM2 = self._cal_fractions(self.fr)
        own = (None, None)
        if snr is not None:
            powratio = float(self.powratio)               # (a complex64 signal carries it in single precision)
            mix = fM1 / fM + fM2 / fM / powratio
            own = (np.asarray(snr) - 10 * np.log10(mix), np.asarray(snr) - 10 * np.log10(mix * powratio))
        gmi = np.stack([p.cal_gmi(synced=synced, snr=s)[0] for p, s in zip((p1, p2), own)], axis=1)
        return gmi, (gmi[:, 0] * fM1 + gmi[:, 1] * fM2) / fM


# ------------------------------------------------------------------------------------------------ pilot frames
_PATTRS = ("_M", "_fb", "_fs", "_coded_symbols", "_symbols", "_pilots", "_frame_len", "_pilot_seq_len", "_pilot_ins_rat",
           "_idx_dat", "_idx_pil", "_Mpilots", "_shiftfctrs", "_synctaps", "_foe")


class PilotSignal(np.ndarray):
    """
    Pilot-frame capture ``(nmodes, nsamples)``: the attributes of ``qampy.signals.SignalWithPilots`` that the pilot receiver
    reads (qampy/signals.py:1430-1760) - frame geometry, pilot sequence / phase pilots, ``shiftfctrs`` / ``synctaps`` after
    :meth:`sync2frame` - on a plain ndarray subclass.  A frame is ``pilot_seq_len`` pilot symbols followed by payload with
    one phase pilot every ``pilot_ins_rat`` symbols (:1532-1545).  Build one from arrays (a received capture plus the known
    pilots); :class:`SignalWithPilots` generates such a signal.

    Parameters
    ----------
    data : (nmodes, N) complex samples
    M : payload QAM order;  fb, fs : symbol / sampling rate
    frame_len, pilot_seq_len, pilot_ins_rat : frame geometry in symbols
    pilots : (nmodes, >= n_pilots_per_frame) complex, pilot sequence first then the phase pilots
    symbols : (nmodes, n_payload_per_frame) transmitted payload (optional, SER only);  Mpilots : pilot QAM order
    """

    def __new__(cls, data, M, fb, fs, frame_len, pilot_seq_len, pilot_ins_rat, pilots, symbols=None, Mpilots=4,
                coded_symbols=None):
        obj = np.atleast_2d(np.asarray(data)).view(cls)
        if not np.iscomplexobj(obj):
            raise ValueError("PilotSignal needs a complex array")
        obj._M, obj._fb, obj._fs, obj._Mpilots = int(M), fb, fs, int(Mpilots)
        obj._frame_len, obj._pilot_seq_len, obj._pilot_ins_rat = int(frame_len), int(pilot_seq_len), pilot_ins_rat
        idx, obj._idx_dat, obj._idx_pil = cls._cal_pilot_idx(frame_len, pilot_seq_len, pilot_ins_rat)
        obj._pilots = np.atleast_2d(np.asarray(pilots))
        if obj._pilots.shape[1] < np.count_nonzero(obj._idx_pil):
            raise ValueError("a frame holds %d pilots, got %d" % (np.count_nonzero(obj._idx_pil), obj._pilots.shape[1]))
        obj._symbols = None if symbols is None else np.atleast_2d(np.asarray(symbols))
        obj._coded_symbols = theory.coded_symbols_qam(M, dtype=obj.dtype) if coded_symbols is None else np.asarray(coded_symbols)
        obj._shiftfctrs = obj._synctaps = None
        obj._foe = 0
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        for a in _PATTRS:
            setattr(self, a, getattr(obj, a, None))

    @staticmethod
    def _cal_pilot_idx(frame_len, pilot_seq_len, pilot_ins_rat):
        """Positions of pilots / payload inside a frame (behaviour of qampy/signals.py:1532-1545)."""
        where = np.arange(frame_len)
        behind = where - pilot_seq_len                   # position counted from the end of the pilot sequence
        idx_pil = behind < 0
        if pilot_ins_rat:
            if (frame_len - pilot_seq_len) % pilot_ins_rat:
                raise ValueError("Frame without pilot sequence divided by pilot rate needs to be an integer")
            idx_pil = idx_pil | (behind % pilot_ins_rat == 0)
        idx = where
        return idx, ~idx_pil, idx_pil

    M = property(lambda self: self._M)
    Mpilots = property(lambda self: self._Mpilots)
    fb = property(lambda self: self._fb)
    fs = property(lambda self: self._fs)
    os = property(lambda self: int(self.fs / self.fb))
    coded_symbols = property(lambda self: self._coded_symbols)
    symbols = property(lambda self: self._symbols)
    pilots = property(lambda self: self._pilots)
    pilot_seq = property(lambda self: self._pilots[:, :self._pilot_seq_len])
    ph_pilots = property(lambda self: self._pilots[:, self._pilot_seq_len:])
    frame_len = property(lambda self: self._frame_len)
    nframes = property(lambda self: self.shape[-1] // (self.os * self.frame_len))
    idx_payload = property(lambda self: np.tile(self._idx_dat, self.nframes)[:self.shape[-1]])
    idx_pilots = property(lambda self: np.tile(~self._idx_dat, self.nframes)[:self.shape[-1]])

    @property
    def shiftfctrs(self):
        return self._shiftfctrs

    @shiftfctrs.setter
    def shiftfctrs(self, value):
        self._shiftfctrs = value

    @property
    def synctaps(self):
        return self._synctaps

    @synctaps.setter
    def synctaps(self, value):
        self._synctaps = value

    def recreate_from_np_array(self, arr, **kwargs):
        out = np.atleast_2d(np.asarray(arr)).view(type(self))
        for a in _PATTRS:
            setattr(out, a, getattr(self, a))
        if "fb" in kwargs and "fs" not in kwargs:
            kwargs["fs"] = self.os * kwargs["fb"]
        for k, v in kwargs.items():
            setattr(out, "_" + k if "_" + k in _PATTRS else k, v)
        return out

    def sync2frame(self, returntaps=False, **kwargs):
        """Find the start of the pilot sequence per mode, reorder the modes accordingly and store ``shiftfctrs`` /
        ``synctaps`` (behaviour of qampy/signals.py:1709-1745; all search windows train in ONE launch)."""
        from .core import pilotbased_receiver
        search = dict(adaptive_stepsize=True, Niter=10, method="cma", Ntaps=17, mu=5e-3)
        search.update(kwargs)
        ntaps = search.pop("Ntaps")
        shift, foe, order, taps, found = pilotbased_receiver.frame_sync(np.asarray(self), np.asarray(self.pilot_seq), self.os, frame_len=self.frame_len,
                                                                        M_pilot=self.Mpilots, Ntaps=ntaps, **search)
        period = self.frame_len * self.os                 # shifts are positions inside one frame period
        self[:, :] = np.asarray(self)[order, :]
        self.shiftfctrs = np.where(np.asarray(shift) < 0, np.asarray(shift) + period, shift)[order]
        self.synctaps, self._foe = ntaps, foe
        return (taps, found) if returntaps else found

    def corr_foe(self, additional_foe=0):
        """Remove the coarse frequency offset found by :meth:`sync2frame` (qampy/signals.py:1747-1750)."""
        from .core import phaserecovery
        foe_off = np.ones(np.asarray(self._foe).shape) * (np.mean(self._foe) + additional_foe)
        self._foe = 0
        self[:, :] = phaserecovery.comp_freq_offset(np.asarray(self), foe_off, self.os)

    def _frame_mask(self, per_frame, frames):
        frames = np.arange(self.nframes) if frames is None else np.atleast_1d(frames)
        idx = np.zeros(self.shape[-1], dtype=bool)
        for i in frames:
            idx[i * self.frame_len:(i + 1) * self.frame_len] = per_frame[:max(0, min(self.frame_len, self.shape[-1] - i * self.frame_len))]
        return idx

    def _split_dev(self, frames, pilots):
        """Payload or pilots of whole frames through ``hip_dsp.pilot_split_dev`` - the host mask's result: frames in ascending order, each
        once.  None when the request is not one of whole frames of a complex64 / complex128 signal (the caller then takes the host path)."""
        from . import _lib
        from .core import hip_dsp
        F, L = self.frame_len, self.shape[-1]
        fr = np.arange(self.nframes) if frames is None else np.unique(np.atleast_1d(frames))
        if fr.size == 0 or not np.issubdtype(fr.dtype, np.integer) or fr.min() < 0 or (fr.max() + 1) * F > L:
            return None
        if self.dtype not in (np.complex64, np.complex128) or self.ndim != 2:
            return None
        count = hip_dsp.pilot_counts(F, self._pilot_seq_len, self._pilot_ins_rat)[0 if pilots else 1]
        if count < 1:
            return None
        E = _lib.DeviceArray.from_host(np.ascontiguousarray(np.asarray(self)))
        out = _lib.DeviceArray((self.shape[0], fr.size * count), self.dtype)
        hip_dsp.pilot_split_dev(E, F, self._pilot_seq_len, self._pilot_ins_rat, fr, **{"pilots" if pilots else "payload": out})
        return out.to_host()

    def _split(self, per_frame, frames, method, pilots):
        if method not in ("pyt", "hip"):
            raise ValueError("method must be 'pyt' (host) or 'hip' (device), not %r" % (method,))
        out = self._split_dev(frames, pilots) if method == "hip" else None
        return np.asarray(self)[:, self._frame_mask(per_frame, frames)].copy() if out is None else out

    def get_data(self, frames=None, method="pyt"):
        """Payload symbols of a frame-aligned, 1 sample/symbol signal (qampy/signals.py:1753-1781).  ``method="hip"``: gathered on the
        device (whole frames; a truncated last frame takes the host path)."""
        return self._split(self._idx_dat, frames, method, False)

    def extract_pilots(self, frames=None, method="pyt"):
        """Pilot symbols of a frame-aligned, 1 sample/symbol signal (qampy/signals.py:1783-1804); ``method`` as in :meth:`get_data`."""
        return self._split(self._idx_pil, frames, method, True)

    def cal_ser(self, frames=None):
        """Symbol error rate of the payload against ``symbols`` (aligned by construction once the frame is synced)."""
        from . import synth
        if self._symbols is None:
            raise ValueError("no transmitted payload attached")
        frames = np.arange(self.nframes) if frames is None else np.atleast_1d(frames)
        rx = self.get_data(frames)
        tx = np.tile(self._symbols, len(frames))
        return np.array([np.mean(synth.decide(r, self._coded_symbols) != synth.decide(t[:r.size], self._coded_symbols)) for r, t in zip(rx, tx)])

    # ---- metrics of the payload (qampy/signals.py:1834-1950): a SignalQAM of the payload against the tiled transmitted payload
    def _payload(self, frames=None):
        if self._symbols is None:
            raise ValueError("no transmitted payload attached")
        frames = np.arange(self.nframes) if frames is None else np.atleast_1d(frames)
        rx = self.get_data(frames)
        tx = np.tile(self._symbols, len(frames))[:, :rx.shape[1]]
        return SignalQAM(rx, self.M, fb=self.fb, fs=self.fb, symbols=tx, coded_symbols=self._coded_symbols)

    def _pilot_signal(self, frames=None):
        """The pilots as a SignalQAM of the pilot alphabet; the transmitted pilots are taken as their nearest pilot point."""
        from . import synth
        frames = np.arange(self.nframes) if frames is None else np.atleast_1d(frames)
        rx = self.extract_pilots(frames)
        alphabet = theory.coded_symbols_qam(self.Mpilots, dtype=rx.dtype)
        npil = np.count_nonzero(self._idx_pil)
        tx = np.tile(alphabet[np.array([synth.decide(p, alphabet) for p in self._pilots[:, :npil]])], len(frames))[:, :rx.shape[1]]
        return SignalQAM(rx, self.Mpilots, fb=self.fb, fs=self.fb, symbols=tx, coded_symbols=alphabet)

    def cal_ber(self, frames=None, synced=True, signal_rx=None, verbose=False):
        """Bit error rate per mode of the payload (signals.py:1834-1860)."""
        return self._payload(frames).cal_ber(signal_rx, synced=synced, verbose=verbose)

    def cal_evm(self, frames=None, synced=True, signal_rx=None, blind=False):
        """EVM per mode of the payload (signals.py:1862-1890)."""
        return self._payload(frames).cal_evm(signal_rx, synced=synced, blind=blind)

    def cal_gmi(self, frames=None, synced=True, snr=None, signal_rx=None, use_pilot_snr=False):
        """``(GMI, GMI_per_bit)`` of the payload (signals.py:1892-1925); ``use_pilot_snr``: at the SNR estimated on the pilots
        (converted to dB, the unit ``snr`` is taken in)."""
        assert not (use_pilot_snr and snr is not None), "use_pilot_snr must not be True if snr is not None"
        if use_pilot_snr:
            snr = 10 * np.log10(self.est_snr(use_pilots=True))
        return self._payload(frames).cal_gmi(signal_rx, synced=synced, snr=snr)

    def est_snr(self, frames=None, synced=True, signal_rx=None, symbols_tx=None, use_pilots=False):
        """Linear SNR per mode from the payload, or (``use_pilots``) from the pilots (signals.py:1927-1950)."""
        sig = self._pilot_signal(frames) if use_pilots else self._payload(frames)
        return sig.est_snr(signal_rx, synced=synced, symbols_tx=symbols_tx)


class SignalWithPilots(PilotSignal):
    """
    ``SignalWithPilots(M, frame_len, pilot_seq_len, pilot_ins_rat, nframes=1, pilot_scale=1, Mpilots=4, dataclass=SignalQAMGrayCoded, nmodes=1,
    dtype=np.complex128, repeat_data=True, repeat_pilots=True, **kwargs)``: ``nframes`` pilot frames ``(nmodes, nframes * frame_len)`` at one
    sample per symbol (qampy/signals.py:1430-1530).  Pilots - ``SignalQAMGrayCoded(Mpilots, NP, ...)`` times ``pilot_scale`` - and payload -
    ``dataclass(M, ND, ...)``, or ``nframes * ND`` symbols without ``repeat_data`` - are made on the device by :class:`SignalQAMGrayCoded` with
    ``**kwargs`` handed to both, as in the reference (so two PRBS sources start from the same bits), and laid out as frames in one launch
    (``hip_dsp.pilot_frame_dev``).  ``pilots`` and ``symbols`` hold what the reference's hold: the scaled pilots and the payload, repeated
    ``nframes`` times.  ``pilot_ins_rat`` 0 or None: a sequence only; ``pilot_seq_len`` 0: position 0 is a phase pilot.
    ``repeat_pilots=False`` raises ``ValueError`` (the reference fails on it).  Everything :class:`PilotSignal` offers is inherited.
    """

    def __new__(cls, M, frame_len, pilot_seq_len, pilot_ins_rat, nframes=1, pilot_scale=1, Mpilots=4, dataclass=SignalQAMGrayCoded, nmodes=1,
                dtype=np.complex128, repeat_data=True, repeat_pilots=True, **kwargs):
        from .core import hip_dsp
        _check_dtype(dtype)
        if not repeat_pilots:
            raise ValueError("repeat_pilots=False is not supported (the reference fails on it: its pilots then fill one frame only)")
        NP, ND = hip_dsp.pilot_counts(frame_len, pilot_seq_len, pilot_ins_rat)
        if int(nframes) != nframes or nframes < 1:
            raise ValueError("nframes must be a positive whole number")
        nframes = int(nframes)
        if NP < 1 or ND < 1:
            raise ValueError("a frame needs at least one pilot and one payload symbol")
        pilots = SignalQAMGrayCoded(Mpilots, NP, nmodes=nmodes, dtype=dtype, **kwargs)
        symbs = dataclass(M, ND if repeat_data else ND * nframes, nmodes=nmodes, dtype=dtype, **kwargs)
        frame = cls._assemble(np.asarray(pilots), np.asarray(symbs), frame_len, pilot_seq_len, pilot_ins_rat, nframes, pilot_scale, repeat_data)
        if repeat_data:
            symbs = np.tile(symbs, (1, nframes))
        fb = kwargs["fb"] if "fb" in kwargs else symbs.fb
        fs = kwargs["fs"] if "fs" in kwargs else symbs.fb
        pilots = np.tile(pilots * pilot_scale, (1, nframes))
        obj = PilotSignal.__new__(cls, frame, M, fb, fs, frame_len, pilot_seq_len, pilot_ins_rat, pilots, symbols=symbs, Mpilots=Mpilots,
                                  coded_symbols=symbs.coded_symbols)
        obj._symbols, obj._pilots = symbs, pilots        # (the signal objects themselves, as in the reference)
        obj._pilot_scale = pilot_scale
        return obj

    def __array_finalize__(self, obj):
        super().__array_finalize__(obj)
        if obj is not None:
            self._pilot_scale = getattr(obj, "_pilot_scale", None)

    def recreate_from_np_array(self, arr, **kwargs):
        out = super().recreate_from_np_array(arr, **kwargs)
        out._pilot_scale = self._pilot_scale
        return out

    pilot_scale = property(lambda self: self._pilot_scale)

    @staticmethod
    def _assemble(pilots, payload, frame_len, pilot_seq_len, pilot_ins_rat, nframes, pilot_scale, repeat_data):
        """The frames ``(nmodes, nframes * frame_len)`` of ``payload``'s dtype from host rows of pilots and payload, on the device.  The pilots
        times ``pilot_scale`` are what numpy's product, stored into an array of that dtype, holds: a scale numpy keeps in the array's
        precision is rounded to it first; the product is then formed in double and rounded once."""
        from . import _lib
        from .core import hip_dsp
        dtype = payload.dtype
        if np.iscomplexobj(pilot_scale) or np.ndim(pilot_scale) != 0:
            raise ValueError("pilot_scale must be one real number")
        scale = float(pilot_scale)
        if (np.zeros(1, dtype) * pilot_scale).dtype == dtype:
            scale = float(np.zeros(1, dtype).real.dtype.type(scale))
        D = _lib.DeviceArray
        frame = D((payload.shape[0], nframes * int(frame_len)), dtype)
        hip_dsp.pilot_frame_dev(D.from_host(np.ascontiguousarray(pilots, dtype=dtype)), D.from_host(np.ascontiguousarray(payload)), frame_len, pilot_seq_len,
                                pilot_ins_rat, nframes, frame, pilot_scale=scale, repeat_data=repeat_data)
        return frame.to_host()

    @classmethod
    def from_symbol_array(cls, payload, frame_len, pilot_seq_len, pilot_ins_rat, pilots=None, pilot_idx=None, nframes=1, pilot_scale=1,
                          payload_is_frame=False, pilot_class=SignalQAMGrayCoded, pilot_kwargs={"M": 4}, payload_class=SignalQAMGrayCoded,
                          payload_kwargs={}, **kwargs):
        """
        Pilot frames around a given payload (qampy/signals.py:1547-1645): ``payload (nmodes, >= ND)`` - an array or a signal object; with
        ``payload_is_frame`` a whole frame, whose pilot positions become the pilots -, ``pilots`` an array or signal object of ``nmodes``
        modes or of one, which is then used for all (None: ``pilot_class(pilot_kwargs["M"], NP, ...) / sqrt(pilot_scale)``, as the reference
        makes them).  Arrays become signal objects through ``from_symbol_array`` of ``pilot_class`` / ``payload_class`` with ``pilot_kwargs`` /
        ``payload_kwargs`` and ``**kwargs``.  The frame is repeated ``nframes`` times; ``symbols`` holds the ``ND`` payload symbols of one frame.
        ``pilot_idx`` (free pilot positions) raises ``NotImplementedError``: only the rule geometry is supported.
        """
        from .core import hip_dsp
        if pilot_idx is not None:
            raise NotImplementedError("pilot_idx (free pilot positions) is not implemented: frames follow pilot_seq_len and pilot_ins_rat")
        nmodes, N = payload.shape
        NP, ND = hip_dsp.pilot_counts(frame_len, pilot_seq_len, pilot_ins_rat)
        if int(nframes) != nframes or nframes < 1:
            raise ValueError("nframes must be a positive whole number")
        if NP < 1 or ND < 1:
            raise ValueError("a frame needs at least one pilot and one payload symbol")
        assert ND <= N, "data frame is to short for the given frame length"
        pilot_kwargs, payload_kwargs = dict(pilot_kwargs), dict(payload_kwargs)
        if "M" in kwargs:
            assert "M" not in payload_kwargs, "M can not be provided as a argument for payload and signal"
            payload_kwargs["M"] = kwargs.pop("M")
        if payload_is_frame:
            idx_pil, idx_dat = hip_dsp.pilot_positions(frame_len, pilot_seq_len, pilot_ins_rat)
            pilots = pilot_class.from_symbol_array(np.asarray(payload)[:, idx_pil], **pilot_kwargs, **kwargs)
            payload = payload_class.from_symbol_array(np.asarray(payload)[:, idx_dat], **payload_kwargs, **kwargs)
        if pilots is None:
            pilots = pilot_class(pilot_kwargs["M"], NP, nmodes=nmodes, dtype=payload.dtype, **kwargs) / np.sqrt(pilot_scale)
        else:
            if pilots.shape[0] not in (1, nmodes):
                raise ValueError("Pilots need to have the same number of modes as data or be one mode")
            if pilots.shape[0] == 1 and nmodes > 1:
                pilots = np.array(np.vstack([pilots] * nmodes))
            if not isinstance(pilots, SignalQAM):
                pilots = pilot_class.from_symbol_array(pilots, **pilot_kwargs, **kwargs)
        if not isinstance(payload, SignalQAM):
            payload = payload_class.from_symbol_array(payload, **payload_kwargs, **kwargs)
        _check_dtype(payload.dtype)
        if pilots.shape[1] != NP:
            raise ValueError("a frame holds %d pilots, got %d" % (NP, pilots.shape[1]))
        frame = cls._assemble(np.asarray(pilots), np.asarray(payload)[:, :ND], frame_len, pilot_seq_len, pilot_ins_rat, int(nframes), 1, True)
        obj = PilotSignal.__new__(cls, frame, payload.M, payload.fb, payload.fb, frame_len, pilot_seq_len, pilot_ins_rat, pilots,
                                  symbols=payload[:, :ND].copy(), Mpilots=pilots.M, coded_symbols=payload.coded_symbols)
        obj._symbols, obj._pilots = payload[:, :ND].copy(), pilots
        obj._pilot_scale = pilot_scale
        return obj
