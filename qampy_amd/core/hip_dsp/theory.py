"""
Theory curves: the last loop of pythran_dsp without a device form, cal_gmi_mc (qampy/core/pythran_dsp.py:181-197, behind
qampy.theory.cal_gmi), and the shaped source of qampy.theory.generate_ps_symbols; kernels in csrc/metrics.hip (awgn_mc_*) and
csrc/source.hip (ps_symbols_kernel).
"""
import numpy as np

from ... import _lib
from ._args import buffer, field, seed64
from .metrics import bits_map_labels

MC_TILE = 256                      # (sent point, draw) pairs per workgroup of the Monte-Carlo kernel (csrc/metrics.hip MET_THREADS)
MC_TRIP = 1024 * MC_TILE           # pairs of one SNR point the capped grid covers in one trip (MET_MAXBLK workgroups)
MC_NSNR_MAX = 65535                # SNR points of one launch
MC_NS_MAX = 2 ** 31                # draws per SNR point
PS_TILE = 1024                     # samples of one mode per workgroup of the shaped source (csrc/source.hip PS_TILE)
PS_LMAX = 64                       # most levels of a rail
PS_ROW_MAX = 2 ** 31               # most samples of a row of the shaped source: one workgroup per tile, no stride (csrc/source.hip SRC_NMAX)


def fresh_seed():
    """A 64-bit seed from the operating system's entropy: what ``seed=None`` means to the Monte-Carlo curves and the shaped source."""
    import os
    return int.from_bytes(os.urandom(8), "little")


def _mc_seed(seed):
    return fresh_seed() if seed is None else seed64(seed)


def _mc_snr(snr, what):
    """The linear SNR points as a contiguous 1-d float64 host array, every one finite and positive."""
    s = np.atleast_1d(np.asarray(snr, dtype=np.float64))
    if s.ndim != 1 or not 1 <= s.size <= MC_NSNR_MAX:
        raise ValueError("%s: between 1 and %d SNR points in one array" % (what, MC_NSNR_MAX))
    if not np.all(np.isfinite(s) & (s > 0)):
        raise ValueError("%s: every linear SNR must be finite and positive" % what)
    return np.ascontiguousarray(s)


def _mc_snr_dev(snr, what):
    """``snr`` on the device: a 1-d float64 DeviceArray as it is (its values are the caller's business), host values checked and uploaded."""
    if hasattr(snr, "ptr"):
        if len(snr.shape) != 1 or np.dtype(snr.dtype) != np.float64 or not 1 <= snr.shape[0] <= MC_NSNR_MAX:
            raise TypeError("%s: snr on the device must be a 1-d float64 DeviceArray of at most %d points" % (what, MC_NSNR_MAX))
        return snr, None
    host = _mc_snr(snr, what)
    return None, host


def _mc_draws(z, nsnr, what):
    """``c`` of the draws, ``(nsnr, ns)`` with ``1 <= ns <= 2**31``."""
    return field(z, what, "z", rows=nsnr, max_len=MC_NS_MAX)[0]


def awgn_mc_noise_dev(z, snr, seed):
    """The Monte-Carlo noise of :func:`awgn_mc_dev` into the ``(nsnr, ns)`` complex DeviceArray ``z``: ``z[p, l] = (g0 + 1j g1) sqrt(1 / (2 snr[p]))``
    with ``(g0, g1)`` the two standard normals of Philox counter ``(l, p, stream 3)`` under ``seed`` - what ``cal_gmi_mc`` draws with
    ``np.random.randn``, here a function of ``(seed, p, l)`` alone, every SNR point with draws of its own.  ``snr``: the linear SNRs, host values
    or a float64 DeviceArray; ``seed=None``: a fresh one.  Nothing is read back.  With ``snr`` on the device the call only enqueues one launch;
    host values go up in a temporary buffer whose release, when the call returns, waits for the device - keep a DeviceArray of the SNRs to stay
    asynchronous."""
    dev, host = _mc_snr_dev(snr, "awgn_mc_noise_dev")
    nsnr = dev.shape[0] if host is None else host.size
    c = _mc_draws(z, nsnr, "awgn_mc_noise_dev")
    seed = _mc_seed(seed)
    if dev is None:
        dev = _lib.DeviceArray.from_host(host)
    _lib.call("qh_awgn_mc_noise_%s_dev" % c, z.ptr, dev.ptr, nsnr, z.shape[1], seed)
    return z


def awgn_mc_dev(alphabet, snr, z, out):
    """Monte-Carlo GMI and MI of ``alphabet`` (``M = 2**nbits`` points in label order, a complex DeviceArray) over AWGN at every linear SNR of
    ``snr`` with the draws ``z`` ``(nsnr, ns)`` of the alphabet's dtype: ``out`` ``(nsnr, 2 + nbits)`` float64 DeviceArray receives ``[gmi, mi,
    gmi of bit 0 .. nbits - 1]`` per point, ``gmi`` what ``pythran_dsp.cal_gmi_mc`` returns for the draws ``z[p]`` and ``mi`` what
    ``cal_mi_mc(z[p], alphabet, 1 / snr[p])`` returns, from one pass (``M**2 ns`` exponentials per point).  All points in one launch of the kernel
    (three launches with the two reductions; beyond 32 MiB of workgroup partials - hundreds of points - in batches of that size); nothing is read
    back; a repeated call is bit-identical.  ``snr`` as host values is uploaded to a temporary buffer whose release waits for the device when the
    call returns: pass a float64 DeviceArray to only enqueue.  The partials live in the calling thread's scratch, which ``cal_metrics_dev`` uses
    too: on two library streams of one thread (``_lib.on_stream``) the two must be ordered by the caller."""
    c, _, M = field(alphabet, "awgn_mc_dev", "alphabet", ndim=(1,))
    nb = int(round(np.log2(M))) if M >= 1 else 0
    if 2 ** nb != M or not 1 <= nb <= 10:
        raise ValueError("awgn_mc_dev: the alphabet must have 2**nbits points, nbits in 1..10, got %d" % M)
    dev, host = _mc_snr_dev(snr, "awgn_mc_dev")
    nsnr = dev.shape[0] if host is None else host.size
    if _mc_draws(z, nsnr, "awgn_mc_dev") != c:
        raise TypeError("awgn_mc_dev: z and the alphabet must have one dtype")
    buffer(out, "awgn_mc_dev", "out", (nsnr, 2 + nb), np.float64)
    if dev is None:
        dev = _lib.DeviceArray.from_host(host)
    _lib.call("qh_awgn_mc_%s_dev" % c, alphabet.ptr, M, dev.ptr, nsnr, z.ptr, z.shape[1], out.ptr)
    return out


def awgn_mc(alphabet, snr, ns, noise=None, seed=None, return_noise=False):
    """:func:`awgn_mc_dev` for a host alphabet (complex64 or complex128, label order): the ``(nsnr, 2 + nbits)`` result on the host.  ``noise``:
    explicit draws ``(nsnr, ns)`` instead of the seeded ones of :func:`awgn_mc_noise_dev`; ``return_noise``: also the draws that were used."""
    al = np.ascontiguousarray(alphabet)
    suf, rt, ct = _lib.suffix(al.dtype)
    if al.ndim != 1 or al.dtype != ct:
        raise TypeError("awgn_mc: the alphabet must be a 1-d complex64 or complex128 array")
    nb = int(round(np.log2(al.size))) if al.size else 0
    if 2 ** nb != al.size or not 1 <= nb <= 10:
        raise ValueError("awgn_mc: the alphabet must have 2**nbits points, nbits in 1..10, got %d" % al.size)
    s = _mc_snr(snr, "awgn_mc")
    if int(ns) != ns or not 1 <= int(ns) <= MC_NS_MAX:
        raise ValueError("awgn_mc: ns must be a whole number in [1, 2**31]")
    ns = int(ns)
    if noise is not None:
        if np.size(noise) != s.size * ns:
            raise ValueError("awgn_mc: noise must hold %d x %d draws" % (s.size, ns))
        noise = np.ascontiguousarray(noise, dtype=ct).reshape(s.size, ns)
    else:
        seed = _mc_seed(seed)
    A, S = _lib.DeviceArray.from_host(al), _lib.DeviceArray.from_host(s)
    if noise is not None:
        Z = _lib.DeviceArray.from_host(noise)
    else:
        Z = awgn_mc_noise_dev(_lib.DeviceArray((s.size, ns), ct), S, seed)
    out = awgn_mc_dev(A, S, Z, _lib.DeviceArray((s.size, 2 + nb), np.float64)).to_host()
    return (out, Z.to_host()) if return_noise else out


def cal_gmi_mc(symbols, snr, ns, bit_map, noise=None, seed=None):
    """Monte-Carlo soft-decision GMI of a labelled alphabet at the linear ``snr`` (``pythran_dsp.cal_gmi_mc``, pythran_dsp.py:181-197): ``nbits -
    sum / (M ns)`` over ``ns`` noise draws ``z = sqrt(1 / snr) (randn + 1j randn) / sqrt(2)``.  ``bit_map`` ``(nbits, M / 2, 2)`` labels the points
    (:func:`bits_map_labels`); the precision is that of ``symbols``.  The reference draws from numpy's global generator inside the function; here
    the draws are counter-based under ``seed`` (None: a fresh one), or ``noise`` gives the ``ns`` values of ``z`` explicitly - with the reference's
    own draws the result is the reference's."""
    sy = np.asarray(symbols)
    suf, rt, ct = _lib.suffix(sy.dtype)
    if sy.ndim != 1 or sy.dtype != ct:
        raise TypeError("cal_gmi_mc: symbols must be a 1-d complex64 or complex128 array")
    alphabet = np.ascontiguousarray(bits_map_labels(bit_map), dtype=ct)
    if alphabet.size != sy.size:
        raise ValueError("cal_gmi_mc: bit_map labels %d points, symbols holds %d" % (alphabet.size, sy.size))
    if np.ndim(snr) != 0:
        raise ValueError("cal_gmi_mc: one linear SNR (theory.cal_gmi takes an array)")
    if noise is not None and np.size(noise) != ns:
        raise ValueError("cal_gmi_mc: noise must hold ns = %d draws" % ns)
    return float(awgn_mc(alphabet, snr, ns, noise=noise, seed=seed)[0, 0])


def ps_cdf(px):
    """The cumulative table of the shaped source: ``cumsum(px) / sum(px)`` in float64, its last entry forced to 1."""
    p = np.asarray(px, dtype=np.float64).ravel()
    if not 1 <= p.size <= PS_LMAX:
        raise ValueError("ps_symbols: between 1 and %d levels" % PS_LMAX)
    if not np.all(np.isfinite(p) & (p >= 0)) or not p.sum() > 0:
        raise ValueError("ps_symbols: the probabilities must be finite, not negative and not all zero")
    cdf = np.cumsum(p) / p.sum()
    cdf[-1] = 1.0
    return np.ascontiguousarray(np.minimum(cdf, 1.0))


def ps_symbols_dev(out, levels, px, seed, labels=None, label_table=None):
    """Probabilistically shaped symbols into the complex DeviceArray ``out`` ``(nmodes, N)`` or ``(N,)``: ``out[m, n] = levels[i] + 1j levels[q]``,
    ``i`` and ``q`` drawn with the probabilities ``px`` - the number of entries of :func:`ps_cdf` that are ``<= u``, ``u = word 2**-32`` of the
    Philox words x (I) and y (Q) of counter ``(n, m, stream 4)`` under ``seed`` (None: a fresh one).  ``levels`` (at most 64) are rounded to the
    row's precision once.  ``labels``: an int32 DeviceArray of ``out``'s shape for ``label_table[i, q]``, ``label_table`` an ``(L, L)`` int32 host
    array or DeviceArray.  At most 2**31 samples per row.  One launch, nothing read back; a host ``label_table`` goes up in a temporary buffer
    whose release waits for the device when the call returns - pass a DeviceArray to only enqueue."""
    c, rows, N = field(out, "ps_symbols_dev", "out", ndim=(1, 2))
    if N > PS_ROW_MAX or rows > 65535:
        raise ValueError("ps_symbols_dev: at most 65535 rows of 2**31 samples")
    lev = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).ravel())
    cdf = ps_cdf(px)
    if lev.size != cdf.size or not np.all(np.isfinite(lev)):
        raise ValueError("ps_symbols_dev: one finite level per probability")
    L = lev.size
    if (labels is None) != (label_table is None):
        raise ValueError("ps_symbols_dev: labels and label_table go together")
    if labels is not None:
        buffer(labels, "ps_symbols_dev", "labels", out.shape, np.int32)
        buffer(label_table, "ps_symbols_dev", "label_table", (L, L), np.int32)                  # (a host array or a DeviceArray)
    seed = _mc_seed(seed)
    if label_table is not None and not hasattr(label_table, "ptr"):
        label_table = _lib.DeviceArray.from_host(np.ascontiguousarray(label_table))
    _lib.call("qh_ps_symbols_%s_dev" % c, out.ptr, rows, N, _lib.ptr(lev), _lib.ptr(cdf), L, seed, None if labels is None else labels.ptr,
              None if label_table is None else label_table.ptr)
    return out
