"""Float64 NumPy restatements of the pilot-frame kernels (csrc/pilot.hip), written from their contracts, and the inputs of their tests.

Geometry: a frame of F symbols is S pilots (the sequence) followed by payload with one phase pilot every R symbols, the first at position S
(R = 0: the sequence only).  Position i is a pilot if i < S, or if R > 0 and (i - S) % R == 0:

    pilot at i < S           ordinal i
    pilot at i >= S          ordinal S + (i - S) / R
    payload at i (R > 0)     ordinal ((i - S) / R) (R - 1) + (i - S) % R - 1
    payload at i (R == 0)    ordinal i - S

Estimates, per mode, over the n used pilots - pilot j at pos_j = where[j % npf] + (j // npf) F as far as pos_j < span, paired with
sent[j % nref] (np.tile(...)[:, :n] of qampy/core/pilotbased_receiver.py:311):

    theta_j = angle(E[pos_j] conj(sent[j % nref]))
    c_j = -1 where theta_j - theta_(j-1) > pi, +1 where it is < -pi, else 0;  K = cumsum(c);  phase_j = theta_j + 2 pi K_j      (np.unwrap)
    knot_k = (phase_k + .. + phase_(k + N - 1)) / N at position pos_(k + N // 2),  k = 0 .. n - N        (a direct sum per window)
    trace = np.interp(arange(span), knot positions, knots);  field = E[:span] exp(-j trace)
    fit: slope = sum (j - jbar)(phase_j - pbar) / sum (j - jbar)^2, intercept = pbar - slope jbar  ->  [slope / (2 pi), intercept]
    constant phase: pbar

``unwrap_margin = min | |theta_j - theta_(j-1)| - pi |`` (inf without a step) says how far every unwrap decision is from flipping; where it
is comfortably above the rounding of a kernel, kernel and restatement take the same decisions and parity is a matter of rounding alone."""
import numpy as np

UW_CHUNK = 1024                          # pilots per workgroup of the unwrap (csrc/unwrap_scan.h)
N_MAX = 1023                             # longest moving average (csrc/pilot.hip PILOT_NMAX)
MARGIN = 0.25                            # rad: what every case keeps between its unwrap decisions and a flip


# ------------------------------------------------------------------------------------------------ geometry
def counts(F, S, R):
    NP = S + ((F - S) // R if R else 0)
    return NP, F - NP


def kind(F, S, R, i):
    """(is_pilot, ordinal) of position i, by the table above."""
    if i < S:
        return True, i
    b = i - S
    if not R:
        return False, b
    if b % R == 0:
        return True, S + b // R
    return False, (b // R) * (R - 1) + b % R - 1


def positions(F, S, R):
    """(pilot positions, payload positions) of a frame, by enumeration."""
    pil = [i for i in range(F) if kind(F, S, R, i)[0]]
    dat = [i for i in range(F) if not kind(F, S, R, i)[0]]
    return np.array(pil, dtype=np.int64), np.array(dat, dtype=np.int64)


def assemble(pilots, payload, F, S, R, nframes, scale=1.0, repeat_data=True, labels=None):
    """frame (nmodes, nframes F) - and, with labels, idx_frame - from pilots (nmodes, NP) and payload (nmodes, ND) or (nmodes, nframes ND)."""
    pilots, payload = np.atleast_2d(pilots), np.atleast_2d(payload)
    NP, ND = counts(F, S, R)
    frame = np.zeros((payload.shape[0], nframes * F), payload.dtype)
    idx = None if labels is None else np.zeros((payload.shape[0], nframes * F), np.int32)
    for f in range(nframes):
        for i in range(F):
            pil, o = kind(F, S, R, i)
            if pil:
                frame[:, f * F + i] = (pilots[:, o].astype(np.complex128) * scale).astype(payload.dtype)
                if idx is not None:
                    idx[:, f * F + i] = -1
            else:
                at = o if repeat_data else f * ND + o
                frame[:, f * F + i] = payload[:, at]
                if idx is not None:
                    idx[:, f * F + i] = labels[:, at]
    return frame if labels is None else (frame, idx)


def split(E, F, S, R, frames):
    """(payload (nmodes, nfr ND), pilots (nmodes, nfr NP)) of the frames ``frames`` of E, in the order of the list."""
    E = np.atleast_2d(E)
    pil, dat = positions(F, S, R)
    return (np.concatenate([E[:, f * F + dat] for f in frames], axis=1), np.concatenate([E[:, f * F + pil] for f in frames], axis=1))


# ------------------------------------------------------------------------------------------------ estimates
def wrap_counts(theta):
    """(c, K, margin) of np.unwrap over a 1-d array of angles."""
    d = np.diff(theta)
    c = np.where(d > np.pi, -1, np.where(d < -np.pi, 1, 0)).astype(np.int64)
    K = np.concatenate([[0], np.cumsum(c)])
    margin = float(np.min(np.abs(np.abs(d) - np.pi))) if d.size else np.inf
    return c, K, margin


def used(where, F, nframes, span):
    pos = (np.arange(nframes, dtype=np.int64)[:, None] * F + np.asarray(where, dtype=np.int64)[None, :]).ravel()
    return pos[pos < span]


def phase(E, where, F, nframes, sent, span=None):
    """(phase (nmodes, n), unwrap margin, positions (n,), turn counts K (nmodes, n))."""
    E, sent = np.atleast_2d(E).astype(np.complex128), np.atleast_2d(sent).astype(np.complex128)
    span = min(nframes * F, E.shape[1]) if span is None else span
    pos = used(where, F, nframes, span)
    ref = sent[:, np.arange(pos.size) % sent.shape[1]]
    theta = np.angle(E[:, pos] * ref.conj())
    out, Ks, margin = np.zeros_like(theta), np.zeros(theta.shape, np.int64), np.inf
    for r in range(theta.shape[0]):
        _, K, m = wrap_counts(theta[r])
        out[r], Ks[r], margin = theta[r] + 2 * np.pi * K, K, min(margin, m)
    return out, margin, pos, Ks


def knots(ph, N, pos):
    """(knot phases (nmodes, n - N + 1), knot positions): every knot a direct sum of its N phases, in order."""
    nk = ph.shape[1] - N + 1
    s = np.zeros((ph.shape[0], nk))
    for t in range(N):
        s += ph[:, t:t + nk]
    return s / N, pos[N // 2:N // 2 + nk]


def cpe(E, where, F, nframes, sent, N, span=None):
    """(field (nmodes, span), trace (nmodes, span), unwrap margin)."""
    E = np.atleast_2d(E).astype(np.complex128)
    span = min(nframes * F, E.shape[1]) if span is None else span
    ph, margin, pos, _ = phase(E, where, F, nframes, sent, span)
    kph, kpos = knots(ph, N, pos)
    trace = np.array([np.interp(np.arange(span), kpos, row) for row in kph])
    return E[:, :span] * np.exp(-1j * trace), trace, margin


def pair_phase(rec, ref):
    rec = np.atleast_2d(rec).astype(np.complex128)
    return phase(rec, [0], 1, rec.shape[1], ref)[:2]


def foe(rec, ref):
    """(fit (nmodes, 2) = [slope / (2 pi), intercept], unwrap margin) from sums centred on both means."""
    ph, margin = pair_phase(rec, ref)
    n = ph.shape[1]
    j = np.arange(n) - 0.5 * (n - 1)
    pbar = ph.mean(axis=1)
    slope = ((ph - pbar[:, None]) * j).sum(axis=1) / (j * j).sum()
    return np.stack([slope / (2 * np.pi), pbar - slope * 0.5 * (n - 1)], axis=1), margin


def const_phase(rec, ref):
    ph, margin = pair_phase(rec, ref)
    return ph.mean(axis=1), margin


# ------------------------------------------------------------------------------------------------ inputs
def _grid(x):
    """Rounded to multiples of 2^-12, so that complex64 and complex128 hold the same values (the convention of foe_ref.qam_tone)."""
    return np.round(np.asarray(x) * 4096) / 4096


def pilot_rows(nm, F, where, nframes, nref, seed, slope=0.05, walk=0.05, noise=0.03, L=None):
    """``(E (nm, L), sent (nm, nref))``: QPSK references, every used pilot its reference turned by ``phi_j = phi_0 + slope j + a random walk
    of standard deviation walk per pilot`` (radians, j counts the pilots) with a little noise, 16-QAM-like payload everywhere else."""
    rng = np.random.default_rng(seed)
    L = nframes * F if L is None else L
    lev = np.array([-3., -1., 1., 3.])
    E = (rng.choice(lev, (nm, L)) + 1j * rng.choice(lev, (nm, L))) / np.sqrt(10)
    sent = _grid((rng.choice([-1., 1.], (nm, nref)) + 1j * rng.choice([-1., 1.], (nm, nref))) / np.sqrt(2))
    pos = used(where, F, nframes, L)
    n = pos.size
    phi = rng.uniform(-np.pi, np.pi, (nm, 1)) + slope * np.arange(n) + np.cumsum(walk * rng.standard_normal((nm, n)), axis=1)
    E[:, pos] = sent[:, np.arange(n) % nref] * np.exp(1j * phi) * (1 + noise * (rng.standard_normal((nm, n)) + 1j * rng.standard_normal((nm, n))))
    return _grid(E), sent


def wrap_ramp(n=2049, at=1024):
    """One noiseless row of ``n`` pilots at the even positions (F = 2, where = [0], reference 1) whose angle climbs by 0.004 per pilot and flips
    between +3.0 and -3.0 at the pilots ``at - 1``, ``at`` and ``at + 1``: np.unwrap corrects at each of the three, by +1, -1 and +1 turns -
    the last pilot of one unwrap chunk and the first two of the next.  Returns ``(E (1, 2 n), sent (1, 1), the three pilot numbers)``."""
    k = np.arange(n)
    U = 3.0 + 0.004 * (k - (at - 2))
    U[at - 1] = U[at - 2] + 0.28
    U[at] = U[at - 2]
    U[at + 1:] = U[at - 2] + 0.28 + 0.004 * (k[at + 1:] - (at + 1))
    E = np.full((1, 2 * n), (1 + 1j) / np.sqrt(2))
    E[0, ::2] = np.exp(1j * U)
    return _grid(E), np.ones((1, 1), np.complex128), (at - 1, at, at + 1)


def cases():
    """The shared case list: dicts with ``name`` and ``make()`` -> ``dict(E, sent, where, F, nframes, span, N)`` (complex128 inputs; ``span``
    None: the whole signal; ``N`` None: too few pilots for an average, phase and constant phase only).  Small shapes that cross what the
    kernels tile by: 1, 2 and N used pilots, rows around one and two unwrap chunks of 1024, a span that cuts the last frame short, more
    references than positions, the shortest and the longest average, one mode and three."""
    out = []

    def add(name, nm, F, where, nframes, N, nref=None, span=None, L=None, **kw):
        seed = 3000 + len(out)

        def make():
            E, sent = pilot_rows(nm, F, where, nframes, len(where) if nref is None else nref, seed, L=L, **kw)
            return dict(E=E, sent=sent, where=np.array(where, dtype=np.int64), F=F, nframes=nframes, span=span, N=N)
        out.append(dict(name=name, make=make))

    add("n1", 1, 16, [3], 1, None)
    add("n2", 3, 16, [0, 8], 1, None)
    add("n5-N5", 1, 20, [0, 4, 8, 12, 16], 1, 5)
    add("n1023-N3", 1, 33, [0, 5, 31], 341, 3)
    add("n1024-N5", 3, 32, [1, 9, 17, 30], 256, 5)
    add("n1025-N3", 1, 40, [0, 8, 16, 24, 39], 205, 3)
    add("n1025-Nmax", 3, 40, [0, 8, 16, 24, 39], 205, N_MAX, slope=0.01, walk=0.02)
    add("n2049-N7", 3, 24, [0, 7, 15], 683, 7)
    add("n2049-Nmax", 1, 24, [0, 7, 15], 683, N_MAX, slope=-0.02, walk=0.02)
    add("span-cut", 3, 32, [1, 9, 17, 30], 4, 3, span=3 * 32 + 12, L=4 * 32 + 5)
    add("nref-6-npf-4", 1, 32, [1, 9, 17, 30], 9, 5, nref=6)
    add("falling", 3, 64, [0, 16, 32, 48], 40, 9, slope=-0.3, walk=0.1)

    def ramp():
        E, sent, _ = wrap_ramp()
        return dict(E=E, sent=sent, where=np.array([0], dtype=np.int64), F=2, nframes=2049, span=None, N=3)
    out.append(dict(name="wrap-ramp", make=ramp))
    return out


# ------------------------------------------------------------------------------------------------ tests/golden/pilotframe.npz
def golden_frame(g, prefix):
    """The reference's values behind the labels of one stored signal: ``dict(frame, pilots, payload, pil_coded, pay_coded)`` (``pilots`` and
    ``payload`` as the reference holds them: scaled, and repeated once per frame)."""
    pil_coded, pay_coded = g[prefix + "pil_coded"], g[prefix + "pay_coded"]
    return dict(frame=np.concatenate([pil_coded, pay_coded])[g[prefix + "frame"]], pilots=pil_coded[g[prefix + "pilots"]],
                payload=pay_coded[g[prefix + "payload"]], payload_labels=g[prefix + "payload"].astype(np.int32), pil_coded=pil_coded, pay_coded=pay_coded)


def golden_cpe_calls(g):
    """The three stored carrier-phase calls as ``(name, phaserec.pilot_cpe keywords, restatement arguments)``: the selection of
    pilot_based_cpe_new (every pilot_rat-th of the first max_blocks positions, the references thinned the same way), restated."""
    M, F, S, R, nfr = (int(v) for v in g["geoms"][0])
    pil = golden_frame(g, "f0_c128_")["pilots"]
    pos = positions(F, S, R)[0]
    x = g["est_x"]
    return [("cpe1", dict(N=5, use_seq=True), dict(E=x, where=pos, F=F, nframes=1, sent=pil, N=5)),
            ("cpe2", dict(N=3, use_seq=False), dict(E=x, where=pos[S:], F=F, nframes=1, sent=pil[:, S:], N=3)),
            ("cpe3", dict(N=4, pilot_rat=2, max_blocks=40, nframes=2), dict(E=x, where=pos[S:][:40:2], F=F, nframes=2, sent=pil[:, S:][:, ::2], N=5))]


def long_row():
    """One row of 2^20 + 1024 used pilots, every position a pilot (F = 1, where = [0]), for N = 5: 1025 unwrap chunks, so every thread of the scan
    of the chunk sums holds more than one chunk; the phase climbs by 3e-5 rad per pilot under a random walk - a trace of more than 20 rad."""
    n = 2 ** 20 + 1024
    E, sent = pilot_rows(1, 1, [0], n, 64, 4242, slope=3e-5, walk=1e-3, noise=0.02)
    return dict(E=E, sent=sent, where=np.array([0], dtype=np.int64), F=1, nframes=n, span=None, N=5)
