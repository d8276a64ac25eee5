"""Float64 numpy restatement of time-domain hybrid QAM as DESIGN.md 3.21 fixes it - the yardstick of csrc/hybrid.hip, where the reference's
own split and metrics raise - and the shared cases of tests/test_hybrid_ref.py and tests/test_gpu_hybrid.py.

A frame is ``fM`` positions, ``fM1`` of format 1 then ``fM2`` of format 2; format-2 symbols are stored over ``sqrt(powratio)``.
"""
import fractions
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hybrid.npz")
DT = {"c64": np.complex64, "c128": np.complex128}
ALIGN_MARGIN = 0.02                # least relative lead of the best alignment over the runner-up a case may have
TIE_MARGIN = 1e-4                  # least gap between a sample's nearest and second-nearest squared distance


def geometry(fr):
    rat = fractions.Fraction(fr).limit_denominator()
    return rat.denominator, rat.denominator - rat.numerator, rat.numerator


def positions(L, fM, fM1):
    n = np.arange(L)
    return n[n % fM < fM1], n[n % fM >= fM1]


def power_ratio(coded1, coded2):
    d1, d2 = (np.min(np.abs(np.diff(np.unique(c)))) for c in (coded1, coded2))
    return (d2 / d1) ** 2


def assemble(part1, part2, fM, fM1, powratio):
    """Parts (nmodes, nframes fM1) and (nmodes, nframes fM2) interleaved; part 2 times 1 / sqrt(powratio), the product formed in double and
    rounded once to the parts' precision (numpy's complex-by-real quotient)."""
    L = part1.shape[1] + part2.shape[1]
    idx1, idx2 = positions(L, fM, fM1)
    out = np.empty((part1.shape[0], L), dtype=part1.dtype)
    out[:, idx1] = part1
    out[:, idx2] = (part2.astype(np.complex128) * (1.0 / np.sqrt(powratio))).astype(part2.dtype)
    return out


def class_sums(x, fM):
    mag = np.abs(np.atleast_2d(x).astype(np.complex128))
    return np.stack([mag[:, r::fM].sum(axis=1) for r in range(fM)], axis=1)


def alignment_means(x, fM, fM1, M):
    """``m[row, j] = mean |x[(H + j) % L]|``, H the positions of the higher-order format (format 1 if M1 > M2, else format 2)."""
    x = np.atleast_2d(x).astype(np.complex128)
    L = x.shape[1]
    if L % fM:
        raise ValueError("the row must hold whole frames")
    idx1, idx2 = positions(L, fM, fM1)
    H = idx1 if M[0] > M[1] else idx2
    mag = np.abs(x)
    return np.array([[mag[m, (H + j) % L].mean() for j in range(fM)] for m in range(x.shape[0])])


def align(x, fM, fM1, M):
    """Per row the first j at which m_j is strictly largest."""
    shifts = []
    for row in alignment_means(x, fM, fM1, M):
        best, top = 0, row[0]
        for j in range(1, fM):
            if row[j] > top:
                best, top = j, row[j]
        shifts.append(best)
    return np.array(shifts, dtype=np.int32)


def align_margin(x, fM, fM1, M):
    """Smallest relative lead of the best m_j over the runner-up, over the rows."""
    m = np.sort(alignment_means(x, fM, fM1, M), axis=1)
    return float(np.min((m[:, -1] - m[:, -2]) / m[:, -1]))


def split(x, fM, fM1, powratio, shifts):
    x = np.atleast_2d(x).astype(np.complex128)
    L = x.shape[1]
    if L % fM:
        raise ValueError("the row must hold whole frames")
    idx1, idx2 = positions(L, fM, fM1)
    shifts = np.broadcast_to(np.asarray(shifts), (x.shape[0],))
    p1 = np.array([x[m, (idx1 + shifts[m]) % L] for m in range(x.shape[0])])
    p2 = np.array([x[m, (idx2 + shifts[m]) % L] for m in range(x.shape[0])]) * np.sqrt(powratio)
    return p1, p2


def _distances(r, coded):
    d = r[:, None] - np.asarray(coded).astype(np.complex128)[None, :]
    return d.real ** 2 + d.imag ** 2


def metrics(x, idx_tx, fM, fM1, powratio, coded1, coded2, shifts):
    """``(sums (nmodes, 2, 4), margin)``: per row and format symbol errors, bit errors, symbols compared and the sum of |r - s_label|^2 - the
    aligned sample against the label at its position, a label outside the alphabet skipped - and the smallest gap between the nearest and the
    second-nearest squared distance over every sample that is compared."""
    p1, p2 = split(x, fM, fM1, powratio, shifts)
    idx1, idx2 = positions(np.atleast_2d(x).shape[1], fM, fM1)
    sums, margin = np.zeros((p1.shape[0], 2, 4)), np.inf
    for k, (part, pos, coded) in enumerate(((p1, idx1, coded1), (p2, idx2, coded2))):
        for m in range(part.shape[0]):
            lab = np.asarray(idx_tx)[m, pos].astype(np.int64)
            keep = (lab >= 0) & (lab < len(coded))
            d = _distances(part[m][keep], coded)
            dec = np.argmin(d, axis=1)
            t = lab[keep]
            if d.shape[1] > 1 and d.shape[0]:
                two = np.partition(d, 1, axis=1)
                margin = min(margin, float(np.min(two[:, 1] - two[:, 0])))
            bit = sum(int(bin(int(v)).count("1")) for v in dec ^ t)
            sums[m, k] = (np.count_nonzero(dec != t), bit, t.size, d[np.arange(t.size), t].sum())
    return sums, margin


def rates(sums, M):
    """SER, BER and EVM, each ``(per format (nmodes, 2), combined (nmodes,))``."""
    se, be, n, sq = (sums[:, :, k] for k in range(4))
    nb = np.log2(np.asarray(M, dtype=np.float64))
    return dict(ser=(se / n, se.sum(axis=1) / n.sum(axis=1)), ber=(be / (n * nb), be.sum(axis=1) / (n * nb).sum(axis=1)),
                evm=(np.sqrt(sq / n), np.sqrt(sq.sum(axis=1) / n.sum(axis=1))))


# ------------------------------------------------------------------------------------------------ golden rows and shared cases
_GOLD = {}


def gold():
    if not _GOLD:
        _GOLD.update(np.load(GOLD))
    return _GOLD


def golden_signal(prefix, dt):
    """What the golden file holds under ``prefix`` (``t0_n2_``, ``tfs_``, ..) for dtype key ``dt``: a dict of the row, the unit-power parts, the
    scaled part 2, the labels at every position, the alphabets, powratio and geometry."""
    g = gold()
    coded1, coded2, scaled2 = (g[prefix + dt + "_" + k] for k in ("coded1", "coded2", "scaled2"))
    fM, fM1, fM2 = (int(v) for v in g[prefix + "geometry"])
    frame = g[prefix + "frame"].astype(np.int64)
    M1 = coded1.size
    return dict(row=np.concatenate([coded1, scaled2])[frame], part1=coded1[g[prefix + "part1"]], part2=coded2[g[prefix + "part2"]],
                part2_scaled=scaled2[g[prefix + "part2"]], labels1=g[prefix + "part1"].astype(np.int32), labels2=g[prefix + "part2"].astype(np.int32),
                idx_tx=np.where(frame < M1, frame, frame - M1).astype(np.int32), coded1=coded1, coded2=coded2, powratio=float(g[prefix + dt + "_powratio"]),
                fM=fM, fM1=fM1, fM2=fM2, M=(coded1.size, coded2.size))


# The received rows of the GPU cases: the rows of the two-mode golden case k (one, both, or both and the first again) plus seeded noise at snr dB
# relative to the row's mean power, rolled by -roll, so that the alignment is (fM - roll) % fM.  Every row has a noise seed of its own: the first
# from 0 on that keeps every sample TIE_MARGIN clear of a decision boundary in both precisions (searched once with find_seeds below;
# tests/test_hybrid_ref.py asserts the condition on every sample).  The third row is rolled one further, so the rows of a call do not share a shift.
CASES = [dict(name="16-4_fr0.3", k=0, snr=12.0, roll=7, shift=3),
         dict(name="64-16_fr0.5", k=1, snr=18.0, roll=1, shift=1),
         dict(name="4-16_fr0.75", k=2, snr=12.0, roll=3, shift=1)]
SEEDS = {"16-4_fr0.3": [2, 0, 6], "64-16_fr0.5": [1, 2, 3], "4-16_fr0.75": [0, 1, 3]}
NMODES = (1, 2, 3)
ROWS = (0, 1, 0)                   # the golden mode behind every row


def noisy_row(clean, snr, seed):
    rng = np.random.default_rng(seed)
    x = clean.astype(np.complex128)
    sd = np.sqrt(np.mean(np.abs(x) ** 2) * 10 ** (-snr / 10) / 2)
    return x + sd * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))


def received(case, nm, dt, seeds=None, rolled=True):
    """``(golden dict, received rows in dtype dt, transmitted labels, expected shifts)`` of a case at ``nm`` modes; without ``rolled`` the same
    rows as they were sent: already aligned, shift 0, and in step with the transmitted sequence."""
    s = golden_signal("t%d_n2_" % case["k"], dt)
    seeds = SEEDS[case["name"]] if seeds is None else seeds
    rolls = [case["roll"], case["roll"], (case["roll"] + 1) % s["fM"]][:nm] if rolled else [0] * nm
    x = np.array([np.roll(noisy_row(s["row"][ROWS[m]], case["snr"], seeds[m]), -rolls[m]) for m in range(nm)]).astype(DT[dt])
    shifts = np.array([(s["fM"] - r) % s["fM"] for r in rolls], dtype=np.int32)
    # the split aligns the format, not the sequence: a rolled row comes out one frame late, and so do the labels it is measured against
    labels = np.ascontiguousarray([np.roll(s["idx_tx"][ROWS[m]], -(rolls[m] + shifts[m])) for m in range(nm)])
    return s, x, labels, shifts


def case_margins(case, nm, dt, seeds=None):
    """``(alignment lead, tie margin)`` of a case on the restatement."""
    s, x, labels, shifts = received(case, nm, dt, seeds)
    _, tie = metrics(x, labels, s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], shifts)
    return align_margin(x, s["fM"], s["fM1"], s["M"]), tie


def find_seeds(case, limit=2000):
    """Per row the first seed that keeps TIE_MARGIN in both precisions (run once when a case is written; the result is in SEEDS)."""
    out = []
    for m in range(len(ROWS)):
        for seed in range(limit):
            ok = True
            for dt in DT:
                s = golden_signal("t%d_n2_" % case["k"], dt)
                x = noisy_row(s["row"][ROWS[m]], case["snr"], seed).astype(DT[dt])[None, :]
                ok = ok and metrics(x, s["idx_tx"][ROWS[m]][None, :], s["fM"], s["fM1"], s["powratio"], s["coded1"], s["coded2"], 0)[1] >= TIE_MARGIN
            if ok and seed not in out:
                out.append(seed)
                break
        else:
            raise RuntimeError("no seed below %d keeps the margin" % limit)
    return out
