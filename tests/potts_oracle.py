"""numpy restatement of the contract of the exact piecewise-constant (Potts) fit (include/raman_mi355x.h
rdn_potts), and a second, independent reference for tiny rows: every segmentation with parts of at most K
samples, its objective evaluated in exact rational arithmetic.  Written for clarity, not speed; shared by the CPU
and GPU tests.
"""
import math
from fractions import Fraction

import numpy as np

QUIET_NAN = np.uint32(0x7FC00000)
MAD_TO_SIGMA = 0.6744897501960817


def potts(x, gamma, max_len=64, parts=False):
    """x float32 (n, L); gamma float64 (n,) or a float; K = max_len.  Returns (y float32 (n, L), nseg int32 (n,)),
    and with ``parts`` each row's part lengths from the left as a tuple (empty for a refused row).
    Each line of the loop over r is one fp64 operation of the contract, vectorised over the rows and over len
    (candidates in the order len = 1 .. min(K, r), so that argmin returns the smallest len that attains the minimum)."""
    x = np.asarray(x, dtype=np.float32)
    n, L = x.shape
    g = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (n,)).copy()
    K = int(max_len)
    assert 1 <= K <= 64 and L >= 1
    lens = np.arange(1, K + 1, dtype=np.float64)
    S1 = np.zeros((n, L + 1))
    S2 = np.zeros((n, L + 1))
    B = np.zeros((n, L + 1))
    A = np.ones((n, L + 1), dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, L + 1):
            v = x[:, i - 1].astype(np.float64)
            S1[:, i] = S1[:, i - 1] + v
            S2[:, i] = S2[:, i - 1] + v * v
        for r in range(1, L + 1):
            k = min(K, r)
            ls = r - np.arange(1, k + 1)                                # l = r - len
            d1 = S1[:, r:r + 1] - S1[:, ls]
            d2 = S2[:, r:r + 1] - S2[:, ls]
            sse = d2 - (d1 * d1) / lens[:k]
            c = (B[:, ls] + g[:, None]) + sse
            A[:, r] = np.argmin(np.where(np.isnan(c), np.inf, c), axis=1) + 1
            B[:, r] = c[np.arange(n), A[:, r] - 1]
        bad = ~(np.isfinite(x).all(axis=1) & (g >= 0) & np.isfinite(g))
        y = np.empty((n, L), dtype=np.float32)
        nseg = np.zeros(n, dtype=np.int32)
        cuts = [[] for _ in range(n)]
        for row in range(n):
            if bad[row]:
                continue
            r = L
            while r > 0:
                ln = int(A[row, r])
                mean = (S1[row, r] - S1[row, r - ln]) / np.float64(ln)
                y[row, r - ln:r] = np.float32(mean)
                nseg[row] += 1
                cuts[row].append(ln)
                r -= ln
    bits = np.where(bad[:, None], QUIET_NAN, y.view(np.uint32)).astype(np.uint32)
    if parts:
        return bits.view(np.float32), nseg, [tuple(reversed(c)) for c in cuts]
    return bits.view(np.float32), nseg


def noise_mad(x):
    """m of rdn_noise_mad / rdn_haar_shrink: the median of |0.5 (x[i] - x[i - 1])|, periodic; NaN for a bad row."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        a = x.astype(np.float64)
        m = np.median(np.abs(0.5 * (a - np.roll(a, 1, axis=-1))), axis=-1)
    return np.where(np.isfinite(x).all(axis=-1), m, np.nan)


def thresholds(penalty, L):
    """The penalty in noise variances: a float, or 'bic' for 2 ln L."""
    return 2.0 * math.log(L) if penalty == "bic" else float(penalty)


def gamma(x, penalty=12.0):
    """gamma of PottsFit(penalty): sigma = m * (sqrt 2 / 0.6745), gamma = penalty * (sigma * sigma)."""
    with np.errstate(all="ignore"):
        sigma = noise_mad(x) * (math.sqrt(2.0) / MAD_TO_SIGMA)
        return thresholds(penalty, np.asarray(x).shape[-1]) * (sigma * sigma)


def compositions(L, K):
    """Every way to write L as an ordered sum of parts in 1 .. K."""
    if L == 0:
        yield ()
        return
    for first in range(1, min(K, L) + 1):
        for rest in compositions(L - first, K):
            yield (first,) + rest


def exact_objective(x_row, parts, g):
    """Σ over the parts of (Σ (x - mean)² + g), in Fractions of the row's fp32 values and of the double g."""
    total, i = Fraction(0), 0
    for ln in parts:
        seg = [Fraction(float(v)) for v in x_row[i:i + ln]]
        s1 = sum(seg)
        total += sum(v * v for v in seg) - s1 * s1 / ln + Fraction(float(g))
        i += ln
    return total


def brute_force(x_row, g, K):
    """(the exact minimum of the objective over all segmentations with parts <= K, the segmentations attaining it)."""
    best, arg = None, []
    for parts in compositions(len(x_row), K):
        v = exact_objective(x_row, parts, g)
        if best is None or v < best:
            best, arg = v, [parts]
        elif v == best:
            arg.append(parts)
    return best, arg
