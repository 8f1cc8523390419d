"""Host restatement of the exact accumulator (csrc/metrics.hpp to_limbs / acc_add) and of the binned
reports built from it (include/raman_mi355x.h), in Python integers and math.fsum (TEST INFRASTRUCTURE).
The constants are literals, not raman_mi355x._lib's: the oracle stays independent of the package."""
import math
from fractions import Fraction

import numpy as np

ACC_LIMBS, ACC_STRIDE, FRAC_BITS = 6, 7, 128


def limbs_of(values):
    """The limbs of one quantity that has accumulated ``values``, each finite with |v| < 2^64."""
    limbs = [0] * ACC_LIMBS
    for v in values:
        f = Fraction(float(v)) * 2 ** FRAC_BITS
        mag = abs(f.numerator) // f.denominator                    # truncation toward zero
        for j in range(ACC_LIMBS):
            c = (mag >> (32 * j)) & 0xffffffff
            limbs[j] += -c if v < 0 else c
    return limbs


def in_range(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 64


def row_words(sel, counts=(1,), skip=0):
    """The int64 words of one row that has accumulated the spectra ``sel`` (n, q): q accumulators (a value
    that is not in_range counts in its quantity's out-of-range word; the first ``skip`` quantities were not
    supplied and stay zero), then one count word per entry of ``counts``: n times that entry."""
    sel = np.asarray(sel, dtype=np.float64)
    q = sel.shape[1]
    row = np.zeros(q * ACC_STRIDE + len(counts), dtype=np.int64)
    for k in range(skip, q):
        ok = np.array([in_range(v) for v in sel[:, k]], dtype=bool)
        row[k * ACC_STRIDE:k * ACC_STRIDE + ACC_LIMBS] = limbs_of(sel[ok, k])
        row[k * ACC_STRIDE + ACC_LIMBS] = int((~ok).sum())
    row[q * ACC_STRIDE:] = [len(sel) * c for c in counts]
    return row


def report_words(per, rows, nbins, counts=(1,), skip=0):
    """The int64 words of the report (nbins + 2 rows of row_words) of spectra with the values ``per``
    (n, q) in report rows ``rows``."""
    return np.concatenate([row_words(per[rows == b], counts, skip) for b in range(nbins + 2)])


def report_sums(per, rows, nbins):
    """(nbins + 3, 1 + q): per report row, then for all spectra: count and the q exact sums rounded once
    (NaN for a quantity with a value that is not in_range)."""
    q = per.shape[1]
    out = np.zeros((nbins + 3, 1 + q))
    sels = [rows == b for b in range(nbins + 2)] + [np.ones(len(rows), dtype=bool)]
    for b, m in enumerate(sels):
        sel = per[m]
        out[b, 0] = len(sel)
        for k in range(q):
            out[b, 1 + k] = math.fsum(sel[:, k]) if all(in_range(v) for v in sel[:, k]) else float("nan")
    return out
