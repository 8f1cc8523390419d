"""Plain-numpy oracle of the SNR report (include/raman_mi355x.h rdn_snr): float64 for the values,
float32 for the bin index, exact (math.fsum) sums.  Shared by test_snr_cpu.py and test_snr_gpu.py."""
import math
from fractions import Fraction

import numpy as np

QUANTITIES = ("MSE", "SSIM", "Smoothness", "Peak2Peak", "SNR_in", "SNR_out", "SNR_gain")
ACC_LIMBS, ACC_STRIDE, FRAC_BITS = 6, 7, 128
ROW_WORDS = 7 * ACC_STRIDE + 2
COUNT, COUNT4 = 7 * ACC_STRIDE, 7 * ACC_STRIDE + 1


def snr_values(x, y, clean):
    """(n, 3) float64 {SNR_in, SNR_out, SNR_gain} in dB with P = mean(clean^2) (数据集产生.py:43);
    zero powers give the IEEE results (inf / NaN), as the device does."""
    x, y, c = (np.asarray(a, dtype=np.float64) for a in (x, y, clean))
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.mean(c ** 2, axis=1)
        Ni = np.mean((x - c) ** 2, axis=1)
        No = np.mean((y - c) ** 2, axis=1)
        s_in = 10.0 * np.log10(P / Ni)
        s_out = 10.0 * np.log10(P / No)
        return np.stack([s_in, s_out, s_out - s_in], axis=1)


def bin_rows(key, lo, hi, nbins):
    """Report row of each key: the header's formula, every operation in float32."""
    key = np.asarray(key, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(nbins) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (key >= lo) & (key < hi)
        t = (np.where(inside, key, lo) - lo) * scale
        i = np.minimum(t.astype(np.int32), nbins - 1)
    rows = np.where(inside, 1 + i, np.where(key < lo, 0, nbins + 1))
    return rows.astype(np.int64)


def limbs_of(values):
    """Host restatement of the device accumulator (metrics.hpp to_limbs) for finite |v| < 2^64."""
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


def report_words(per7, rows, nbins, have4=True):
    """The int64 words of the report of spectra with the seven values per7 (n, 7) in report rows `rows`."""
    rep = np.zeros((nbins + 2, ROW_WORDS), dtype=np.int64)
    for b in range(nbins + 2):
        sel = per7[rows == b]
        rep[b, COUNT] = len(sel)
        rep[b, COUNT4] = len(sel) if have4 else 0
        for k in range(0 if have4 else 4, 7):
            col = sel[:, k]
            ok = np.array([in_range(v) for v in col], dtype=bool)
            rep[b, k * ACC_STRIDE:k * ACC_STRIDE + ACC_LIMBS] = limbs_of(col[ok])
            rep[b, k * ACC_STRIDE + ACC_LIMBS] = int((~ok).sum())
    return rep.reshape(-1)


def report_sums(per7, rows, nbins):
    """(nbins + 3, 8): per report row, then for all spectra: count and the seven exact sums rounded once
    (NaN for a quantity with a value that is not finite)."""
    out = np.zeros((nbins + 3, 8))
    sels = [rows == b for b in range(nbins + 2)] + [np.ones(len(rows), dtype=bool)]
    for b, m in enumerate(sels):
        sel = per7[m]
        out[b, 0] = len(sel)
        for k in range(7):
            out[b, 1 + k] = math.fsum(sel[:, k]) if all(in_range(v) for v in sel[:, k]) else float("nan")
    return out
