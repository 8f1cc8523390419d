"""Plain-numpy oracle of the SNR report (include/raman_mi355x.h rdn_snr): float64 for the values,
float32 for the bin index, exact (math.fsum) sums.  Shared by test_snr_cpu.py and test_snr_gpu.py."""
import numpy as np

import exact_acc as E
from exact_acc import in_range, limbs_of, report_sums  # noqa: F401  (the names the tests have always used)

QUANTITIES = ("MSE", "SSIM", "Smoothness", "Peak2Peak", "SNR_in", "SNR_out", "SNR_gain")
ACC_LIMBS, ACC_STRIDE, FRAC_BITS = E.ACC_LIMBS, E.ACC_STRIDE, E.FRAC_BITS
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


def report_words(per7, rows, nbins, have4=True):
    """The int64 words of the report of spectra with the seven values per7 (n, 7) in report rows `rows`."""
    return E.report_words(per7, rows, nbins, counts=(1, int(have4)), skip=0 if have4 else 4)
