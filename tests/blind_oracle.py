"""Plain-numpy oracle of the blind residual report (include/raman_mi355x.h rdn_blind): float64 on the stored
float32 values, every sum over the positions of a spectrum exact (math.fsum) and rounded once, float32 for
the bin index.  Shared by test_blind_cpu.py and test_blind_gpu.py (TEST INFRASTRUCTURE).  The constants are
literals, not raman_mi355x._lib's: the oracle stays independent of the package."""
import math

import numpy as np

import exact_acc as E
from snr_oracle import bin_rows  # noqa: F401  (the rows of a blind report are the SNR report's)

QUANTITIES = ("Mean", "RMS", "Ratio", "Rho1", "RhoMax", "Q", "SNR_est")
MAX_LAGS = 32
ACC_STRIDE = 7
COUNT, FLAGGED, ROW_WORDS = 7 * ACC_STRIDE, 7 * ACC_STRIDE + 1, 7 * ACC_STRIDE + 2
SIGMA_PER_MAD = math.sqrt(2.0) / 0.6744897501960817


def _sum(a):
    """The exact sum of a float64 vector rounded once; the IEEE result where a term is not finite."""
    if np.isfinite(a).all():
        return np.float64(math.fsum(a.tolist()))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(np.sum(a))


def blind_spectrum(x, y, sigma, lags):
    """(seven values, rho[lags]) of one spectrum, by the header's definitions."""
    a, b = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    L, sigma = len(a), np.float64(sigma)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = a - b
        mean = _sum(r) / L
        rms = np.sqrt(_sum(r * r) / L)
        d = r - mean
        D = _sum(d * d)
        rho = np.array([_sum(d[:L - k] * d[k:]) / D for k in range(1, lags + 1)])
        rho_max = np.float64("nan") if np.isnan(rho).any() else np.abs(rho).max()
        q = np.float64(0.0)
        for k in range(1, lags + 1):
            q = q + (rho[k - 1] * rho[k - 1]) / np.float64(L - k)
        Q = (np.float64(L) * np.float64(L + 2)) * q
        S, s2 = _sum(a * a) / L, sigma * sigma
        snr_est = 10.0 * np.log10((S - s2) / s2)
        ratio = rms / sigma
    return np.array([mean, rms, ratio, rho[0], rho_max, Q, snr_est]), rho


def blind_values(x, y, sigma, lags):
    """(per (n, 7), rho (n, lags)) float64 of the spectra x, y (n, L) with the noise levels sigma (n,)."""
    x, y = np.asarray(x), np.asarray(y)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(x),))
    out = [blind_spectrum(x[i], y[i], sigma[i], lags) for i in range(len(x))]
    return (np.array([o[0] for o in out]).reshape(len(x), 7), np.array([o[1] for o in out]).reshape(len(x), lags))


def flagged(per, q_crit):
    """Q > q_crit, false for a NaN Q."""
    with np.errstate(invalid="ignore"):
        return np.asarray(per)[:, 5] > q_crit


def q_crit(lags, z=2.3263478740408408):
    """Wilson and Hilferty's chi-square quantile; z: the normal 0.99 quantile."""
    k = float(lags)
    return k * (1.0 - 2.0 / (9.0 * k) + z * math.sqrt(2.0 / (9.0 * k))) ** 3


def noise_sigma(x):
    """The project's blind noise estimate: the median of |0.5 (x[i] - x[i-1])| over the periodic spectrum, in
    float64, times sqrt(2) / 0.6745."""
    x = np.asarray(x, dtype=np.float64)
    return np.median(np.abs(0.5 * (x - np.roll(x, 1, axis=-1))), axis=-1) * SIGMA_PER_MAD


def report_words(per, rows, nbins, flags):
    """The int64 words of the report of spectra with the seven values per (n, 7) in report rows ``rows``, those
    with ``flags`` set flagged: per row seven accumulators, the count, the flagged count."""
    per, rows, flags = np.asarray(per), np.asarray(rows), np.asarray(flags, dtype=bool)
    out = []
    for b in range(nbins + 2):
        m = rows == b
        w = E.row_words(per[m], counts=(1, 0))
        w[FLAGGED] = int(flags[m].sum())
        out.append(w)
    return np.concatenate(out)
