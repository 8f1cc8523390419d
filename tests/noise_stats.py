"""Is the simulator's noise standard normal and independent?  Test infrastructure beside spike_stats.

From (clean, noisy, noise_std) of SPIKE-FREE spectra (extreme_noise_prob = 0) the residual
z = (noisy − clean)/σ, formed in float64, is what the generator drew: N(0, 1), independent over
positions and spectra (数据集产生.py:43-47, ``np.random.normal(0, noise_std, shape)``).  Every statistic
below is returned as a z-score, (estimate − expectation) / sampling error under that null for the
number of terms it averages (N = n·L samples; a lag-k product has n·(L−k) terms):

    mean                      E z   = 0,  se 1/√N
    var                       E z²  = 1,  se √(2/N)         Var z² = 3 − 1
    m3                        E z³  = 0,  se √(15/N)        Var z³ = E z⁶ = 15
    m4                        E z⁴  = 3,  se √(96/N)        Var z⁴ = E z⁸ − 9 = 105 − 9
    acf1, acf2, acf4          E z_p z_{p+k} = 0, se 1/√terms     (the engine's positions p..p+3 share
                              one Philox block and one Box-Muller pair: lags 1 and 2 stay inside a
                              block, lag 4 pairs the same lane of neighbouring counters)
    cross                     E z_{i,p} z_{i+1,p} = 0, se 1/√terms      (neighbouring spectrum indices)
    clean                     Σ z·c / √(Σ c²) with c = clean − its row mean: exactly N(0, 1) given clean

plus ``chi2``, Pearson's χ² of z over CHI2_BINS equiprobable N(0, 1) bins (CHI2_BINS − 1 degrees of
freedom), and ``max_abs``.  A Box-Muller transform fed u1 >= 2^-24 cannot exceed MAX_ABS_CEILING.

The float32 rounding of noisy = clean + σ·z moves z by at most ~2^-24·|noisy|/σ (1e-5 at the largest
SNR the generator is run at): far below every sampling error here.
"""
from statistics import NormalDist

import numpy as np

CHI2_BINS = 32
ZSCORES = ("mean", "var", "m3", "m4", "acf1", "acf2", "acf4", "cross", "clean")
MAX_ABS_CEILING = float(np.sqrt(2.0 * 24.0 * np.log(2.0)))          # sqrt(-2 ln 2^-24) = 5.768...
# the bounds the tests hold both the oracle and the device to: sampling theory, not measurements
Z_BOUND = 4.0                                                       # per z-score: two-sided p = 6e-5
CHI2_BOUND = 61.1                                                   # chi2(31) at p = 1e-3


def collect(clean, noisy, noise_std):
    clean = np.asarray(clean, np.float64)
    noisy = np.asarray(noisy, np.float64)
    sigma = np.asarray(noise_std, np.float64).reshape(-1, 1)
    if clean.ndim != 2 or clean.shape != noisy.shape or sigma.shape[0] != clean.shape[0]:
        raise ValueError(f"need (n, L) clean and noisy and n noise_std, got {clean.shape} {noisy.shape} {sigma.shape}")
    if not (np.all(sigma > 0) and np.all(np.isfinite(sigma))):
        raise ValueError("every spectrum needs a finite noise_std > 0")
    n, L = clean.shape
    z = (noisy - clean) / sigma
    N = z.size
    out = {
        "mean": z.mean() * np.sqrt(N),
        "var": ((z * z).mean() - 1.0) / np.sqrt(2.0 / N),
        "m3": (z ** 3).mean() / np.sqrt(15.0 / N),
        "m4": ((z ** 4).mean() - 3.0) / np.sqrt(96.0 / N),
    }
    for k in (1, 2, 4):
        prod = z[:, :-k] * z[:, k:]
        out[f"acf{k}"] = prod.mean() * np.sqrt(prod.size)
    prod = z[:-1] * z[1:]
    out["cross"] = prod.mean() * np.sqrt(prod.size)
    c = clean - clean.mean(axis=1, keepdims=True)
    out["clean"] = (z * c).sum() / np.sqrt((c * c).sum())
    nd = NormalDist()
    inner = np.array([nd.inv_cdf(k / CHI2_BINS) for k in range(1, CHI2_BINS)])
    obs = np.bincount(np.searchsorted(inner, z.ravel()), minlength=CHI2_BINS).astype(np.float64)
    exp = N / CHI2_BINS
    out = {k: float(v) for k, v in out.items()}
    out["chi2"] = float(((obs - exp) ** 2 / exp).sum())
    out["max_abs"] = float(np.abs(z).max())
    return out


def check(st):
    """Assert the bounds above on collect()'s result."""
    for k in ZSCORES:
        assert abs(st[k]) < Z_BOUND, (k, st[k], st)
    assert st["chi2"] < CHI2_BOUND, st
    assert st["max_abs"] <= MAX_ABS_CEILING, st
