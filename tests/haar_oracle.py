"""numpy restatement of the contract of the translation-invariant Haar shrinkage (include/raman_mi355x.h
rdn_haar_shrink), and a second, independent reference: cycle spinning of the decimated orthonormal Haar
transform.  Written for clarity, not speed; shared by the CPU and GPU tests.
"""
import numpy as np

QUIET_NAN = np.uint32(0x7FC00000)
MAD_TO_SIGMA = 0.6744897501960817


def haar_shrink(x, k, mode):
    """x float32 (..., L); k float64 (J,); mode 'soft' or 'hard'.  Returns (y float32, m float64 (...,)): each
    line below is one fp64 operation of the contract, vectorised over the samples only."""
    x = np.asarray(x, dtype=np.float32)
    k = np.asarray(k, dtype=np.float64)
    J, L = k.shape[0], x.shape[-1]
    assert mode in ("soft", "hard") and 1 <= J <= 7 and L >= 2 ** J
    with np.errstate(all="ignore"):
        a = x.astype(np.float64)
        m = np.median(np.abs(0.5 * (a - np.roll(a, 1, axis=-1))), axis=-1)
        e = []
        for j in range(1, J + 1):
            q = np.roll(a, 2 ** (j - 1), axis=-1)                  # a_{j-1}[idx(i - s)]
            d = 0.5 * (a - q)
            a = 0.5 * (a + q)
            t = (k[j - 1] * m)[..., None]
            if mode == "hard":
                e.append(np.where(np.abs(d) > t, d, 0.0))
            else:
                e.append(np.where(d > t, d - t, np.where(d < -t, d + t, 0.0)))
        for j in range(J, 0, -1):
            s = 2 ** (j - 1)
            a = 0.5 * ((a + e[j - 1]) + (np.roll(a, -s, axis=-1) - np.roll(e[j - 1], -s, axis=-1)))
        y = a.astype(np.float32)
    bad = ~np.isfinite(x).all(axis=-1)
    bits = np.where(bad[..., None], QUIET_NAN, y.view(np.uint32)).astype(np.uint32)
    return bits.view(np.float32), np.where(bad, np.nan, m)


def thresholds(levels, lam):
    """k of the contract for a threshold of lam noise standard deviations."""
    return np.array([lam * 2.0 ** ((1 - j) / 2) / MAD_TO_SIGMA for j in range(1, levels + 1)], dtype=np.float64)


def cycle_spin(x, levels, lam, mode):
    """The average over all 2^levels circular shifts of: shift, decimated orthonormal Haar transform (pairs
    (v[2i], v[2i+1]) -> ((u + w) / sqrt 2, (u - w) / sqrt 2)), details thresholded at lam * sigma, inverse
    transform, shift back.  sigma = m sqrt 2 / 0.6745, m the median of |x[i] - x[i-1]| / 2 over the periodic
    spectrum.  Needs 2^levels | L.  float64 in and out."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-1]
    assert L % 2 ** levels == 0
    r2 = np.sqrt(2.0)
    m = np.median(np.abs(x - np.roll(x, 1, axis=-1)) / 2, axis=-1)
    T = (lam * m * r2 / MAD_TO_SIGMA)[..., None]
    acc = np.zeros_like(x)
    for h in range(2 ** levels):
        a = np.roll(x, -h, axis=-1)
        det = []
        for _ in range(levels):
            u, w = a[..., 0::2], a[..., 1::2]
            d = (u - w) / r2
            a = (u + w) / r2
            det.append(np.where(np.abs(d) > T, d, 0.0) if mode == "hard" else np.sign(d) * np.maximum(np.abs(d) - T, 0.0))
        for d in reversed(det):
            up = np.empty(a.shape[:-1] + (2 * a.shape[-1],))
            up[..., 0::2] = (a + d) / r2
            up[..., 1::2] = (a - d) / r2
            a = up
        acc += np.roll(a, h, axis=-1)
    return acc / 2 ** levels


def noisy_steps(n, L, seed, sigma=0.03):
    """Piecewise-constant spectra in [0, 1] (segments of 1-40 samples) under white Gaussian noise, fp32."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, L))
    for r in range(n):
        x[r] = np.repeat(rng.uniform(0, 1, L), rng.integers(1, 41, size=L))[:L]
    return (x + rng.normal(0, sigma, (n, L))).astype(np.float32)
