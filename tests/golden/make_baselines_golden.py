"""Writes tests/golden/baselines.npz: small fp32 spectra and what scipy's filters make of them in float64.

    python tests/golden/make_baselines_golden.py          (scipy 1.15; numpy's default_rng(20251020))

Inputs ``x_<L>``: 3 spectra at each L of LENGTHS -- piecewise constant with segments of 1-40 samples, Gaussian
noise and one spike.  Outputs, float64 (the median's float32: it returns input samples):
  savgol_<w>_<p>_<mode>_<L>   scipy.signal.savgol_filter(x, w, p, mode=mode), mode in interp / mirror, w <= L
  uniform_9_<L>               scipy.ndimage.uniform_filter1d(x, 9, mode='mirror')
  gauss_<sigma>_<L>           scipy.ndimage.gaussian_filter1d(x, sigma, mode='mirror')
  median_<w>_<L>              scipy.ndimage.median_filter(x, size=(1, w), mode='mirror'), w <= L
"""
import os

import numpy as np
import scipy.ndimage as ndi
import scipy.signal as sig

LENGTHS = (21, 22, 255, 256, 1000)
SAVGOL = ((3, 0), (5, 2), (21, 3), (21, 0), (11, 5), (255, 3))
GAUSS = (1.0, 2.5)
MEDIAN = (3, 21, 101)


def spectra(rng, n, L):
    x = np.empty((n, L), dtype=np.float64)
    for r in range(n):
        pos = 0
        while pos < L:
            seg = int(rng.integers(1, 41))
            x[r, pos:pos + seg] = rng.uniform(0.0, 1.0)
            pos += seg
        x[r] += rng.normal(0.0, 0.05, L)
        x[r, int(rng.integers(0, L))] += 3.0
    return x.astype(np.float32)


def main():
    rng = np.random.default_rng(20251020)
    out = {}
    for L in LENGTHS:
        x = spectra(rng, 3, L)
        x64 = x.astype(np.float64)
        out[f"x_{L}"] = x
        for w, p in SAVGOL:
            if w <= L:
                for mode in ("interp", "mirror"):
                    out[f"savgol_{w}_{p}_{mode}_{L}"] = sig.savgol_filter(x64, w, p, axis=-1, mode=mode)
        out[f"uniform_9_{L}"] = ndi.uniform_filter1d(x64, 9, axis=-1, mode="mirror")
        for s in GAUSS:
            out[f"gauss_{s}_{L}"] = ndi.gaussian_filter1d(x64, s, axis=-1, mode="mirror")
        for w in MEDIAN:
            if w <= L:
                out[f"median_{w}_{L}"] = ndi.median_filter(x, size=(1, w), mode="mirror")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "baselines.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
