"""Writes tests/golden/snr.npz: 8 spectra of the REFERENCE generator (数据集产生.py:5-64, loaded through
_refload without running the script), L = 2000, no extreme noise, stored as float32, with the nominal
SNR the generator drew (``snrs``) and the SNR_in that plain numpy float64 measures on the stored arrays
with P = mean(clean^2).  Run in the build container only (it reads the reference); tests read the .npz.

The fixture anchors the definition: were P anything but the generator's own signal power, the measured
SNR_in would not estimate ``snrs``.  The estimate's spread is that of a variance estimate over L samples,
sd(10 log10(Ni)) = (10 / ln 10) sqrt(2 / L); the check below allows five of them."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

SEED = 20250411
N, L = 8, 2000


def main():
    gen = _refload.load_generate_signals()
    np.random.seed(SEED)
    clean, noisy, snrs, noise_std = gen(N, signal_length=L, extreme_noise_prob=0)
    clean32, noisy32 = clean.astype(np.float32), noisy.astype(np.float32)
    c, x = clean32.astype(np.float64), noisy32.astype(np.float64)
    snr_in = 10.0 * np.log10(np.mean(c ** 2, axis=1) / np.mean((x - c) ** 2, axis=1))
    snrs = snrs.reshape(-1)
    bound = 5 * (10 / math.log(10)) * math.sqrt(2 / L)
    dev = np.abs(snr_in - snrs)
    print("nominal", snrs, "\nmeasured", snr_in, f"\nmax |diff| {dev.max():.4f} dB, bound {bound:.4f} dB")
    assert np.all(dev <= bound), "pick another seed; the bound stays"
    np.savez_compressed(os.path.join(HERE, "snr.npz"), clean=clean32, noisy=noisy32, snrs=snrs, snr_in=snr_in,
                        seed=np.int64(SEED))


if __name__ == "__main__":
    main()
