"""Translation-invariant Haar wavelet shrinkage: the classical denoiser of a piecewise-constant signal under
white noise (Coifman & Donoho's cycle spinning), beside the networks and the linear filters of baselines.py.

``HaarShrink`` is a parameter-free ``nn.Module`` with the networks' calling convention -- ``forward(x: (N, 1, L))
-> (N, 1, L)``.  Each spectrum is taken through ``levels`` levels of the undecimated Haar transform with periodic
indexing; detail plane j is thresholded at ``k[j - 1] * m``, where m is the spectrum's own median |d_1| (so the
threshold follows a blind noise estimate, sigma = m * sqrt(2) / 0.6745); the inverse transform averages the
2^levels shifted reconstructions.  On a CUDA tensor without an autograd graph the forward is the HIP kernel
(engine.haar_shrink); otherwise ``eager_forward``, the same recurrence in torch float64 ops on any device, bit
for bit.  The arithmetic contract is in include/raman_mi355x.h (rdn_haar_shrink).
"""
import math

import numpy as np
import torch

from . import engine
from .baselines import _Baseline

MAX_LEVELS = engine.HAAR_MAX_LEVELS
MAD_TO_SIGMA = 0.6744897501960817          # the median of |N(0, 1)|


def _check_levels(levels):
    if isinstance(levels, bool) or int(levels) != levels or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be an integer in [1, {MAX_LEVELS}], got {levels!r}")
    return int(levels)


def haar_thresholds(levels, threshold, L):
    """The float64 factors k (levels,) of rdn_haar_shrink for a threshold of ``threshold`` noise standard
    deviations: k[j - 1] = threshold * 2^((1 - j) / 2) / 0.6744897501960817 (plane j of the undecimated
    transform carries noise of sigma / 2^(j/2); sigma is estimated as m * sqrt(2) / 0.6745).  ``threshold``: a
    positive float, or 'universal' for sqrt(2 ln L).  ``L``: the spectra's length, >= 2^levels."""
    J = _check_levels(levels)
    if isinstance(L, bool) or int(L) != L or L < 2 ** J:
        raise ValueError(f"L must be an integer >= 2^{J}, got {L!r}")
    if isinstance(threshold, str):
        if threshold != "universal":
            raise ValueError(f"threshold must be a positive float or 'universal', got {threshold!r}")
        lam = math.sqrt(2.0 * math.log(int(L)))
    else:
        if isinstance(threshold, bool):
            raise ValueError(f"threshold must be a positive float or 'universal', got {threshold!r}")
        lam = float(threshold)
        if not 0.0 < lam < float("inf"):
            raise ValueError(f"threshold must be positive and finite, got {threshold!r}")
    return np.array([lam * 2.0 ** ((1 - j) / 2) / MAD_TO_SIGMA for j in range(1, J + 1)], dtype=np.float64)


def _median_abs_d1(a0):
    """(m, finite) per row of a0 (..., L) float64: numpy's median of |0.5 (a0[i] - a0[i - 1])|, periodic."""
    d1 = (0.5 * (a0 - torch.roll(a0, 1, -1))).abs()
    L = a0.shape[-1]
    srt = d1.sort(dim=-1).values
    m = srt[..., (L - 1) // 2] if L % 2 else 0.5 * (srt[..., L // 2 - 1] + srt[..., L // 2])
    return m, torch.isfinite(a0).all(dim=-1)


class HaarShrink(_Baseline):
    """Translation-invariant Haar shrinkage over ``levels`` levels at ``threshold`` estimated noise standard
    deviations (a positive float or 'universal'), ``mode`` 'hard' or 'soft'."""

    def __init__(self, levels=4, threshold=3.0, mode="hard"):
        super().__init__()
        self.levels = _check_levels(levels)
        if mode not in engine.HAAR_MODES:
            raise ValueError(f"mode must be 'soft' or 'hard', got {mode!r}")
        haar_thresholds(self.levels, threshold, 2 ** self.levels)       # refuses a bad threshold here
        self.threshold, self.mode = threshold, mode

    def factors(self, L):
        return haar_thresholds(self.levels, self.threshold, L)

    def engine_forward(self, x):
        return engine.haar_shrink(x, self.factors(x.shape[-1]), self.mode)[0]

    def _check(self, x):
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{type(self).__name__}: expected input (N, 1, L), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}: expected float32 input, got {x.dtype}")
        if x.shape[-1] < 2 ** self.levels:
            raise ValueError(f"spectra of {x.shape[-1]} samples are shorter than 2^{self.levels}")

    def eager_forward(self, x):
        self._check(x)
        k = self.factors(x.shape[-1])
        a = x.to(torch.float64)
        m, finite = _median_abs_d1(a)
        m = m.unsqueeze(-1)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        planes = []
        for j in range(1, self.levels + 1):
            q = torch.roll(a, 2 ** (j - 1), -1)                          # a_{j-1}[i - s]
            d = 0.5 * (a - q)
            a = 0.5 * (a + q)
            t = float(k[j - 1]) * m
            if self.mode == "hard":
                planes.append(torch.where(d.abs() > t, d, zero))
            else:
                planes.append(torch.where(d > t, d - t, torch.where(d < -t, d + t, zero)))
        for j in range(self.levels, 0, -1):
            e, s = planes[j - 1], 2 ** (j - 1)
            a = 0.5 * ((a + e) + (torch.roll(a, -s, -1) - torch.roll(e, -s, -1)))
        y = a.to(torch.float32)
        return torch.where(finite.unsqueeze(-1), y, torch.full_like(y, float("nan")))     # 0x7fc00000

    def noise_std(self, x):
        """The blind noise estimate of each spectrum of ``x`` (N, 1, L): sigma = m * sqrt(2) / 0.6745, float64
        (N,); NaN for a spectrum with a NaN or an infinity.  On the device this is the whole engine.haar_shrink
        call -- the median comes with a denoised output that is dropped here -- so a caller who wants both takes
        them from one engine.haar_shrink call."""
        self._check(x)
        if self.uses_engine(x):
            m = engine.haar_shrink(x.contiguous(), self.factors(x.shape[-1]), self.mode)[1]
        else:
            m, finite = _median_abs_d1(x.to(torch.float64).squeeze(1))
            m = torch.where(finite, m, torch.full_like(m, float("nan")))
        return m * (math.sqrt(2.0) / MAD_TO_SIGMA)
