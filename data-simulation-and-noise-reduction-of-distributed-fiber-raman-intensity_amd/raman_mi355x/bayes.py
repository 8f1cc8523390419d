"""The Bayesian change-point smoother: the posterior mean under the simulator's own signal model -- runs of 1 to
``max_len`` equal samples, levels uniform on a range, white Gaussian noise -- beside the exact piecewise-constant
fit of potts.py, which is the point estimate of the same model with a hand-set penalty.

``BayesSteps`` is a parameter-free ``nn.Module`` with the networks' calling convention -- ``forward(x: (N, 1, L)) ->
(N, 1, L)``.  Each spectrum is replaced by the mean over ALL segmentations into runs of at most ``max_len`` samples,
each weighted by its posterior probability given the spectrum's noise level sigma (an exact forward-backward
recursion over the run boundaries, fp64).  For this signal model and this sigma it is the estimate of least mean
squared error: no denoiser can be better on average, so its gain is the floor a network's is to be read against.
Nothing is tuned: the weight of a jump follows from sigma, ``max_len`` and ``level_range``.  The same recursion gives
the posterior probability that a run starts at each sample (``jump_probability``) and the log evidence of each
spectrum (``log_evidence``).  On a CUDA tensor without an autograd graph the forward is the HIP kernel
(engine.noise_mad, engine.bayes_steps); otherwise ``eager_forward``, the same recursion in torch float64 ops on
any device, differentiable by plain autograd.  The arithmetic contract is in include/raman_mi355x.h
(rdn_bayes_steps).
"""
import math

import torch
import torch.nn.functional as F

from . import engine
from .baselines import _Baseline
from .wavelets import MAD_TO_SIGMA, _median_abs_d1

MAX_LEN = engine.BAYES_MAX_LEN
SQRT_2PI = 2.5066282746310002


def _sweep(a, prev, base, h, rn, K, reverse):
    """One sweep of the contract over a (N, L) float64: the boundary values (N, L + 1) (G right to left, F left to
    right) and, per step, what the second sweep needs: (M, e, S, mean) of the step's LSE.  ``prev`` (N,): the value
    at the sweep's first boundary (0)."""
    N, L = a.shape
    vals = [prev]
    win = prev.new_full((N, 0), 0.0)                               # the values at the last k boundaries, nearest first
    mean = prev.new_zeros((N, 0))
    M2 = prev.new_zeros((N, 0))
    zero = prev.new_zeros((N, 1))
    steps = []
    for i in range(L):
        v = (a[:, L - 1 - i] if reverse else a[:, i]).unsqueeze(-1)
        k = min(K, i + 1)
        win = torch.cat([vals[-1].unsqueeze(-1), win[:, :K - 1]], dim=1)
        m_old = torch.cat([zero, mean[:, :K - 1]], dim=1)          # n = 1 starts from (0, 0): mean = v, M2 = 0
        M2_old = torch.cat([zero, M2[:, :K - 1]], dim=1)
        d = v - m_old
        mean = m_old + d * rn[:k]
        M2 = M2_old + d * (v - mean)
        t = win + (base[:, :k] - M2 * h)
        M = t.max(dim=1, keepdim=True).values.detach()
        e = torch.exp(t - M)
        S = e.sum(dim=1, keepdim=True)
        vals.append((M + torch.log(S)).squeeze(-1))
        steps.append((M, e, S, mean))
    out = torch.stack(vals[::-1] if reverse else vals, dim=1)
    return out, steps


def _posterior(a, sigma, K, W):
    """The contract on a (N, L) float64 and sigma (N,) float64: (y (N, L) float64, jump (N, L) float64, logZ (N,),
    bad (N,) bool).  Differentiable."""
    N, L = a.shape
    lens = torch.arange(1, K + 1, dtype=torch.float64, device=a.device)
    rn = 1.0 / lens
    c0 = torch.log((SQRT_2PI * sigma) / (W * float(K)))
    h = (1.0 / ((2.0 * sigma) * sigma)).unsqueeze(-1)
    base = c0.unsqueeze(-1) - 0.5 * torch.log(lens)
    bad = ~(torch.isfinite(a).all(dim=-1) & (sigma > 0) & torch.isfinite(sigma) & torch.isfinite(h.squeeze(-1)))
    zero = sigma.new_zeros(N)
    G, _ = _sweep(a, zero, base, h, rn, K, reverse=True)
    logZ = G[:, 0]
    _, steps = _sweep(a, zero, base, h, rn, K, reverse=False)
    jump = [torch.ones_like(logZ)]
    contrib = []
    for t in range(1, L + 1):
        M, e, S, mean = steps[t - 1]
        c = torch.exp((M + G[:, t:t + 1]) - logZ.unsqueeze(-1))
        if t < L:
            jump.append((S * c).squeeze(-1))
        q = (e * c) * mean                                          # column n - 1: the run [t - n, t)
        q = q.flip(1).cumsum(dim=1).flip(1)                         # column d - 1: what sample t - d receives
        contrib.append(F.pad(q, (0, K - q.shape[1])))
    C = torch.stack(contrib, dim=1)                                 # (N, L, K)
    y = a.new_zeros((N, L))
    for d in range(1, min(K, L) + 1):                               # in the order of the run ends
        y = y + F.pad(C[:, d - 1:, d - 1], (0, d - 1))
    return y, torch.stack(jump, dim=1), logZ, bad


class BayesSteps(_Baseline):
    """The posterior mean over every segmentation into runs of at most ``max_len`` samples (1 to 64; the default,
    40, is the simulator's max_repeat) with levels uniform on a range of width ``level_range`` (the default, 1, is
    the normalised intensity range).  ``sigma``: the noise's standard deviation, a float for every spectrum or a
    tensor with one per spectrum; None: each spectrum's own blind estimate (PottsFit.noise_std's: the median
    |d_1| times sqrt(2) / 0.6745).  A spectrum whose blind estimate is 0 (a constant spectrum, or one whose
    neighbouring samples are mostly equal) has no noise level to weigh a jump against: the engine refuses it and
    it comes back NaN; give ``sigma=`` for such data."""

    def __init__(self, max_len=40, level_range=1.0, sigma=None):
        super().__init__()
        if isinstance(max_len, bool) or int(max_len) != max_len or not 1 <= max_len <= MAX_LEN:
            raise ValueError(f"max_len must be an integer in [1, {MAX_LEN}], got {max_len!r}")
        if isinstance(level_range, bool) or not 0.0 < float(level_range) < float("inf"):
            raise ValueError(f"level_range must be positive and finite, got {level_range!r}")
        if sigma is not None and not torch.is_tensor(sigma):
            if isinstance(sigma, bool) or not 0.0 < float(sigma) < float("inf"):
                raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
            sigma = float(sigma)
        self.max_len = int(max_len)
        self.level_range = float(level_range)
        self.sigma = sigma

    def _check(self, x):
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{type(self).__name__}: expected input (N, 1, L), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}: expected float32 input, got {x.dtype}")
        if x.shape[-1] < 1:
            raise ValueError("spectra must have at least one sample")

    def noise_std(self, x):
        """The noise level used for each spectrum of ``x`` (N, 1, L), float64 (N,): ``sigma`` if it was given,
        else the blind estimate m * sqrt(2) / 0.6745 (NaN for a spectrum with a NaN or an infinity)."""
        self._check(x)
        n = x.shape[0]
        if torch.is_tensor(self.sigma):
            s = self.sigma.detach().to(device=x.device, dtype=torch.float64).reshape(-1)
            if s.numel() != n:
                raise ValueError(f"sigma has {s.numel()} entries for {n} spectra")
            return s.contiguous()
        if self.sigma is not None:
            return torch.full((n,), self.sigma, dtype=torch.float64, device=x.device)
        with torch.no_grad():
            if self.uses_engine(x):
                m = engine.noise_mad(x.contiguous())
            else:
                m, finite = _median_abs_d1(x.to(torch.float64).squeeze(1))
                m = torch.where(finite, m, torch.full_like(m, float("nan")))
            return m * (math.sqrt(2.0) / MAD_TO_SIGMA)

    def _engine(self, x):
        x = x.contiguous()
        return engine.bayes_steps(x, self.noise_std(x), self.max_len, self.level_range)

    def _eager(self, x):
        self._check(x)
        y, jump, logz, bad = _posterior(x.to(torch.float64).squeeze(1), self.noise_std(x), self.max_len,
                                        self.level_range)
        nan = bad.unsqueeze(-1)
        y = torch.where(nan, torch.full_like(y, float("nan")), y).to(torch.float32)
        jump = torch.where(nan, torch.full_like(jump, float("nan")), jump).to(torch.float32)
        return y.unsqueeze(1), jump.unsqueeze(1), torch.where(bad, torch.full_like(logz, float("nan")), logz)

    def engine_forward(self, x):
        return self._engine(x)[0]

    def eager_forward(self, x):
        return self._eager(x)[0]

    def _all(self, x):
        self._check(x)
        return self._engine(x) if self.uses_engine(x) else self._eager(x)

    def jump_probability(self, x):
        """The posterior probability that a run starts at each sample, float32 (N, 1, L); 1 at the first."""
        return self._all(x)[1]

    def log_evidence(self, x):
        """The log evidence of each spectrum under the model, float64 (N,) (up to the constant the contract
        drops: comparable between sigma, max_len and level_range on the same spectrum)."""
        return self._all(x)[2]
