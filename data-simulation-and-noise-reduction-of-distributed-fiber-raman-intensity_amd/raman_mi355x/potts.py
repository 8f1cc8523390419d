"""The exact piecewise-constant (Potts) fit: the estimator that matches the simulator's signal model -- runs of
equal samples under white noise -- beside the networks, the linear filters of baselines.py and the wavelet
shrinkage of wavelets.py.

``PottsFit`` is a parameter-free ``nn.Module`` with the networks' calling convention -- ``forward(x: (N, 1, L)) ->
(N, 1, L)``.  Each spectrum is replaced by the step function, with runs of at most ``max_len`` samples, that
minimises Σ (x - fit)² + gamma · #runs exactly (dynamic programming over the run ends); gamma = ``penalty`` ·
sigma², sigma the spectrum's own blind noise estimate (HaarShrink's: the median |d_1| times sqrt(2) / 0.6745).  On
a CUDA tensor without an autograd graph the forward is the HIP kernel (engine.noise_mad, engine.potts); otherwise
``eager_forward``, the same recurrence in torch float64 ops on any device, bit for bit, differentiable with the
segmentation held fixed.  The arithmetic contract is in include/raman_mi355x.h (rdn_potts).
"""
import math

import torch

from . import engine
from .baselines import _Baseline
from .wavelets import MAD_TO_SIGMA, _median_abs_d1

MAX_LEN = engine.POTTS_MAX_LEN


def _fit(a, g, K):
    """The contract's recurrence on a (N, L) float64 and g (N,) float64.  Returns (S1 (N, L + 1), start, end
    (N, L) int64: the run [start, end) that holds each position, nseg (N,) int32, bad (N,) bool)."""
    N, L = a.shape
    dev = a.device
    S1 = torch.zeros((N, L + 1), dtype=torch.float64, device=dev)
    S2 = torch.zeros_like(S1)
    B = torch.zeros_like(S1)
    A = torch.ones((N, L + 1), dtype=torch.int64, device=dev)
    lens = torch.arange(1, K + 1, dtype=torch.int64, device=dev)
    lensf = lens.to(torch.float64)
    gcol = g.unsqueeze(-1)
    s1 = torch.zeros(N, dtype=torch.float64, device=dev)
    s2 = torch.zeros_like(s1)
    for r in range(1, L + 1):
        v = a[:, r - 1]
        s1 = s1 + v
        s2 = s2 + v * v
        S1[:, r], S2[:, r] = s1, s2
        k = min(K, r)                                               # candidates len = 1 .. k: l = r - 1 .. r - k
        d1 = s1.unsqueeze(-1) - S1[:, r - k:r].flip(-1)
        d2 = s2.unsqueeze(-1) - S2[:, r - k:r].flip(-1)
        sse = d2 - (d1 * d1) / lensf[:k]
        c = (B[:, r - k:r].flip(-1) + gcol) + sse
        m = c.min(dim=-1).values
        B[:, r] = m
        A[:, r] = torch.where(c == m.unsqueeze(-1), lens[:k], k).min(dim=-1).values     # the smallest len that attains it
    rows = torch.arange(N, device=dev)
    ends = torch.zeros((N, L + 1), dtype=torch.bool, device=dev)
    ends[:, 0] = True
    nseg = torch.zeros(N, dtype=torch.int32, device=dev)
    r = torch.full((N,), L, dtype=torch.int64, device=dev)
    while bool((r > 0).any()):
        ends[rows, r] = True
        nseg += (r > 0).to(torch.int32)
        r = r - torch.where(r > 0, A[rows, r], torch.zeros_like(r))
    idx = torch.arange(L + 1, dtype=torch.int64, device=dev).expand(N, L + 1)
    start = torch.where(ends, idx, torch.zeros_like(idx))[:, :L].cummax(dim=-1).values
    end = torch.where(ends, idx, torch.full_like(idx, L + 1))[:, 1:].flip(-1).cummin(dim=-1).values.flip(-1)
    bad = ~(torch.isfinite(a).all(dim=-1) & (g >= 0) & torch.isfinite(g))
    return S1, start, end, torch.where(bad, torch.zeros_like(nseg), nseg), bad


class _PottsFunction(torch.autograd.Function):
    """y = the run means of the fit; backward: the upstream gradient averaged over each run (the segmentation is
    piecewise constant in x, so it is held fixed; gamma gets no gradient)."""

    @staticmethod
    def forward(ctx, x, g, K):
        a = x.detach().to(torch.float64).reshape(x.shape[0], x.shape[-1])
        S1, start, end, _, bad = _fit(a, g.detach(), K)
        mean = (S1.gather(1, end) - S1.gather(1, start)) / (end - start).to(torch.float64)
        y = mean.to(torch.float32)
        y = torch.where(bad.unsqueeze(-1), torch.full_like(y, float("nan")), y)           # 0x7fc00000
        ctx.save_for_backward(start, end, bad)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, grad):
        start, end, bad = ctx.saved_tensors
        N, L = start.shape
        G = torch.zeros((N, L + 1), dtype=torch.float64, device=grad.device)
        G[:, 1:] = grad.reshape(N, L).to(torch.float64).cumsum(dim=-1)
        gx = (G.gather(1, end) - G.gather(1, start)) / (end - start).to(torch.float64)
        gx = torch.where(bad.unsqueeze(-1), torch.zeros_like(gx), gx)
        return gx.to(grad.dtype).reshape(grad.shape), None, None


class PottsFit(_Baseline):
    """The exact piecewise-constant fit with runs of at most ``max_len`` samples (1 to 64) and a jump penalty of
    ``penalty`` estimated noise variances per run: a positive float, or 'bic' for 2 ln L.  The default, 12, is the
    middle of the flat optimum (10 to 14) on the reference generator's spectra."""

    def __init__(self, penalty=12.0, max_len=MAX_LEN):
        super().__init__()
        if isinstance(max_len, bool) or int(max_len) != max_len or not 1 <= max_len <= MAX_LEN:
            raise ValueError(f"max_len must be an integer in [1, {MAX_LEN}], got {max_len!r}")
        if isinstance(penalty, str):
            if penalty != "bic":
                raise ValueError(f"penalty must be a positive float or 'bic', got {penalty!r}")
        elif isinstance(penalty, bool) or not 0.0 < float(penalty) < float("inf"):
            raise ValueError(f"penalty must be positive and finite, got {penalty!r}")
        self.penalty = penalty if isinstance(penalty, str) else float(penalty)
        self.max_len = int(max_len)

    def factor(self, L):
        """The penalty in noise variances for spectra of L samples."""
        return 2.0 * math.log(L) if self.penalty == "bic" else self.penalty

    def _check(self, x):
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{type(self).__name__}: expected input (N, 1, L), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}: expected float32 input, got {x.dtype}")
        if x.shape[-1] < 1:
            raise ValueError("spectra must have at least one sample")

    def noise_std(self, x):
        """The blind noise estimate of each spectrum of ``x`` (N, 1, L): sigma = m * sqrt(2) / 0.6745, float64 (N,),
        HaarShrink.noise_std's; NaN for a spectrum with a NaN or an infinity."""
        self._check(x)
        with torch.no_grad():
            if self.uses_engine(x):
                m = engine.noise_mad(x.contiguous())
            else:
                m, finite = _median_abs_d1(x.to(torch.float64).squeeze(1))
                m = torch.where(finite, m, torch.full_like(m, float("nan")))
            return m * (math.sqrt(2.0) / MAD_TO_SIGMA)

    def gamma(self, x):
        """The jump penalty of each spectrum: penalty * sigma², float64 (N,)."""
        sigma = self.noise_std(x)
        return self.factor(x.shape[-1]) * (sigma * sigma)

    def engine_forward(self, x):
        return engine.potts(x, self.gamma(x), self.max_len)[0]

    def eager_forward(self, x):
        self._check(x)
        return _PottsFunction.apply(x, self.gamma(x), self.max_len)

    def segments(self, x):
        """The number of runs of each spectrum's fit, int32 (N,); 0 where the fit is NaN."""
        self._check(x)
        if self.uses_engine(x):
            return engine.potts(x.contiguous(), self.gamma(x), self.max_len)[1]
        with torch.no_grad():
            return _fit(x.detach().to(torch.float64).squeeze(1), self.gamma(x), self.max_len)[3]
