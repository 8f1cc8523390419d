"""Classical baseline filters beside the networks: the yardstick a denoising result is read against.

``MovingAverage``, ``SavitzkyGolay``, ``GaussianSmooth`` and ``MedianFilter`` are parameter-free
``nn.Module``s with the networks' calling convention -- ``forward(x: (N, 1, L)) -> (N, 1, L)`` -- so they go
wherever a network goes: ``evaluate``, ``evaluate_synthetic``, the SNR and PhysicsAwareLoss reports.  On a
CUDA tensor without an autograd graph the forward is the HIP kernel (engine.fir / engine.median: sequential
fp64 accumulation, one rounding to fp32; the contract is in include/raman_mi355x.h); otherwise it is
``eager_forward``, the same arithmetic in torch ops on any device.

The filters follow scipy: ``savgol_filter`` (mode 'interp' or 'mirror'), ``uniform_filter1d``,
``gaussian_filter1d`` and ``median_filter`` with mode='mirror'.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine

MAX_WINDOW = engine.FILTER_MAX_WINDOW


def _check_window(window):
    if isinstance(window, bool) or int(window) != window or window % 2 == 0 or not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"the window must be an odd integer in [1, {MAX_WINDOW}], got {window!r}")
    return int(window)


def savgol_taps(window, polyorder):
    """Savitzky-Golay smoothing coefficients as (taps (window,), edge_taps (window - 1, window)), float64.

    A polynomial of degree ``polyorder`` is fitted by least squares to ``window`` samples on the abscissa
    (k - h) / h, h = (window - 1) / 2 (centred and scaled to [-1, 1], which keeps the fit well conditioned
    up to the widest window); ``taps`` evaluates it at the centre.  Row j < h of ``edge_taps`` evaluates the
    fit of a spectrum's first ``window`` samples at position j, row h + j the fit of its last ``window``
    samples at position L - h + j: scipy's savgol_filter(mode='interp')."""
    w = _check_window(window)
    if isinstance(polyorder, bool) or int(polyorder) != polyorder or not 0 <= polyorder <= 5 or polyorder >= w:
        raise ValueError(f"polyorder must be an integer in [0, 5] below the window {w}, got {polyorder!r}")
    h = (w - 1) // 2
    t = (np.arange(w, dtype=np.float64) - h) / max(h, 1)
    A = np.vander(t, int(polyorder) + 1, increasing=True)            # (w, p + 1)
    P = np.linalg.pinv(A)                                             # coefficients = P @ samples
    rows = np.vander(t, int(polyorder) + 1, increasing=True) @ P      # row i: the fit evaluated at position i
    return rows[h].copy(), np.concatenate([rows[:h], rows[h + 1:]], axis=0)


def gaussian_taps(sigma, truncate=4.0):
    """The normalised Gaussian kernel of scipy.ndimage.gaussian_filter1d: radius int(truncate * sigma + 0.5)."""
    sigma, truncate = float(sigma), float(truncate)
    if not (0 < sigma < float("inf") and 0 <= truncate < float("inf")):
        raise ValueError(f"need finite sigma > 0 and truncate >= 0, got {sigma}, {truncate}")
    r = int(truncate * sigma + 0.5)
    if 2 * r + 1 > MAX_WINDOW:
        raise ValueError(f"sigma {sigma} with truncate {truncate} needs a window of {2 * r + 1} > {MAX_WINDOW}")
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


class _Baseline(nn.Module):
    """A parameter-free filter with _EngineNet's forward split (without its training-mode clause: there is
    nothing to train)."""

    window = 1

    def uses_engine(self, x):
        """Whether ``forward(x)`` runs the HIP kernel (True) or the eager torch ops: a CUDA tensor and no
        autograd graph requested through the input."""
        return torch.is_tensor(x) and x.is_cuda and not (torch.is_grad_enabled() and x.requires_grad)

    def engine_forward(self, x):
        raise NotImplementedError

    def eager_forward(self, x):
        raise NotImplementedError

    def forward(self, x):
        if not self.uses_engine(x):
            return self.eager_forward(x)
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{type(self).__name__}: expected input (N, 1, L), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}: expected float32 input, got {x.dtype}")
        return self.engine_forward(x.contiguous())

    def _mirror(self, x):
        """x (N, 1, L) in fp64 with h mirrored samples on each side (no repeated edge sample)."""
        h = (self.window - 1) // 2
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{type(self).__name__}: expected input (N, 1, L), got {tuple(x.shape)}")
        if x.shape[-1] < self.window:
            raise ValueError(f"spectra of {x.shape[-1]} samples are shorter than the window {self.window}")
        return F.pad(x, (h, h), mode="reflect") if h else x


def _sequential(coef, windows):
    """Σ_k coef[..., k] * windows(k) accumulated in order from 0.0: each product and each sum rounded to fp64."""
    acc = None
    for k in range(coef.shape[-1]):
        term = coef[..., k] * windows(k)
        acc = term + 0.0 if acc is None else acc + term
    return acc


class _Fir(_Baseline):
    """A FIR filter: ``taps`` (and, for an edge table, ``edge_taps``) live in non-persistent float64 buffers:
    ``.to(device)`` moves them, ``state_dict()`` is empty."""

    def __init__(self, taps, edge_taps=None):
        super().__init__()
        taps = np.asarray(taps, dtype=np.float64)
        self.window = _check_window(taps.shape[0])
        self.register_buffer("taps", torch.from_numpy(taps.copy()), persistent=False)
        self.register_buffer("edge_taps", None if edge_taps is None else
                             torch.from_numpy(np.asarray(edge_taps, dtype=np.float64).copy()), persistent=False)

    def _coefficients(self, device):
        if self.taps.dtype != torch.float64:
            raise TypeError(f"{type(self).__name__}: the taps were cast to {self.taps.dtype}; the filter's "
                            "arithmetic is float64 (move the module with .to(device), not .float() / .half())")
        if self.taps.device != device:
            raise ValueError(f"{type(self).__name__}: taps on {self.taps.device} but input on {device}; "
                             "move the module with .to(device)")
        return self.taps, self.edge_taps

    def engine_forward(self, x):
        taps, edge = self._coefficients(x.device)
        return engine.fir(x, taps, edge_taps=edge)

    def eager_forward(self, x):
        taps, edge = self._coefficients(x.device)
        w, h, L = self.window, (self.window - 1) // 2, x.shape[-1]
        xp = self._mirror(x.to(torch.float64))
        y = _sequential(taps, lambda k: xp[..., k:k + L])
        if edge is not None and h:
            x64 = x.to(torch.float64)
            head = _sequential(edge[:h], lambda k: x64[..., k:k + 1])
            tail = _sequential(edge[h:], lambda k: x64[..., L - w + k:L - w + k + 1])
            y = torch.cat([head, y[..., h:L - h], tail], dim=-1)
        return y.to(torch.float32)


class MovingAverage(_Fir):
    """Mean over ``window`` samples, mirror edges (scipy.ndimage.uniform_filter1d(mode='mirror'))."""

    def __init__(self, window):
        w = _check_window(window)
        super().__init__(np.full(w, 1.0 / w, dtype=np.float64))


class SavitzkyGolay(_Fir):
    """scipy.signal.savgol_filter(window, polyorder, mode=...): 'interp' fits the first and last ``window``
    samples for the edges (an edge table), 'mirror' mirrors the spectrum."""

    def __init__(self, window, polyorder, mode="interp"):
        if mode not in ("interp", "mirror"):
            raise ValueError(f"mode must be 'interp' or 'mirror', got {mode!r}")
        taps, edge = savgol_taps(window, polyorder)
        super().__init__(taps, edge if mode == "interp" and len(edge) else None)
        self.polyorder, self.mode = int(polyorder), mode


class GaussianSmooth(_Fir):
    """scipy.ndimage.gaussian_filter1d(sigma, truncate=..., mode='mirror')."""

    def __init__(self, sigma, truncate=4.0):
        super().__init__(gaussian_taps(sigma, truncate))
        self.sigma, self.truncate = float(sigma), float(truncate)


def _keys(x):
    """The monotone key (int64 in [0, 2^32)) of float32 samples: -0 < +0, the infinities ordinary values;
    every NaN gets the largest key."""
    bits = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    return torch.where(torch.isnan(x), torch.full_like(key, 0xFFFFFFFF), key)


class MedianFilter(_Baseline):
    """Running median over ``window`` samples, mirror edges (scipy.ndimage.median_filter(mode='mirror')):
    each output is one of the inputs; a window that holds a NaN gives NaN."""

    def __init__(self, window):
        super().__init__()
        self.window = _check_window(window)

    def engine_forward(self, x):
        return engine.median(x, self.window)

    def eager_forward(self, x):
        if x.dtype != torch.float32:
            raise TypeError(f"MedianFilter: expected float32 input, got {x.dtype}")
        w, h = self.window, (self.window - 1) // 2
        win = self._mirror(x).unfold(-1, w, 1)                       # (N, 1, L, w)
        key = _keys(win.detach())
        pick = key.kthvalue(h + 1, dim=-1).indices.unsqueeze(-1)
        y = win.gather(-1, pick).squeeze(-1)
        return torch.where(key.amax(dim=-1) == 0xFFFFFFFF, torch.full_like(y, float("nan")), y)   # 0x7fc00000


BASELINES = {cls.__name__: cls for cls in (MovingAverage, SavitzkyGolay, GaussianSmooth, MedianFilter)}
