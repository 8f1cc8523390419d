"""Drop-in ``PhysicsAwareLoss`` (PIDN/train.py:109-146; APIDN/train.py:162-199 is the same class).

``criterion = PhysicsAwareLoss()`` works in the reference's training loop unchanged: whenever a gradient
is wanted (or the tensors are on the CPU, or of another dtype) ``forward`` is the reference's formula on
torch ops -- differentiable, the eager path.  When only the value is wanted -- validation under
``torch.no_grad()``, a report -- and the tensors are contiguous CUDA float32 (clean float32 or float64),
one launch of the fp64 device kernel (engine.physics) computes the per-spectrum totals and the loss is
their mean, taken on the device without a host sync: the engine path.
"""
import torch
import torch.nn as nn

from . import engine


def physics_terms(pred, clean, noisy):
    """The four terms of the loss over the whole batch, on torch ops (differentiable):
    (MSE, Smooth, Peak, Noise) as 0-dim tensors -- the reference's mse_loss, smooth_loss, peak_loss and
    poisson_loss."""
    mse = torch.mean((pred - clean) ** 2)
    smooth = torch.mean(torch.abs(torch.diff(pred, dim=-1) - torch.diff(clean, dim=-1)))
    mask = (torch.diff(clean, n=2, dim=-1) < 0).float()
    peak = torch.mean((pred[..., 1:-1] * mask - clean[..., 1:-1] * mask) ** 2)
    noise = noisy - clean
    var = torch.var(noise, dim=-1, keepdim=True)
    poisson = torch.mean((noise ** 2 - var) ** 2)
    return mse, smooth, peak, poisson


class PhysicsAwareLoss(nn.Module):
    """MSE + alpha * smoothness (L1 of the first differences) + beta * peak retention (MSE at the positions
    where clean's second difference is negative) + gamma * noise model (variance stability of
    noisy - clean)."""

    def __init__(self, alpha=0.1, beta=0.05, gamma=0.01):
        super().__init__()
        self.alpha = alpha
        self.beta = beta
        self.gamma = gamma

    def uses_engine(self, pred, clean, noisy):
        """Whether forward() takes the engine path for these tensors."""
        ts = (pred, clean, noisy)
        if not all(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() for t in ts):
            return False
        if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
            return False
        if pred.dtype != torch.float32 or noisy.dtype != torch.float32 or clean.dtype not in (torch.float32, torch.float64):
            return False
        if pred.shape != clean.shape or pred.shape != noisy.shape or pred.device != clean.device or pred.device != noisy.device:
            return False
        if not (pred.dim() == 2 or (pred.dim() == 3 and pred.shape[1] == 1)):
            return False
        return pred.shape[0] >= 1 and pred.shape[-1] >= 3

    def forward(self, pred, clean, noisy):
        if self.uses_engine(pred, clean, noisy):
            per, _ = engine.physics(noisy, pred, clean, weights=(self.alpha, self.beta, self.gamma))
            return per[:, 4].mean().to(pred.dtype)
        mse, smooth, peak, poisson = physics_terms(pred, clean, noisy)
        return mse + self.alpha * smooth + self.beta * peak + self.gamma * poisson
