"""Drop-in ``PhysicsAwareLoss`` (PIDN/train.py:109-146; APIDN/train.py:162-199 is the same class).

``criterion = PhysicsAwareLoss()`` works in the reference's training loop unchanged: whenever a gradient
is wanted (or the tensors are on the CPU, or of another dtype) ``forward`` is the reference's formula on
torch ops -- differentiable, the eager path.  When only the value is wanted -- validation under
``torch.no_grad()``, a report -- and the tensors are contiguous CUDA float32 (clean float32 or float64),
one launch of the fp64 device kernel (engine.physics) computes the per-spectrum totals and the loss is
their mean, taken on the device without a host sync: the engine path.

``PhysicsAwareLoss(fused_backward=True)`` takes the device into the training step as well: when ``pred``
wants a gradient (and ``clean`` and ``noisy`` do not) and the tensors are what the engine path takes, one
launch (engine.physics_grad) gives the per-spectrum totals and d loss / d pred, the loss is the same bits
as the engine path's, and backward is that gradient times the incoming one: the fused path.  It is not
differentiable twice.  Everything else takes the paths above.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

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


class _FusedPhysicsLoss(torch.autograd.Function):
    """The loss and d loss / d pred from one launch (engine.physics_grad with scale = 1 / N)."""

    @staticmethod
    def forward(ctx, pred, clean, noisy, weights):
        per, grad = engine.physics_grad(noisy, pred, clean, weights=weights)
        ctx.save_for_backward(grad)
        return per[:, 4].mean().to(pred.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return grad_output * grad, None, None, None


class PhysicsAwareLoss(nn.Module):
    """MSE + alpha * smoothness (L1 of the first differences) + beta * peak retention (MSE at the positions
    where clean's second difference is negative) + gamma * noise model (variance stability of
    noisy - clean).  ``fused_backward``: compute the gradient with respect to ``pred`` on the device, in
    the launch that computes the value (module docstring); off by default."""

    def __init__(self, alpha=0.1, beta=0.05, gamma=0.01, fused_backward=False):
        super().__init__()
        self.alpha = alpha
        self.beta = beta
        self.gamma = gamma
        self.fused_backward = bool(fused_backward)

    @staticmethod
    def _engine_tensors(pred, clean, noisy):
        """What both device paths ask of the tensors: contiguous CUDA float32 (clean float32 or float64) of
        one (N, L) or (N, 1, L) shape on one device, N >= 1, L >= 3."""
        ts = (pred, clean, noisy)
        if not all(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() for t in ts):
            return False
        if pred.dtype != torch.float32 or noisy.dtype != torch.float32 or clean.dtype not in (torch.float32, torch.float64):
            return False
        if pred.shape != clean.shape or pred.shape != noisy.shape or pred.device != clean.device or pred.device != noisy.device:
            return False
        if not (pred.dim() == 2 or (pred.dim() == 3 and pred.shape[1] == 1)):
            return False
        return pred.shape[0] >= 1 and pred.shape[-1] >= 3

    def uses_engine(self, pred, clean, noisy):
        """Whether forward() takes the engine path for these tensors."""
        ts = (pred, clean, noisy)
        if not all(torch.is_tensor(t) for t in ts):
            return False
        if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
            return False
        return self._engine_tensors(pred, clean, noisy)

    def uses_fused_backward(self, pred, clean, noisy):
        """Whether forward() takes the fused path for these tensors: value and gradient from one launch."""
        if not (self.fused_backward and torch.is_grad_enabled()):
            return False
        if not all(torch.is_tensor(t) for t in (pred, clean, noisy)):
            return False
        if not pred.requires_grad or clean.requires_grad or noisy.requires_grad:
            return False
        return self._engine_tensors(pred, clean, noisy)

    def forward(self, pred, clean, noisy):
        weights = (self.alpha, self.beta, self.gamma)
        if self.uses_engine(pred, clean, noisy):
            per, _ = engine.physics(noisy, pred, clean, weights=weights)
            return per[:, 4].mean().to(pred.dtype)
        if self.uses_fused_backward(pred, clean, noisy):
            return _FusedPhysicsLoss.apply(pred, clean, noisy, weights)
        mse, smooth, peak, poisson = physics_terms(pred, clean, noisy)
        return mse + self.alpha * smooth + self.beta * peak + self.gamma * poisson
