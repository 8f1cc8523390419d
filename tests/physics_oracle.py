"""Plain-numpy oracle of the PhysicsAwareLoss report (include/raman_mi355x.h rdn_physics): float64 for
the values, clean's own type for the mask, exact (math.fsum) sums for a report.  Shared by
test_physics_cpu.py and test_physics_gpu.py."""
import numpy as np

import exact_acc as E
from exact_acc import report_sums, report_words  # noqa: F401  (one count word per row: the defaults)

QUANTITIES = ("MSE", "Smooth", "Peak", "Noise", "Total", "PeakCount")
WEIGHTS = (0.1, 0.05, 0.01)
ACC_LIMBS, ACC_STRIDE = E.ACC_LIMBS, E.ACC_STRIDE
ROW_WORDS = 6 * ACC_STRIDE + 1
COUNT = 6 * ACC_STRIDE


def peak_mask(clean):
    """(n, L - 2) bool: torch.diff(clean, n=2) < 0, both first differences formed and compared in
    clean's own storage type (float32 arithmetic for float32 clean, float64 for float64 clean)."""
    c = np.asarray(clean)
    assert c.dtype in (np.float32, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = c[:, 1:] - c[:, :-1]                                      # rounded to c.dtype
        assert d.dtype == c.dtype
        return d[:, 1:] < d[:, :-1]


def physics_values(x, y, clean, weights=WEIGHTS, dtype=np.float64):
    """(n, 6) {MSE, Smooth, Peak, Noise, Total, PeakCount} per spectrum, the header's formulas in
    ``dtype`` arithmetic (float64: the oracle; np.longdouble: the check on the oracle's own rounding) on
    the stored values; the mask in clean's type."""
    alpha, beta, gamma = (dtype(w) for w in weights)
    m = peak_mask(clean).astype(dtype)
    x, p, c = (np.asarray(a).astype(dtype) for a in (x, y, clean))
    L = c.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        mse = np.sum((p - c) ** 2, axis=1) / L
        smooth = np.sum(np.abs((p[:, 1:] - p[:, :-1]) - (c[:, 1:] - c[:, :-1])), axis=1) / (L - 1)
        peak = np.sum((m * p[:, 1:-1] - m * c[:, 1:-1]) ** 2, axis=1) / (L - 2)
        d = x - c
        mu = np.sum(d, axis=1, keepdims=True) / L
        v = np.sum((d - mu) ** 2, axis=1, keepdims=True) / (L - 1)
        noise = np.sum((d * d - v) ** 2, axis=1) / L
        total = ((mse + alpha * smooth) + beta * peak) + gamma * noise
    return np.stack([mse, smooth, peak, noise, total, np.sum(m, axis=1)], axis=1)
