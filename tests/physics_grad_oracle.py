"""Plain-numpy oracle of the PhysicsAwareLoss gradient (include/raman_mi355x.h rdn_physics_grad): the
header's formula in float64 on the stored values, the mask in clean's own type (physics_oracle.peak_mask),
and the bar a computed gradient is held to.  Shared by test_physics_grad_cpu.py and test_physics_grad_gpu.py.

The bar, derived and not chosen: |got - ref| <= 2^-24 |ref| + 2^-48 M_i.  The first term is the one rounding
to fp32 (ref must be a normal fp32 number or exactly 0, which the tests assert).  The second: either side
evaluates g_i with at most eight rounded fp64 operations, each with a relative error of at most 2^-53 on
a partial result no larger than M_i = |scale| (2 |r_i| / L + 2 alpha / (L - 1) + 2 beta |r_i| / (L - 2)), the
sum of the magnitudes of the three terms: 8 * 2^-53 M_i a side, 16 * 2^-53 M_i for both, doubled once:
32 * 2^-53 = 2^-48."""
import numpy as np

from physics_oracle import WEIGHTS, peak_mask

FP32_MIN_NORMAL = 2.0 ** -126


def _parts(y, clean):
    p, c = np.asarray(y).astype(np.float64), np.asarray(clean).astype(np.float64)
    assert p.ndim == 2 and p.shape == c.shape and p.shape[1] >= 3
    m = np.zeros(p.shape)
    m[:, 1:-1] = peak_mask(clean)
    return p, c, m


def physics_grad(y, clean, weights=WEIGHTS, scale=None):
    """(n, L) float64: scale * d Total / d y per spectrum; ``scale`` = None means 1 / n (the gradient of the
    mean of Total over the batch: the reference's loss.backward()).  gamma takes no part."""
    alpha, beta, _ = (float(w) for w in weights)
    p, c, m = _parts(y, clean)
    n, L = p.shape
    scale = 1.0 / n if scale is None else float(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        r = p - c
        e = (p[:, 1:] - p[:, :-1]) - (c[:, 1:] - c[:, :-1])
        s = (e > 0).astype(np.float64) - (e < 0).astype(np.float64)          # 0 for 0 and for NaN
        ds = np.zeros(p.shape)
        ds[:, 1:] += s                                                       # s_{i-1}, i >= 1
        ds[:, :-1] -= s                                                      # s_i, i <= L - 2
        g = 2.0 * r / L + alpha * ds / (L - 1)
        # the peak term exists at the centre positions only: selected, not multiplied by zero
        g[:, 1:-1] += (beta * 2.0 * m * (m * p - m * c) / (L - 2))[:, 1:-1]
        return scale * g


def magnitude(y, clean, weights=WEIGHTS, scale=None):
    """(n, L) float64 M_i = |scale| (2 |r_i| / L + 2 alpha / (L - 1) + 2 beta |r_i| / (L - 2)): what the fp64
    rounding errors of g_i are relative to (|alpha|, |beta| for weights of either sign)."""
    alpha, beta, _ = (abs(float(w)) for w in weights)
    p, c, _ = _parts(y, clean)
    n, L = p.shape
    scale = 1.0 / n if scale is None else abs(float(scale))
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(p - c)
        return scale * (2.0 * r / L + 2.0 * alpha / (L - 1) + 2.0 * beta * r / (L - 2))


def assert_reference_is_fp32_normal(ref):
    """Every finite reference gradient is a normal fp32 number or exactly 0 (2^-24 |ref| is then one
    rounding to fp32)."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    fin = np.isfinite(a)
    assert np.all((a[fin] == 0) | ((a[fin] >= FP32_MIN_NORMAL) & (a[fin] < 2.0 ** 128)))


def assert_meets_bar(got, ref, M, extra=0.0):
    """|got - ref| <= 2^-24 |ref| + 2^-48 M (+ ``extra``: a recorded distance, for a triangle inequality) at
    every position where ref is finite; prints the largest ratio to the bar before it asserts."""
    got, ref, M = (np.asarray(a, dtype=np.float64) for a in (got, ref, M))
    assert got.shape == ref.shape == M.shape
    assert_reference_is_fp32_normal(ref)
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(got[fin])) and np.all(np.isfinite(M[fin]))
    err = np.abs(got[fin] - ref[fin])
    bar = 2.0 ** -24 * np.abs(ref[fin]) + 2.0 ** -48 * M[fin] + extra
    ratio = np.where(err == 0, 0.0, err / np.where(bar == 0, np.finfo(np.float64).tiny, bar))
    print(f"gradient vs reference: largest error / bar {ratio.max() if ratio.size else 0.0:.3f} over {int(fin.sum())} positions")
    assert np.all(err <= bar), (float(ratio.max()), int(np.argmax(ratio)))


def assert_same_nonfinite(got, ref):
    """NaN at the same positions, +inf and -inf at the same positions."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
