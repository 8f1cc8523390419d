"""numpy restatement of the contract of the Bayesian change-point smoother (include/raman_mi355x.h
rdn_bayes_steps), vectorised over the rows and the candidates with a loop over the positions, and a second,
independent reference for tiny rows: every composition of L into parts of at most K samples, its weight
multiplied out directly.  Written for clarity, not speed; shared by the CPU and GPU tests.
"""
import math

import numpy as np

from potts_oracle import compositions

QUIET_NAN = np.uint32(0x7FC00000)
SQRT_2PI = 2.5066282746310002


def _sweep(a, base, h, rn, K, reverse):
    """Boundary values (n, L + 1) of one sweep (G right to left, F left to right) and, for the left-to-right sweep,
    each step's (M, e, S, mean)."""
    n, L = a.shape
    out = np.zeros((n, L + 1))
    mean = np.zeros((n, 0))
    M2 = np.zeros((n, 0))
    zero = np.zeros((n, 1))
    steps = []
    for i in range(L):
        pos = L - 1 - i if reverse else i                           # the sample the step takes in
        k = min(K, i + 1)
        v = a[:, pos:pos + 1]
        m_old = np.concatenate([zero, mean[:, :K - 1]], axis=1)     # candidate n continues candidate n - 1
        M2_old = np.concatenate([zero, M2[:, :K - 1]], axis=1)
        d = v - m_old
        mean = m_old + d * rn[:k]
        M2 = M2_old + d * (v - mean)
        # the boundary values the candidates n = 1 .. k lean on, nearest first
        win = out[:, pos + 1:pos + 1 + k] if reverse else out[:, pos - k + 1:pos + 1][:, ::-1]
        t = win + (base[:, :k] - M2 * h)
        M = t.max(axis=1, keepdims=True)
        e = np.exp(t - M)
        S = e.sum(axis=1, keepdims=True)
        out[:, pos if reverse else pos + 1] = (M + np.log(S))[:, 0]
        if not reverse:
            steps.append((M, e, S, mean))
    return out, steps


def bayes_steps(x, sigma, max_len=40, level_range=1.0, full=False):
    """x float32 (n, L); sigma float64 (n,) or a float; K = max_len; W = level_range.  Returns (y float32 (n, L),
    jump float32 (n, L), logZ float64 (n,)); with ``full`` the float64 (y, jump, logZ, F, G) before the rounding and
    the refusals."""
    x = np.asarray(x, dtype=np.float32)
    n, L = x.shape
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,)).copy()
    K, W = int(max_len), float(level_range)
    assert 1 <= K <= 64 and L >= 1 and W > 0
    lens = np.arange(1, K + 1, dtype=np.float64)
    rn = 1.0 / lens
    with np.errstate(all="ignore"):
        a = x.astype(np.float64)
        c0 = np.log((SQRT_2PI * sg) / (W * float(K)))
        h = (1.0 / ((2.0 * sg) * sg))[:, None]
        base = c0[:, None] - 0.5 * np.log(lens)
        G, _ = _sweep(a, base, h, rn, K, True)
        F, steps = _sweep(a, base, h, rn, K, False)
        logZ = G[:, 0].copy()
        y = np.zeros((n, L))
        jump = np.ones((n, L))
        for t in range(1, L + 1):
            M, e, S, mean = steps[t - 1]
            c = np.exp((M + G[:, t:t + 1]) - logZ[:, None])
            if t < L:
                jump[:, t] = (S * c)[:, 0]
            q = (e * c) * mean                                       # column n - 1: the run [t - n, t)
            k = q.shape[1]
            y[:, t - k:t] += np.cumsum(q[:, ::-1], axis=1)           # sample t - d: the runs with n >= d
        if full:
            return y, jump, logZ, F, G
        bad = ~(np.isfinite(x).all(axis=1) & (sg > 0) & np.isfinite(sg) & np.isfinite(h[:, 0]))
    yb = np.where(bad[:, None], QUIET_NAN, y.astype(np.float32).view(np.uint32)).astype(np.uint32)
    jb = np.where(bad[:, None], QUIET_NAN, jump.astype(np.float32).view(np.uint32)).astype(np.uint32)
    return yb.view(np.float32), jb.view(np.float32), np.where(bad, np.nan, logZ)


def brute_force(x_row, sigma, K, W=1.0):
    """(y, jump, logZ) of one tiny row from the explicit sum over every segmentation: the weight of a segmentation
    is the product of its runs' w, each multiplied out directly (two-pass mean and M2, no logarithms but the last)."""
    a = np.asarray(x_row, dtype=np.float32).astype(np.float64)
    L = len(a)
    Z = 0.0
    y = np.zeros(L)
    jump = np.zeros(L)
    for parts in compositions(L, K):
        w, i = 1.0, 0
        fit = np.empty(L)
        starts = []
        for ln in parts:
            seg = a[i:i + ln]
            m = seg.sum() / ln
            M2 = ((seg - m) ** 2).sum()
            w *= math.sqrt(2.0 * math.pi) * sigma / (W * K) / math.sqrt(ln) * math.exp(-M2 / (2.0 * sigma * sigma))
            fit[i:i + ln] = m
            starts.append(i)
            i += ln
        Z += w
        y += w * fit
        jump[starts] += w
    return y / Z, jump / Z, math.log(Z)


def true_segmentation_mean(noisy, clean):
    """The ceiling: the run means of ``noisy`` under ``clean``'s own runs (a jump wherever clean changes)."""
    noisy = np.asarray(noisy, dtype=np.float64)
    out = np.empty_like(noisy)
    for r in range(noisy.shape[0]):
        cuts = np.flatnonzero(np.diff(clean[r]) != 0) + 1
        for s, e in zip(np.r_[0, cuts], np.r_[cuts, noisy.shape[1]]):
            out[r, s:e] = noisy[r, s:e].mean()
    return out
