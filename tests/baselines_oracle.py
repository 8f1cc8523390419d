"""numpy restatement of the two contracts of the baseline filters (include/raman_mi355x.h rdn_fir, rdn_median).

FIR: acc = 0.0; for k: acc = acc + taps[k] * float64(x[idx(i - h + k)]) -- each product and each sum an fp64
operation of its own, vectorised over the outputs only -- then one rounding to fp32.  Median: sort the window's
monotone keys and pick rank h.  Written for clarity, not speed; shared by the CPU and GPU tests.
"""
import os

import numpy as np

QUIET_NAN = np.uint32(0x7FC00000)


def mirror_index(L, h):
    """idx(j) for j = -h .. L - 1 + h: -j below 0, 2 (L - 1) - j above L - 1 (no repeated edge sample)."""
    j = np.arange(-h, L + h)
    j = np.where(j < 0, -j, j)
    return np.where(j > L - 1, 2 * (L - 1) - j, j)


def fir(x, taps, edge_taps=None):
    """x float32 (..., L); taps float64 (w,); edge_taps None or float64 (w - 1, w).  Returns float32."""
    x = np.asarray(x, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float64)
    w, L = taps.shape[0], x.shape[-1]
    h = (w - 1) // 2
    assert w % 2 == 1 and L >= w
    xp = x[..., mirror_index(L, h)].astype(np.float64)
    with np.errstate(all="ignore"):
        acc = np.zeros(x.shape, dtype=np.float64)
        for k in range(w):
            acc = acc + taps[k] * xp[..., k:k + L]
        if edge_taps is not None and h:
            edge = np.asarray(edge_taps, dtype=np.float64)
            assert edge.shape == (w - 1, w)
            x64 = x.astype(np.float64)
            for j in range(h):
                a = np.zeros(x.shape[:-1], dtype=np.float64)
                b = np.zeros(x.shape[:-1], dtype=np.float64)
                for k in range(w):
                    a = a + edge[j, k] * x64[..., k]
                    b = b + edge[h + j, k] * x64[..., L - w + k]
                acc[..., j] = a
                acc[..., L - h + j] = b
        return acc.astype(np.float32)


def keys(x):
    """Monotone uint32 key of float32 bits: -0 < +0, -inf and +inf ordinary values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def median(x, w):
    """Rank-h sample of each mirror-extended window, bit for bit an input; quiet NaN where a window holds a NaN."""
    x = np.asarray(x, dtype=np.float32)
    L, h = x.shape[-1], (w - 1) // 2
    assert w % 2 == 1 and L >= w
    xp = np.ascontiguousarray(x[..., mirror_index(L, h)])
    win = np.lib.stride_tricks.sliding_window_view(xp, w, axis=-1)         # (..., L, w)
    k = np.sort(keys(win), axis=-1)[..., h]
    bits = np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    bits = np.where(np.isnan(win).any(axis=-1), QUIET_NAN, bits).astype(np.uint32)
    return bits.view(np.float32)


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between finite float32 arrays (0 for equal bits; -0 and +0
    are 1 apart)."""
    ka = keys(np.asarray(a, dtype=np.float32)).astype(np.int64)
    kb = keys(np.asarray(b, dtype=np.float32)).astype(np.int64)
    return np.abs(ka - kb)


# ---- the scipy fixture (tests/golden/baselines.npz, make_baselines_golden.py), shared by the CPU and GPU tests ----
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baselines.npz"))


def golden_cases():
    """(golden key, x, module factory) for every output of the fixture."""
    from raman_mi355x import baselines as B
    for key in G.files:
        parts = key.split("_")
        if parts[0] == "x":
            continue
        x = G[f"x_{parts[-1]}"]
        if parts[0] == "savgol":
            w, p, mode = int(parts[1]), int(parts[2]), parts[3]
            yield key, x, (lambda w=w, p=p, mode=mode: B.SavitzkyGolay(w, p, mode))
        elif parts[0] == "uniform":
            yield key, x, (lambda w=int(parts[1]): B.MovingAverage(w))
        elif parts[0] == "gauss":
            yield key, x, (lambda s=float(parts[1]): B.GaussianSmooth(s))
        else:
            yield key, x, (lambda w=int(parts[1]): B.MedianFilter(w))


def oracle_of(module, x):
    """The numpy oracle's output for a baseline module."""
    from raman_mi355x import baselines as B
    if isinstance(module, B.MedianFilter):
        return median(x, module.window)
    edge = None if module.edge_taps is None else module.edge_taps.cpu().numpy()
    return fir(x, module.taps.cpu().numpy(), edge)


def check_against_golden(key, y):
    gold = G[key]
    assert y.dtype == np.float32 and y.shape == gold.shape
    if key.startswith("median"):
        assert gold.dtype == np.float32 and np.array_equal(y.view(np.uint32), gold.view(np.uint32)), key
    else:
        assert gold.dtype == np.float64 and ulp_distance(y, gold.astype(np.float32)).max() <= 1, key
