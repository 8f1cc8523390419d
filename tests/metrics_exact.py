"""Exact-arithmetic arbiter of the four evaluation metrics (TEST INFRASTRUCTURE).

MSE, SSIM, Smoothness and Peak2Peak are rational functions of the stored values, and every fp32 / fp64
value is a dyadic rational, so each metric of a spectrum has an exact value; ``exact_metrics`` computes
it in Python integers and rounds it ONCE to double.  It is written from the definitions (the header
comment of csrc/metrics.hpp): it shares no arithmetic with oracle/metrics.py or with the kernel, so it
can arbitrate between them where fp64's own error (the window variance E[x^2] - E[x]^2 of data with an
offset) is as large as the bar.

Definitions, for y = denoised (fp32) and c = clean (fp32 or fp64), both of length L >= 7:
    MSE        = sum (y - c)^2 / L
    Smoothness = sum |y[p+1] - y[p]| / (L - 1)
    Peak2Peak  = max y - min y
    SSIM       = mean over window starts i = 0 .. L-7 of
                 (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
                 ux, uy the 7-sample means of c and y, vx = 7/6 (mean c^2 - ux^2), vy alike,
                 vxy = 7/6 (mean c y - ux uy), C1 = (K1 R)^2, C2 = (K2 R)^2, K1 = 1/100, K2 = 3/100,
                 R = max c - min c.
With the inputs scaled to integers X = c D, Y = y D (D a power of two) and the window sums SX, SY, SXX,
SYY, SXY of those integers, every factor of a window's S is an integer over the same denominator, which
cancels:
    S = (2e4 SX SY + 49 Rn^2)(2e4 (7 SXY - SX SY) + 378 Rn^2)
        / ((1e4 (SX^2 + SY^2) + 49 Rn^2)(1e4 (7 SXX - SX^2 + 7 SYY - SY^2) + 378 Rn^2)),   Rn = R D.
A window whose denominator is zero has a zero numerator too (SX = SY = R = 0, or zero variances and
R = 0, hence a zero covariance): 0/0, NaN, as in IEEE arithmetic.

Non-finite inputs get what numpy's evaluation of the definitions gives (IEEE arithmetic on the extended
reals), by class: a sum with a NaN term, or with inf - inf, is NaN; otherwise one with an infinite term
is +inf; max / min propagate NaN; every SSIM window holds an inf - inf (its variance) or a NaN, and
every sample lies in some window, so SSIM is NaN whenever any input is not finite.
"""
import functools
import math

import numpy as np

import exact_acc

WIN = 7
FIX = 320            # fractional bits of the SSIM sum's fixed-point bracket


def _scaled_ints(*rows):
    """Python integers v * D of every row's finite values, for the smallest power of two D that makes all integral."""
    ratios = [[float(v).as_integer_ratio() for v in r] for r in rows]
    D = max((d for r in ratios for _, d in r), default=1)
    return [[n * (D // d) for n, d in r] for r in ratios], D


def _ratio(num, den):
    """num / den rounded once to double (Python's integer true division is correctly rounded)."""
    if num == 0:
        return 0.0
    try:
        return num / den
    except OverflowError:
        return math.copysign(math.inf, num) * math.copysign(1.0, den)


def _sum_pairs(pairs):
    """Exact sum of the fractions (n, d) as one unreduced fraction: pairwise, so the big products are few."""
    while len(pairs) > 1:
        nxt = [(a * d + c * b, b * d) for (a, b), (c, d) in zip(pairs[0::2], pairs[1::2])]
        if len(pairs) & 1:
            nxt.append(pairs[-1])
        pairs = nxt
    return pairs[0]


def _ssim_exact(X, Y):
    L = len(X)
    Rn = max(X) - min(X)
    r49, r378 = 49 * Rn * Rn, 378 * Rn * Rn
    sx, sy = sum(X[:WIN]), sum(Y[:WIN])
    sxx, syy = sum(v * v for v in X[:WIN]), sum(v * v for v in Y[:WIN])
    sxy = sum(a * b for a, b in zip(X[:WIN], Y[:WIN]))
    pairs = []
    for i in range(L - WIN + 1):
        if i:                                                      # slide: integers, so nothing cancels
            a0, b0, a1, b1 = X[i - 1], Y[i - 1], X[i + WIN - 1], Y[i + WIN - 1]
            sx += a1 - a0
            sy += b1 - b0
            sxx += a1 * a1 - a0 * a0
            syy += b1 * b1 - b0 * b0
            sxy += a1 * b1 - a0 * b0
        num = (20000 * sx * sy + r49) * (20000 * (7 * sxy - sx * sy) + r378)
        den = (10000 * (sx * sx + sy * sy) + r49) * (10000 * (7 * sxx - sx * sx + 7 * syy - sy * sy) + r378)
        if den == 0:
            assert num == 0
            return math.nan
        pairs.append((num, den))
    # The exact sum lies in [Q, Q + nwin) / 2^FIX for Q the sum of the quotients' floors at FIX fractional
    # bits.  Rounding is monotone, so where both ends round to the same double that is the exact sum
    # rounded once; otherwise (a sum near zero or on a rounding boundary) the fractions are added exactly.
    nwin = L - WIN + 1
    Q = sum((n << FIX) // d for n, d in pairs)
    lo, hi = _ratio(Q, nwin << FIX), _ratio(Q + nwin, nwin << FIX)
    if lo == hi:
        return lo
    n, d = _sum_pairs(pairs)
    return _ratio(n, d * nwin)


def _sum_class(terms):
    """Class of an IEEE sum of non-negative extended-real terms that is not finite: NaN or +inf."""
    return math.nan if np.isnan(terms).any() else math.inf


def exact_metrics(y, clean):
    """[MSE, SSIM, Smoothness, Peak2Peak] of one spectrum, each the exact value rounded once to double."""
    y, clean = np.asarray(y), np.asarray(clean)
    assert y.dtype == np.float32 and clean.dtype in (np.float32, np.float64), (y.dtype, clean.dtype)
    assert y.ndim == 1 and y.shape == clean.shape and y.size >= WIN, (y.shape, clean.shape)
    L = y.size
    if np.isfinite(y).all() and np.isfinite(clean).all():
        (Y, X), D = _scaled_ints(y, clean)
        return np.array([_ratio(sum((a - b) ** 2 for a, b in zip(Y, X)), D * D * L),
                         _ssim_exact(X, Y),
                         _ratio(sum(abs(b - a) for a, b in zip(Y, Y[1:])), D * (L - 1)),
                         _ratio(max(Y) - min(Y), D)])
    # Non-finite inputs.  float64 differences and squares of the stored values have the IEEE class of
    # the exact ones (an fp32 value squared cannot overflow a double), so the classes are read off them;
    # a metric that stays finite (Smoothness and Peak2Peak of a finite y beside a non-finite clean) is
    # computed exactly as above.
    y64, c64 = y.astype(np.float64), clean.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.array([_sum_class((y64 - c64) ** 2), math.nan, math.nan, math.nan])
        if np.isfinite(y).all():
            (Y,), D = _scaled_ints(y)
            out[2] = _ratio(sum(abs(b - a) for a, b in zip(Y, Y[1:])), D * (L - 1))
            out[3] = _ratio(max(Y) - min(Y), D)
        else:
            out[2] = _sum_class(np.abs(np.diff(y64)))
            out[3] = math.nan if np.isnan(y64).any() else y64.max() - y64.min()
    return out


def exact_per_spectrum(y, clean):
    """float64 (n, 4) of exact_metrics over the rows of y (fp32, (n, L)) and clean (fp32 / fp64)."""
    y, clean = np.atleast_2d(y), np.atleast_2d(clean)
    return np.stack([exact_metrics(a, c) for a, c in zip(y, clean)])


def exact_total(values):
    """The exact sum of finite doubles, rounded once."""
    pairs = [float(v).as_integer_ratio() for v in values]
    n, d = _sum_pairs(pairs) if pairs else (0, 1)
    return _ratio(n, d)


def rel_err(got, exact):
    """|got - exact| / |exact| per element in exact arithmetic (0 where both are 0 or both NaN, inf where
    only one is NaN or only the exact value is 0)."""
    from fractions import Fraction
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    out = np.empty(got.shape)
    for i, (g, e) in enumerate(zip(got.ravel(), exact.ravel())):
        if np.isnan(g) or np.isnan(e) or np.isinf(g) or np.isinf(e):
            same = (np.isnan(g) and np.isnan(e)) or g == e
            out.flat[i] = 0.0 if same else math.inf
        elif g == e:
            out.flat[i] = 0.0
        elif e == 0:
            out.flat[i] = math.inf
        else:
            out.flat[i] = float(abs(Fraction(g) - Fraction(e)) / abs(Fraction(e)))
    return out


def ssim_err(got, exact):
    """The SSIM error the bars speak of: relative, but absolute where the exact SSIM is below 1e-9 in
    magnitude (a value that is rounding noise over the variance, e.g. 0 for a constant clean)."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    noise = np.abs(exact) < 1e-9
    with np.errstate(invalid="ignore"):
        return np.where(noise, np.abs(got - exact), rel_err(got, np.where(noise, 1.0, exact)))


def acc_words(per):
    """The exact accumulator (int64 words, RDN_ACC_WORDS) that the per-spectrum values ``per`` (n, 4) give:
    a value that is not finite or is >= 2^64 in magnitude counts in its metric's out-of-range word, every
    other one goes into its limbs (exact_acc.row_words, the host restatement of the device's accumulator)."""
    return exact_acc.row_words(per).tolist()


# ---- the input families of the metric domain tests (CPU: oracle against arbiter; GPU: device against arbiter) ----
FAMILY_NAMES = ("normalised", "simulator", "small 1e-3", "offset 1", "offset 100", "offset 4096", "short L=7",
                "short L=8", "short L=13", "y == clean", "constant clean", "all zero", "anti-correlated", "one-hot")
ONE_HOT_L = 1100
ONE_HOT_P = (0, 63, 64, 511, 512, 1023, 1024, ONE_HOT_L - 1)     # lane, wave, partition and tail boundaries


def _f64(clean, rng):
    """An fp64 clean holding bits no fp32 has (a path that read it as fp32 would differ)."""
    return clean.astype(np.float64) + 1e-9 * rng.uniform(0, 1, clean.shape)


def families(f64):
    """[(name, y fp32 (n, L), clean fp32 or fp64 (n, L))]: 4-8 spectra each, L <= 2000."""
    from oracle import generator
    rng = np.random.default_rng(20250611)
    cast = (lambda c: _f64(c, rng)) if f64 else (lambda c: c)
    exact = (lambda c: c.astype(np.float64)) if f64 else (lambda c: c)
    f32 = lambda a: np.asarray(a, np.float32)
    out = []

    def noisy(c, sd):
        return f32(c + rng.normal(0, sd, c.shape))

    c = f32(rng.uniform(0, 1, (4, 2000)))
    out.append(("normalised", noisy(c, 0.05), cast(c)))
    sc, sn, _, _, _ = generator.generate(20250611, 3, 4, L=1100)
    out.append(("simulator", f32(sn), cast(f32(sc))))
    c = f32(rng.uniform(0, 1e-3, (4, 1100)))
    out.append(("small 1e-3", noisy(c, 5e-5), cast(c)))
    base = f32(rng.uniform(0, 1, (4, 1100)))
    for off in (1, 100, 4096):
        c = f32(base + np.float32(off))
        out.append((f"offset {off}", noisy(c, 0.05), cast(c)))
    for L in (7, 8, 13):
        c = f32(rng.uniform(0, 1, (8, L)))
        out.append((f"short L={L}", noisy(c, 0.05), cast(c)))
    c = f32(rng.uniform(0, 1, (4, 1100)))
    out.append(("y == clean", c.copy(), exact(c)))
    c = np.full((4, 1100), 0.3, np.float32)
    out.append(("constant clean", noisy(c, 0.05), exact(c)))
    z = np.zeros((4, 600), np.float32)
    out.append(("all zero", z.copy(), exact(z)))
    c = f32(rng.uniform(0, 1, (4, 1100)))
    y = f32(2 * c.mean(axis=1, keepdims=True) - c)                # clean reflected about its mean
    out.append(("anti-correlated", y, cast(c)))
    n = len(ONE_HOT_P)
    y, c = np.zeros((n, ONE_HOT_L), np.float32), np.zeros((n, ONE_HOT_L), np.float32)
    for i, p in enumerate(ONE_HOT_P):
        y[i, p] = 0.75 if i & 1 else -0.75
        c[i, ONE_HOT_P[(i + 3) % n]] = -1.0 if i & 2 else 1.0       # its single extreme, at another boundary
    out.append(("one-hot", y, exact(c)))
    return out


@functools.lru_cache(maxsize=None)
def family_table(f64):
    """{name: (y, clean, exact (n, 4), oracle (n, 4))}, computed once and shared by the tests (read-only)."""
    from oracle.metrics import per_spectrum
    out = {}
    for name, y, clean in families(f64):
        with np.errstate(invalid="ignore", divide="ignore"):
            orc = per_spectrum(y, clean)
        arrs = (y, clean, exact_per_spectrum(y, clean), orc)
        for a in arrs:
            a.setflags(write=False)
        out[name] = arrs
    assert tuple(out) == FAMILY_NAMES
    return out
