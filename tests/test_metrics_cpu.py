"""The exact-arithmetic metric arbiter (tests/metrics_exact.py) against the skimage golden, and the float64
numpy oracle (oracle/metrics.py) against the arbiter on the input families of test_metrics_domain_gpu.py.

MSE and Smoothness are sums of L non-negative terms, each rounded once: whatever the summation order, the
float64 result is within (L + 4) 2^-53 of the exact value (L - 1 additions, the term's rounding, the
division, and the arbiter's own rounding).  Peak2Peak is one fp64 subtraction of two fp32 values: exact
or rounded once either way, so bit-equal.  The oracle's SSIM forms each window variance as
E[x^2] - E[x]^2 and loses digits with the data's offset; its distance from exact is measured and printed
here, not bounded: it is the yardstick the device's SSIM is held to.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from metrics_exact import exact_metrics, exact_per_spectrum, family_table, rel_err, ssim_err

U = 2.0 ** -53


def test_arbiter_matches_skimage_golden():
    """The bars test_cpu_host.py holds the oracle to against the same fixture."""
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    p = exact_per_spectrum(g["den"], g["clean"])
    ref = g["per_spectrum"]
    np.testing.assert_allclose(p[:, :2], ref[:, :2], rtol=1e-10)      # MSE, SSIM (fp64 in both)
    np.testing.assert_allclose(p[:, 2:], ref[:, 2:], rtol=1e-6)       # reference: float32 diff/ptp


def test_arbiter_by_hand():
    """Values small enough to do on paper: y one-hot of height 2 at the end of 8 samples, clean zero."""
    y = np.zeros(8, np.float32)
    y[7] = 2.0
    m = exact_metrics(y, np.zeros(8, np.float32))
    assert m[0] == 0.5 and np.isnan(m[1]) and m[2] == 2.0 / 7.0 and m[3] == 2.0   # window 0 is 0/0
    c = np.arange(8, dtype=np.float64)
    m = exact_metrics(c.astype(np.float32), c)
    assert m[0] == 0.0 and m[1] == 1.0 and m[2] == 1.0 and m[3] == 7.0


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
def test_oracle_against_arbiter(f64):
    print(f"\n{'family':18s} {'L':>5s}  oracle: MSE rel    Smooth rel  SSIM err")
    for name, (y, clean, exact, orc) in family_table(f64).items():
        L = y.shape[1]
        e = rel_err(orc, exact)
        es = ssim_err(orc[:, 1], exact[:, 1])
        print(f"{name:18s} {L:5d}  {e[:, 0].max():10.2e}  {e[:, 2].max():10.2e}  {es.max():10.2e}")
        assert e[:, 0].max() <= (L + 4) * U, (name, "MSE")
        assert e[:, 2].max() <= (L + 4) * U, (name, "Smoothness")
        assert np.array_equal(orc[:, 3], exact[:, 3]), (name, "Peak2Peak")
        assert np.array_equal(np.isnan(orc[:, 1]), np.isnan(exact[:, 1])), (name, "SSIM NaN")


NONFINITE = [("nan", [(3, np.nan)]), ("+inf", [(3, np.inf)]), ("-inf", [(0, -np.inf)]),
             ("+inf and -inf", [(2, np.inf), (9, -np.inf)]), ("two +inf apart", [(2, np.inf), (9, np.inf)]),
             ("two +inf adjacent", [(4, np.inf), (5, np.inf)]), ("nan and inf", [(1, np.nan), (6, np.inf)])]


@pytest.mark.parametrize("where", ["y", "clean", "both"])
@pytest.mark.parametrize("name,puts", NONFINITE, ids=[n for n, _ in NONFINITE])
def test_arbiter_nonfinite_is_what_numpy_gives(name, puts, where):
    """Non-finite inputs: the arbiter's classes against numpy's IEEE evaluation of the definitions (the
    oracle, which is plain numpy), NaN-equal; the metrics a non-finite clean leaves finite stay exact."""
    from oracle.metrics import per_spectrum
    rng = np.random.default_rng(11)
    c = rng.uniform(0, 1, 12).astype(np.float32)
    y = (c + rng.normal(0, 0.05, 12)).astype(np.float32)
    for p, v in puts:
        if where in ("y", "both"):
            y[p] = v
        if where in ("clean", "both"):
            c[p] = v
    with np.errstate(invalid="ignore", over="ignore"):
        ref = per_spectrum(y[None], c[None])[0]
    got = exact_metrics(y, c)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (got, ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-14)
    y[:] = np.nan
    assert np.isnan(exact_metrics(y, c)).all()
