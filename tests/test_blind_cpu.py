"""Blind residual report, the parts that need no GPU: the new entry points exist (ABI v6, detected by symbol),
argument checking before any device call, the host conversion of a report (rdn_blind_value), the
Wilson-Hilferty critical value, the numpy oracle against an independent restatement, and -- on the reference
generator's spectra -- that the report separates a signal-preserving output from an over-smoothed one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import blind_oracle as O
import exact_acc as E
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from raman_mi355x import _lib
    return _lib.lib()


def test_entry_points_and_constants_match_the_header(lib):
    from raman_mi355x import _lib, engine
    for name in ("rdn_blind", "rdn_blind_value"):
        assert hasattr(lib, name) and name in _lib.EXPORTED, name
    assert lib.rdn_version() == 6
    with open(os.path.join(ROOT, "include", "raman_mi355x.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define RDN_BLIND_MAX_LAGS (\d+)", header).group(1)) == _lib.BLIND_MAX_LAGS == O.MAX_LAGS == 32
    assert int(re.search(r"#define RDN_BLIND_QUANTITIES (\d+)", header).group(1)) == _lib.BLIND_QUANTITIES == 7
    assert int(re.search(r"#define RDN_BLIND_LDS_L (\d+)", header).group(1)) == _lib.BLIND_LDS_L == engine.BLIND_LDS_L
    assert 8 * _lib.BLIND_LDS_L + 64 <= 160 * 1024                       # the staged residual fits a CU's LDS
    assert (_lib.BLIND_COUNT, _lib.BLIND_FLAGGED, _lib.BLIND_ROW_WORDS) == (O.COUNT, O.FLAGGED, O.ROW_WORDS) == (49, 50, 51)
    assert _lib.blind_words(17) == 19 * 51 and _lib.BLIND_VALUES == 9
    assert engine.BLIND_QUANTITIES == O.QUANTITIES
    assert re.search(r"int rdn_blind\(const float\* x, const float\* y, const double\* sigma", header)
    assert "SAME bin formula as rdn_snr" in header


def test_argument_checks_need_no_device(lib):
    """Every RDN_EINVAL case of rdn_blind, for n = 0 too, through ctypes with host pointers: the checks come
    before any device call (this test runs without a GPU)."""
    from raman_mi355x import _lib
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    # n = 2, L = 64: x, y 512 B each; sigma 16 B; key 8 B; per7 112 B; rho (16 lags) 256 B; report 4 rows
    x, y, sigma, key = base, base + 1024, base + 2048, base + 2304
    per7, rho, report = base + 4096, base + 8192, base + 12288
    EINVAL = -1                                                                # RDN_EINVAL

    def call(x=x, y=y, sigma=sigma, n=2, L=64, lags=16, q_crit=32.0, per7=per7, rho=rho, key=key, lo=0.0, hi=1.0,
             nbins=2, report=report):
        return lib.rdn_blind(x, y, sigma, n, L, lags, q_crit, per7, rho, key, lo, hi, nbins, report, None)

    for n in (2, 0):
        assert call(n=n, sigma=None) == EINVAL and b"null sigma" in lib.rdn_last_error()
        for lags in (0, -1, 33, 1000):
            assert call(n=n, lags=lags) == EINVAL and b"lags" in lib.rdn_last_error(), (n, lags)
        for L in (16, 1, 0, -5, 2 ** 31, 2 ** 40):
            assert call(n=n, L=L) == EINVAL and b"lags < L < 2^31" in lib.rdn_last_error(), (n, L)
        assert call(n=n, L=1, lags=1) == EINVAL
        for q in (float("nan"), -1.0, -float("inf")):
            assert call(n=n, q_crit=q) == EINVAL and b"q_crit" in lib.rdn_last_error(), (n, q)
        assert call(n=n, per7=None, rho=None, report=None, key=None) == EINVAL and b"none of" in lib.rdn_last_error()
        for nbins in (0, -1, 65):
            assert call(n=n, nbins=nbins) == EINVAL and b"nbins" in lib.rdn_last_error(), (n, nbins)
        for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (-float("inf"), 0.0)):
            assert call(n=n, lo=lo, hi=hi) == EINVAL and b"finite lo < hi" in lib.rdn_last_error(), (n, lo, hi)
        assert call(n=n, report=None) == EINVAL and b"key feeds the report" in lib.rdn_last_error()
    assert call(n=-1) == EINVAL and b"n >= 0" in lib.rdn_last_error()
    for null in ("x", "y"):
        assert call(**{null: None}) == EINVAL and b"null pointer" in lib.rdn_last_error(), null
    # any output overlapping an input or another output (first and last bytes)
    words = 4 * 51 * 8
    for out, size in (("per7", 112), ("rho", 256), ("report", words)):
        for inp, isize in ((x, 512), (y, 512), (sigma, 16), (key, 8)):
            assert call(**{out: inp}) == EINVAL and b"overlap" in lib.rdn_last_error(), (out, inp)
            assert call(**{out: inp + isize - 1}) == EINVAL and call(**{out: inp - size + 1}) == EINVAL, (out, inp)
    assert call(rho=per7) == EINVAL and b"overlap" in lib.rdn_last_error()
    assert call(rho=per7 + 111) == EINVAL and call(rho=per7 - 255) == EINVAL
    assert call(report=per7 + 111) == EINVAL and call(report=rho - words + 1) == EINVAL
    assert call(per7=report + words - 1) == EINVAL
    # n = 0 launches nothing and accepts NULL data pointers; +inf is a legal q_crit; each output alone is enough
    assert call(x=None, y=None, n=0) == _lib.RDN_OK
    assert call(x=None, y=None, n=0, q_crit=float("inf"), key=None, report=None, rho=None) == _lib.RDN_OK
    assert call(x=None, y=None, n=0, per7=None, key=None, report=None) == _lib.RDN_OK
    assert call(x=None, y=None, n=0, per7=None, rho=None, key=None) == _lib.RDN_OK
    assert call(x=None, y=None, n=0, L=2 ** 31 - 1, lags=32, q_crit=0.0) == _lib.RDN_OK
    assert call(x=None, y=None, n=0, L=2, lags=1) == _lib.RDN_OK               # the smallest shape, L = K + 1
    assert lib.rdn_blind_value(None, 1, None) == EINVAL and b"null pointer" in lib.rdn_last_error()
    w, o = (ctypes.c_int64 * (67 * 51))(), (ctypes.c_double * (68 * 9))()
    for nbins in (0, 65):
        assert lib.rdn_blind_value(w, nbins, o) == EINVAL and b"nbins" in lib.rdn_last_error()


def _values(nbins):
    """Seven columns of values per report row, negative, tiny and huge ones included, and which are flagged."""
    rng = np.random.default_rng(12)
    per, rows = [], []
    for b in range(nbins + 2):
        if b == 2:
            continue                                                  # an empty bin
        m = 3 + 5 * b
        v = rng.uniform(-1, 1, (m, 7)) * 10.0 ** rng.integers(-12, 12, (m, 7))
        v[0] = [1e-40, -3e-39, 2.0 ** 63, -(2.0 ** 62), 0.1, -0.2, -40.0]
        per.append(v)
        rows += [b] * m
    per, rows = np.concatenate(per), np.array(rows)
    return per, rows, rng.uniform(size=len(rows)) < 0.4


def test_blind_value_agrees_with_the_exact_sums():
    """rdn_blind_value on hand-built report words: count, the seven exact sums rounded once, the flagged count,
    per row and in total; an out-of-range word makes that quantity NaN in its row and in the totals only."""
    from raman_mi355x import _lib, engine
    nbins = 4
    per, rows, flags = _values(nbins)
    words = O.report_words(per, rows, nbins, flags)
    assert words.shape == (_lib.blind_words(nbins),)
    got = engine.blind_value(torch.from_numpy(words), nbins).numpy()
    want = E.report_sums(per, rows, nbins)
    assert got.shape == (nbins + 3, 9)
    # math.fsum rounds the sum of the doubles; the accumulator truncates each below 2^-128 first: equal unless a
    # value carries bits below 2^-128 (row 0 of each bin does: compare those columns to 1e-38 absolute)
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.array_equal(got[:, 3:8], want[:, 3:8])
    np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=1e-15, atol=1e-37)
    for b in range(nbins + 2):
        assert got[b, 8] == flags[rows == b].sum()
    assert got[nbins + 2, 8] == flags.sum() > 0 and np.all(got[2] == 0)
    bad = words.copy()
    bad[1 * _lib.BLIND_ROW_WORDS + 5 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] = 2      # row 1, Q
    nan = engine.blind_value(torch.from_numpy(bad), nbins).numpy()
    mask = np.zeros_like(got, dtype=bool)
    mask[1, 6] = mask[nbins + 2, 6] = True
    assert np.all(np.isnan(nan[mask])) and np.array_equal(nan[~mask], got[~mask])
    with pytest.raises(ValueError, match="words"):
        engine.blind_value(torch.from_numpy(words[:-1]), nbins)


def test_q_crit_is_the_chi_square_quantile():
    """Wilson and Hilferty's cube against the tabulated chi-square 0.99 quantiles, within 0.2 % (it is for every
    K from 5 to 32; at K = 4 the approximation itself is 0.22 % off, at K = 1 0.8 %)."""
    from raman_mi355x import blind_q_crit, engine
    table = {8: 20.090, 10: 23.209, 16: 32.000, 24: 42.980, 32: 53.486}
    for k, q in table.items():
        got = blind_q_crit(k)
        print(f"K = {k}: {got:.4f} against {q}")
        assert abs(got - q) <= 0.002 * q, (k, got)
        assert got == blind_q_crit(k, alpha=0.01) == engine.blind_q_crit(k) == pytest.approx(O.q_crit(k), rel=1e-12)
    assert blind_q_crit(16, 0.05) == pytest.approx(26.296, rel=0.002)         # another alpha, same table
    assert blind_q_crit(16, 0.001) > blind_q_crit(16) > blind_q_crit(16, 0.5) > 14.0
    for bad in (0, 33, 1.5, True):
        with pytest.raises(ValueError):
            blind_q_crit(bad)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            blind_q_crit(16, bad)


def test_oracle_agrees_with_an_independent_restatement():
    """blind_oracle against np.correlate of the centred residual (another route to every lag product), 1e-12."""
    rng = np.random.default_rng(5)
    for L, K in ((17, 16), (33, 32), (64, 1), (257, 16), (1000, 32)):
        x = (rng.normal(size=(3, L)) + np.linspace(0, 2, L)).astype(np.float32)
        y = (x + 0.3 * rng.normal(size=(3, L)) + 0.05).astype(np.float32)
        sigma = np.array([0.3, 0.1, 2.0])
        per, rho = O.blind_values(x, y, sigma, K)
        for i in range(3):
            r = x[i].astype(np.float64) - y[i].astype(np.float64)
            d = r - r.mean()
            c = np.correlate(d, d, "full")[L - 1:]                     # c[k] = sum_i d_i d_{i+k}
            want_rho = c[1:K + 1] / c[0]
            np.testing.assert_allclose(rho[i], want_rho, rtol=0, atol=1e-12)
            q = L * (L + 2) * sum(want_rho[k - 1] ** 2 / (L - k) for k in range(1, K + 1))
            with np.errstate(invalid="ignore"):                       # sigma = 2 exceeds the signal: NaN on both sides
                s_est = 10 * np.log10((np.mean(x[i].astype(np.float64) ** 2) - sigma[i] ** 2) / sigma[i] ** 2)
            want = [r.mean(), np.sqrt(np.mean(r * r)), np.sqrt(np.mean(r * r)) / sigma[i], want_rho[0],
                    np.abs(want_rho).max(), q, s_est]
            np.testing.assert_allclose(per[i], want, rtol=1e-12, atol=1e-12)
    # the IEEE patterns: y = x gives D = 0, a NaN sample poisons all seven, a zero sigma divides by zero
    x = rng.normal(size=(1, 40)).astype(np.float32)
    per, rho = O.blind_values(x, x, [0.5], 4)
    assert per[0, 0] == per[0, 1] == per[0, 2] == 0 and np.isnan(per[0, 3:6]).all() and np.isnan(rho).all()
    assert not O.flagged(per, 0.0)[0]
    y = x.copy()
    y[0, 7] = np.nan
    per, rho = O.blind_values(x, y, [0.5], 4)
    assert np.isnan(per[0, :6]).all() and np.isnan(rho).all() and np.isfinite(per[0, 6])     # SNR_est reads x alone
    per, _ = O.blind_values(x, 0.5 * x, [0.0], 4)
    assert np.isinf(per[0, 2]) and np.isinf(per[0, 6]) and np.isfinite(per[0, [0, 1, 3, 4, 5]]).all()


@pytest.fixture(scope="module")
def refgen_set():
    """256 x 2048 spectra of the reference generator (fixed seed), stored as float32 like a saved dataset."""
    from oracle.refgen import generate_signals
    clean, noisy, snrs, sigma = generate_signals(256, 2048, rng=np.random.RandomState(20250410))
    return clean.astype(np.float32), noisy.astype(np.float32), snrs.reshape(-1), sigma.reshape(-1)


def _moving_average(x, w):
    h = w // 2
    p = np.pad(x.astype(np.float64), ((0, 0), (h, h)), mode="reflect")
    return np.stack([np.convolve(row, np.full(w, 1.0 / w), "valid") for row in p]).astype(np.float32)


def test_reference_spectra_separate_a_faithful_output_from_an_over_smoothed_one(refgen_set):
    """On the reference generator's spectra with the blind noise estimate, 16 lags, alpha = 0.01: y = clean is
    flagged in at most 15 % of spectra (alpha plus the spiked ones; this set gives 5.1 %), a 9-point moving
    average in all of them (minimum Q 315 against 32), and SNR_est lies within 1 dB of the true (measured) input
    SNR for at least 85 % of spectra (95.7 %; the rest are spiked).  The caps are conditions on the method, not
    measurements."""
    clean, noisy, snrs, sigma_true = refgen_set
    K, q_crit = 16, O.q_crit(16)
    sig = O.noise_sigma(noisy)
    per_clean, _ = O.blind_values(noisy, clean, sig, K)
    per_ma, _ = O.blind_values(noisy, _moving_average(noisy, 9), sig, K)
    share_clean = O.flagged(per_clean, q_crit).mean()
    share_ma = O.flagged(per_ma, q_crit).mean()
    c64, n64 = clean.astype(np.float64), noisy.astype(np.float64)
    true_snr = 10 * np.log10(np.mean(c64 ** 2, axis=1) / np.mean((n64 - c64) ** 2, axis=1))
    within = (np.abs(per_clean[:, 6] - true_snr) <= 1.0).mean()
    within_nominal = (np.abs(per_clean[:, 6] - snrs) <= 1.0).mean()
    print(f"y = clean: flagged {share_clean:.3f}, median Q {np.median(per_clean[:, 5]):.1f}, "
          f"median RMS / sigma-hat {np.median(per_clean[:, 2]):.3f}, sigma-hat / sigma {np.median(sig / sigma_true):.3f}")
    print(f"moving average 9: flagged {share_ma:.3f}, median Q {np.median(per_ma[:, 5]):.0f}, min Q {per_ma[:, 5].min():.0f}, "
          f"median RMS / sigma-hat {np.median(per_ma[:, 2]):.2f}")
    print(f"SNR_est within 1 dB of the measured input SNR: {within:.3f}; of the nominal one: {within_nominal:.3f}")
    assert share_clean <= 0.15
    assert share_ma == 1.0
    assert within >= 0.85
