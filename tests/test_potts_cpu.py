"""The exact piecewise-constant (Potts) fit without a device: the ABI's symbols and argument checks, the numpy oracle
(tests/potts_oracle.py) against exhaustive enumeration in exact arithmetic, the module's eager path against the
oracle's bits, its gradient, and the method's claims on the reference generator's spectra.

Bar of the gradient.  The backward is a float64 prefix sum of the upstream gradient, a difference and a division per
position, rounded to fp32; the test's reference is numpy's float64 mean of the same fp32 values over the same run.
Both are within a few 2^-53 relative of the run's true mean times the cancellation of at most 300 terms of order 1
(~1e-13 absolute), so after the rounding to fp32 they agree to 1 fp32 ulp (6e-8 relative at the values' size):
the bar is 1e-6 absolute on gradients of order 1."""
import ctypes
import re

import numpy as np
import pytest
import torch

import haar_oracle as H
import potts_oracle as P


def test_abi_symbols_and_constants():
    from raman_mi355x import _lib, engine
    lib = _lib.lib()
    for name in ("rdn_potts", "rdn_noise_mad"):
        assert hasattr(lib, name) and name in _lib.EXPORTED
    assert lib.rdn_version() == 6
    with open(_lib.HEADER) as fh:
        header = fh.read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (RDN_POTTS_\w+) (\d+)", header, re.M)}
    assert consts == {"RDN_POTTS_MAX_LEN": 64}                       # no LDS limit: the back-pointers live in `work`
    assert _lib.POTTS_MAX_LEN == engine.POTTS_MAX_LEN == 64
    assert re.search(r"int rdn_noise_mad\(const float\* x, double\* med, int64_t n, int64_t L, void\* stream\);", header)
    assert re.search(r"int rdn_potts\(const float\* x, float\* y, int32_t\* nseg", header)


def test_argument_checks_need_no_device():
    """Every RDN_EINVAL case of rdn_potts and rdn_noise_mad, for n = 0 too, through ctypes with host pointers: the
    checks come before any device call (this test runs without a GPU)."""
    from raman_mi355x import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    x, y, work, nseg, gamma = base, base + 128 * 4, base + 256 * 4, base + 512 * 4, base + 768 * 4
    EINVAL = -1                                                                # RDN_EINVAL

    def call(x=x, y=y, nseg=nseg, gamma=gamma, n=1, L=128, max_len=64, work=work, work_bytes=128):
        return lib.rdn_potts(x, y, nseg, gamma, n, L, max_len, work, work_bytes, None)

    for n in (1, 0):
        assert call(n=n, gamma=None) == EINVAL and b"null gamma" in lib.rdn_last_error()
        for max_len in (0, -1, 65, 1000):
            assert call(n=n, max_len=max_len) == EINVAL and b"max_len" in lib.rdn_last_error(), (n, max_len)
        for L in (0, -5, 2 ** 31, 2 ** 40):
            assert call(n=n, L=L, work_bytes=2 ** 62) == EINVAL and b"L < 2^31" in lib.rdn_last_error(), (n, L)
    assert call(n=-1) == EINVAL and b"n >= 0" in lib.rdn_last_error()
    for null in ("x", "y", "work"):
        assert call(**{null: None}) == EINVAL and b"null pointer" in lib.rdn_last_error(), null
    assert call(work_bytes=127) == EINVAL and b"work_bytes" in lib.rdn_last_error()
    assert call(n=2, L=64, work_bytes=127) == EINVAL
    assert call(y=x) == EINVAL and call(y=x + 127 * 4) == EINVAL and b"x and y overlap" in lib.rdn_last_error()
    assert call(x=y, y=x + 1 * 4) == EINVAL                                    # ... from the other side
    assert call(work=x + 127 * 4) == EINVAL and b"work overlaps" in lib.rdn_last_error()    # x's last sample
    assert call(work=y - 1, work_bytes=128) == EINVAL                          # x's last byte
    assert call(work=y + 511) == EINVAL and call(work=y - 128 + 1) == EINVAL   # y's last byte, y's first
    assert call(work=work, work_bytes=10 ** 6) == EINVAL                       # the stated extent runs over nseg ... and beyond
    assert call(nseg=x + 127 * 4) == EINVAL and b"nseg overlaps" in lib.rdn_last_error()
    assert call(nseg=y) == EINVAL and call(nseg=y + 127 * 4) == EINVAL
    assert call(nseg=work + 127) == EINVAL and call(nseg=work - 3) == EINVAL
    # n = 0 launches nothing and accepts NULL data pointers; nseg may be NULL
    assert call(x=None, y=None, nseg=None, work=None, work_bytes=0, n=0) == _lib.RDN_OK
    assert call(x=None, y=None, nseg=None, work=None, work_bytes=0, n=0, L=2 ** 31 - 1, max_len=1) == _lib.RDN_OK

    med = base + 512 * 4

    def mad(x=x, med=med, n=1, L=128):
        return lib.rdn_noise_mad(x, med, n, L, None)

    for n in (1, 0):
        for L in (0, -1, 2 ** 31):
            assert mad(n=n, L=L) == EINVAL and b"1 <= L < 2^31" in lib.rdn_last_error(), (n, L)
    assert mad(n=-1) == EINVAL
    assert mad(x=None) == EINVAL and mad(med=None) == EINVAL and b"null pointer" in lib.rdn_last_error()
    assert mad(med=x + 127 * 4) == EINVAL and mad(med=x - 4) == EINVAL and b"med overlaps" in lib.rdn_last_error()
    assert mad(x=None, med=None, n=0) == _lib.RDN_OK and mad(x=None, med=None, n=0, L=1) == _lib.RDN_OK


def test_engine_refuses_host_input():
    from raman_mi355x import engine
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.potts(torch.zeros(2, 32), 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.noise_mad(torch.zeros(2, 32))


def test_module_arguments():
    import raman_mi355x as R
    from raman_mi355x.potts import PottsFit
    assert R.PottsFit is PottsFit and "PottsFit" in R.__all__ and "PottsFit" not in R.BASELINES
    m = PottsFit()
    assert (m.penalty, m.max_len) == (12.0, 64) and len(m.state_dict()) == 0 and isinstance(m, R.baselines._Baseline)
    assert PottsFit("bic").factor(2000) == P.thresholds("bic", 2000) and PottsFit(10).factor(5) == 10.0
    for kw in (dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=float("inf")), dict(penalty=float("nan")),
               dict(penalty="aic"), dict(penalty=True), dict(max_len=0), dict(max_len=65), dict(max_len=2.5),
               dict(max_len=True)):
        with pytest.raises(ValueError):
            PottsFit(**kw)
    with pytest.raises(ValueError, match=r"\(N, 1, L\)"):
        m(torch.zeros(3, 20))
    with pytest.raises(TypeError):
        m(torch.zeros(3, 1, 20, dtype=torch.float64))


@pytest.mark.parametrize("K", [1, 2, 3, 10])
def test_oracle_attains_the_exact_minimum(K):
    """L = 1 .. 10, 20 random rows each, continuous values (no ties): the oracle's segmentation is the one that
    attains the minimum over every segmentation with parts <= K, the objective evaluated in Fractions."""
    rng = np.random.default_rng(100 + K)
    for L in range(1, 11):
        x = rng.uniform(0, 1, (20, L)).astype(np.float32)
        g = rng.uniform(0.0, 0.3, 20)
        y, nseg, parts = P.potts(x, g, K, parts=True)
        for r in range(20):
            best, arg = P.brute_force(x[r], g[r], K)
            assert len(arg) == 1 and parts[r] == arg[0], (L, r, parts[r], arg)
            assert P.exact_objective(x[r], parts[r], g[r]) == best and nseg[r] == len(parts[r]) and max(parts[r]) <= K
            i = 0
            for ln in parts[r]:                                  # the fit is the mean of each part, to fp32 rounding
                assert np.allclose(y[r, i:i + ln], x[r, i:i + ln].astype(np.float64).mean(), rtol=1.2e-7, atol=0)
                i += ln


def _bits(a):
    return (a.detach().numpy() if torch.is_tensor(a) else a).view(np.uint32)


@pytest.mark.parametrize("penalty", [7.5, "bic"])
@pytest.mark.parametrize("K", [1, 40, 64])
@pytest.mark.parametrize("L", [1, 2, 65, 300])
def test_eager_path_matches_oracle_bits(L, K, penalty):
    import raman_mi355x as R
    x = H.noisy_steps(3, L, 31 * L + K)
    m = R.PottsFit(penalty, K)
    xt = torch.from_numpy(x).unsqueeze(1)
    assert not m.uses_engine(xt)
    g = P.gamma(x, penalty)
    ref, nseg = P.potts(x, g, K)
    assert np.array_equal(m.gamma(xt).numpy().view(np.uint64), g.view(np.uint64))
    assert np.array_equal(m.noise_std(xt).numpy(), P.noise_mad(x) * (np.sqrt(2.0) / P.MAD_TO_SIGMA))
    y = m(xt)
    assert y.shape == xt.shape and y.dtype == torch.float32 and np.array_equal(_bits(y.squeeze(1)), ref.view(np.uint32))
    assert m.segments(xt).dtype == torch.int32 and np.array_equal(m.segments(xt).numpy(), nseg)
    xg = xt.clone().requires_grad_()
    yg = m(xg)                                                             # a graph, the same bits
    assert yg.requires_grad and np.array_equal(_bits(yg.squeeze(1)), ref.view(np.uint32))


def test_eager_special_values_match_oracle():
    from raman_mi355x.potts import _PottsFunction
    x = H.noisy_steps(8, 100, 3)
    x[0, 7], x[1, 0], x[2, 99] = np.nan, np.inf, -np.inf
    x[3, 10:16] = np.array([1e-41, -1e-41, 1e-45, 0.0, -0.0, 3e-39], dtype=np.float32)
    g = np.array([0.01, 0.01, 0.01, 0.01, -1.0, np.nan, np.inf, 0.0])
    ref, nseg = P.potts(x, g, 64)
    y = _PottsFunction.apply(torch.from_numpy(x).unsqueeze(1), torch.from_numpy(g), 64).squeeze(1)
    assert np.array_equal(_bits(y), ref.view(np.uint32))
    assert np.all(ref.view(np.uint32)[[0, 1, 2, 4, 5, 6]] == 0x7FC00000) and np.all(nseg[[0, 1, 2, 4, 5, 6]] == 0)
    assert np.isfinite(ref[[3, 7]]).all() and nseg[3] > 0 and nseg[7] == 100       # g = 0: every sample its own run


def test_gradient_is_the_segment_average():
    import raman_mi355x as R
    x = H.noisy_steps(4, 300, 8)
    m = R.PottsFit()
    _, _, parts = P.potts(x, P.gamma(x), 64, parts=True)
    xg = torch.from_numpy(x).unsqueeze(1).requires_grad_()
    up = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (4, 1, 300)).astype(np.float32))
    m(xg).backward(up)
    want = np.empty((4, 300))
    for r in range(4):
        i = 0
        for ln in parts[r]:
            want[r, i:i + ln] = up[r, 0, i:i + ln].numpy().astype(np.float64).mean()
            i += ln
    err = np.abs(xg.grad.squeeze(1).numpy() - want).max()
    print(f"max |grad - segment average| = {err:.3g}")
    assert xg.grad.dtype == torch.float32 and err <= 1e-6


@pytest.fixture(scope="module")
def reference_spectra():
    from oracle.refgen import generate_signals
    np.random.seed(7)
    clean, noisy, _, _ = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    return clean.astype(np.float32), noisy.astype(np.float32)


def _gain_db(x, y, clean):
    c = clean.astype(np.float64)
    return 10 * np.log10(((x - c) ** 2).mean(axis=1) / ((y - c) ** 2).mean(axis=1))


def test_gains_on_reference_spectra(reference_spectra):
    """The reference generator's spectra (seed 7, 256 x 2000, no extreme noise, stored as fp32) through the oracle
    with the default module's gamma: every spectrum gains, and more than HaarShrink() does on it; the mean gain
    exceeds Haar's (measured 11.12 against 7.79 dB); nseg / the true run count lies in [0.7, 1.1] (measured
    0.788 .. 1.022)."""
    import raman_mi355x as R
    clean, noisy = reference_spectra
    y, nseg = P.potts(noisy, P.gamma(noisy, R.PottsFit().penalty), R.PottsFit().max_len)
    gain = _gain_db(noisy, y, clean)
    haar = _gain_db(noisy, R.HaarShrink()(torch.from_numpy(noisy).unsqueeze(1)).squeeze(1).numpy(), clean)
    runs = 1 + (np.diff(clean, axis=1) != 0).sum(axis=1)
    ratio = nseg / runs
    print(f"potts12: mean gain {gain.mean():+.2f} dB, worst {gain.min():+.2f}; haar4_3h: {haar.mean():+.2f} dB, best "
          f"{haar.max():+.2f}; nseg / runs {ratio.min():.3f} .. {ratio.max():.3f}")
    assert gain.min() > 0 and np.all(gain > haar)
    assert gain.mean() > haar.mean()
    assert ratio.min() >= 0.7 and ratio.max() <= 1.1
