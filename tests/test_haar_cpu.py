"""Translation-invariant Haar shrinkage without a device: the ABI's argument checks, haar_thresholds, the numpy
oracle (tests/haar_oracle.py) against an independent cycle-spinning reference, the module's eager path against
the oracle's bits, and the method's claims on the reference generator's spectra.

Bar of the cycle-spin identity.  The two references evaluate the same real-valued estimator in different
orders: the contract divides by 2 at every level (exact scalings), cycle spinning divides by sqrt 2 twice per
level and averages 2^J reconstructions.  Each of its ~4 J + 2^J float64 operations carries 2^-53 relative error
on values of order 1: ~1e-14 absolute, nine orders below an fp32 ulp at 1 (6e-8).  The contract's output is the
fp32 rounding of its float64 value, so it lies within half an fp32 ulp of that value and hence within 1 fp32
ulp of the cycle-spin value rounded to fp32 -- unless a hard threshold's comparison falls differently in the
two, which takes |d| within ~1e-15 of t: the seeds are fixed, and this file checks that they meet the bar."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import haar_oracle as H
from baselines_oracle import ulp_distance


def test_abi_symbol_and_constants():
    from raman_mi355x import _lib, engine
    lib = _lib.lib()
    assert hasattr(lib, "rdn_haar_shrink") and "rdn_haar_shrink" in _lib.EXPORTED and lib.rdn_version() == 6
    with open(_lib.HEADER) as fh:
        header = fh.read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (RDN_HAAR_\w+) (\d+)", header, re.M)}
    assert consts["RDN_HAAR_MAX_LEVELS"] == _lib.HAAR_MAX_LEVELS == engine.HAAR_MAX_LEVELS == 7
    assert consts["RDN_HAAR_TILE"] == _lib.HAAR_TILE == engine.HAAR_TILE
    assert consts["RDN_HAAR_SELECT_LDS_L"] == _lib.HAAR_SELECT_LDS_L == engine.HAAR_SELECT_LDS_L
    assert re.search(r"enum \{ RDN_HAAR_SOFT = 0, RDN_HAAR_HARD = 1 \}", header)
    assert (_lib.HAAR_SOFT, _lib.HAAR_HARD) == (0, 1) and engine.HAAR_MODES == {"soft": 0, "hard": 1}


def test_argument_checks_need_no_device():
    """Every RDN_EINVAL case of rdn_haar_shrink, for n = 0 too, through ctypes with host pointers: the checks
    come before any device call (this test runs without a GPU)."""
    from raman_mi355x import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 512)()
    medbuf = (ctypes.c_double * 4)()
    base = ctypes.addressof(buf)
    x, y, med = base, base + 256 * 4, ctypes.addressof(medbuf)
    EINVAL = -1                                                                # RDN_EINVAL

    def call(x=x, y=y, med=med, n=1, L=128, levels=3, k=(1.0, 0.5, 0.0), mode=1):
        kk = None if k is None else (ctypes.c_double * max(len(k), 1))(*k)
        return lib.rdn_haar_shrink(x, y, med, n, L, levels, kk, mode, None)

    for n in (1, 0):
        assert call(n=n, k=None) == EINVAL and b"null" in lib.rdn_last_error()
        for bad in (-1.0, -1e-300, float("inf"), float("nan")):
            for pos in range(3):
                k = [1.0, 0.5, 0.25]
                k[pos] = bad
                assert call(n=n, k=k) == EINVAL, (n, bad, pos)
        for levels in (0, -1, 8, 100):
            assert call(n=n, levels=levels, k=(1.0,) * 8, L=4096) == EINVAL, (n, levels)
        for mode in (-1, 2, 7):
            assert call(n=n, mode=mode) == EINVAL, (n, mode)
        assert call(n=n, L=7) == EINVAL                                        # L < 2^levels
        assert call(n=n, L=127, levels=7, k=(1.0,) * 7) == EINVAL
        assert call(n=n, L=2 ** 31) == EINVAL                                  # L >= 2^31
        assert call(n=-1) == EINVAL
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(med=None) == EINVAL
    assert call(y=x) == EINVAL and call(y=x + 127 * 4) == EINVAL               # x and y overlapping
    assert b"overlap" in lib.rdn_last_error()
    assert call(x=y, y=x + 129 * 4) == EINVAL                                  # ... from the other side
    assert call(med=x + 127 * 4) == EINVAL and b"med overlaps" in lib.rdn_last_error()     # med over x's last sample
    assert call(med=y) == EINVAL and call(med=y - 4) == EINVAL                 # ... over y, and over y's first sample
    # n = 0 launches nothing and accepts NULL data pointers; a negative zero is a zero
    assert call(x=None, y=None, med=None, n=0) == _lib.RDN_OK
    assert call(x=None, y=None, med=None, n=0, L=2 ** 31 - 1, levels=7, k=(0.0, -0.0, 1.0, 2.0, 3.0, 4.0, 5.0)) == _lib.RDN_OK
    assert call(x=None, y=None, med=None, n=0, L=8) == _lib.RDN_OK             # L = 2^levels


def test_engine_refuses_host_input():
    from raman_mi355x import engine
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.haar_shrink(torch.zeros(2, 32), [1.0, 1.0])


def test_haar_thresholds():
    import raman_mi355x as R
    from raman_mi355x.wavelets import haar_thresholds
    assert R.haar_thresholds is haar_thresholds and "haar_thresholds" in R.__all__ and "HaarShrink" in R.__all__
    k = haar_thresholds(4, 3.0, 2000)
    assert k.dtype == np.float64 and k.shape == (4,)
    assert np.array_equal(k, H.thresholds(4, 3.0))
    c = 0.6744897501960817
    np.testing.assert_allclose(k, [3 / c, 3 / (math.sqrt(2) * c), 1.5 / c, 1.5 / (math.sqrt(2) * c)], rtol=1e-15)
    assert np.array_equal(haar_thresholds(3, "universal", 1000), H.thresholds(3, math.sqrt(2 * math.log(1000))))
    assert np.array_equal(haar_thresholds(1, 2, 2), H.thresholds(1, 2.0))      # an int threshold, L = 2^levels
    for levels, thr, L in ((0, 3.0, 100), (8, 3.0, 1000), (2.5, 3.0, 100), (True, 3.0, 100), (3, 0.0, 100),
                           (3, -1.0, 100), (3, float("inf"), 100), (3, float("nan"), 100), (3, "sure", 100),
                           (3, True, 100), (3, 3.0, 7), (3, 3.0, 10.5)):
        with pytest.raises(ValueError):
            haar_thresholds(levels, thr, L)
    for kw in (dict(levels=8), dict(threshold=-1.0), dict(mode="firm"), dict(threshold="sure")):
        with pytest.raises(ValueError):
            R.HaarShrink(**kw)
    m = R.HaarShrink()
    assert (m.levels, m.threshold, m.mode) == (4, 3.0, "hard") and len(m.state_dict()) == 0
    assert isinstance(m, R.baselines._Baseline) and "HaarShrink" not in R.BASELINES


def _bits(a):
    return (a.detach().numpy() if torch.is_tensor(a) else a).view(np.uint32)


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("levels,thr,L", [(1, 3.0, 2), (1, 1.0, 3), (3, 1.5, 9), (4, 3.0, 2000), (4, "universal", 777),
                                          (7, 2.0, 128), (7, 3.0, 1001)])
def test_eager_path_matches_oracle_bits(levels, thr, L, mode):
    import raman_mi355x as R
    x = H.noisy_steps(3, L, 17 * L + levels)
    m = R.HaarShrink(levels, thr, mode)
    xt = torch.from_numpy(x).unsqueeze(1)
    assert not m.uses_engine(xt)
    y = m(xt)
    ref, med = H.haar_shrink(x, m.factors(L), mode)
    assert y.shape == xt.shape and y.dtype == torch.float32
    assert np.array_equal(_bits(y.squeeze(1)), ref.view(np.uint32))
    sig = m.noise_std(xt)
    assert sig.dtype == torch.float64 and np.array_equal(sig.numpy(), med * (math.sqrt(2.0) / H.MAD_TO_SIGMA))
    xg = xt.clone().requires_grad_()
    yg = m(xg)                                                             # a graph, the same bits
    assert yg.requires_grad and np.array_equal(_bits(yg.squeeze(1)), ref.view(np.uint32))
    yg.sum().backward()
    assert torch.isfinite(xg.grad).all()


def test_eager_special_values_match_oracle():
    import raman_mi355x as R
    x = H.noisy_steps(5, 100, 3)
    x[0, 7], x[1, 0], x[2, 99] = np.nan, np.inf, -np.inf
    x[3, 10:16] = np.array([1e-41, -1e-41, 1e-45, 0.0, -0.0, 3e-39], dtype=np.float32)
    for mode in ("soft", "hard"):
        m = R.HaarShrink(3, 2.0, mode)
        y = m(torch.from_numpy(x).unsqueeze(1)).squeeze(1)
        ref, med = H.haar_shrink(x, m.factors(100), mode)
        assert np.array_equal(_bits(y), ref.view(np.uint32))
        assert np.all(ref.view(np.uint32)[:3] == 0x7FC00000) and np.isnan(med[:3]).all() and np.isfinite(med[3:]).all()
        assert np.array_equal(np.isnan(m.noise_std(torch.from_numpy(x).unsqueeze(1)).numpy()), np.isnan(med))


# seeds at which no hard comparison falls differently in the two references (checked by the test itself)
@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("L,levels,seed", [(64, 3, 11), (96, 5, 12), (2000, 4, 13)])
def test_oracle_is_cycle_spinning(L, levels, seed, mode):
    lam = 3.0 if mode == "hard" else 1.5
    x = H.noisy_steps(4, L, seed)
    y, _ = H.haar_shrink(x, H.thresholds(levels, lam), mode)
    import raman_mi355x as R
    eager = R.HaarShrink(levels, lam, mode)(torch.from_numpy(x).unsqueeze(1)).squeeze(1)
    assert np.array_equal(_bits(eager), y.view(np.uint32))                # the module, with haar_thresholds' factors
    ref = H.cycle_spin(x, levels, lam, mode)
    err = np.abs(y.astype(np.float64) - ref).max()
    print(f"L={L} J={levels} {mode}: max |oracle - cycle spin| = {err:.3g}, "
          f"max ulp distance {ulp_distance(y, ref.astype(np.float32)).max()}")
    assert ulp_distance(y, ref.astype(np.float32)).max() <= 1
    assert np.abs(y - x).max() > 1e-3                                      # the shrinkage did something


def test_zero_thresholds_reconstruct_bit_for_bit():
    rng = np.random.default_rng(5)
    import raman_mi355x as R
    for L, J in ((2, 1), (9, 3), (128, 7), (1000, 4), (2001, 7)):
        x = rng.uniform(0, 1.5, (3, L)).astype(np.float32)
        x[0, :2] = [0.0, 1.5]
        for mode in ("soft", "hard"):
            y, _ = H.haar_shrink(x, np.zeros(J), mode)
            assert np.array_equal(y.view(np.uint32), x.view(np.uint32)), (L, J, mode)
    # ... and so does the eager path when the estimate is 0: two equal neighbours in more than half the places
    x = np.repeat(rng.uniform(0, 1.5, (2, 100)).astype(np.float32), 3, axis=1)
    y = R.HaarShrink(4, 3.0, "hard")(torch.from_numpy(x).unsqueeze(1)).squeeze(1)
    assert np.array_equal(_bits(y), x.view(np.uint32))


@pytest.fixture(scope="module")
def reference_spectra():
    from oracle.refgen import generate_signals
    np.random.seed(7)
    clean, noisy, _, sigma = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    return clean.astype(np.float32), noisy.astype(np.float32), np.asarray(sigma).reshape(-1)


def _gain_db(x, y, clean):
    c = clean.astype(np.float64)
    return 10 * np.log10(((x - c) ** 2).mean(axis=1) / ((y - c) ** 2).mean(axis=1))


def test_gains_on_reference_spectra(reference_spectra):
    """The reference generator's spectra (seed 7, 256 x 2000, no extreme noise, stored as fp32): the default
    module gains on every spectrum and on average more than the 3-point median; its noise estimate is within
    [0.9, 1.25] of the generator's sigma (the clean signal's jumps bias the MAD upward)."""
    import raman_mi355x as R
    clean, noisy, sigma = reference_spectra
    xt = torch.from_numpy(noisy).unsqueeze(1)
    m = R.HaarShrink()
    gain = _gain_db(noisy, m(xt).squeeze(1).numpy(), clean)
    med3 = _gain_db(noisy, R.MedianFilter(3)(xt).squeeze(1).numpy(), clean)
    ratio = m.noise_std(xt).numpy() / sigma
    print(f"haar4_3h: mean gain {gain.mean():+.2f} dB, worst {gain.min():+.2f}; median 3: {med3.mean():+.2f} dB; "
          f"sigma ratio {ratio.min():.3f} .. {ratio.max():.3f}, mean {ratio.mean():.3f}")
    assert gain.min() > 0 and gain.mean() > med3.mean()
    assert ratio.min() >= 0.9 and ratio.max() <= 1.25
