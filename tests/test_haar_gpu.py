"""Translation-invariant Haar shrinkage on the device (rdn_haar_shrink, engine.haar_shrink, wavelets.HaarShrink)
against the numpy oracle (tests/haar_oracle.py).

Bar.  The kernels run the oracle's recurrence operation for operation (fp64, never fused, one rounding to fp32;
the median an exact rank selection), so the device is held to the oracle's BITS, for y and for med."""
import math

import numpy as np
import pytest
import torch

import haar_oracle as H

pytestmark = pytest.mark.gpu

T = 512             # engine.HAAR_TILE (asserted below)
LIMIT = 12288       # engine.HAAR_SELECT_LDS_L


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _spectra(n, L, seed, frac=0.5):
    """The tie-heavy spectra of the filter tests: piecewise constant (segments of 1-40 samples) with noise on half
    the samples, fp32: about a quarter of |d_1| is exactly 0.  With noise on a fifth of the samples (frac = 0.2)
    more than half of |d_1| is 0 in a row of some length: m = 0 and the call is the identity."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, size=(n, L))
    x = np.empty((n, L), dtype=np.float32)
    for r in range(n):
        x[r] = np.repeat(rng.uniform(0, 1, L), lens[r])[:L]
    noisy = rng.random((n, L)) < frac
    return (x + noisy * rng.normal(0, 0.05, (n, L))).astype(np.float32)


def _assert_matches_oracle(x, k, mode, tag):
    from raman_mi355x import engine
    y, med = engine.haar_shrink(_cuda(x), k, mode)
    ref, m = H.haar_shrink(x, k, mode)
    assert y.shape == x.shape and med.shape == (x.shape[0],) and med.dtype == torch.float64
    assert np.array_equal(med.cpu().numpy().view(np.uint64), m.view(np.uint64)), (tag, med.cpu().numpy(), m)
    assert np.array_equal(_bits(y), ref.view(np.uint32)), tag


def test_constants():
    from raman_mi355x import engine
    assert engine.HAAR_TILE == T and engine.HAAR_SELECT_LDS_L == LIMIT and engine.HAAR_MAX_LEVELS == 7


def _lengths(J):
    return sorted({2 ** J, 2 ** J + 1, 2 ** J + 2, T - 1, T, T + 1, T + 2 ** J - 1, 2 * T + 1, 3 * T + 1})


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("J", [1, 4, 7])
def test_smallest_shapes_match_oracle(J, mode):
    """n = 3 at L = 2^J (the row is all halo), 2^J + 1, 2^J + 2 (odd and even medians), around one tile, and two
    and three tiles and a sample (both tile edges, an interior tile); tie-heavy, fully noisy and sparsely noisy
    spectra; random k, so that a misplaced level shows."""
    rng = np.random.default_rng(10 * J + (mode == "hard"))
    for L in _lengths(J):
        k = rng.uniform(0.2, 3.0, J)
        _assert_matches_oracle(_spectra(3, L, 1000 * J + L), k, mode, ("ties", J, L))
        _assert_matches_oracle(H.noisy_steps(3, L, 2000 * J + L, sigma=0.05), k, mode, ("noisy", J, L))
        sparse = _spectra(3, L, 3000 * J + L, frac=0.2)
        _assert_matches_oracle(sparse, k, mode, ("sparse", J, L))
    assert (H.haar_shrink(sparse, k, mode)[1] == 0).all()              # at 3 T + 1 samples: m = 0, the identity
    assert np.array_equal(H.haar_shrink(sparse, k, mode)[0], sparse)


@pytest.mark.parametrize("L", [LIMIT - 1, LIMIT, LIMIT + 1, LIMIT + 2])
def test_select_on_both_sides_of_its_lds_limit(L):
    k = np.array([2.5, 1.0, 0.7, 1.9])
    _assert_matches_oracle(H.noisy_steps(2, L, L), k, "hard", L)
    _assert_matches_oracle(_spectra(2, L, L + 1), k, "soft", L)


def test_rows_do_not_depend_on_the_batch():
    from raman_mi355x import engine
    x = np.concatenate([H.noisy_steps(3, 2 * T + 1, 77), _spectra(2, 2 * T + 1, 78)])
    dx = _cuda(x)
    for J, mode in ((4, "hard"), (7, "soft")):
        k = H.thresholds(J, 2.0)
        y, med = engine.haar_shrink(dx, k, mode)
        for r in range(5):
            yr, mr = engine.haar_shrink(dx[r:r + 1].clone(), k, mode)
            assert torch.equal(yr.view(torch.int32), y[r:r + 1].view(torch.int32)), (J, r)
            assert torch.equal(mr.view(torch.int64), med[r:r + 1].view(torch.int64)), (J, r)


def test_special_values():
    """NaN, the infinities, signed zeros and subnormals: the stated results."""
    from raman_mi355x import engine
    L = T + 300
    x = H.noisy_steps(6, L, 5)
    x[0, 100], x[1, L - 1], x[2, 0] = np.nan, np.inf, -np.inf
    x[3, 50], x[3, T + 7] = np.inf, -np.inf
    x[4, 19:25] = [0.5, -0.0, 0.0, -0.0, -0.0, 0.5]
    x[4, 600:610] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 1e-38, 0.0, -0.0, 1e-40, -2e-40], dtype=np.float32)
    x[5] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 0.0, -0.0, 1e-40] * (L // 8 + 1), dtype=np.float32)[:L]
    for J, mode in ((1, "hard"), (4, "hard"), (4, "soft"), (7, "soft")):
        k = H.thresholds(J, 1.0)
        _assert_matches_oracle(x, k, mode, (J, mode))
        y, med = engine.haar_shrink(_cuda(x), k, mode)
        assert np.all(_bits(y)[:4] == 0x7FC00000) and torch.isnan(med[:4]).all()
        assert torch.isfinite(y[4:]).all() and torch.isfinite(med[4:]).all()
    # zero thresholds: a row of subnormals and signed zeros comes back as its values (-0 may lose its sign)
    y, med = engine.haar_shrink(_cuda(x[5:]), np.zeros(3), "hard")
    assert np.array_equal(y.cpu().numpy(), x[5:]) and float(med[0]) > 0
    # ... and spectra in [0, 1.5] bit for bit
    u = np.random.default_rng(1).uniform(0, 1.5, (3, 2 * T + 3)).astype(np.float32)
    for J in (1, 4, 7):
        for mode in ("soft", "hard"):
            assert np.array_equal(_bits(engine.haar_shrink(_cuda(u), np.zeros(J), mode)[0]), u.view(np.uint32)), (J, mode)


def test_empty_batch_out_reuse_and_refusals():
    from raman_mi355x import engine
    k = [2.0, 1.5, 1.0]
    for shape in ((0, 100), (0, 1, 100)):
        y, med = engine.haar_shrink(torch.empty(shape, device="cuda"), k)
        assert y.shape == shape and med.shape == (0,) and med.dtype == torch.float64
    x = _cuda(H.noisy_steps(4, 300, 9))
    ref_y, ref_m = engine.haar_shrink(x, k)
    out, med = torch.full_like(x, -1.0), torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    y, m = engine.haar_shrink(x, k, out=out, med=med)
    assert y is out and m is med and torch.equal(out, ref_y) and torch.equal(med, ref_m)
    assert torch.equal(engine.haar_shrink(x, np.array(k), "hard")[0], ref_y)               # k as an array
    assert not torch.equal(engine.haar_shrink(x, k, "soft")[0], ref_y)
    x3 = x.view(4, 1, 300)
    y3, m3 = engine.haar_shrink(x3, k)
    assert y3.shape == (4, 1, 300) and torch.equal(y3.view(4, 300), ref_y) and torch.equal(m3, ref_m)
    buf = torch.zeros(4 * 300 + 300, device="cuda")
    a, b = buf[:1200].view(4, 300), buf[300:].view(4, 300)
    with pytest.raises(ValueError, match="overlap"):
        engine.haar_shrink(a, k, out=a)
    with pytest.raises(ValueError, match="overlap"):
        engine.haar_shrink(a, k, out=b)
    with pytest.raises(ValueError, match="shape"):
        engine.haar_shrink(x, k, out=torch.empty(4, 299, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        engine.haar_shrink(x, k, med=torch.empty(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        engine.haar_shrink(x, k, out=torch.empty(4, 300, device="cuda", dtype=torch.float64))
    with pytest.raises(TypeError):
        engine.haar_shrink(x, k, med=torch.empty(4, device="cuda"))
    with pytest.raises(ValueError, match="med must not overlap"):
        engine.haar_shrink(x, k, med=x.view(-1)[:8].view(torch.float64))                   # a float64 view of x's storage
    with pytest.raises(ValueError, match="med must not overlap"):
        engine.haar_shrink(x, k, out=out, med=out.view(-1)[-8:].view(torch.float64))
    wide = _cuda(H.noisy_steps(4, 600, 10))
    for bad in (wide[:, ::2], wide.t()):
        with pytest.raises(ValueError, match="contiguous"):
            engine.haar_shrink(bad, k)
    with pytest.raises(TypeError):
        engine.haar_shrink(x.double(), k)
    with pytest.raises(ValueError):
        engine.haar_shrink(x.view(2, 2, 300), k)
    with pytest.raises(ValueError, match="mode"):
        engine.haar_shrink(x, k, "firm")
    for bad_k in ([], [1.0] * 8, [1.0, -1.0], [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            engine.haar_shrink(x, bad_k)
    with pytest.raises(ValueError, match="shorter"):
        engine.haar_shrink(x[:, :100].contiguous(), [1.0] * 7)                             # L < 2^7


def test_module_forward_is_the_engine_call_and_eager_under_grad():
    import raman_mi355x as R
    from raman_mi355x import engine
    x = _cuda(np.concatenate([H.noisy_steps(2, T + 37, 21), _spectra(1, T + 37, 22)])).unsqueeze(1)
    for m in (R.HaarShrink(), R.HaarShrink(3, 1.5, "soft"), R.HaarShrink(4, "universal"), R.HaarShrink(7, 2.0, "hard")):
        assert m.uses_engine(x) and len(m.state_dict()) == 0
        y = m(x)
        want, med = engine.haar_shrink(x, m.factors(T + 37), m.mode)
        assert y.shape == x.shape and torch.equal(y.view(torch.int32), want.view(torch.int32))
        assert torch.equal(m.noise_std(x), med * (math.sqrt(2.0) / H.MAD_TO_SIGMA))
        xg = x.clone().requires_grad_()
        assert not m.uses_engine(xg)
        yg = m(xg)                                     # the eager path: the same arithmetic in torch ops, with a graph
        assert yg.requires_grad and yg.grad_fn is not None
        assert torch.equal(yg.detach().view(torch.int32), y.view(torch.int32))
        assert torch.equal(m.noise_std(xg).detach().view(torch.int64), m.noise_std(x).view(torch.int64))
        with torch.no_grad():
            assert m.uses_engine(xg)
    with pytest.raises(ValueError, match=r"\(N, 1, L\)"):
        R.HaarShrink()(x.squeeze(1))


def test_evaluate_synthetic_meters_the_module_like_a_network():
    """256 simulator spectra of 2000 samples: the module's accumulator and report words are those of
    engine.metrics / engine.snr on its separately computed output, and the same for two batch sizes."""
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate_synthetic
    bins = (20, 37, 17)
    models = {"haar4_3h": R.HaarShrink(), "haar3_1.5s": R.HaarShrink(3, 1.5, "soft")}
    kw = dict(signal_length=2000, snr_bins=bins)
    a = evaluate_synthetic(models, 256, batch_size=256, **kw)
    b = evaluate_synthetic(models, 256, batch_size=100, **kw)
    assert list(a) == list(models)
    clean, noisy, snr_db, _ = engine.generate(256, 20250410, signal_length=2000)
    for name, m in models.items():
        for key in ("acc", "report", "means", "SNR_in", "SNR_out", "SNR_gain", "by_snr"):
            assert a[name][key] == b[name][key], (name, key)
        y = m(noisy.view(256, 1, 2000))
        acc, rep = engine.new_acc("cuda"), engine.new_report(17, "cuda")
        per, _ = engine.metrics(y.view(256, 2000), clean, acc=acc)
        engine.snr(noisy, y, clean, key=snr_db, bins=bins, per4=per, report=rep, per_spectrum=False)
        assert acc.cpu().tolist() == a[name]["acc"] and rep.cpu().tolist() == a[name]["report"], name
        assert sum(e["count"] for e in a[name]["by_snr"]) == 256
    print(f"simulator spectra: haar4_3h {a['haar4_3h']['SNR_gain']:+.2f} dB, haar3_1.5s {a['haar3_1.5s']['SNR_gain']:+.2f} dB")


def test_gains_on_reference_spectra():
    """The gain test of test_haar_cpu.py on the device: the reference generator's spectra (seed 7, 256 x 2000, no
    extreme noise, stored as fp32); the default module gains on every spectrum and on average more than the
    3-point median; its noise estimate is within [0.9, 1.25] of the generator's sigma."""
    import raman_mi355x as R
    from oracle.refgen import generate_signals
    from raman_mi355x import engine
    np.random.seed(7)
    clean, noisy, _, sigma = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    c, x = _cuda(clean.astype(np.float32)), _cuda(noisy.astype(np.float32))
    m = R.HaarShrink()
    gain = engine.snr(x, m(x.unsqueeze(1)), c)[0][:, 2].cpu().numpy()
    med3 = engine.snr(x, R.MedianFilter(3)(x.unsqueeze(1)), c)[0][:, 2].cpu().numpy()
    ratio = m.noise_std(x.unsqueeze(1)).cpu().numpy() / np.asarray(sigma).reshape(-1)
    print(f"haar4_3h: mean gain {gain.mean():+.2f} dB, worst {gain.min():+.2f}; median 3: {med3.mean():+.2f} dB; "
          f"sigma ratio {ratio.min():.3f} .. {ratio.max():.3f}, mean {ratio.mean():.3f}")
    assert gain.min() > 0 and gain.mean() > med3.mean()
    assert ratio.min() >= 0.9 and ratio.max() <= 1.25
