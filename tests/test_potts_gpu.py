"""The exact piecewise-constant (Potts) fit on the device (rdn_potts, rdn_noise_mad, engine.potts, potts.PottsFit)
against the numpy oracle (tests/potts_oracle.py).

Bar.  The kernel runs the oracle's recurrence operation for operation (fp64, never fused, a minimum and the smallest
length that attains it, one rounding to fp32), so the device is held to the oracle's BITS, for y and for nseg."""
import math

import numpy as np
import pytest
import torch

import haar_oracle as H
import potts_oracle as P
from test_haar_gpu import _spectra

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _assert_matches_oracle(x, g, K, tag):
    from raman_mi355x import engine
    gd = _cuda(np.asarray(g, dtype=np.float64)) if np.ndim(g) else float(g)
    y, nseg = engine.potts(_cuda(x), gd, K)
    ref, segs = P.potts(x, g, K)
    assert y.shape == x.shape and nseg.shape == (x.shape[0],) and nseg.dtype == torch.int32
    assert np.array_equal(nseg.cpu().numpy(), segs), (tag, nseg.cpu().numpy(), segs)
    assert np.array_equal(_bits(y), ref.view(np.uint32)), tag
    return ref, segs


LENGTHS = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 257)


@pytest.mark.parametrize("K", [1, 2, 40, 63, 64])
def test_smallest_shapes_match_oracle(K):
    """n = 3 around one and two 64-sample chunks and at four chunks and a sample; tie-heavy and fully noisy spectra; a
    different gamma per row, and a scrambled gamma shows."""
    rng = np.random.default_rng(K)
    shown = False
    for L in LENGTHS:
        g = rng.uniform(0.002, 0.05, 3)
        _assert_matches_oracle(_spectra(3, L, 1000 * K + L), g, K, ("ties", K, L))
        x = H.noisy_steps(3, L, 2000 * K + L, sigma=0.05)
        ref, _ = _assert_matches_oracle(x, g, K, ("noisy", K, L))
        g2 = g * np.array([1.0, 30.0, 0.03])
        ref2, _ = _assert_matches_oracle(x, g2, K, ("scaled", K, L))
        shown |= not np.array_equal(ref[1:], ref2[1:]) and np.array_equal(ref[0], ref2[0])
    assert shown or K == 1                                             # K = 1: one segmentation, whatever gamma is


def test_long_rows():
    x = np.concatenate([H.noisy_steps(1, 10000, 5), _spectra(1, 10000, 6)])
    _, segs = _assert_matches_oracle(x, P.gamma(x), 64, "10000")
    assert 300 < segs[0] < 700


def test_rows_past_2_to_the_31_samples():
    """n * L just above 2^31: the last rows' offsets into x, y (elements) and work (bytes) do not fit 32 bits.  The bulk
    is uniform noise; the first two and the last three rows are spectra held to the oracle."""
    from raman_mi355x import engine
    L = 4099                                                            # 64 chunks and three samples
    n = 2 ** 31 // L + 5
    assert (n - 3) * L > 2 ** 31
    x = torch.rand((n, L), device="cuda")
    rows = np.concatenate([H.noisy_steps(3, L, 41), _spectra(2, L, 42)])
    x[:2] = _cuda(rows[:2])
    x[-3:] = _cuda(rows[2:])
    y, nseg = engine.potts(x, 0.012, 64)
    ref, segs = P.potts(rows, 0.012, 64)
    got = torch.cat([y[:2], y[-3:]])
    assert np.array_equal(_bits(got), ref.view(np.uint32))
    assert np.array_equal(torch.cat([nseg[:2], nseg[-3:]]).cpu().numpy(), segs)
    assert int(nseg.min()) >= 1 and int(nseg.max()) <= L


def test_constant_zero_and_huge_penalty_rows():
    """Exactly constant rows (every candidate ties at sse = 0: the smallest len wins the tie, yet the fit has the fewest
    segments, since a shorter last part never costs less), g = 0 (every sample a run of its own, or a tie) and
    g = 1e30 (the fewest runs: ceil(L / K))."""
    for K in (1, 7, 64):
        for L in (1, 64, 65, 200):
            x = np.repeat(np.array([[0.5], [0.0], [1.0 / 3]], dtype=np.float32), L, axis=1)
            for g in (0.01, 1e30):
                ref, segs = _assert_matches_oracle(x, g, K, ("const", K, L, g))
                assert np.all(segs == -(-L // K)) and np.array_equal(ref[0], x[0]) and np.array_equal(ref[1], x[1])
            _assert_matches_oracle(x, 0.0, K, ("const g=0", K, L))
            noisy = H.noisy_steps(3, L, L + K)
            _assert_matches_oracle(noisy, 0.0, K, ("g=0", K, L))       # costs of order 1e-17, of either sign
            _, segs = _assert_matches_oracle(noisy, 1e30, K, ("g=1e30", K, L))
            assert np.all(segs == -(-L // K))
            _assert_matches_oracle(_spectra(3, L, L + K + 1), np.array([0.0, 1e30, -0.0]), K, ("ties g=0", K, L))


def test_rows_do_not_depend_on_the_batch():
    from raman_mi355x import engine
    x = np.concatenate([H.noisy_steps(4, 193, 77), _spectra(5, 193, 78)])          # 9 rows: three workgroups
    dx, g = _cuda(x), _cuda(P.gamma(x))
    for K in (40, 64):
        y, nseg = engine.potts(dx, g, K)
        for r in range(9):
            yr, nr = engine.potts(dx[r:r + 1].clone(), g[r:r + 1].clone(), K)
            assert torch.equal(yr.view(torch.int32), y[r:r + 1].view(torch.int32)), (K, r)
            assert torch.equal(nr, nseg[r:r + 1]), (K, r)


def test_special_values():
    """A NaN, +inf and -inf row and rows with g in {-1, NaN, inf}: all 0x7fc00000 and nseg = 0, the other rows of the
    same call correct; subnormal and signed-zero rows equal the oracle."""
    from raman_mi355x import engine
    L = 300
    x = H.noisy_steps(10, L, 5)
    x[0, 100], x[1, L - 1], x[2, 0] = np.nan, np.inf, -np.inf
    g = np.full(10, 0.01)
    g[3], g[4], g[5] = -1.0, np.nan, np.inf
    x[6, 19:25] = [0.5, -0.0, 0.0, -0.0, -0.0, 0.5]
    x[6, 200:210] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 1e-38, 0.0, -0.0, 1e-40, -2e-40], dtype=np.float32)
    x[7] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 0.0, -0.0, 1e-40] * (L // 8 + 1), dtype=np.float32)[:L]
    x[8] = np.array([0.0, -0.0, -0.0, 0.0, 0.0] * (L // 5), dtype=np.float32)
    g[7], g[8] = 1e-85, 0.0
    for K in (5, 64):
        ref, segs = _assert_matches_oracle(x, g, K, K)
        assert np.all(ref.view(np.uint32)[:6] == 0x7FC00000) and np.all(segs[:6] == 0)
        assert np.isfinite(ref[6:]).all() and np.all(segs[6:] > 0)
    y, nseg = engine.potts(_cuda(x), _cuda(g), 64)
    assert np.all(_bits(y)[:6] == 0x7FC00000) and torch.isfinite(y[6:]).all() and nseg[:6].sum() == 0


@pytest.mark.parametrize("L", [1, 2, 3, 12288, 12289])
def test_noise_mad_is_haar_shrinks_median(L):
    from raman_mi355x import engine
    x = np.concatenate([H.noisy_steps(2, L, L), _spectra(2, L, L + 1)])
    x[3, L // 2] = np.inf
    m = engine.noise_mad(_cuda(x))
    assert m.dtype == torch.float64 and m.shape == (4,) and bool(torch.isnan(m[3]))
    if L >= 2:
        want = engine.haar_shrink(_cuda(x), [1.0])[1]
        assert torch.equal(m.view(torch.int64), want.view(torch.int64))
    assert np.array_equal(m.cpu().numpy().view(np.uint64), P.noise_mad(x).view(np.uint64))


def test_empty_batch_out_reuse_and_refusals():
    from raman_mi355x import engine
    for shape in ((0, 100), (0, 1, 100)):
        y, nseg = engine.potts(torch.empty(shape, device="cuda"), 0.01)
        assert y.shape == shape and nseg.shape == (0,) and nseg.dtype == torch.int32
        assert engine.noise_mad(torch.empty(shape, device="cuda")).shape == (0,)
    x = _cuda(H.noisy_steps(4, 300, 9))
    g = _cuda(P.gamma(x.cpu().numpy()))
    ref_y, ref_n = engine.potts(x, g)
    out, nseg = torch.full_like(x, -1.0), torch.full((4,), -1, dtype=torch.int32, device="cuda")
    work = torch.zeros(4 * 300 + 17, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                                  # a second call on the used scratch
        y, n = engine.potts(x, g, out=out, nseg=nseg, work=work)
        assert y is out and n is nseg and torch.equal(out, ref_y) and torch.equal(nseg, ref_n)
    assert torch.equal(engine.potts(x, float(g[0]))[0][0], ref_y[0])    # a float is broadcast
    assert not torch.equal(engine.potts(x, g, 5)[0], ref_y)
    x3 = x.view(4, 1, 300)
    y3, n3 = engine.potts(x3, g)
    assert y3.shape == (4, 1, 300) and torch.equal(y3.view(4, 300), ref_y) and torch.equal(n3, ref_n)
    med = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    assert engine.noise_mad(x3, out=med) is med and torch.equal(med, engine.noise_mad(x))
    buf = torch.zeros(4 * 300 + 300, device="cuda")
    a, b = buf[:1200].view(4, 300), buf[300:].view(4, 300)
    with pytest.raises(ValueError, match="overlap"):
        engine.potts(a, g, out=a)
    with pytest.raises(ValueError, match="overlap"):
        engine.potts(a, g, out=b)
    with pytest.raises(ValueError, match="shape"):
        engine.potts(x, g, out=torch.empty(4, 299, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        engine.potts(x, g, nseg=torch.empty(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        engine.potts(x, g[:3])
    with pytest.raises(TypeError):
        engine.potts(x, g, out=torch.empty(4, 300, device="cuda", dtype=torch.float64))
    with pytest.raises(TypeError):
        engine.potts(x, g, nseg=torch.empty(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        engine.potts(x, g.float())
    with pytest.raises(TypeError):
        engine.potts(x, g, work=torch.empty(1200, dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError, match="N \\* L"):
        engine.potts(x, g, work=torch.empty(1199, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="work must not overlap"):
        engine.potts(x, g, work=x.view(-1).view(torch.uint8))
    with pytest.raises(ValueError, match="work must not overlap"):
        engine.potts(x, g, out=out, work=out.view(-1).view(torch.uint8)[-1200:])
    with pytest.raises(ValueError, match="nseg must not overlap"):
        engine.potts(x, g, nseg=x.view(-1)[:4].view(torch.int32))
    with pytest.raises(ValueError, match="nseg must not overlap"):
        engine.potts(x, g, work=work, nseg=work[:16].view(torch.int32))
    with pytest.raises(ValueError, match="out must not overlap"):
        engine.noise_mad(x, out=x.view(-1)[:8].view(torch.float64))
    with pytest.raises(TypeError):
        engine.noise_mad(x, out=torch.empty(4, device="cuda"))
    wide = _cuda(H.noisy_steps(4, 600, 10))
    for bad in (wide[:, ::2], wide.t()):
        with pytest.raises(ValueError, match="contiguous"):
            engine.potts(bad, 0.01)
        with pytest.raises(ValueError, match="contiguous"):
            engine.noise_mad(bad)
    with pytest.raises(TypeError):
        engine.potts(x.double(), g)
    with pytest.raises(ValueError):
        engine.potts(x.view(2, 2, 300), g[:2])
    for bad_k in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="max_len"):
            engine.potts(x, g, bad_k)


def test_module_forward_is_the_engine_call_and_eager_under_grad():
    import raman_mi355x as R
    from raman_mi355x import engine
    L = 165
    x = _cuda(np.concatenate([H.noisy_steps(2, L, 21), _spectra(1, L, 22)])).unsqueeze(1)
    for m in (R.PottsFit(), R.PottsFit(8.0, 40), R.PottsFit("bic"), R.PottsFit(16.0, 1)):
        assert m.uses_engine(x) and len(m.state_dict()) == 0
        y = m(x)
        sigma = engine.noise_mad(x) * (math.sqrt(2.0) / P.MAD_TO_SIGMA)
        g = m.factor(L) * (sigma * sigma)
        want, nseg = engine.potts(x, g, m.max_len)
        assert y.shape == x.shape and torch.equal(y.view(torch.int32), want.view(torch.int32))
        assert torch.equal(m.noise_std(x), sigma) and torch.equal(m.gamma(x), g) and torch.equal(m.segments(x), nseg)
        assert np.array_equal(g.cpu().numpy().view(np.uint64), P.gamma(x.squeeze(1).cpu().numpy(), m.penalty).view(np.uint64))
        xg = x.clone().requires_grad_()
        assert not m.uses_engine(xg)
        yg = m(xg)                                     # the eager path: the same arithmetic in torch ops, with a graph
        assert yg.requires_grad and yg.grad_fn is not None
        assert torch.equal(yg.detach().view(torch.int32), y.view(torch.int32))
        assert torch.equal(m.segments(xg), nseg) and torch.equal(m.noise_std(xg).view(torch.int64), sigma.view(torch.int64))
        with torch.no_grad():
            assert m.uses_engine(xg)
    with pytest.raises(ValueError, match=r"\(N, 1, L\)"):
        R.PottsFit()(x.squeeze(1))


def test_evaluate_synthetic_meters_the_module_like_a_network():
    """256 simulator spectra of 2000 samples: the module's accumulator and report words are those of
    engine.metrics / engine.snr on its separately computed output, and the same for two batch sizes."""
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate_synthetic
    bins = (20, 37, 17)
    models = {"potts12": R.PottsFit(), "haar4_3h": R.HaarShrink()}
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
    print(f"simulator spectra: potts12 {a['potts12']['SNR_gain']:+.2f} dB, haar4_3h {a['haar4_3h']['SNR_gain']:+.2f} dB")


def test_gains_on_reference_spectra():
    """The gain test of test_potts_cpu.py on the device: the reference generator's spectra (seed 7, 256 x 2000, no
    extreme noise, stored as fp32); every spectrum gains, and more than HaarShrink() on it; the mean exceeds Haar's;
    nseg / the true run count lies in [0.7, 1.1]."""
    import raman_mi355x as R
    from oracle.refgen import generate_signals
    from raman_mi355x import engine
    np.random.seed(7)
    clean, noisy, _, _ = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    clean = clean.astype(np.float32)
    c, x = _cuda(clean), _cuda(noisy.astype(np.float32))
    m = R.PottsFit()
    gain = engine.snr(x, m(x.unsqueeze(1)), c)[0][:, 2].cpu().numpy()
    haar = engine.snr(x, R.HaarShrink()(x.unsqueeze(1)), c)[0][:, 2].cpu().numpy()
    ratio = m.segments(x.unsqueeze(1)).cpu().numpy() / (1 + (np.diff(clean, axis=1) != 0).sum(axis=1))
    print(f"potts12: mean gain {gain.mean():+.2f} dB, worst {gain.min():+.2f}; haar4_3h: {haar.mean():+.2f} dB; "
          f"nseg / runs {ratio.min():.3f} .. {ratio.max():.3f}")
    assert gain.min() > 0 and np.all(gain > haar)
    assert gain.mean() > haar.mean()
    assert ratio.min() >= 0.7 and ratio.max() <= 1.1
