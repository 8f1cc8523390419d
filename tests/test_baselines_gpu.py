"""The baseline filters on the device (rdn_fir / rdn_median, engine.fir / engine.median, baselines.py) against
the numpy oracle (tests/baselines_oracle.py) and scipy's outputs (tests/golden/baselines.npz).

Bars.  The kernels run the oracle's recurrence operation for operation (fp64 products and sums, never fused,
one rounding to fp32; a rank-h pick of the inputs' bits), so the device is held to the oracle's BITS; against
scipy's float64 outputs the bar is the oracle's own: <= 1 fp32 ulp for the FIR filters, equal bits for the
median (test_baselines_cpu.py).  A NaN compares as a NaN in FIR outputs (IEEE leaves its sign and payload to
the implementation); the median's NaN is the quiet NaN 0x7fc00000 and is compared bit for bit."""
import numpy as np
import pytest
import torch

import baselines_oracle as O
from baselines_oracle import G, check_against_golden, golden_cases, oracle_of
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu

T = 2048            # engine.FILTER_TILE (asserted below)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _assert_fir_bits(y, ref):
    y = y.cpu().numpy() if torch.is_tensor(y) else y
    assert y.shape == ref.shape
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(y.view(np.uint32)[ok], ref.view(np.uint32)[ok])


def _spectra(n, L, seed):
    """Piecewise-constant spectra (segments of 1-40 samples, so windows hold many ties) plus noise, fp32."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, size=(n, L))
    x = np.empty((n, L), dtype=np.float32)
    for r in range(n):
        x[r] = np.repeat(rng.uniform(0, 1, L), lens[r])[:L]
    noisy = rng.random((n, L)) < 0.5                               # half the samples keep exact ties
    return (x + noisy * rng.normal(0, 0.05, (n, L))).astype(np.float32)


def test_tile_constant():
    from raman_mi355x import engine
    assert engine.FILTER_TILE == T and engine.FILTER_MAX_WINDOW == 255


@pytest.mark.parametrize("key", [k for k in G.files if not k.startswith("x_")])
def test_device_matches_oracle_and_golden(key):
    _, x, make = next(c for c in golden_cases() if c[0] == key)
    m = make().cuda()
    y = m(_cuda(x).unsqueeze(1)).squeeze(1).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), oracle_of(m, x).view(np.uint32))
    check_against_golden(key, y)


def _lengths(w):
    h = (w - 1) // 2
    # ... and 3 T + 1, where the middle tile is interior for every window (the kernels' unmirrored staging)
    return sorted({w, w + 1, T - 1, T, T + 1, T + h, 2 * T + 1, 3 * T + 1} | ({T - h, 2 * T - h + 1} if h else set()))


@pytest.mark.parametrize("edge", [False, True], ids=["mirror", "edge_table"])
@pytest.mark.parametrize("w", [1, 3, 21, 255])
def test_fir_smallest_shapes_match_oracle(w, edge):
    """n = 3 at L = w (every output an edge), w + 1, and around one and two tiles; random taps and a random
    edge table, so that a misplaced row or tap shows."""
    from raman_mi355x import engine
    rng = np.random.default_rng(100 + w)
    taps = rng.normal(0, 1, w)
    table = rng.normal(0, 1, (w - 1, w)) if edge else None
    d_taps, d_table = _cuda(taps), _cuda(table) if edge else None
    for L in _lengths(w):
        x = _spectra(3, L, 1000 * w + L)
        y = engine.fir(_cuda(x), d_taps, edge_taps=d_table)
        _assert_fir_bits(y, O.fir(x, taps, table))


@pytest.mark.parametrize("w", [1, 3, 5, 7, 9, 21, 25, 27, 255])
def test_median_smallest_shapes_match_oracle(w):
    """The same lengths for the median; 3 to 25 are the sorting-network kernels, 1, 27 and wider the radix select."""
    from raman_mi355x import engine
    for L in _lengths(w):
        x = _spectra(3, L, 2000 * w + L)
        y = engine.median(_cuda(x), w)
        assert np.array_equal(_bits(y), O.median(x, w).view(np.uint32)), (w, L)


def test_rows_do_not_depend_on_the_batch():
    from raman_mi355x import baselines as B
    x = _spectra(5, 2 * T + 1, 77)
    dx = _cuda(x).unsqueeze(1)
    for m in (B.SavitzkyGolay(21, 3), B.GaussianSmooth(2.5), B.MedianFilter(3), B.MedianFilter(21), B.MedianFilter(31)):
        m = m.cuda()
        batch = m(dx)
        for r in range(5):
            assert torch.equal(m(dx[r:r + 1].clone()).view(torch.int32), batch[r:r + 1].view(torch.int32)), (type(m), r)


def test_special_values():
    """NaN, the infinities, signed zeros and subnormals: the stated results."""
    from raman_mi355x import engine
    L = T + 300
    x = _spectra(3, L, 5)
    x[0, 100], x[0, T - 1], x[0, T + 150] = np.nan, np.nan, -np.nan
    x[1, 50], x[1, 400], x[1, 401], x[1, T] = np.inf, np.inf, -np.inf, -np.inf
    x[2, 19:25] = [0.5, -0.0, 0.0, -0.0, -0.0, 0.5]
    x[2, 600:610] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 1e-38, 0.0, -0.0, 1e-40, -2e-40], dtype=np.float32)
    dx = _cuda(x)
    for w in (3, 7, 21, 27):
        h = (w - 1) // 2
        y = engine.median(dx, w).cpu().numpy()
        assert np.array_equal(y.view(np.uint32), O.median(x, w).view(np.uint32)), w
        nan = np.flatnonzero(np.isnan(y[0]))                      # a NaN poisons exactly the windows that hold it
        want = np.unique(np.concatenate([np.arange(p - h, p + h + 1) for p in (100, T - 1, T + 150)]))
        assert np.array_equal(nan, want) and np.all(y.view(np.uint32)[0, nan] == 0x7FC00000)
        assert not np.isnan(y[1:]).any()                          # the infinities are ordinary values
        taps = np.full(w, 1.0 / w)
        f = engine.fir(dx, taps).cpu().numpy()
        _assert_fir_bits(f, O.fir(x, taps))
        assert np.array_equal(np.flatnonzero(np.isnan(f[0])), want)
        assert np.all(f[1, 50 - h:50 + h + 1] == np.inf)
        assert np.isnan(f[1, 401 - h:400 + h + 1]).all()          # +inf and -inf in one window
    assert np.signbit(engine.median(dx, 3).cpu().numpy()[2, 20:24]).tolist() == [False, True, True, True]
    # the identity filter returns subnormals as they are (read as their values, one rounding at the end)
    ident = engine.fir(dx[2:], np.array([0.0, 1.0, 0.0])).cpu().numpy()
    assert np.array_equal(ident[0, 600:606].view(np.uint32), x[2, 600:606].view(np.uint32))
    # non-finite taps: the IEEE result of the recurrence
    for taps in (np.array([0.5, np.inf, 0.5]), np.array([np.nan, 1.0, 0.0])):
        _assert_fir_bits(engine.fir(dx[1:], taps), O.fir(x[1:], taps))


def test_empty_batch_out_reuse_and_refusals():
    from raman_mi355x import engine
    taps = _cuda(np.full(5, 0.2))
    for shape in ((0, 100), (0, 1, 100)):
        e = torch.empty(shape, device="cuda")
        assert engine.fir(e, taps).shape == shape and engine.median(e, 5).shape == shape
    x = _cuda(_spectra(4, 300, 9))
    out = torch.full_like(x, -1.0)
    ref_f, ref_m = engine.fir(x, taps), engine.median(x, 5)
    assert engine.fir(x, taps, out=out) is out and torch.equal(out, ref_f)
    assert engine.median(x, 5, out=out) is out and torch.equal(out, ref_m)       # the buffer reused
    x3 = x.view(4, 1, 300)
    assert engine.median(x3, 5).shape == (4, 1, 300) and torch.equal(engine.median(x3, 5).view(4, 300), ref_m)
    buf = torch.zeros(4 * 300 + 300, device="cuda")
    a, b = buf[:1200].view(4, 300), buf[300:].view(4, 300)
    for call in (lambda **k: engine.fir(a, taps, **k), lambda **k: engine.median(a, 5, **k)):
        with pytest.raises(ValueError, match="overlap"):
            call(out=a)
        with pytest.raises(ValueError, match="overlap"):
            call(out=b)
        with pytest.raises(ValueError, match="shape"):
            call(out=torch.empty(4, 299, device="cuda"))
        with pytest.raises(TypeError):
            call(out=torch.empty(4, 300, device="cuda", dtype=torch.float64))
    wide = _cuda(_spectra(4, 600, 10))
    for bad in (wide[:, ::2], wide.t()):
        with pytest.raises(ValueError, match="contiguous"):
            engine.fir(bad, taps)
        with pytest.raises(ValueError, match="contiguous"):
            engine.median(bad, 5)
    with pytest.raises(TypeError):
        engine.median(x.double(), 5)
    with pytest.raises(ValueError):
        engine.median(x, 4)
    with pytest.raises(ValueError):
        engine.median(x, 301)                                                    # L < w
    with pytest.raises(ValueError):
        engine.fir(x, _cuda(np.full(4, 0.25)))
    with pytest.raises(ValueError, match="shape"):
        engine.fir(x, taps, edge_taps=_cuda(np.zeros((5, 5))))
    with pytest.raises(ValueError):
        engine.fir(x.view(2, 2, 300), taps)


def test_module_forward_is_the_engine_call_and_eager_under_grad():
    from raman_mi355x import baselines as B, engine
    x = _cuda(_spectra(3, T + 37, 21)).unsqueeze(1)
    for m in (B.MovingAverage(5), B.SavitzkyGolay(21, 3), B.SavitzkyGolay(11, 5, "mirror"), B.GaussianSmooth(1.0),
              B.MedianFilter(7)):
        m = m.cuda()
        assert m.uses_engine(x) and len(m.state_dict()) == 0
        y = m(x)
        want = engine.median(x, m.window) if isinstance(m, B.MedianFilter) else engine.fir(x, m.taps, edge_taps=m.edge_taps)
        assert y.shape == x.shape and torch.equal(y.view(torch.int32), want.view(torch.int32))
        xg = x.clone().requires_grad_()
        assert not m.uses_engine(xg)
        yg = m(xg)                                     # the eager path: the same arithmetic in torch ops, with a graph
        assert yg.requires_grad and yg.grad_fn is not None
        assert torch.equal(yg.detach().view(torch.int32), y.view(torch.int32))
        with torch.no_grad():
            assert m.uses_engine(xg)
    with pytest.raises(ValueError, match=r"\(N, 1, L\)"):
        B.MedianFilter(3)(x.squeeze(1))
    with pytest.raises(ValueError, match="move the module"):
        B.MovingAverage(3)(x)                          # taps left on the host


@pytest.fixture(scope="module")
def cnn():
    import raman_mi355x as R
    m = R.DenoiseCNN()
    m.load_state_dict(golden_state_dict("DenoiseCNN", "trained"), strict=True)
    return m.cuda().eval()


def test_evaluate_synthetic_meters_baselines_like_networks(cnn, monkeypatch, tmp_path):
    """One call meters a network and two filters over 512 simulator spectra.  A filter's accumulator and
    report words are those of engine.metrics / engine.snr on its output computed separately, the same for
    batch sizes 512 and 100, and the network's entry is what a call without the filters gives."""
    from raman_mi355x import baselines as B, engine
    from raman_mi355x.evaluate import evaluate, evaluate_synthetic, write_comparison
    monkeypatch.setenv("RDN_SHORT_TILES", "0")         # one forward geometry for the network at both batch sizes
    monkeypatch.setenv("RDN_WALK", "1")
    bins = (20, 37, 17)
    models = {"cnn": cnn, "med3": B.MedianFilter(3), "ma5": B.MovingAverage(5).cuda()}
    kw = dict(signal_length=2000, snr_bins=bins)
    a = evaluate_synthetic(models, 512, batch_size=512, **kw)
    b = evaluate_synthetic(models, 512, batch_size=100, **kw)
    alone = evaluate_synthetic({"cnn": cnn}, 512, batch_size=512, **kw)["cnn"]
    assert list(a) == ["cnn", "med3", "ma5"]
    for name in models:
        for k in ("acc", "report", "means", "SNR_in", "SNR_out", "SNR_gain", "by_snr"):
            assert a[name][k] == b[name][k], (name, k)
    for k in ("acc", "report", "means", "by_snr"):
        assert alone[k] == a["cnn"][k], k
    clean, noisy, snr_db, _ = engine.generate(512, 20250410, signal_length=2000)
    for name in ("med3", "ma5"):
        y = models[name](noisy.view(512, 1, 2000))
        acc, rep = engine.new_acc("cuda"), engine.new_report(17, "cuda")
        per, _ = engine.metrics(y.view(512, 2000), clean, acc=acc)
        engine.snr(noisy, y, clean, key=snr_db, bins=bins, per4=per, report=rep, per_spectrum=False)
        assert acc.cpu().tolist() == a[name]["acc"] and rep.cpu().tolist() == a[name]["report"], name
        assert sum(e["count"] for e in a[name]["by_snr"]) == 512
    # evaluate() takes a parameter-free module's device from its buffers, or the current device
    n = noisy[:64].cpu().numpy()
    c = clean[:64].cpu().numpy()
    for name in ("med3", "ma5"):
        r = evaluate(models[name], n, c, batch_size=40, snr_bins=bins, snrs=snr_db[:64])
        per3, _ = engine.snr(noisy[:64], models[name](noisy[:64].unsqueeze(1)), clean[:64])
        np.testing.assert_allclose(r["SNR_gain"], float(per3[:, 2].mean()), rtol=1e-12)
    root = write_comparison(a, str(tmp_path))
    assert len(open(f"{root}/comparison.txt").read().splitlines()) == 4


def test_median_gains_and_moving_average_loses_on_reference_spectra():
    """The reference generator's spectra (seed 7, 256 x 2000, no extreme noise, stored as fp32): the clean
    signal is piecewise constant with segments of 1-40 samples, so a 3-point median gains on the noisy half
    (+2.6 dB over nominal SNR < 25 dB with scipy on the host) and a 5-point mean loses (-8.9 dB over all)."""
    from oracle.refgen import generate_signals
    from raman_mi355x import baselines as B, engine
    np.random.seed(7)
    clean, noisy, snrs, _ = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    c, x = _cuda(clean.astype(np.float32)), _cuda(noisy.astype(np.float32))
    snrs = np.asarray(snrs).reshape(-1)
    gain = {}
    for name, m in (("med3", B.MedianFilter(3)), ("ma5", B.MovingAverage(5).cuda())):
        per, _ = engine.snr(x, m(x.unsqueeze(1)), c)
        gain[name] = per[:, 2].cpu().numpy()
    low = snrs < 25
    print(f"median 3: mean gain {gain['med3'][low].mean():+.2f} dB over {int(low.sum())} spectra below 25 dB; "
          f"moving average 5: {gain['ma5'].mean():+.2f} dB over all")
    assert low.sum() > 20 and gain["med3"][low].mean() > 0
    assert gain["ma5"].mean() < 0
