"""The blind residual report on the device (rdn_blind / engine.blind, evaluate_blind, evaluate(blind=...)) against
the numpy oracle (tests/blind_oracle.py: float64 values, every sum over the positions exact, float32 bin index).

Tolerances.  The device's sums differ from the oracle's only in summation order: a sum of L terms t taken in any
order is within (L - 1) 2^-53 sum|t| of the exact one, below 3e-12 relative at every length here (L <= 20480).
With delta = 3 L 2^-53 (a sum, its divisor's sum, and the rounding of the centring; 7e-12 at most):
  RMS, Ratio   one such sum of non-negative terms, a division and a square root: rtol 1e-9.
  Mean         sum|r| <= L RMS (Cauchy-Schwarz), so |error| <= L 2^-53 RMS: atol 1e-9 RMS.
  rho_k        |numerator error| <= L 2^-53 sum|d_i d_{i+k}| <= L 2^-53 D (Cauchy-Schwarz), D's own relative
               error is of that size and |rho_k| <= 1: |error| <= delta, atol 1e-9, for Rho1 and RhoMax as well.
               This holds while the rounding of d_i = r_i - Mean (2^-53 |r_i|) is of the size of 2^-53 |d_i|,
               that is while |Mean| does not exceed the centred standard deviation: asserted on the oracle.
  Q            a sum of K squares of rho_k with positive weights: relative error at most 2 delta sum|rho_k| /
               sum rho_k^2 <= 2 delta sqrt(K) / |rho|_2, asserted on the oracle to be below 1e-9: rtol 1e-8.
  SNR_est      S within delta relative, (S - s2) / s2 within delta S / |S - s2|, times 10 / ln 10 in dB,
               asserted on the oracle to be below 1e-10: atol 1e-9 dB.
A report's means are exact sums rounded once on both sides: rtol 1e-10, the metric tests' bound."""
import numpy as np
import pytest
import torch

import blind_oracle as O

pytestmark = pytest.mark.gpu

LDS_L = 20000                                    # RDN_BLIND_LDS_L (asserted below)
BINS = (15.0, 40.0, 5)


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared cases are read-only


def _median3(x):
    p = np.pad(x, ((0, 0), (1, 1)), mode="reflect")
    return np.median(np.stack([p[:, :-2], p[:, 1:-1], p[:, 2:]]), axis=0).astype(np.float32)


def _smooth3(x):
    p = np.pad(x.astype(np.float64), ((0, 0), (1, 1)), mode="reflect")
    return ((p[:, :-2] + p[:, 1:-1] + p[:, 2:]) / 3.0).astype(np.float32)


def _spectra(n, L, seed, snr_db=None):
    """Noisy piecewise-constant spectra x in about [0, 1] (the simulator's shape, 25 dB unless ``snr_db`` says
    otherwise per spectrum) and a denoised y: the 3-point median of x for even rows, the 3-point mean for odd."""
    rng = np.random.default_rng(seed)
    c = np.repeat(rng.uniform(0.05, 1, (n, L // 7 + 1)), 7, axis=1)[:, :L]
    snr_db = np.full(n, 25.0) if snr_db is None else np.asarray(snr_db, dtype=np.float64)
    std = np.sqrt(np.mean(c ** 2, axis=1) / 10 ** (snr_db / 10))
    x = (c + rng.normal(0, 1, c.shape) * std[:, None]).astype(np.float32)
    y = _median3(x)
    y[1::2] = _smooth3(x)[1::2]
    return x, y


_CASES = {}


def _case(L, K, n):
    """x, y, sigma and the oracle's (per, rho) for a shape, computed once and shared (left unchanged)."""
    key = (L, K, n)
    if key not in _CASES:
        x, y = _spectra(n, L, 7919 * L + 31 * K + n)
        sigma = O.noise_sigma(x) if L > 2 else np.full(n, 0.03)
        per, rho = O.blind_values(x, y, sigma, K)
        for a in (x, y, sigma, per, rho):
            a.setflags(write=False)
        _CASES[key] = (x, y, sigma, per, rho)
    return _CASES[key]


def _n_for(L, K):
    """n in {1, 3, 70}: many spectra where they are short or the lags few (the oracle's cost is n (K + 1) L)."""
    if L <= 65 or K == 1:
        return 70
    return 3 if L <= 2345 or K == 2 else 1


def _lengths(K):
    return sorted({K + 1, K + 2, 63, 64, 65, 511, 512, 513, 1000, 2345, LDS_L - 1, LDS_L, LDS_L + 1,
                   (LDS_L // 512 + 1) * 512})


def _assert_close(per, rho, ref_per, ref_rho, scale=1.0):
    """The module docstring's bounds; ``scale`` widens those of the centred quantities (the biased case)."""
    rms = ref_per[:, 1]
    np.testing.assert_allclose(per[:, 1:3], ref_per[:, 1:3], rtol=1e-9, atol=0)
    assert np.all(np.abs(per[:, 0] - ref_per[:, 0]) <= 1e-9 * rms)
    np.testing.assert_allclose(rho, ref_rho, rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(per[:, 3:5], ref_per[:, 3:5], rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(per[:, 5], ref_per[:, 5], rtol=1e-8 * scale, atol=0)
    np.testing.assert_allclose(per[:, 6], ref_per[:, 6], rtol=0, atol=1e-9)


@pytest.mark.parametrize("K", [1, 2, 16, 32])
@pytest.mark.parametrize("pos", range(14))
def test_values_match_oracle(pos, K):
    """Every length at which the kernel takes another path -- L = K + 1 (one lag product per lag at most), the
    512-thread partition's edges, both sides of the LDS staging limit -- for 1, 2, 16 and 32 lags (each of the
    kernel's three window sizes, and K below the window's size) and n = 1, 3 and 70 workgroups."""
    from raman_mi355x import _lib, engine
    assert _lib.BLIND_LDS_L == LDS_L
    L = _lengths(K)[pos]
    n = _n_for(L, K)
    x, y, sigma, ref_per, ref_rho = _case(L, K, n)
    assert np.all(np.isfinite(ref_per)) and np.all(np.isfinite(ref_rho)) and np.all(sigma > 0)
    # the premises of the module docstring's bounds, on the oracle
    D_over_L = ref_per[:, 1] ** 2 - ref_per[:, 0] ** 2                    # the centred variance
    assert np.all(ref_per[:, 0] ** 2 <= D_over_L)                         # |Mean| <= the centred deviation
    delta = 3 * L * 2.0 ** -53
    S, s2 = np.mean(x.astype(np.float64) ** 2, axis=1), sigma ** 2
    assert np.all(2 * delta * np.sqrt(K) / np.sqrt((ref_rho ** 2).sum(axis=1)) < 1e-9)        # Q: a tenth of rtol
    assert np.all(delta * S / np.abs(S - s2) * 10 / np.log(10) < 1e-10)                       # SNR_est: of atol
    per, rho, rep = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, rho=True)
    assert rep is None and per.shape == (n, 7) and rho.shape == (n, K) and per.dtype == rho.dtype == torch.float64
    per, rho = per.cpu().numpy(), rho.cpu().numpy()
    _assert_close(per, rho, ref_per, ref_rho)
    assert np.array_equal(per[:, 3], rho[:, 0])                           # Rho1 is rho_1


def test_a_biased_residual_keeps_the_bounds_scaled_by_its_conditioning():
    """y carries an offset of 100 centred deviations, so r_i = m + d_i with |m| = 100 s.  The centred values are
    then formed from numbers 100 times their size: d_i = r_i - Mean is rounded to 2^-53 |r_i|, not 2^-53 |d_i|,
    and Mean itself is off by up to L 2^-53 RMS.  With e_i the error of d_i, |e|_2 <= sqrt(L) (L 2^-53 RMS) and
    a lag sum moves by |sum (d_i e_{i+k} + e_i d_{i+k})| <= 2 |d|_2 |e|_2 = 2 L 2^-53 sqrt(D) sqrt(L RMS^2)
    = 2 L 2^-53 D sqrt(kappa), kappa = RMS^2 L / D = 1 + (m / s)^2 >= 1: the unbiased bound L 2^-53 D times at most
    2 sqrt(kappa) <= kappa (kappa >= 4).  rho_k, Rho1, RhoMax and Q are therefore compared with their bounds times
    kappa (about 10^4 here); Mean, RMS, Ratio and SNR_est do not involve the centring and keep theirs."""
    from raman_mi355x import engine
    n, L, K = 3, 3000, 16
    x, y = _spectra(n, L, 99)
    r = x.astype(np.float64) - y.astype(np.float64)
    y = (y.astype(np.float64) - 100.0 * r.std(axis=1, keepdims=True)).astype(np.float32)
    sigma = O.noise_sigma(x)
    ref_per, ref_rho = O.blind_values(x, y, sigma, K)
    D_over_L = ref_per[:, 1] ** 2 - ref_per[:, 0] ** 2
    bias = np.abs(ref_per[:, 0]) / np.sqrt(D_over_L)
    kappa = ref_per[:, 1] ** 2 / D_over_L
    assert np.all((bias > 95) & (bias < 105)) and np.all(kappa > 9000)
    per, rho, _ = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, rho=True)
    per, rho = per.cpu().numpy(), rho.cpu().numpy()
    print("biased case: max |rho error|", np.abs(rho - ref_rho).max(), "kappa", kappa.min())
    _assert_close(per, rho, ref_per, ref_rho, scale=float(kappa.min()))


@pytest.mark.parametrize("L", [1000, LDS_L, LDS_L + 1])
def test_a_spectrum_has_the_same_bits_wherever_it_runs(L):
    """The same spectrum at row 0 of n = 1 and at row 41 of n = 70, staged in LDS (L <= RDN_BLIND_LDS_L) and
    recomputed through L2 (beyond it), and in two runs: bitwise the same seven values and rho row."""
    from raman_mi355x import engine
    K = 16
    x, y = _spectra(70, L, 5 + L)
    sigma = O.noise_sigma(x)
    one = engine.blind(_cuda(x[41:42]), _cuda(y[41:42]), sigma=_cuda(sigma[41:42]), lags=K, rho=True)
    runs = [engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, rho=True) for _ in range(2)]
    for a, b in zip(runs[0][:2], runs[1][:2]):
        assert np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))
    for whole, alone in zip(runs[0][:2], one[:2]):
        assert np.array_equal(whole[41].cpu().numpy().view(np.int64), alone[0].cpu().numpy().view(np.int64))
    # and with the report on, with other lags computed by the same window (K = 9 runs the 16-lag kernel too)
    per_r, rho_r, _ = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, rho=True, bins=BINS)
    assert np.array_equal(per_r.cpu().numpy().view(np.int64), runs[0][0].cpu().numpy().view(np.int64))
    rho9 = engine.blind(_cuda(x[:3]), _cuda(y[:3]), sigma=_cuda(sigma[:3]), lags=9, rho=True)[1].cpu().numpy()
    assert np.array_equal(rho9.view(np.int64), runs[0][1][:3, :9].cpu().numpy().view(np.int64))


@pytest.fixture(scope="module")
def report_set():
    """70 spectra of 300 samples between 12 and 43 dB, the oracle's values for 16 lags and a critical value that
    lies between the two middle Q, more than 1e-6 relative from every Q."""
    n, L, K = 70, 300, 16
    x, y = _spectra(n, L, 4242, snr_db=np.random.default_rng(1).uniform(12, 43, n))
    sigma = O.noise_sigma(x)
    per, _ = O.blind_values(x, y, sigma, K)
    q = np.sort(per[:, 5])
    q_crit = 0.5 * (q[n // 2 - 1] + q[n // 2])
    assert np.all(np.abs(per[:, 5] - q_crit) > 1e-6 * q_crit)
    flags = O.flagged(per, q_crit)
    assert flags.sum() == n // 2
    return x, y, sigma, K, per, q_crit, flags


def test_report_words_are_the_exact_accumulation_of_the_per_spectrum_values(report_set):
    """The report's words equal (np.array_equal) the host restatement of the accumulator applied to the device's
    own per-spectrum values, in the oracle's rows, with the oracle's flags; two half batches accumulate to the
    whole batch's words; key=None bins by (float)SNR_est."""
    from raman_mi355x import _lib, engine
    x, y, sigma, K, ref, q_crit, flags = report_set
    n, nbins = len(x), BINS[2]
    key = np.random.default_rng(2).uniform(10, 45, n).astype(np.float32)      # under- and overflow rows too
    key[5] = np.nan
    args = dict(lags=K, q_crit=q_crit, bins=BINS)
    per, _, rep = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), key=_cuda(key), **args)
    per, words = per.cpu().numpy(), rep.cpu().numpy()
    np.testing.assert_allclose(per[:, 5], ref[:, 5], rtol=1e-8)
    rows = O.bin_rows(key, BINS[0], BINS[1], nbins)
    assert set(rows) == set(range(nbins + 2)) and rows[5] == nbins + 1
    assert words.shape == (_lib.blind_words(nbins),)
    assert np.array_equal(words, O.report_words(per, rows, nbins, flags))
    v = engine.blind_value(rep, nbins).numpy()
    assert v[nbins + 2, 0] == n and v[nbins + 2, 8] == flags.sum()
    np.testing.assert_allclose(v[nbins + 2, 1:8] / n, ref.mean(axis=0), rtol=1e-8, atol=1e-12)
    # two halves into one report
    half = engine.new_blind_report(nbins, "cuda")
    for s in (slice(0, 33), slice(33, n)):
        out = engine.blind(_cuda(x[s]), _cuda(y[s]), sigma=_cuda(sigma[s]), key=_cuda(key[s]), report=half,
                           per_spectrum=False, **args)
        assert out[0] is None and out[1] is None and out[2] is half
    assert np.array_equal(half.cpu().numpy(), words)
    # no key: the spectrum's own SNR_est, rounded to fp32, by the SNR report's bin formula
    per2, _, rep2 = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), **args)
    assert np.array_equal(per2.cpu().numpy().view(np.int64), per.view(np.int64))
    rows2 = O.bin_rows(per[:, 6].astype(np.float32), BINS[0], BINS[1], nbins)
    assert len(set(rows2)) >= 4
    assert np.array_equal(rep2.cpu().numpy(), O.report_words(per, rows2, nbins, flags))
    # q_crit = +inf flags nothing, 0 everything
    for q, want in ((float("inf"), 0), (0.0, n)):
        r = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, q_crit=q, bins=BINS, per_spectrum=False)[2]
        assert engine.blind_value(r, nbins)[nbins + 2, 8] == want


def test_special_values_give_the_ieee_results_and_are_counted():
    """y = x (D = 0), a NaN sample, an infinite sample, sigma = 0, NaN and negative: the oracle's NaN / inf
    pattern, each non-finite value in its quantity's out-of-range word, every spectrum in the count."""
    from raman_mi355x import _lib, engine
    n, L, K = 8, 700, 16
    x, y = _spectra(n, L, 17)
    x, y = x.copy(), y.copy()
    sigma = O.noise_sigma(x).copy()
    y[1] = x[1]
    y[2, 300] = np.nan
    x[3, 699] = np.inf
    sigma[4], sigma[5], sigma[6] = 0.0, np.nan, -sigma[6]
    x[7, 0] = -np.inf
    y[7, 0] = -np.inf                                                    # inf - inf: a NaN residual sample
    ref, ref_rho = O.blind_values(x, y, sigma, K)
    assert ref[1, 0] == ref[1, 1] == 0 and np.isnan(ref[1, 3:6]).all() and np.isfinite(ref[1, 6])
    assert np.isnan(ref[2, :6]).all() and np.isfinite(ref[2, 6])
    assert ref[3, 0] == ref[3, 1] == ref[3, 2] == ref[3, 6] == np.inf and np.isnan(ref[3, 3:6]).all()
    assert ref[4, 2] == ref[4, 6] == np.inf and np.isnan(ref[5, [2, 6]]).all() and ref[6, 2] < 0
    assert np.isfinite(ref[[0, 4, 5, 6]][:, [0, 1, 3, 4, 5]]).all() and np.isfinite(ref[6]).all()
    per, rho, rep = engine.blind(_cuda(x), _cuda(y), sigma=_cuda(sigma), lags=K, rho=True, bins=(0.0, 1.0, 1),
                                 key=_cuda(np.full(n, 0.5, dtype=np.float32)))
    per, rho, words = per.cpu().numpy(), rho.cpu().numpy(), rep.cpu().numpy()
    for got, want in ((per, ref), (rho, ref_rho)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)]))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(per[fin], ref[fin], rtol=1e-8, atol=1e-9)
    row = words[_lib.BLIND_ROW_WORDS:2 * _lib.BLIND_ROW_WORDS]
    assert row[_lib.BLIND_COUNT] == n
    oor = [int(row[q * _lib.ACC_STRIDE + _lib.ACC_LIMBS]) for q in range(7)]
    assert oor == (~fin).sum(axis=0).tolist() and sum(oor) > 10
    assert np.array_equal(words, O.report_words(per, np.ones(n, dtype=np.int64), 1, O.flagged(ref, O.q_crit(K))))
    assert np.isnan(engine.blind_value(rep, 1).numpy()[3, 1:8]).all()
    # a NaN SNR_est is a NaN key: the overflow row
    rep = engine.blind(_cuda(x[5:6]), _cuda(y[5:6]), sigma=_cuda(sigma[5:6]), lags=K, bins=BINS, per_spectrum=False)[2]
    assert int(rep.cpu()[(BINS[2] + 1) * _lib.BLIND_ROW_WORDS + _lib.BLIND_COUNT]) == 1


def test_python_surface_checks_and_defaults():
    from raman_mi355x import engine
    x, y = (_cuda(a) for a in _spectra(4, 200, 3))
    per = engine.blind(x, y)[0].cpu().numpy()                            # sigma=None: the project's blind estimate
    sig = engine.noise_mad(x) * (np.sqrt(2.0) / 0.6744897501960817)
    again = engine.blind(x.unsqueeze(1), y.unsqueeze(1), sigma=sig, q_crit=engine.blind_q_crit(16))[0].cpu().numpy()
    assert np.array_equal(per.view(np.int64), again.view(np.int64))
    flat = engine.blind(x, y, sigma=0.03)[0].cpu().numpy()
    assert np.array_equal(flat[:, :2], per[:, :2]) and not np.array_equal(flat[:, 2], per[:, 2])
    e = engine.blind(x[:0], y[:0], rho=True, bins=BINS)
    assert e[0].shape == (0, 7) and e[1].shape == (0, 16) and int(e[2].sum()) == 0
    for kw, exc in ((dict(lags=0), ValueError), (dict(lags=33), ValueError), (dict(lags=200), ValueError),
                    (dict(q_crit=-1.0), ValueError), (dict(q_crit=float("nan")), ValueError),
                    (dict(key=torch.zeros(4, device="cuda")), ValueError), (dict(per_spectrum=False), ValueError),
                    (dict(sigma=torch.ones(4, device="cuda")), TypeError), (dict(sigma=True), TypeError),
                    (dict(bins=BINS, report=torch.zeros(7, dtype=torch.int64, device="cuda")), ValueError)):
        with pytest.raises(exc):
            engine.blind(x, y, **kw)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.blind(x, y[:, :100])
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.blind(x.cpu(), y)


@pytest.fixture(scope="module")
def simulator_set():
    from raman_mi355x import engine
    _, noisy, _, _ = engine.generate(64, 20250410, signal_length=1500)
    return noisy


@pytest.mark.parametrize("which", ["MovingAverage9", "PottsFit"])
def test_evaluate_blind_is_exact_over_batches_and_agrees_with_the_oracle(which, simulator_set, tmp_path):
    """64 x 1500 simulator spectra through evaluate_blind in one batch of 64 and in batches of 17: the same bits;
    the means are the oracle's (on the module's own output, with the numpy restatement of the noise estimate)."""
    import raman_mi355x as R
    from raman_mi355x.evaluate import write_blind_report
    model = R.MovingAverage(9).cuda() if which == "MovingAverage9" else R.PottsFit()     # .cuda() moves the taps
    noisy = simulator_set
    a = R.evaluate_blind(model, noisy, batch_size=64, bins=BINS)
    b = R.evaluate_blind(model, noisy.cpu().numpy(), batch_size=17, bins=BINS)
    assert a == b
    flat = R.evaluate_blind(model, noisy, batch_size=17)
    assert "by_snr" not in flat and {k: a[k] for k in flat} == flat
    y = model(noisy.view(64, 1, 1500)).view(64, 1500).cpu().numpy()
    x = noisy.cpu().numpy()
    ref, _ = O.blind_values(x, y, O.noise_sigma(x), 16)
    assert a["lags"] == 16 and a["alpha"] == 0.01 and a["q_crit"] == R.blind_q_crit(16) and a["count"] == 64
    assert np.all(np.abs(ref[:, 5] - a["q_crit"]) > 1e-6 * a["q_crit"]) and np.isfinite(ref).all()
    for i, k in enumerate(O.QUANTITIES):
        assert a[k] == pytest.approx(ref[:, i].mean(), rel=1e-10), k
    assert a["flagged_fraction"] == O.flagged(ref, a["q_crit"]).mean()
    assert sum(e["count"] for e in a["by_snr"]) + a["under"]["count"] + a["over"]["count"] == 64
    print(f"{which}: Ratio {a['Ratio']:.3f}, Q {a['Q']:.1f}, flagged {a['flagged_fraction']:.3f}, SNR_est {a['SNR_est']:.2f} dB")
    if which == "MovingAverage9":
        assert a["flagged_fraction"] == 1.0 and a["Ratio"] > 1.5          # it removes signal: every spectrum says so
    # a given sigma: one value for all, or one per spectrum
    s = R.evaluate_blind(model, noisy, batch_size=17, sigma=0.02)
    assert s["RMS"] == a["RMS"] and s["Ratio"] == pytest.approx(np.mean(ref[:, 1] / 0.02), rel=1e-10)
    s = R.evaluate_blind(model, noisy, batch_size=17, sigma=O.noise_sigma(x), lags=16)
    assert s == flat
    root = write_blind_report(a, str(tmp_path / "blind"))
    lines = open(root + "/blind_report.txt").read().splitlines()
    assert len(lines) == 4 + 8 + 1 + BINS[2] + 2 and lines[0] == "lags: 16"


def test_evaluators_with_blind_keep_every_other_result():
    """evaluate_synthetic(..., blind=True) and evaluate(..., blind=...): the means, the accumulator and the SNR
    report's words are the same bits as without it, one key is added, binned like the SNR report."""
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate_synthetic, write_metrics
    models = {"median3": R.MedianFilter(3), "ma9": R.MovingAverage(9).cuda()}
    kw = dict(total=96, signal_length=1500, batch_size=40, snr_bins=(20.0, 37.0, 4))
    plain = evaluate_synthetic(models, **kw)
    blind = evaluate_synthetic(models, blind=True, **kw)
    other = evaluate_synthetic(models, blind={"lags": 8, "alpha": 0.05}, **dict(kw, batch_size=96))
    clean, noisy, snr_db, _ = engine.generate(96, 20250410, signal_length=1500)
    for name, m in models.items():
        assert set(blind[name]) == set(plain[name]) | {"blind"}
        for k in ("means", "acc", "report", "by_snr", "SNR_gain"):
            assert blind[name][k] == plain[name][k] == other[name][k], (name, k)
        e = blind[name]["blind"]
        assert e["count"] == 96 and [b["count"] for b in e["by_snr"]] == [b["count"] for b in plain[name]["by_snr"]]
        assert other[name]["blind"]["lags"] == 8 and other[name]["blind"]["q_crit"] == R.blind_q_crit(8, 0.05)
        rep = engine.blind(noisy, m(noisy.view(96, 1, 1500)), key=snr_db, bins=kw["snr_bins"], per_spectrum=False)[2]
        assert rep.cpu().tolist() == e["report"]
    assert blind["ma9"]["blind"]["flagged_fraction"] > blind["median3"]["blind"]["flagged_fraction"] - 1e-9
    # evaluate(): with and without nominal SNRs, with physics beside it
    m = models["ma9"]
    base = R.evaluate(m, noisy.cpu().numpy(), clean.cpu().numpy(), batch_size=50, snr_bins=(20.0, 37.0, 4))
    for extra in (dict(), dict(snrs=snr_db.cpu().numpy()), dict(physics=True)):
        ref = R.evaluate(m, noisy.cpu().numpy(), clean.cpu().numpy(), batch_size=50, snr_bins=(20.0, 37.0, 4), **extra)
        got = R.evaluate(m, noisy.cpu().numpy(), clean.cpu().numpy(), batch_size=50, snr_bins=(20.0, 37.0, 4), blind=True,
                         **extra)
        assert set(got) == set(ref) | {"blind"} and all(got[k] == ref[k] for k in ref)
        assert [b["count"] for b in got["blind"]["by_snr"]] == [b["count"] for b in got["by_snr"]]
    assert all(base[k] == ref[k] for k in base)
    unbinned = R.evaluate(m, noisy.cpu().numpy(), clean.cpu().numpy(), batch_size=50, blind=True)
    assert set(unbinned) == {"MSE", "SSIM", "Smoothness", "Peak2Peak", "blind"} and "by_snr" not in unbinned["blind"]
    assert unbinned["blind"]["count"] == 96 and unbinned["blind"]["Q"] == blind["ma9"]["blind"]["Q"]
    assert R.evaluate(m, noisy.cpu().numpy(), clean.cpu().numpy(), blind=None).keys() == {"MSE", "SSIM", "Smoothness", "Peak2Peak"}
