"""The Bayesian change-point smoother on the device (rdn_bayes_steps, engine.bayes_steps, bayes.BayesSteps) against
the numpy oracle (tests/bayes_oracle.py): the oracle's fp64 result rounded to fp32.

Bars.  The kernel runs the oracle's recursion in fp64 with its own exp and log and its own order of each sum, so
both sides round nearly the same fp64 number to fp32: y and jump within one fp32 ulp of max(1, |value|),
2^-23 * max(1, |v|), and -- a condition of its own -- at most 1e-3 of the elements compared in a test may differ at
all (the two fp64 numbers differ by ~1e-12 at most, the oracle's own disagreement under reversal, against an fp32
spacing of 6e-8: a rounding falls between them for about one element in 1e4; an implementation that is merely close
everywhere fails this).  logZ within 1e-12 relative: 1000 times the oracle's own forward / backward disagreement
(1e-15), the margin for the device's exp and log and the summation order."""
import math

import numpy as np
import pytest
import torch

import bayes_oracle as B
import haar_oracle as H
import potts_oracle as P

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
MAX_SHARE = 1e-3
LOGZ_RTOL = 1e-12


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


class Tally:
    """What a test compared: elements, those that differ at all, the worst differences."""

    def __init__(self):
        self.elements = self.differ = 0
        self.worst = {"y": 0.0, "jump": 0.0, "logZ": 0.0}

    def values(self, got, ref, what, tag):
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        assert got.shape == ref.shape and got.dtype == np.float32, tag
        nan = np.isnan(ref)
        assert np.array_equal(got.view(np.uint32)[nan], ref.view(np.uint32)[nan]), tag     # 0x7fc00000 where refused
        g, r = got[~nan].astype(np.float64), ref[~nan].astype(np.float64)
        err = np.abs(g - r) / np.maximum(1.0, np.abs(r))
        self.elements += g.size
        self.differ += int((g != r).sum())
        if g.size:
            self.worst[what] = max(self.worst[what], float(err.max()))
            assert err.max() <= ULP, (tag, what, float(err.max()))

    def logz(self, got, ref, tag):
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        assert got.dtype == np.float64 and got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), tag
        ok = ~np.isnan(ref)
        if ok.any():
            rel = np.abs(got[ok] / ref[ok] - 1.0).max()
            self.worst["logZ"] = max(self.worst["logZ"], float(rel))
            assert rel <= LOGZ_RTOL, (tag, float(rel))

    def close(self, name):
        share = self.differ / max(self.elements, 1)
        print(f"{name}: {self.differ} of {self.elements} elements differ ({share:.2g}); worst |y| {self.worst['y'] / ULP:.3g} ulp, "
              f"|jump| {self.worst['jump'] / ULP:.3g} ulp, logZ {self.worst['logZ']:.3g} relative")
        assert share <= MAX_SHARE, (self.differ, self.elements)


def _assert_matches_oracle(x, sigma, K, W, tag, tally):
    from raman_mi355x import engine
    sd = _cuda(np.asarray(sigma, dtype=np.float64)) if np.ndim(sigma) else float(sigma)
    y, jump, logz = engine.bayes_steps(_cuda(x), sd, K, W)
    ref = B.bayes_steps(x, sigma, K, W)
    tally.values(y, ref[0], "y", tag)
    tally.values(jump, ref[1], "jump", tag)
    tally.logz(logz, ref[2], tag)
    ok = ~np.isnan(ref[2])
    assert np.all(jump.cpu().numpy()[ok, 0] == 1.0), tag
    return ref


def B_sigma(x):
    return P.noise_mad(x) * (math.sqrt(2.0) / P.MAD_TO_SIGMA)


LENGTHS = (1, 2, 63, 64, 65, 128, 129, 257)


@pytest.mark.parametrize("K", [1, 2, 40, 63, 64])
def test_smallest_shapes_match_oracle(K):
    """n = 3 around one and two 64-sample chunks and at four chunks and a sample; step spectra and pure noise; a
    different sigma per row, and a scrambled sigma shows; two level ranges."""
    rng = np.random.default_rng(K)
    tally, shown = Tally(), False
    for L in LENGTHS:
        for W in (1.0, 2.5):
            s = rng.uniform(0.02, 0.08, 3)
            x = H.noisy_steps(3, L, 2000 * K + L, sigma=0.05)
            ref = _assert_matches_oracle(x, s, K, W, ("steps", K, L, W), tally)
            s2 = s * np.array([1.0, 3.0, 0.3])
            ref2 = _assert_matches_oracle(x, s2, K, W, ("scaled", K, L, W), tally)
            shown |= not np.array_equal(ref[2][1:], ref2[2][1:]) and np.array_equal(ref[0][0], ref2[0][0])
            noise = (0.5 + rng.normal(0, 0.05, (3, L))).astype(np.float32)
            _assert_matches_oracle(noise, s, K, W, ("noise", K, L, W), tally)
    assert shown
    tally.close(f"smallest shapes, K = {K}")


def test_long_rows():
    rng = np.random.default_rng(5)
    x = np.concatenate([H.noisy_steps(1, 10000, 5), (0.3 + rng.normal(0, 0.03, (1, 10000))).astype(np.float32)])
    tally = Tally()
    _, jump, _ = _assert_matches_oracle(x, B_sigma(x), 40, 1.0, "10000", tally)
    steps, flat = jump[:, 1:].astype(np.float64).sum(axis=1)          # expected run starts: ~10000 / 20.5 in the steps
    assert 300 < steps < 700 and flat < steps                          # row; fewer, each of small probability, in the flat
    tally.close("two rows of 10000")


def test_rows_past_2_to_the_31_samples():
    """n * L just above 2^31: the last rows' offsets into x, y (elements) and work (doubles) do not fit 32 bits; jump
    NULL bounds the memory.  The bulk is uniform noise; the first two and the last three rows are spectra held to
    the oracle."""
    from raman_mi355x import _lib, engine
    L = 4099                                                            # 64 chunks and three samples
    n = 2 ** 31 // L + 5
    assert (n - 3) * L > 2 ** 31
    x = torch.rand((n, L), device="cuda")
    rows = H.noisy_steps(5, L, 41)
    x[:2] = _cuda(rows[:2])
    x[-3:] = _cuda(rows[2:])
    sigma = torch.full((n,), 0.03, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    logz = torch.empty(n, dtype=torch.float64, device="cuda")
    work = torch.empty(n * (L + 1), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().rdn_bayes_steps(x.data_ptr(), y.data_ptr(), None, logz.data_ptr(), sigma.data_ptr(), n, L, 40,
                                          1.0, work.data_ptr(), work.numel() * 8, None), "rdn_bayes_steps")
    torch.cuda.synchronize()
    ref = B.bayes_steps(rows, 0.03, 40, 1.0)
    tally = Tally()
    tally.values(torch.cat([y[:2], y[-3:]]), ref[0], "y", "2^31")
    tally.logz(torch.cat([logz[:2], logz[-3:]]), ref[2], "2^31")
    assert bool(torch.isfinite(logz).all())
    tally.close("rows past 2^31")


def test_rows_do_not_depend_on_the_batch():
    """The bits of a spectrum's y, jump and logZ for n = 1, 4, 5 and 9 and at any row position."""
    from raman_mi355x import engine
    rng = np.random.default_rng(3)
    x = np.concatenate([H.noisy_steps(5, 193, 77), (0.5 + rng.normal(0, 0.05, (4, 193))).astype(np.float32)])
    dx, s = _cuda(x), _cuda(B_sigma(x))
    y, jump, logz = engine.bayes_steps(dx, s)
    for r in range(9):
        for lo, hi in ((r, r + 1), (max(r - 3, 0), max(r - 3, 0) + 4), (min(r, 4), min(r, 4) + 5)):
            yr, jr, zr = engine.bayes_steps(dx[lo:hi].clone(), s[lo:hi].clone())
            i = r - lo
            assert torch.equal(yr[i].view(torch.int32), y[r].view(torch.int32)), (r, lo, hi)
            assert torch.equal(jr[i].view(torch.int32), jump[r].view(torch.int32)), (r, lo, hi)
            assert torch.equal(zr[i].view(torch.int64), logz[r].view(torch.int64)), (r, lo, hi)
    perm = torch.tensor([8, 3, 0, 7, 1, 6, 2, 5, 4], device="cuda")
    yp, jp, zp = engine.bayes_steps(dx[perm].contiguous(), s[perm].contiguous())
    assert torch.equal(yp.view(torch.int32), y[perm].view(torch.int32)) and torch.equal(jp.view(torch.int32), jump[perm].view(torch.int32))
    assert torch.equal(zp.view(torch.int64), logz[perm].view(torch.int64))


def test_special_values():
    """A NaN, +inf and -inf row and rows with sigma in {0, -1, NaN, inf}: all 0x7fc00000 with logZ NaN, the other rows
    of the same call correct; subnormal and signed-zero rows equal the oracle; jump[:, 0] == 1 exactly."""
    from raman_mi355x import engine
    L = 300
    x = H.noisy_steps(11, L, 5)
    x[0, 100], x[1, L - 1], x[2, 0] = np.nan, np.inf, -np.inf
    s = np.full(11, 0.03)
    s[3], s[4], s[5], s[6] = 0.0, -1.0, np.nan, np.inf
    x[7, 19:25] = [0.5, -0.0, 0.0, -0.0, -0.0, 0.5]
    x[7, 200:210] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 1e-38, 0.0, -0.0, 1e-40, -2e-40], dtype=np.float32)
    x[8] = np.array([1e-41, -1e-41, 1e-45, -1e-45, 3e-39, 0.0, -0.0, 1e-40] * (L // 8 + 1), dtype=np.float32)[:L]
    x[9] = np.array([0.0, -0.0, -0.0, 0.0, 0.0] * (L // 5), dtype=np.float32)
    tally = Tally()
    for K in (5, 40, 64):
        y, jump, logz = _assert_matches_oracle(x, s, K, 1.0, K, tally)
        assert np.all(y.view(np.uint32)[:7] == 0x7FC00000) and np.all(jump.view(np.uint32)[:7] == 0x7FC00000)
        assert np.isnan(logz[:7]).all() and np.isfinite(y[7:]).all() and np.isfinite(logz[7:]).all()
    y, jump, logz = engine.bayes_steps(_cuda(x), _cuda(s))
    assert np.all(_bits(y)[:7] == 0x7FC00000) and np.all(_bits(jump)[:7] == 0x7FC00000) and bool(torch.isnan(logz[:7]).all())
    assert bool(torch.isfinite(y[7:]).all()) and bool((jump[7:, 0] == 1.0).all())
    tally.close("special values")


def test_empty_batch_out_reuse_and_refusals():
    from raman_mi355x import engine
    for shape in ((0, 100), (0, 1, 100)):
        y, jump, logz = engine.bayes_steps(torch.empty(shape, device="cuda"), 0.03)
        assert y.shape == shape and jump.shape == shape and logz.shape == (0,) and logz.dtype == torch.float64
    x = _cuda(H.noisy_steps(4, 300, 9))
    s = _cuda(B_sigma(x.cpu().numpy()))
    ref = engine.bayes_steps(x, s)
    out, jump = torch.full_like(x, -1.0), torch.full_like(x, -1.0)
    logz = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(4 * 301 + 17, dtype=torch.float64, device="cuda")
    for _ in range(2):                                                  # a second call on the used scratch
        got = engine.bayes_steps(x, s, out=out, jump=jump, logz=logz, work=work)
        assert got[0] is out and got[1] is jump and got[2] is logz
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert torch.equal(engine.bayes_steps(x, float(s[0]))[0][0], ref[0][0])    # a float is broadcast
    assert not torch.equal(engine.bayes_steps(x, s, 5)[0], ref[0])
    assert not torch.equal(engine.bayes_steps(x, s, level_range=2.5)[0], ref[0])
    x3 = x.view(4, 1, 300)
    y3, j3, z3 = engine.bayes_steps(x3, s)
    assert y3.shape == j3.shape == (4, 1, 300) and torch.equal(y3.view(4, 300), ref[0]) and torch.equal(z3, ref[2])
    buf = torch.zeros(4 * 300 + 300, device="cuda")
    a, b = buf[:1200].view(4, 300), buf[300:].view(4, 300)
    with pytest.raises(ValueError, match="overlap"):
        engine.bayes_steps(a, s, out=a)
    with pytest.raises(ValueError, match="overlap"):
        engine.bayes_steps(a, s, out=b)
    with pytest.raises(ValueError, match="jump must not overlap"):
        engine.bayes_steps(a, s, jump=b)
    with pytest.raises(ValueError, match="jump must not overlap out"):
        engine.bayes_steps(x, s, out=out, jump=out)
    for kw in (dict(out=torch.empty(4, 299, device="cuda")), dict(jump=torch.empty(4, 299, device="cuda")),
               dict(logz=torch.empty(3, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError, match="shape"):
            engine.bayes_steps(x, s, **kw)
    with pytest.raises(ValueError, match="shape"):
        engine.bayes_steps(x, s[:3])
    for kw in (dict(out=torch.empty(4, 300, device="cuda", dtype=torch.float64)),
               dict(jump=torch.empty(4, 300, device="cuda", dtype=torch.float64)),
               dict(logz=torch.empty(4, device="cuda")), dict(work=torch.empty(1204, device="cuda"))):
        with pytest.raises(TypeError):
            engine.bayes_steps(x, s, **kw)
    with pytest.raises(TypeError):
        engine.bayes_steps(x, s.float())
    with pytest.raises(ValueError, match=r"N \* \(L \+ 1\)"):
        engine.bayes_steps(x, s, work=torch.empty(1203, dtype=torch.float64, device="cuda"))
    big = torch.zeros(4 * 301 * 2, device="cuda")                      # 4 * 301 doubles, the input in front
    with pytest.raises(ValueError, match="work must not overlap the input"):
        engine.bayes_steps(big[:1200].view(4, 300), s, work=big.view(torch.float64))
    with pytest.raises(ValueError, match="work must not overlap out"):
        engine.bayes_steps(x, s, out=big[:1200].view(4, 300), work=big.view(torch.float64))
    with pytest.raises(ValueError, match="logz must not overlap"):
        engine.bayes_steps(x, s, work=work, logz=work[:4])
    with pytest.raises(ValueError, match="sigma must not overlap"):
        engine.bayes_steps(x, work[:4], work=work)
    wide = _cuda(H.noisy_steps(4, 600, 10))
    for bad in (wide[:, ::2], wide.t()):
        with pytest.raises(ValueError, match="contiguous"):
            engine.bayes_steps(bad, 0.03)
    with pytest.raises(TypeError):
        engine.bayes_steps(x.double(), s)
    with pytest.raises(ValueError):
        engine.bayes_steps(x.view(2, 2, 300), s[:2])
    for bad_k in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="max_len"):
            engine.bayes_steps(x, s, bad_k)
    for bad_w in (0.0, -1.0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="level_range"):
            engine.bayes_steps(x, s, level_range=bad_w)


def test_module_forward_is_the_engine_call_and_eager_under_grad():
    import raman_mi355x as R
    from raman_mi355x import engine
    L = 165
    x = _cuda(H.noisy_steps(3, L, 21)).unsqueeze(1)
    per_row = torch.tensor([0.02, 0.04, 0.08], dtype=torch.float64)
    for m in (R.BayesSteps(), R.BayesSteps(64, 2.5), R.BayesSteps(1), R.BayesSteps(sigma=0.05), R.BayesSteps(8, sigma=per_row)):
        assert m.uses_engine(x) and len(m.state_dict()) == 0
        y = m(x)
        sigma = (engine.noise_mad(x) * (math.sqrt(2.0) / P.MAD_TO_SIGMA) if m.sigma is None else
                 per_row.cuda() if torch.is_tensor(m.sigma) else torch.full((3,), m.sigma, dtype=torch.float64, device="cuda"))
        want, jump, logz = engine.bayes_steps(x, sigma, m.max_len, m.level_range)
        assert y.shape == x.shape and torch.equal(y.view(torch.int32), want.view(torch.int32))
        assert torch.equal(m.noise_std(x), sigma)
        assert torch.equal(m.jump_probability(x).view(torch.int32), jump.view(torch.int32))
        assert torch.equal(m.log_evidence(x).view(torch.int64), logz.view(torch.int64))
        xg = x.clone().requires_grad_()
        assert not m.uses_engine(xg)
        yg = m(xg)                                     # the eager path: the same recursion in torch ops, with a graph
        assert yg.requires_grad and yg.grad_fn is not None
        assert float((yg.detach().double() - y.double()).abs().max()) <= ULP * max(1.0, float(y.abs().max()))
        assert float((m.log_evidence(xg).detach() / logz - 1).abs().max()) <= 1e-10
        yg.sum().backward()
        assert xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
        with torch.no_grad():
            assert m.uses_engine(xg)
    with pytest.raises(ValueError, match=r"\(N, 1, L\)"):
        R.BayesSteps()(x.squeeze(1))
    const = torch.full((2, 1, 50), 0.25, device="cuda")               # the blind sigma is 0: refused, as documented
    assert bool(torch.isnan(R.BayesSteps()(const)).all()) and bool(torch.isfinite(R.BayesSteps(sigma=0.01)(const)).all())


def test_evaluate_synthetic_meters_the_module_like_a_network():
    """256 simulator spectra of 2000 samples: the module's accumulator and report words are those of
    engine.metrics / engine.snr on its separately computed output, and the same for two batch sizes."""
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate_synthetic
    bins = (20, 37, 17)
    models = {"BayesSteps": R.BayesSteps()}
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
    print(f"simulator spectra: BayesSteps {a['BayesSteps']['SNR_gain']:+.2f} dB")


def test_gain_and_calibration_on_reference_spectra():
    """The gain and calibration test of test_bayes_cpu.py on the device, with the same bars."""
    import raman_mi355x as R
    from oracle.refgen import generate_signals
    from test_bayes_cpu import check_gain_and_calibration
    np.random.seed(7)
    clean, noisy, _, _ = generate_signals(256, signal_length=2000, extreme_noise_prob=0)
    clean, noisy = clean.astype(np.float32), noisy.astype(np.float32)
    x = _cuda(noisy).unsqueeze(1)
    m = R.BayesSteps()
    y, jump = m(x).squeeze(1).cpu().numpy(), m.jump_probability(x).squeeze(1).cpu().numpy()
    check_gain_and_calibration(clean, noisy, y, jump, "device")
