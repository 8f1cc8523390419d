"""PhysicsAwareLoss on the device (rdn_physics / engine.physics, the PhysicsAwareLoss module's engine path,
evaluate(physics=...)) against the numpy oracle (tests/physics_oracle.py: float64 values, the mask in
clean's own type, exact sums) and the reference class's recorded values (tests/golden/physics.npz).

Tolerances.  PeakCount is an integer: exact.  Each of the five values is a sum of at most 16384
non-negative fp64 terms that differs from the oracle's only in the summation order and in fused
multiply-adds: relative error at most about L 2^-53 = 1.8e-12, so rtol 1e-11 leaves about 5x for the
partition.  A report's means are exact sums rounded once on both sides: rtol 1e-10, the
existing report bar.  Against the reference's own float32 run the bound is the triangle inequality with
the recorded distance d32 between its float32 and float64 runs: no margin is chosen."""
import math
import os

import numpy as np
import pytest
import torch

import physics_oracle as O
import snr_oracle as S
from conftest import GOLDEN, golden_state_dict

pytestmark = pytest.mark.gpu

W = O.WEIGHTS


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spectra(n, L, seed, seg=7, f64=False, dc=0.0):
    """Piecewise-constant clean spectra in [0, 1] (segments of ``seg`` samples: the simulator's shape; 1: every
    sample its own level), noisy x at about 25 dB (+ ``dc``) and a denoised y that keeps a third of the noise.
    ``f64``: clean in float64 with values that are not float32-representable."""
    rng = np.random.default_rng(seed)
    c = np.repeat(rng.uniform(0.05, 1, (n, L // seg + 1)), seg, axis=1)[:, :L].astype(np.float32)
    std = np.sqrt(np.mean(c.astype(np.float64) ** 2, axis=1) / 10 ** 2.5)
    noise = rng.normal(0, 1, c.shape) * std[:, None]
    x = (c + noise + dc).astype(np.float32)
    y = (c + noise / 3 + rng.normal(0, 1, c.shape) * std[:, None] / 10).astype(np.float32)
    if f64:
        c = c.astype(np.float64) + rng.uniform(0, 1e-9, c.shape)
        assert not np.array_equal(c, c.astype(np.float32))
    return x, y, c


def _check_values(got, ref):
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 5], ref[:, 5]), (got[:, 5], ref[:, 5])          # PeakCount: exact
    assert np.all(np.isfinite(ref))
    np.testing.assert_allclose(got[:, :5], ref[:, :5], rtol=1e-11, atol=0)


# the ends of the L - 1 and L - 2 sums (3, 4, 7), both sides of the 512-thread partition, its unrolled-by-4
# main loop with and without a remainder (1025, 16384)
@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("L", [3, 4, 7, 511, 512, 513, 1025, 16384])
def test_per_spectrum_values_match_oracle(L, n, f64):
    from raman_mi355x import engine
    x, y, c = _spectra(n, L, 1000 * L + n, f64=f64)
    per, rep = engine.physics(_cuda(x), _cuda(y), _cuda(c))
    assert rep is None and per.shape == (n, 6) and per.dtype == torch.float64
    ref = O.physics_values(x, y, c)
    if L >= 511:
        assert 0 < ref[:, 5].min() and ref[:, 5].max() < L - 2                   # the mask is neither empty nor full
    _check_values(per.cpu().numpy(), ref)


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("case", ["unit_segments", "dc_offset", "other_weights"])
def test_per_spectrum_values_special_cases(case, f64):
    """Unit-length segments (a mask that changes at every position), a DC offset of +1.0 on x (a one-pass
    variance would lose digits: the bar is the same), and other weights than the default."""
    from raman_mi355x import engine
    n, L = 3, 1025
    x, y, c = _spectra(n, L, 77, seg=1 if case == "unit_segments" else 7, f64=f64, dc=1.0 if case == "dc_offset" else 0.0)
    w = (0.3, 0.7, 2.0) if case == "other_weights" else W
    per, _ = engine.physics(_cuda(x), _cuda(y), _cuda(c), weights=w)
    ref = O.physics_values(x, y, c, weights=w)
    if case == "unit_segments":
        assert np.all(ref[:, 5] > L // 4)
    _check_values(per.cpu().numpy(), ref)
    # (N, 1, L) inputs are the same rows
    per3, _ = engine.physics(_cuda(x).unsqueeze(1), _cuda(y).unsqueeze(1), _cuda(c).unsqueeze(1), weights=w)
    assert torch.equal(per3, per)


def test_mask_is_formed_in_cleans_own_type():
    """A clean row whose float64 second difference has another sign than the float32 one: the mask follows
    the storage type (torch.diff(clean, n=2) < 0), so PeakCount differs between the two."""
    from raman_mi355x import engine
    L = 600
    rng = np.random.default_rng(3)
    c64 = np.repeat(rng.uniform(0.05, 1, (2, L // 7 + 1)), 7, axis=1)[:, :L] + rng.uniform(0, 1e-9, (2, L))
    c32 = c64.astype(np.float32)
    x = (c64 + rng.normal(0, 0.01, c64.shape)).astype(np.float32)
    y = (c64 + rng.normal(0, 0.003, c64.shape)).astype(np.float32)
    r32, r64 = O.physics_values(x, y, c32), O.physics_values(x, y, c64)
    assert np.all(r64[:, 5] > r32[:, 5] + 100)           # inside a segment float32 differences are 0, float64 ones not
    for c, ref in ((c32, r32), (c64, r64)):
        per, _ = engine.physics(_cuda(x), _cuda(y), _cuda(c))
        _check_values(per.cpu().numpy(), ref)


def _word(report, row, q, w):
    from raman_mi355x import _lib
    return int(report[row * _lib.PHYS_ROW_WORDS + q * _lib.ACC_STRIDE + w])


def test_degenerate_rows():
    """A NaN in y at an unmasked position: MSE, Smooth, Peak and Total are NaN (the mask multiplies, it does
    not select), Noise is finite; y == clean: MSE, Smooth and Peak exactly 0; a constant clean: PeakCount 0.
    The other spectra are unaffected; a report counts the non-finite values per quantity."""
    from raman_mi355x import engine, _lib
    n, L = 6, 700
    x, y, c = _spectra(n, L, 9)
    mask = O.peak_mask(c)
    i = 1 + int(np.flatnonzero(~mask[1])[5])             # an unmasked centre position of spectrum 1
    assert not mask[1, i - 1]
    y[1, i] = np.nan
    y[2] = c[2]
    c[3] = 0.5
    y[4, L - 1] = np.inf                                  # the row's last sample: in MSE and Smooth, not in Peak
    ref = O.physics_values(x, y, c)
    assert np.isnan(ref[1, [0, 1, 2, 4]]).all() and np.isfinite(ref[1, 3]) and ref[1, 5] == mask[1].sum()
    assert ref[3, 5] == 0 and ref[3, 2] == 0
    assert ref[4, 0] == np.inf and ref[4, 1] == np.inf and np.isfinite(ref[4, 2]) and ref[4, 4] == np.inf
    key = np.array([21, 22, 30, 31, 36, 36], dtype=np.float32)        # rows 1, 1, 2, 2, 2, 2 of two bins
    per, rep = engine.physics(_cuda(x), _cuda(y), _cuda(c), key=_cuda(key), bins=(20, 37, 2))
    got = per.cpu().numpy()
    assert np.array_equal(got[:, 5], ref[:, 5])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.all(got[2, :3] == 0) and got[3, 5] == 0 and got[3, 2] == 0
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-11, atol=0)           # rows 0, 5 and every finite value
    rep = rep.cpu().numpy()
    oor = [[_word(rep, r, q, _lib.ACC_LIMBS) for q in range(6)] for r in range(4)]
    assert oor == [[0] * 6, [1, 1, 1, 0, 1, 0], [1, 1, 0, 0, 1, 0], [0] * 6]
    v = engine.physics_value(torch.from_numpy(rep), 2).numpy()
    assert v[:, 0].tolist() == [0, 2, 4, 0, 6]
    assert np.isnan(v[1, [1, 2, 3, 5]]).all() and np.isnan(v[2, [1, 2, 5]]).all() and np.isnan(v[4, [1, 2, 3, 5]]).all()
    np.testing.assert_allclose(v[1, 4], ref[:2, 3].sum(), rtol=1e-10)            # the finite quantities of the rows
    np.testing.assert_allclose(v[2, 3], ref[2:, 2].sum(), rtol=1e-10)
    assert v[4, 6] == ref[:, 5].sum()


# ---- the report: 37 spectra, L = 300, four bins over (20, 37) ----------------------------------------
N, L_REP = 37, 300
BINS = (20.0, 37.0, 4)


def _keys():
    """Keys below, inside, on an edge, above and NaN, then every bin."""
    f = np.float32
    k = np.random.default_rng(5).uniform(17.0, 40.0, N).astype(np.float32)
    k[:10] = [20.0, 37.0, np.nextafter(f(37), f(0)), np.nextafter(f(20), f(0)), np.nan, np.inf, -np.inf, 24.25, 28.5, 32.75]
    return k


@pytest.fixture(scope="module")
def rep_case():
    x, y, c = _spectra(N, L_REP, 42)
    return dict(x=_cuda(x), y=_cuda(y), c=_cuda(c), per6=O.physics_values(x, y, c))


def test_report_rows_and_totals_match_oracle(rep_case):
    from raman_mi355x import engine
    k = _keys()
    rows = np.array([engine.report_bin(v, BINS) for v in k])
    assert np.array_equal(rows, S.bin_rows(k, *BINS)) and rows[:10].tolist() == [1, 5, 4, 0, 5, 5, 0, 2, 3, 4]
    assert set(rows.tolist()) == set(range(6))
    per, rep = engine.physics(rep_case["x"], rep_case["y"], rep_case["c"], key=_cuda(k), bins=BINS)
    _check_values(per.cpu().numpy(), rep_case["per6"])
    v = engine.physics_value(rep, BINS[2]).numpy()
    ref = O.report_sums(rep_case["per6"], rows, BINS[2])
    assert np.array_equal(v[:, 0], ref[:, 0]) and np.array_equal(v[:, 6], ref[:, 6]) and v[-1, 0] == N
    np.testing.assert_allclose(v[:, 1:6], ref[:, 1:6], rtol=1e-10, atol=0)
    # the words themselves: the oracle's limbs of the device's own per-spectrum values
    assert np.array_equal(rep.cpu().numpy(), O.report_words(per.cpu().numpy(), rows, BINS[2]))


def test_null_key_puts_everything_into_row_1(rep_case):
    from raman_mi355x import engine, _lib
    for bins in (BINS, (0.0, 1.0, 1)):
        per, rep = engine.physics(rep_case["x"], rep_case["y"], rep_case["c"], bins=bins)
        words = rep.cpu().numpy().reshape(bins[2] + 2, _lib.PHYS_ROW_WORDS)
        assert words[1, _lib.PHYS_COUNT] == N and not words[[0] + list(range(2, bins[2] + 2))].any()
        assert np.array_equal(words[1], O.report_words(per.cpu().numpy(), np.ones(N, dtype=np.int64), 1).reshape(3, -1)[1])
        v = engine.physics_value(rep, bins[2]).numpy()
        assert np.array_equal(v[1], v[-1])
        np.testing.assert_allclose(v[-1, 1:], O.report_sums(rep_case["per6"], np.ones(N, dtype=np.int64), 1)[-1, 1:], rtol=1e-10)
    no_per, rep = engine.physics(rep_case["x"], rep_case["y"], rep_case["c"], bins=BINS, per_spectrum=False)
    assert no_per is None and torch.equal(rep.cpu().reshape(6, -1)[1], torch.from_numpy(words[1]))


@pytest.mark.parametrize("keyed", [True, False])
def test_report_is_independent_of_the_batch_split(rep_case, keyed):
    from raman_mi355x import engine
    k = _cuda(_keys()) if keyed else None
    x, y, c = (rep_case[s] for s in ("x", "y", "c"))

    def run(lo, hi, report=None):
        return engine.physics(x[lo:hi], y[lo:hi], c[lo:hi], key=k[lo:hi].contiguous() if keyed else None, bins=BINS,
                              report=report, per_spectrum=False)[1]

    whole = run(0, N)
    for cut in (5, 32):
        a, b = run(0, cut), run(cut, N)
        assert torch.equal(a + b, whole), cut
        assert torch.equal(run(cut, N, report=run(0, cut)), whole), cut       # accumulated into one report
    assert int(engine.physics_value(whole, BINS[2])[-1, 0]) == N


def test_wrapper_checks_on_device_tensors(rep_case):
    from raman_mi355x import engine
    x, y, c = rep_case["x"], rep_case["y"], rep_case["c"]
    with pytest.raises(ValueError, match="bins"):
        engine.physics(x, y, c, key=_cuda(_keys()))
    with pytest.raises(ValueError, match="shape"):
        engine.physics(x, y, c, key=_cuda(_keys()[:5]), bins=BINS)
    with pytest.raises(TypeError):
        engine.physics(x, y, c, key=_cuda(_keys().astype(np.float64)), bins=BINS)
    with pytest.raises(ValueError, match="shape"):
        engine.physics(x, y, c, bins=BINS, report=engine.new_physics_report(5, "cuda"))
    with pytest.raises(ValueError, match="mismatch"):
        engine.physics(x[:3], y, c)
    with pytest.raises(TypeError):
        engine.physics(x.double(), y, c)
    with pytest.raises(ValueError, match="three samples"):
        engine.physics(x[:, :2], y[:, :2], c[:, :2])
    with pytest.raises(ValueError, match="finite"):
        engine.physics(x, y, c, weights=(0.1, float("nan"), 0.01))


# ---- the reference's recorded values -----------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "physics.npz")))


def test_fixture_against_the_reference(gold):
    from raman_mi355x import engine
    per, _ = engine.physics(_cuda(gold["noisy"]), _cuda(gold["pred"]), _cuda(gold["clean"]))
    per = per.cpu().numpy()
    np.testing.assert_allclose(per[:, 4], gold["ref64_each"], rtol=1e-11, atol=0)
    assert per[:, 5].astype(np.int64).tolist() == gold["counts"].tolist()
    v = math.fsum(per[:, 4]) / 8
    ref64, ref32, d32 = float(gold["ref64_batch"]), float(gold["ref32_batch"]), float(gold["d32"])
    np.testing.assert_allclose(v, ref64, rtol=1e-11, atol=0)
    print(f"engine {v!r} reference float64 {ref64!r} float32 {ref32!r} d32 {d32:.3e}")
    assert abs(v - ref32) <= d32 * abs(v) + 1e-11 * abs(v)
    # the generator's float64 clean
    per64, _ = engine.physics(_cuda(gold["noisy"][:2]), _cuda(gold["pred"][:2]), _cuda(gold["clean64"]))
    per64 = per64.cpu().numpy()
    np.testing.assert_allclose(per64[:, 4], gold["ref64_each_clean64"], rtol=1e-11, atol=0)
    assert per64[:, 5].astype(np.int64).tolist() == gold["counts64"].tolist()


@pytest.mark.parametrize("dim3", [True, False], ids=["N1L", "NL"])
def test_loss_module_engine_path_under_no_grad(gold, dim3):
    from raman_mi355x import PhysicsAwareLoss, engine
    crit = PhysicsAwareLoss()
    pred, clean, noisy = (_cuda(gold[k]).unsqueeze(1) if dim3 else _cuda(gold[k]) for k in ("pred", "clean", "noisy"))
    with torch.no_grad():
        assert crit.uses_engine(pred, clean, noisy)
        got = crit(pred, clean, noisy)
    per, _ = engine.physics(noisy, pred, clean)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    assert torch.equal(got, per[:, 4].mean().to(torch.float32))                   # the same bits
    ref64 = float(gold["ref64_batch"])
    assert abs(got.item() - ref64) <= (2.0 ** -24 + 1e-11) * abs(ref64)
    # inputs that want no gradient take the engine path with grad enabled too; float64 clean as well
    assert crit.uses_engine(pred, clean, noisy) and torch.equal(crit(pred, clean, noisy), got)
    assert crit.uses_engine(pred, clean.double(), noisy)
    assert abs(crit(pred, clean.double(), noisy).item() - ref64) <= (2.0 ** -24 + 1e-11) * abs(ref64)
    # other weights reach the kernel
    w = (0.3, 0.7, 2.0)
    with torch.no_grad():
        gw = PhysicsAwareLoss(*w)(pred, clean, noisy)
    refw = O.physics_values(gold["noisy"], gold["pred"], gold["clean"], weights=w)[:, 4].mean()
    assert abs(gw.item() - refw) <= (2.0 ** -24 + 1e-11) * abs(refw)


def test_loss_module_takes_the_eager_path_when_a_gradient_is_wanted(gold):
    from raman_mi355x import PhysicsAwareLoss
    crit = PhysicsAwareLoss()
    pred, clean, noisy = (_cuda(gold[k]).unsqueeze(1) for k in ("pred", "clean", "noisy"))
    pred.requires_grad_(True)
    assert not crit.uses_engine(pred, clean, noisy)
    loss = crit(pred, clean, noisy)
    assert loss.requires_grad and loss.dtype == torch.float32
    np.testing.assert_allclose(loss.item(), float(gold["ref32_batch"]), rtol=1e-5)
    loss.backward()
    g = pred.grad
    assert g.shape == pred.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # not contiguous, or float64 pred: eager as well
    with torch.no_grad():
        assert not crit.uses_engine(pred.double(), clean.double(), noisy.double())
        assert not crit.uses_engine(pred[:, :, ::2], clean[:, :, ::2], noisy[:, :, ::2])
        half = crit(pred[:, :, ::2], clean[:, :, ::2], noisy[:, :, ::2])
        assert half.dtype == torch.float32 and bool(torch.isfinite(half))


# ---- end to end --------------------------------------------------------------------------------------
def _model(arch, dtype):
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(golden_state_dict(arch, "trained"), strict=True)
    return m.cuda().eval().set_engine_dtype(dtype)


@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_evaluate_with_physics_on_pidn(dtype, tmp_path):
    from oracle.refgen import generate_signals
    from raman_mi355x import engine
    from raman_mi355x.evaluate import KEYS, evaluate, write_metrics, write_physics_report
    np.random.seed(20250412)
    n, L = 6, 1000
    clean, noisy, snrs, _ = generate_signals(n, signal_length=L)
    m = _model("PIDN", dtype)
    # one batch, as engine.forward below: a network's output bits may depend on the tile geometry its batch size selects
    plain = evaluate(m, noisy, clean, batch_size=n)
    got = evaluate(m, noisy, clean, batch_size=n, physics=True)
    assert set(plain) == set(KEYS) and set(got) == set(KEYS) | {"physics"}
    for k in KEYS:
        assert got[k] == plain[k], k                                   # the same bits
    # the oracle on the engine's own outputs
    x = torch.tensor(noisy, dtype=torch.float32).unsqueeze(1).cuda()
    y = engine.forward(m.ARCH, m.engine_code, m.packed_weights(x.device), x)
    x32, y32 = x.cpu().numpy()[:, 0], y.cpu().numpy()[:, 0]
    ref = O.physics_values(x32, y32, clean)
    assert clean.dtype == np.float64 and np.all(np.isfinite(ref))
    ph = got["physics"]
    assert ph["weights"] == list(W) and ph["count"] == n and "by_snr" not in ph
    for i, k in enumerate(O.QUANTITIES):
        np.testing.assert_allclose(ph[k], math.fsum(ref[:, i]) / n, rtol=1e-10, err_msg=k)
    np.testing.assert_allclose(ph["PeakMasked"], math.fsum(ref[:, 2]) * (L - 2) / ref[:, 5].sum(), rtol=1e-10)
    w = (0.3, 0.7, 2.0)
    other = evaluate(m, noisy, clean, batch_size=n, physics=w)["physics"]
    np.testing.assert_allclose(other["Total"], math.fsum(O.physics_values(x32, y32, clean, weights=w)[:, 4]) / n, rtol=1e-10)
    assert other["MSE"] == ph["MSE"] and other["PeakCount"] == ph["PeakCount"]
    # binned: the bins' counts are the SNR report's, with the nominal SNRs and with the measured SNR_in
    bins = (20.0, 37.0, 4)
    for kw in (dict(snrs=snrs), dict()):
        b = evaluate(m, noisy, clean, batch_size=n, snr_bins=bins, physics=True, **kw)
        s = evaluate(m, noisy, clean, batch_size=n, snr_bins=bins, **kw)
        assert set(b) == set(s) | {"physics"} and all(b[k] == s[k] for k in s)
        pb = b["physics"]
        assert [e["count"] for e in pb["by_snr"]] == [e["count"] for e in s["by_snr"]]
        assert (pb["under"]["count"], pb["over"]["count"]) == (s["snr_under"]["count"], s["snr_over"]["count"])
        assert sum(e["count"] for e in pb["by_snr"]) + pb["under"]["count"] + pb["over"]["count"] == n
        assert all(pb[k] == ph[k] for k in O.QUANTITIES + ("PeakMasked", "count"))
    rows = S.bin_rows(snrs.reshape(-1), *bins)
    b = evaluate(m, noisy, clean, batch_size=n, snr_bins=bins, snrs=snrs, physics=True)
    assert [e["count"] for e in b["physics"]["by_snr"]] == [int((rows == 1 + i).sum()) for i in range(4)]
    for i, e in enumerate(b["physics"]["by_snr"]):
        if e["count"]:
            np.testing.assert_allclose(e["Total"], math.fsum(ref[rows == 1 + i, 4]) / e["count"], rtol=1e-10)
    # metrics.txt does not change; the physics entry has its own files
    d0 = write_metrics(plain, root=str(tmp_path / "plain"))
    d1 = write_metrics(b, root=str(tmp_path / "physics"))
    d2 = write_metrics(s, root=str(tmp_path / "snr"))
    txt = [open(os.path.join(d, "metrics.txt"), "rb").read() for d in (d0, d1, d2)]
    assert txt[0] == txt[1] == txt[2] and len(txt[0].splitlines()) == 4
    write_physics_report(b, d1)
    assert os.path.getsize(os.path.join(d1, "physics_report.json")) > 0
    assert len(open(os.path.join(d1, "physics_report.txt")).read().splitlines()) == 9 + 1 + 4 + 2


def test_evaluate_synthetic_physics_same_bits_for_any_batch_size(monkeypatch):
    """64 simulator spectra in chunks of 24 + 24 + 16 and in one of 64: the report is exact accumulators, so
    the physics entry is the same bits (one forward geometry pinned for both, as in the SNR test)."""
    from raman_mi355x.evaluate import evaluate_synthetic
    monkeypatch.setenv("RDN_SHORT_TILES", "1")
    monkeypatch.setenv("RDN_WALK", "0")
    m = _model("PIDN", "f16")
    kw = dict(total=64, signal_length=1000, physics=True)
    a = evaluate_synthetic({"PIDN": m}, batch_size=24, **kw)["PIDN"]
    one = evaluate_synthetic({"PIDN": m}, batch_size=64, **kw)["PIDN"]
    assert a["physics"]["count"] == 64 and "by_snr" not in a["physics"]
    assert a["physics"] == one["physics"] and a["acc"] == one["acc"]
    assert a["physics"]["Total"] > 0 and a["physics"]["PeakCount"] > 0
    plain = evaluate_synthetic({"PIDN": m}, total=64, signal_length=1000, batch_size=24)["PIDN"]
    assert "physics" not in plain and plain["acc"] == a["acc"] and plain["means"] == a["means"]
    binned = evaluate_synthetic({"PIDN": m}, batch_size=24, snr_bins=(20.0, 37.0, 17), **kw)["PIDN"]
    assert [e["count"] for e in binned["physics"]["by_snr"]] == [e["count"] for e in binned["by_snr"]]
    assert binned["physics"]["Total"] == a["physics"]["Total"]
