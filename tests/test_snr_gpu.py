"""The SNR report on the device (rdn_snr / engine.snr, evaluate(snr_bins=...)) against the numpy oracle
(tests/snr_oracle.py: float64 values, float32 bin index, exact sums) and a reference-generator fixture.

Tolerances.  P, Ni and No differ from the oracle only in summation order (relative error at most about
L 2^-53), so a dB value differs by at most L 2^-53 10 / ln 10 -- 8e-12 dB at L = 16384 -- plus the
device log10's few ulp of a value near 30 (4e-15): atol 1e-9 dB leaves two orders of margin.  A report's
means are exact sums rounded once on both sides: rtol 1e-10, the metric tests' bound."""
import math
import os

import numpy as np
import pytest
import torch

import snr_oracle as O
from conftest import GOLDEN, golden_state_dict

pytestmark = pytest.mark.gpu

BINS = (20.0, 37.0, 4)
EDGES = np.linspace(20.0, 37.0, 5)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spectra(n, L, seed, snr_db=None):
    """Piecewise-constant clean spectra in [0, 1] (the simulator's shape), noisy x at about snr_db (per
    spectrum; default 25 dB) and a denoised y that keeps a third of the noise."""
    rng = np.random.default_rng(seed)
    c = np.repeat(rng.uniform(0.05, 1, (n, L // 7 + 1)), 7, axis=1)[:, :L].astype(np.float32)
    snr_db = np.full(n, 25.0) if snr_db is None else np.asarray(snr_db, dtype=np.float64)
    std = np.sqrt(np.mean(c.astype(np.float64) ** 2, axis=1) / 10 ** (snr_db / 10))
    noise = rng.normal(0, 1, c.shape) * std[:, None]
    x = (c + noise).astype(np.float32)
    y = (c + noise / 3 + rng.normal(0, 1, c.shape) * std[:, None] / 10).astype(np.float32)
    return x, y, c


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("L", [1, 7, 511, 512, 513, 1500, 16384])
def test_per_spectrum_values_match_oracle(L, n, f64):
    from raman_mi355x import engine
    x, y, c = _spectra(n, L, 1000 * L + n)
    c = c.astype(np.float64) + (np.random.default_rng(L).uniform(0, 1e-9, c.shape) if f64 else 0)   # not fp32 values
    c = c if f64 else c.astype(np.float32)
    per, rep = engine.snr(_cuda(x), _cuda(y), _cuda(c))
    assert rep is None and per.shape == (n, 3) and per.dtype == torch.float64
    ref = O.snr_values(x, y, c)
    assert np.all(np.isfinite(ref))
    np.testing.assert_allclose(per.cpu().numpy(), ref, rtol=0, atol=1e-9)


def _word(report, row, q, w):
    from raman_mi355x import _lib
    return int(report[row * _lib.REPORT_ROW_WORDS + q * _lib.ACC_STRIDE + w])


def test_degenerate_rows_give_ieee_values_and_are_counted():
    """y == clean: SNR_out = +inf; an all-zero clean: SNR_in = SNR_out = -inf, gain NaN.  The other
    spectra are unaffected; a report counts such values in the quantity's out-of-range word."""
    from raman_mi355x import engine, _lib
    n, L = 5, 300
    x, y, c = _spectra(n, L, 7)
    y[1] = c[1]
    c[3] = 0
    ref = O.snr_values(x, y, c)
    assert ref[1, 1] == np.inf and ref[1, 2] == np.inf and np.isfinite(ref[1, 0])
    assert ref[3, 0] == -np.inf and ref[3, 1] == -np.inf and np.isnan(ref[3, 2])
    key = np.array([21, 22, 30, 31, 36], dtype=np.float32)            # rows 1, 1, 2, 2, 2 of two bins
    per, rep = engine.snr(_cuda(x), _cuda(y), _cuda(c), key=_cuda(key), bins=(20, 37, 2))
    got = per.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)           # inf and NaN compare as equal
    rep = rep.cpu().numpy()
    oor = [[_word(rep, r, q, _lib.ACC_LIMBS) for q in (4, 5, 6)] for r in range(4)]
    assert oor == [[0, 0, 0], [0, 1, 1], [1, 1, 1], [0, 0, 0]]
    v = engine.report_value(torch.from_numpy(rep), 2).numpy()
    assert v[:, 0].tolist() == [0, 2, 3, 0, 5] and np.all(v[:, 8] == 0) and np.all(v[:, 1:5] == 0)
    assert np.isnan(v[1, 6]) and np.isnan(v[2, 5]) and np.isnan(v[4, 5:8]).all()
    np.testing.assert_allclose(v[1, 5], ref[:2, 0].sum(), rtol=1e-12)  # the finite quantity of that row
    # binned by the measured SNR_in: the -inf spectrum lands in the underflow row
    _, rep2 = engine.snr(_cuda(x), _cuda(y), _cuda(c), bins=(20, 37, 2), per_spectrum=False)
    rep2 = rep2.cpu().numpy()
    assert int(rep2[_lib.REPORT_COUNT]) == 1 and _word(rep2, 0, 4, _lib.ACC_LIMBS) == 1


# ---- the report: 64 spectra, L = 500, four bins over (20, 37) ----------------------------------------
N, L_REP = 64, 500
# nominal SNRs from 17 to 40 dB in a fixed shuffled order: under, over and every bin, measured SNRs included
TARGET = np.random.default_rng(5).permutation(np.linspace(17.0, 40.0, N))


def _keys():
    """Keys that cover the underflow and overflow rows, NaN, +-inf, every bin and both ends of [lo, hi)."""
    f = np.float32
    k = TARGET.astype(np.float32).copy()
    k[:10] = [20.0, 37.0, np.nextafter(f(37), f(0)), np.nextafter(f(20), f(0)), np.nan, np.inf, -np.inf, 24.25, 28.5, 32.75]
    return k


@pytest.fixture(scope="module")
def rep_case():
    """Inputs on the device, the device per4 (engine.metrics), and the oracle's seven values per spectrum."""
    from raman_mi355x import engine
    x, y, c = _spectra(N, L_REP, 42, TARGET)
    dx, dy, dc = _cuda(x), _cuda(y), _cuda(c)
    per4, _ = engine.metrics(dy, dc)
    torch.cuda.synchronize()
    per7 = np.concatenate([per4.cpu().numpy(), O.snr_values(x, y, c)], axis=1)
    return dict(x=dx, y=dy, c=dc, per4=per4, per7=per7)


def _check_report(rep, per7, rows, nbins, have4=True):
    from raman_mi355x import engine
    v = engine.report_value(rep, nbins).numpy()
    ref = O.report_sums(per7, rows, nbins)
    assert v[:, 0].astype(np.int64).tolist() == ref[:, 0].astype(np.int64).tolist()
    assert v[:, 8].tolist() == (ref[:, 0] if have4 else 0 * ref[:, 0]).tolist()
    first = 0 if have4 else 4
    for b in range(nbins + 3):
        if ref[b, 0]:
            np.testing.assert_allclose(v[b, 1 + first:8] / ref[b, 0], ref[b, 1 + first:] / ref[b, 0], rtol=1e-10, err_msg=str(b))
    if not have4:
        assert np.all(v[:, 1:5] == 0)
    return v


def test_report_matches_oracle_with_given_keys(rep_case):
    from raman_mi355x import engine
    k = _keys()
    rows = O.bin_rows(k, *BINS)
    assert set(rows.tolist()) == set(range(6)) and rows[:10].tolist() == [1, 5, 4, 0, 5, 5, 0, 2, 3, 4]
    per, rep = engine.snr(rep_case["x"], rep_case["y"], rep_case["c"], key=_cuda(k), bins=BINS, per4=rep_case["per4"])
    np.testing.assert_allclose(per.cpu().numpy(), rep_case["per7"][:, 4:], rtol=0, atol=1e-9)
    _check_report(rep, rep_case["per7"], rows, BINS[2])
    # the words themselves: the oracle's limbs of the device's own per-spectrum values
    per7 = np.concatenate([rep_case["per4"].cpu().numpy(), per.cpu().numpy()], axis=1)
    assert np.array_equal(rep.cpu().numpy(), O.report_words(per7, rows, BINS[2]))


def test_report_matches_oracle_binned_by_measured_snr(rep_case):
    from raman_mi355x import engine
    measured = rep_case["per7"][:, 4]
    # the oracle alone: every measured SNR_in is at least 1e-3 dB from every edge, so the device's last
    # bits (1e-9 dB) cannot move a spectrum across one
    assert np.abs(measured[:, None] - EDGES[None, :]).min() >= 1e-3
    rows = O.bin_rows(measured.astype(np.float32), *BINS)
    assert set(rows.tolist()) == set(range(6))
    _, rep = engine.snr(rep_case["x"], rep_case["y"], rep_case["c"], bins=BINS, per4=rep_case["per4"], per_spectrum=False)
    _check_report(rep, rep_case["per7"], rows, BINS[2])
    _, rep = engine.snr(rep_case["x"], rep_case["y"], rep_case["c"], bins=BINS, per_spectrum=False)
    _check_report(rep, rep_case["per7"], rows, BINS[2], have4=False)


@pytest.mark.parametrize("keyed", [True, False])
def test_report_is_independent_of_the_batch_split(rep_case, keyed):
    from raman_mi355x import engine
    k = _cuda(_keys()) if keyed else None
    x, y, c, p4 = (rep_case[s] for s in ("x", "y", "c", "per4"))

    def run(lo, hi, report=None):
        return engine.snr(x[lo:hi], y[lo:hi], c[lo:hi], key=k[lo:hi].contiguous() if keyed else None, bins=BINS,
                          per4=p4[lo:hi].contiguous(), report=report, per_spectrum=False)[1]

    whole = run(0, N)
    for cut in (1, 32):
        a, b = run(0, cut), run(cut, N)
        assert torch.equal(a + b, whole), cut
        assert torch.equal(run(cut, N, report=run(0, cut)), whole), cut       # accumulated into one report
    assert int(engine.report_value(whole, BINS[2])[-1, 0]) == N


def test_wrapper_checks_on_device_tensors(rep_case):
    from raman_mi355x import engine
    x, y, c = rep_case["x"], rep_case["y"], rep_case["c"]
    with pytest.raises(ValueError, match="bins"):
        engine.snr(x, y, c, key=_cuda(_keys()))
    with pytest.raises(ValueError, match="shape"):
        engine.snr(x, y, c, key=_cuda(_keys()[:5]), bins=BINS)
    with pytest.raises(TypeError):
        engine.snr(x, y, c, key=_cuda(_keys().astype(np.float64)), bins=BINS)
    with pytest.raises(ValueError, match="shape"):
        engine.snr(x, y, c, bins=BINS, report=engine.new_report(5, "cuda"))
    with pytest.raises(ValueError, match="mismatch"):
        engine.snr(x[:3], y, c)
    with pytest.raises(TypeError):
        engine.snr(x.double(), y, c)


# ---- end to end --------------------------------------------------------------------------------------
def _model(arch, dtype):
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(golden_state_dict(arch, "trained"), strict=True)
    return m.cuda().eval().set_engine_dtype(dtype)


@pytest.mark.parametrize("arch,dtype", [("RRCDNet", "f16"), ("ADSDN", "fp32")])
def test_evaluate_with_snr_bins(arch, dtype, tmp_path):
    from oracle.refgen import generate_signals
    from raman_mi355x import engine
    from raman_mi355x.evaluate import KEYS, evaluate, write_metrics, write_snr_report
    np.random.seed(20250412)
    clean, noisy, snrs, _ = generate_signals(16, signal_length=1000)
    m = _model(arch, dtype)
    plain = evaluate(m, noisy, clean, batch_size=16)
    got = evaluate(m, noisy, clean, batch_size=16, snr_bins=BINS, snrs=snrs)
    assert set(plain) == set(KEYS)
    for k in KEYS:
        assert got[k] == plain[k], k                                   # the same bits
    # the module's own outputs through engine.snr
    x = torch.tensor(noisy, dtype=torch.float32).unsqueeze(1).cuda()
    with torch.no_grad():
        y = m(x)
    per, _ = engine.snr(x, y, torch.tensor(clean).cuda())
    per = per.cpu().numpy()
    for i, k in enumerate(("SNR_in", "SNR_out", "SNR_gain")):
        np.testing.assert_allclose(got[k], math.fsum(per[:, i]) / 16, rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(per, O.snr_values(x.cpu().numpy()[:, 0], y.cpu().numpy()[:, 0], clean), rtol=0, atol=1e-9)
    rows = O.bin_rows(snrs.reshape(-1), *BINS)
    assert [e["count"] for e in got["by_snr"]] == [int((rows == 1 + b).sum()) for b in range(BINS[2])]
    assert sum(e["count"] for e in got["by_snr"]) + got["snr_under"]["count"] + got["snr_over"]["count"] == 16
    for b, e in enumerate(got["by_snr"]):
        if e["count"]:
            np.testing.assert_allclose(e["SNR_gain"], math.fsum(per[rows == 1 + b, 2]) / e["count"], rtol=1e-12)
            assert set(e) == {"lo", "hi", "count"} | set(engine.REPORT_QUANTITIES)
    # binned by the measured SNR_in when the dataset carries no nominal one
    auto = evaluate(m, noisy, clean, batch_size=16, snr_bins=BINS)
    assert auto["SNR_gain"] == got["SNR_gain"] and sum(e["count"] for e in auto["by_snr"]) <= 16
    d = write_metrics(got, root=str(tmp_path))
    assert len(open(os.path.join(d, "metrics.txt")).read().splitlines()) == 4
    write_snr_report(got, d)
    assert len(open(os.path.join(d, "snr_report.txt")).read().splitlines()) == 4 + BINS[2] + 2


def test_evaluate_synthetic_report_same_bits_for_any_batch_size(monkeypatch):
    """64 simulator spectra at L = 1500, binned by the generator's nominal SNR: the report and the means
    are the same bits in one chunk of 64 and in four of 16 (one forward geometry for both: the walk, whose
    epilogue supplies per4)."""
    from raman_mi355x.evaluate import evaluate_synthetic
    monkeypatch.setenv("RDN_SHORT_TILES", "0")
    monkeypatch.setenv("RDN_WALK", "1")
    m = _model("RRCDNet", "f16")
    kw = dict(seed=20250410, signal_length=1500, first_index=77, snr_bins=(20.0, 37.0, 17))
    a = evaluate_synthetic({"RRCDNet": m}, 64, batch_size=64, **kw)["RRCDNet"]
    b = evaluate_synthetic({"RRCDNet": m}, 64, batch_size=16, **kw)["RRCDNet"]
    assert sum(e["count"] for e in a["by_snr"]) == 64 and len(a["by_snr"]) == 17
    assert a["report"] == b["report"] and a["acc"] == b["acc"] and a["means"] == b["means"]
    for k in ("SNR_in", "SNR_out", "SNR_gain", "by_snr", "snr_under", "snr_over"):
        assert a[k] == b[k], k
    # the nominal SNRs are U(20, 37); the briefly trained fixture network is no denoiser (it loses dB), so
    # only the consistency of the three means is held: mean gain = mean out - mean in
    assert 20 < a["SNR_in"] < 37
    assert abs(a["SNR_gain"] - (a["SNR_out"] - a["SNR_in"])) <= 1e-12 * abs(a["SNR_in"])
    plain = evaluate_synthetic({"RRCDNet": m}, 64, batch_size=16, **dict(kw, snr_bins=None))["RRCDNet"]
    assert plain["acc"] == a["acc"] and "by_snr" not in plain


def test_reference_generator_fixture():
    """tests/golden/snr.npz (make_snr_golden.py): 8 spectra of the reference generator without extreme
    noise.  The device SNR_in equals the stored numpy float64 one; and -- the check on the definition,
    that P is mean(clean^2) -- it estimates the nominal SNR the generator drew within five standard
    deviations of a variance estimate over L samples, 5 (10 / ln 10) sqrt(2 / L) = 0.69 dB."""
    from raman_mi355x import engine
    g = np.load(os.path.join(GOLDEN, "snr.npz"))
    clean, noisy = g["clean"], g["noisy"]
    assert clean.dtype == np.float32 and clean.shape == (8, 2000)
    assert np.all(np.abs(g["snr_in"] - g["snrs"]) <= 5 * (10 / math.log(10)) * math.sqrt(2 / 2000))
    per, _ = engine.snr(_cuda(noisy), _cuda(noisy), _cuda(clean))
    per = per.cpu().numpy()
    np.testing.assert_allclose(per[:, 0], g["snr_in"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(per[:, 1], g["snr_in"], rtol=0, atol=1e-9)   # y = x: no gain
    assert np.all(per[:, 2] == 0)
