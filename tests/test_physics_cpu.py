"""PhysicsAwareLoss report, the parts that need no GPU: the new entry points exist (ABI v6, detected by
symbol), argument checking, the host conversion of a report (rdn_physics_value), the numpy oracle against
the reference class's recorded values (tests/golden/physics.npz, make_physics_golden.py), and the eager
path of the drop-in PhysicsAwareLoss module."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import physics_oracle as O
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    from raman_mi355x import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "physics.npz")))


def test_entry_points_present_without_a_version_bump(lib):
    import raman_mi355x as R
    from raman_mi355x import _lib, engine
    for name in ("rdn_physics", "rdn_physics_value"):
        assert hasattr(lib, name) and name in _lib.EXPORTED, name
    assert lib.rdn_version() == 6
    assert engine.PHYS_QUANTITIES == O.QUANTITIES
    assert R.PhysicsAwareLoss is not None and "PhysicsAwareLoss" in R.__all__ and "write_physics_report" in R.__all__


def test_layout_constants_match_the_header():
    from raman_mi355x import _lib
    with open(os.path.join(ROOT, "include", "raman_mi355x.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define RDN_PHYS_QUANTITIES (\d+)", header).group(1)) == _lib.PHYS_QUANTITIES == 6
    for macro in ("RDN_PHYS_COUNT (RDN_PHYS_QUANTITIES * RDN_ACC_STRIDE)", "RDN_PHYS_ROW_WORDS (RDN_PHYS_COUNT + 1)",
                  "RDN_PHYS_WORDS(nbins) (RDN_REPORT_ROWS(nbins) * RDN_PHYS_ROW_WORDS)",
                  "RDN_PHYS_VALUES (RDN_PHYS_QUANTITIES + 1)"):
        assert "#define " + macro in header, macro
    assert (_lib.PHYS_COUNT, _lib.PHYS_ROW_WORDS, _lib.PHYS_VALUES) == (O.COUNT, O.ROW_WORDS, 7) == (42, 43, 7)
    assert _lib.phys_words(17) == 19 * 43


def test_argument_errors_need_no_device(lib):
    fake = [ctypes.c_void_p((i + 1) << 32) for i in range(5)]        # addresses that are never read
    x, y, c, per, rep = fake

    def phys(x=x, y=y, c=c, f64=0, n=4, L=100, w=(0.1, 0.05, 0.01), per=per, key=None, lo=20.0, hi=37.0, nbins=4, rep=rep):
        return lib.rdn_physics(x, y, c, f64, n, L, w[0], w[1], w[2], per, key, lo, hi, nbins, rep, None)

    for bad in (dict(L=2), dict(L=0), dict(L=1 << 31), dict(n=-1), dict(f64=2), dict(x=None), dict(y=None), dict(c=None),
                dict(nbins=0), dict(nbins=65), dict(hi=20.0), dict(hi=19.0), dict(lo=float("nan")), dict(hi=float("inf")),
                dict(per=None, rep=None), dict(rep=None, key=fake[0]), dict(w=(float("nan"), 0.05, 0.01)),
                dict(w=(0.1, float("inf"), 0.01)), dict(w=(0.1, 0.05, float("-inf")))):
        assert phys(**bad) == -1, bad
        assert lib.rdn_last_error() != b""
    assert b"L" in (phys(L=2), lib.rdn_last_error())[1]
    # n = 0 launches nothing and accepts NULL data, but still checks L, the weights and the bins
    assert phys(n=0, x=None, y=None, c=None) == 0
    assert phys(n=0, x=None, y=None, c=None, L=3) == 0
    assert phys(n=0, x=None, y=None, c=None, L=2) == -1
    assert phys(n=0, x=None, y=None, c=None, nbins=0) == -1
    assert phys(n=0, rep=None, nbins=0) == 0                         # no report: the bins are not used
    out = (ctypes.c_double * 1)()
    words = (ctypes.c_int64 * 1)()
    assert lib.rdn_physics_value(None, 4, out) == -1 and lib.rdn_physics_value(words, 4, None) == -1
    assert lib.rdn_physics_value(words, 0, out) == -1 and lib.rdn_physics_value(words, 65, out) == -1


def _values(nbins):
    """Six columns of values per report row, tiny and huge ones included; PeakCount an integer."""
    rng = np.random.default_rng(13)
    per6, rows = [], []
    for b in range(nbins + 2):
        if b == 2:
            continue                                                  # an empty bin
        m = 3 + 4 * b
        v = rng.uniform(0, 1, (m, 6)) * 10.0 ** rng.integers(-12, 6, (m, 6))
        v[:, 5] = rng.integers(0, 2000, m)
        v[0, :5] = [1e-40, 3e-39, 2.0 ** 63, 0.1, 2.0 ** 62]
        per6.append(v)
        rows += [b] * m
    return np.concatenate(per6), np.array(rows)


def test_physics_value_rounds_the_exact_sums_once_and_totals_the_rows():
    from raman_mi355x import engine
    nbins = 3
    per6, rows = _values(nbins)
    got = engine.physics_value(torch.from_numpy(O.report_words(per6, rows, nbins)), nbins).numpy()
    ref = O.report_sums(per6, rows, nbins)
    assert got.shape == (nbins + 3, 7)
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 6], ref[:, 6])    # counts: exact
    # values below 2^-128 resolution lose their tail (truncation): at most 2^-128 per value
    np.testing.assert_allclose(got[:, 1:6], ref[:, 1:6], rtol=1e-15, atol=len(rows) * 2.0 ** -128)
    assert np.all(got[2] == 0)                                        # the empty bin
    assert got[nbins + 2, 0] == len(rows) and got[nbins + 2, 6] == per6[:, 5].sum()


def test_physics_value_out_of_range_word_gives_nan_for_that_quantity_only():
    from raman_mi355x import engine, _lib
    nbins = 2
    per6, rows = _values(nbins)
    words = O.report_words(per6, rows, nbins)
    clean = engine.physics_value(torch.from_numpy(words), nbins).numpy()
    words = words.copy()
    words[1 * _lib.PHYS_ROW_WORDS + 2 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] = 2       # row 1, Peak
    got = engine.physics_value(torch.from_numpy(words), nbins).numpy()
    bad = np.zeros_like(got, dtype=bool)
    bad[1, 1 + 2] = bad[nbins + 2, 1 + 2] = True                                   # the row and the totals
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], clean[~bad])
    # hand-built limbs: 2.25 in row 1's Total, 0.5 in row 2's (limb 4 holds the units)
    rep = np.zeros(_lib.phys_words(nbins), dtype=np.int64)
    r1, r2 = 1 * _lib.PHYS_ROW_WORDS, 2 * _lib.PHYS_ROW_WORDS
    rep[r1 + 4 * _lib.ACC_STRIDE + 4], rep[r1 + 4 * _lib.ACC_STRIDE + 3], rep[r1 + _lib.PHYS_COUNT] = 2, 1 << 30, 1
    rep[r2 + 4 * _lib.ACC_STRIDE + 3], rep[r2 + _lib.PHYS_COUNT] = 1 << 31, 2
    rep[r2 + 0 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] = 1                            # row 2: an out-of-range MSE
    v = engine.physics_value(torch.from_numpy(rep), nbins).numpy()
    assert v[1, 5] == 2.25 and v[2, 5] == 0.5 and v[4, 5] == 2.75 and v[4, 0] == 3
    assert np.isnan(v[2, 1]) and np.isnan(v[4, 1]) and v[1, 1] == 0
    # the oracle's own words count non-finite values the same way
    p = per6.copy()
    p[rows == 1, 2] = [np.inf, np.nan] + [1.0] * (int((rows == 1).sum()) - 2)
    assert O.report_words(p, rows, nbins)[1 * _lib.PHYS_ROW_WORDS + 2 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] == 2


def test_oracle_equals_the_reference_float64(gold):
    per = O.physics_values(gold["noisy"], gold["pred"], gold["clean"])
    assert gold["clean"].dtype == np.float32 and gold["clean"].shape == (8, 2000) and gold["clean64"].dtype == np.float64
    np.testing.assert_allclose(per[:, 4], gold["ref64_each"], rtol=1e-12)
    np.testing.assert_allclose(np.mean(per[:, 4]), gold["ref64_batch"], rtol=1e-12)
    assert per[:, 5].astype(np.int64).tolist() == gold["counts"].tolist()
    # the generator's float64 clean for two spectra: values and the type-faithful mask
    per64 = O.physics_values(gold["noisy"][:2], gold["pred"][:2], gold["clean64"])
    np.testing.assert_allclose(per64[:, 4], gold["ref64_each_clean64"], rtol=1e-12)
    assert per64[:, 5].astype(np.int64).tolist() == gold["counts64"].tolist()
    assert abs(gold["ref32_batch"] - gold["ref64_batch"]) / abs(gold["ref64_batch"]) == gold["d32"] < 1e-6


def test_float64_oracle_is_within_1e12_of_longdouble(gold):
    for c, n in ((gold["clean"], 8), (gold["clean64"], 2)):
        a = O.physics_values(gold["noisy"][:n], gold["pred"][:n], c)
        b = O.physics_values(gold["noisy"][:n], gold["pred"][:n], c, dtype=np.longdouble)
        assert b.dtype == np.longdouble
        rel = np.abs(a - b) / np.abs(b)
        print("float64 oracle vs longdouble, max relative difference per quantity:", rel.max(axis=0).astype(np.float64))
        assert np.all(rel <= 1e-12) and np.array_equal(a[:, 5], b[:, 5].astype(np.float64))


def _t(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt).unsqueeze(1)


def test_eager_loss_float64_and_float32_against_the_reference(gold):
    from raman_mi355x import PhysicsAwareLoss
    crit = PhysicsAwareLoss()
    assert (crit.alpha, crit.beta, crit.gamma) == (0.1, 0.05, 0.01) and isinstance(crit, torch.nn.Module)
    args64 = [_t(gold[k], torch.float64) for k in ("pred", "clean", "noisy")]
    assert not crit.uses_engine(*args64)
    got = crit(*args64)
    assert got.dtype == torch.float64 and got.dim() == 0
    np.testing.assert_allclose(got.item(), gold["ref64_batch"], rtol=1e-11)
    got2d = crit(*[a.squeeze(1) for a in args64])                     # (N, L) works like (N, 1, L)
    np.testing.assert_allclose(got2d.item(), gold["ref64_batch"], rtol=1e-11)
    args32 = [_t(gold[k], torch.float32) for k in ("pred", "clean", "noisy")]
    got32 = crit(*args32)
    assert got32.dtype == torch.float32 and got32.dim() == 0
    np.testing.assert_allclose(got32.item(), gold["ref32_batch"], rtol=1e-5)
    # the smallest weighted term is far above that bar: a dropped or mis-weighted term fails it
    per = O.physics_values(gold["noisy"], gold["pred"], gold["clean"])
    share = np.array([per[:, 0].mean(), 0.1 * per[:, 1].mean(), 0.05 * per[:, 2].mean(), 0.01 * per[:, 3].mean()]) \
        / per[:, 4].mean()
    assert share.min() > 50 * 1e-5, share
    # other weights: the eager path is the formula, Total = ((MSE + a S) + b P) + g N
    w = (0.3, 0.7, 2.0)
    np.testing.assert_allclose(PhysicsAwareLoss(*w)(*args64).item(),
                               O.physics_values(gold["noisy"], gold["pred"], gold["clean"], weights=w)[:, 4].mean(),
                               rtol=1e-11)


def test_eager_gradient_against_the_reference_float64(gold):
    from raman_mi355x import PhysicsAwareLoss
    n, L = gold["grad64"].shape
    assert (n, L) == (2, 64)
    p = _t(gold["pred"][:n, :L], torch.float64).requires_grad_(True)
    loss = PhysicsAwareLoss()(p, _t(gold["clean"][:n, :L], torch.float64), _t(gold["noisy"][:n, :L], torch.float64))
    loss.backward()
    g = p.grad.squeeze(1).numpy()
    assert np.all(np.isfinite(g)) and np.abs(gold["grad64"]).max() > 0
    np.testing.assert_allclose(g, gold["grad64"], rtol=1e-10, atol=0)


def test_python_surface_refuses_what_the_kernel_cannot_take():
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate
    t = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.physics(t, t, t)
    for bad in ((0.1, 0.05), (0.1, 0.05, float("nan")), (0.1, float("inf"), 0.01), "abc", 0.1):
        with pytest.raises(ValueError):
            engine._weights(bad)
    assert engine._weights((1, 2, 3)) == (1.0, 2.0, 3.0)
    with pytest.raises(ValueError):
        engine.new_physics_report(0, "cpu")
    assert engine.new_physics_report(17, "cpu").shape == (19 * 43,)
    with pytest.raises(ValueError, match="words"):
        engine.physics_value(torch.zeros(10, dtype=torch.int64), 4)
    # evaluate() is refused on a CPU device exactly as before, with or without physics
    m = R.DenoiseCNN()
    z = np.zeros((2, 100))
    for kw in ({}, {"physics": None}, {"physics": True}, {"physics": (0.1, 0.05, 0.01)},
               {"physics": True, "snr_bins": (20, 37, 4)}):
        with pytest.raises(RuntimeError, match="runs its metrics on the GPU"):
            evaluate(m, z, z, device="cpu", **kw)


def test_summary_and_written_report(tmp_path):
    """physics_summary / write_physics_report on a hand-built report; write_metrics keeps its four lines."""
    from raman_mi355x.evaluate import physics_summary, write_metrics, write_physics_report
    nbins, L = 4, 1000
    per6, rows = _values(nbins)
    words = torch.from_numpy(O.report_words(per6, rows, nbins))
    ref = O.report_sums(per6, rows, nbins)
    s = physics_summary(words, (0.1, 0.05, 0.01), L, (20, 37, nbins))
    assert s["weights"] == [0.1, 0.05, 0.01] and s["count"] == len(rows)
    for k, name in enumerate(O.QUANTITIES):
        np.testing.assert_allclose(s[name], ref[nbins + 2, 1 + k] / len(rows), rtol=1e-12)
    np.testing.assert_allclose(s["PeakMasked"], ref[nbins + 2, 3] * (L - 2) / ref[nbins + 2, 6], rtol=1e-12)
    assert [e["count"] for e in s["by_snr"]] == ref[1:nbins + 1, 0].astype(int).tolist()
    assert (s["under"]["count"], s["over"]["count"]) == (ref[0, 0], ref[nbins + 1, 0])
    assert [(e["lo"], e["hi"]) for e in s["by_snr"]] == [(20 + 4.25 * b, 24.25 + 4.25 * b) for b in range(nbins)]
    assert set(s["by_snr"][1]) == {"lo", "hi", "count"}               # the empty bin (report row 2)
    np.testing.assert_allclose(s["by_snr"][0]["Total"], ref[1, 5] / ref[1, 0], rtol=1e-12)
    # an unbinned report: everything in row 1 of one bin
    one = O.report_words(per6, np.ones(len(rows), dtype=np.int64), 1)
    u = physics_summary(torch.from_numpy(one), (0.1, 0.05, 0.01), L)
    assert "by_snr" not in u and u["count"] == len(rows) and u["Total"] == s["Total"]
    result = {"MSE": 1.0, "SSIM": 0.5, "Smoothness": 0.25, "Peak2Peak": 2.0}
    d0 = write_metrics(result, root=str(tmp_path / "a"))
    d = write_metrics(dict(result, physics=s), root=str(tmp_path / "b"))
    assert open(os.path.join(d, "metrics.txt")).read() == open(os.path.join(d0, "metrics.txt")).read()
    assert write_physics_report(dict(result, physics=s), d) == d
    back = json.load(open(os.path.join(d, "physics_report.json")))
    assert back["by_snr"] == s["by_snr"] and back["Total"] == s["Total"]
    table = open(os.path.join(d, "physics_report.txt")).read().splitlines()
    assert len(table) == 2 + 7 + 1 + nbins + 2 and table[9].split() == ["lo", "hi", "count"] + list(O.QUANTITIES) + ["PeakMasked"]
    write_physics_report(dict(result, physics=u), str(tmp_path / "c"))
    assert len(open(os.path.join(str(tmp_path / "c"), "physics_report.txt")).read().splitlines()) == 9
    with pytest.raises(ValueError, match="physics"):
        write_physics_report(result, d)
    assert math.isnan(physics_summary(torch.from_numpy(O.report_words(per6 * [1, 1, 1, 1, 1, 0], rows, nbins)),
                                      (0.1, 0.05, 0.01), L, (20, 37, nbins))["PeakMasked"])
