"""SNR report, the parts that need no GPU: the new entry points exist (ABI v6, detected by symbol), the
host conversion of a report (rdn_report_value), the fp32 bin formula (rdn_report_bin against the numpy
restatement of the header), argument checking, and the Python surface around them."""
import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import snr_oracle as O
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from raman_mi355x import _lib
    return _lib.lib()


def test_entry_points_present_without_a_version_bump(lib):
    from raman_mi355x import _lib
    for name in ("rdn_snr", "rdn_report_bin", "rdn_report_value"):
        assert hasattr(lib, name) and name in _lib.EXPORTED, name
    assert lib.rdn_version() == 6


def test_report_layout_constants_match_the_header():
    from raman_mi355x import _lib
    with open(os.path.join(ROOT, "include", "raman_mi355x.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define RDN_REPORT_QUANTITIES (\d+)", header).group(1)) == _lib.REPORT_QUANTITIES == 7
    assert int(re.search(r"#define RDN_REPORT_MAX_BINS (\d+)", header).group(1)) == _lib.REPORT_MAX_BINS == 64
    assert (_lib.REPORT_COUNT, _lib.REPORT_COUNT4, _lib.REPORT_ROW_WORDS) == (O.COUNT, O.COUNT4, O.ROW_WORDS) == (49, 50, 51)
    assert _lib.report_words(17) == 19 * 51 and _lib.REPORT_VALUES == 9


def _values(nbins):
    """Seven columns of values per report row, negative, tiny and huge ones included."""
    rng = np.random.default_rng(11)
    per7, rows = [], []
    for b in range(nbins + 2):
        if b == 2:
            continue                                                  # an empty bin
        m = 3 + 5 * b
        v = rng.uniform(-1, 1, (m, 7)) * 10.0 ** rng.integers(-12, 12, (m, 7))
        v[0] = [1e-40, -3e-39, 2.0 ** 63, -(2.0 ** 62), 0.1, -0.2, -40.0]
        per7.append(v)
        rows += [b] * m
    return np.concatenate(per7), np.array(rows)


def test_report_value_rounds_the_exact_sums_once():
    from raman_mi355x import engine
    nbins = 4
    per7, rows = _values(nbins)
    got = engine.report_value(torch.from_numpy(O.report_words(per7, rows, nbins)), nbins).numpy()
    assert got.shape == (nbins + 3, 9)
    for b in list(range(nbins + 2)) + [nbins + 2]:
        sel = per7[rows == b] if b < nbins + 2 else per7
        assert got[b, 0] == got[b, 8] == len(sel)
        for k in range(7):
            # the exact total of the 2^-128-truncated values, rounded once (negative sums included)
            exact = sum(math.floor(abs(Fraction(v)) * 2 ** 128) * (1 if v >= 0 else -1) for v in sel[:, k])
            assert got[b, 1 + k] == float(Fraction(exact) / 2 ** 128), (b, k)
    assert np.all(got[2] == 0)                                        # the empty bin
    assert (got[:nbins + 2, 0].sum(), got[nbins + 2, 0]) == (len(rows), len(rows))
    assert np.any(got[:, 1:8] < 0)


def test_report_value_out_of_range_word_gives_nan_for_that_quantity_only():
    from raman_mi355x import engine, _lib
    nbins = 2
    per7, rows = _values(nbins)
    words = O.report_words(per7, rows, nbins)
    clean = engine.report_value(torch.from_numpy(words), nbins).numpy()
    words = words.copy()
    words[1 * _lib.REPORT_ROW_WORDS + 5 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] = 2      # row 1, SNR_out
    got = engine.report_value(torch.from_numpy(words), nbins).numpy()
    bad = np.zeros_like(got, dtype=bool)
    bad[1, 1 + 5] = bad[nbins + 2, 1 + 5] = True                                   # the row and the totals
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], clean[~bad])
    # the oracle's own words count non-finite values the same way
    v = per7.copy()
    v[rows == 1, 5] = [np.inf, np.nan] + [1.0] * (int((rows == 1).sum()) - 2)
    w = O.report_words(v, rows, nbins)
    assert w[1 * _lib.REPORT_ROW_WORDS + 5 * _lib.ACC_STRIDE + _lib.ACC_LIMBS] == 2


def test_report_without_per4_keeps_the_first_four_at_zero():
    from raman_mi355x import engine
    nbins = 3
    per7, rows = _values(nbins)
    got = engine.report_value(torch.from_numpy(O.report_words(per7, rows, nbins, have4=False)), nbins).numpy()
    assert np.all(got[:, 1:5] == 0) and np.all(got[:, 8] == 0) and got[nbins + 2, 0] == len(rows)
    assert np.all(got[[0, 1, 3, 4], 5:8] != 0)


def test_reports_add_as_integers():
    """Splitting the spectra across two reports and adding the int64 words gives the same doubles (and
    the same words) as one report: what makes the report independent of batch split and world size."""
    from raman_mi355x import engine
    nbins = 4
    per7, rows = _values(nbins)
    one = O.report_words(per7, rows, nbins)
    pick = np.random.default_rng(2).uniform(size=len(rows)) < 0.4
    two = O.report_words(per7[pick], rows[pick], nbins) + O.report_words(per7[~pick], rows[~pick], nbins)
    assert np.array_equal(one, two)
    a = engine.report_value(torch.from_numpy(one), nbins).numpy()
    b = engine.report_value(torch.from_numpy(two), nbins).numpy()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("lo,hi,nbins", [(20.0, 37.0, 17), (20.0, 37.0, 4), (0.0, 1.0, 64), (-3.5, 41.25, 7), (20.0, 37.0, 1),
                                         (0.1, 0.7, 3)])
def test_bin_formula_matches_the_float32_restatement(lo, hi, nbins):
    from raman_mi355x import engine
    f = np.float32
    lo32, hi32 = f(lo), f(hi)
    edge = {"lo": lo32, "hi": hi32, "below lo": np.nextafter(lo32, f(-np.inf)), "above lo": np.nextafter(lo32, f(np.inf)),
            "below hi": np.nextafter(hi32, f(-np.inf)), "above hi": np.nextafter(hi32, f(np.inf)), "nan": f(np.nan),
            "-inf": f(-np.inf), "+inf": f(np.inf)}
    want = {"lo": 1, "hi": nbins + 1, "below lo": 0, "above lo": 1, "below hi": nbins, "above hi": nbins + 1,
            "nan": nbins + 1, "-inf": 0, "+inf": nbins + 1}
    for name, k in edge.items():
        assert engine.report_bin(k, (lo, hi, nbins)) == want[name] == O.bin_rows([k], lo, hi, nbins)[0], name
    # interior edges and their neighbours, and random keys: the C formula and the numpy one agree bit for bit
    inner = (lo32 + (hi32 - lo32) * np.arange(nbins + 1, dtype=np.float32) / f(nbins)).astype(np.float32)
    keys = np.concatenate([inner, np.nextafter(inner, f(-np.inf)), np.nextafter(inner, f(np.inf)),
                           np.random.default_rng(nbins).uniform(lo - 3, hi + 3, 2000).astype(np.float32)])
    rows = O.bin_rows(keys, lo, hi, nbins)
    assert [engine.report_bin(k, (lo, hi, nbins)) for k in keys] == rows.tolist()
    assert rows.min() == 0 and rows.max() == nbins + 1 and len(set(rows.tolist())) == nbins + 2


def test_argument_errors(lib):
    fake = [ctypes.c_void_p((i + 1) << 32) for i in range(5)]        # addresses that are never read
    x, y, c, per, rep = fake

    def snr(x=x, y=y, c=c, f64=0, n=4, L=100, per=per, key=None, lo=20.0, hi=37.0, nbins=4, per4=None, rep=rep):
        return lib.rdn_snr(x, y, c, f64, n, L, per, key, lo, hi, nbins, per4, rep, None)

    for bad in (dict(nbins=0), dict(nbins=65), dict(hi=20.0), dict(hi=19.0), dict(lo=float("nan")),
                dict(lo=float("-inf")), dict(hi=float("inf")), dict(x=None), dict(y=None), dict(c=None), dict(L=0),
                dict(n=-1), dict(f64=2), dict(L=1 << 31), dict(per=None, rep=None), dict(rep=None, key=fake[0]),
                dict(rep=None, per4=fake[0])):
        assert snr(**bad) == -1, bad
        assert lib.rdn_last_error() != b""
    assert b"nbins" in (snr(nbins=65), lib.rdn_last_error())[1]
    # n = 0 launches nothing and accepts NULL data, but still checks the bins
    assert snr(n=0, x=None, y=None, c=None) == 0
    assert snr(n=0, x=None, y=None, c=None, nbins=0) == -1
    assert snr(n=0, rep=None, nbins=0) == 0                          # no report: the bins are not used
    row = ctypes.c_int()
    assert lib.rdn_report_bin(1.0, 2.0, 2.0, 4, ctypes.byref(row)) == -1
    assert lib.rdn_report_bin(1.0, 0.0, 2.0, 4, None) == -1
    out = (ctypes.c_double * 1)()
    assert lib.rdn_report_value(None, 4, out) == -1
    words = (ctypes.c_int64 * 1)()
    assert lib.rdn_report_value(words, 0, out) == -1 and lib.rdn_report_value(words, 65, out) == -1


def test_python_surface_refuses_what_the_kernel_cannot_take():
    import raman_mi355x as R
    from raman_mi355x import engine
    from raman_mi355x.evaluate import evaluate
    t = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.snr(t, t, t)
    for bad in ((20, 37, 0), (20, 37, 65), (37, 20, 4), (20, 20, 4), (20, float("inf"), 4), (20, 37, 2.5), (20, 37)):
        with pytest.raises(ValueError):
            engine._bins(bad)
    with pytest.raises(ValueError):
        engine.new_report(0, "cpu")
    assert engine.new_report(17, "cpu").shape == (19 * 51,)
    with pytest.raises(ValueError, match="words"):
        engine.report_value(torch.zeros(10, dtype=torch.int64), 4)
    # evaluate() is refused on a CPU device exactly as before, with or without snr_bins
    m = R.DenoiseCNN()
    z = np.zeros((2, 100))
    for kw in ({}, {"snr_bins": None}, {"snr_bins": (20, 37, 4)}):
        with pytest.raises(RuntimeError, match="runs its metrics on the GPU"):
            evaluate(m, z, z, device="cpu", **kw)


def test_summary_and_written_table(tmp_path):
    """snr_summary / write_snr_report on a hand-built report; write_metrics keeps its four lines."""
    from raman_mi355x.evaluate import snr_summary, write_metrics, write_snr_report
    nbins = 4
    per7, rows = _values(nbins)
    s = snr_summary(torch.from_numpy(O.report_words(per7, rows, nbins)), (20, 37, nbins))
    ref = O.report_sums(per7, rows, nbins)
    assert [e["count"] for e in s["by_snr"]] == ref[1:nbins + 1, 0].astype(int).tolist() and len(s["by_snr"]) == nbins
    assert (s["snr_under"]["count"], s["snr_over"]["count"]) == (ref[0, 0], ref[nbins + 1, 0])
    assert [(e["lo"], e["hi"]) for e in s["by_snr"]] == [(20 + 4.25 * b, 24.25 + 4.25 * b) for b in range(nbins)]
    for b, e in enumerate(s["by_snr"]):
        if e["count"] == 0:
            assert set(e) == {"lo", "hi", "count"}
            continue
        for k, name in enumerate(O.QUANTITIES):
            np.testing.assert_allclose(e[name], ref[1 + b, 1 + k] / e["count"], rtol=1e-12)
    for k, name in enumerate(O.QUANTITIES[4:]):
        np.testing.assert_allclose(s[name], ref[nbins + 2, 5 + k] / len(rows), rtol=1e-12)
    result = dict({"MSE": 1.0, "SSIM": 0.5, "Smoothness": 0.25, "Peak2Peak": 2.0}, **s)
    d = write_metrics(result, root=str(tmp_path))
    assert open(os.path.join(d, "metrics.txt")).read().splitlines() == ["MSE: 1.000000", "SSIM: 0.500000",
                                                                         "Smoothness: 0.250000", "Peak2Peak: 2.000000"]
    assert write_snr_report(result, d) == d
    back = json.load(open(os.path.join(d, "snr_report.json")))
    assert back["by_snr"] == s["by_snr"] and back["SNR_gain"] == s["SNR_gain"]
    table = open(os.path.join(d, "snr_report.txt")).read().splitlines()
    assert len(table) == 3 + 1 + nbins + 2 and table[3].split() == ["lo", "hi", "count"] + list(O.QUANTITIES)
    assert table[4 + 1 + 1].split()[2:] == ["0"] + ["-"] * 7          # the empty bin (report row 2)
    with pytest.raises(ValueError, match="snr_bins"):
        write_snr_report({"MSE": 1.0}, d)
