"""The device metrics (csrc/metrics.hpp spectrum_metrics: the standalone kernel and the walk kernels' epilogue)
against the exact-arithmetic arbiter (tests/metrics_exact.py) over their input domain, their non-finite
contract (include/raman_mi355x.h beside rdn_metrics) and the device half of the exact accumulator (to_limbs).

Bars, all against the arbiter (exact value rounded once), never against the device's other path:
  MSE, Smoothness   relative error <= (L + 4) 2^-53: any summation order of L non-negative terms, each
                    rounded once, then one division (and the arbiter's own rounding);
  Peak2Peak         bit-equal: one fp64 subtraction of two fp32 values;
  SSIM              per case, max over its spectra of the error <= 8 x the float64 oracle's max over the
                    same spectra + (64 + L/512 + 11) 2^-53.  64: about the rounded operations of one
                    window's S at condition number 1; L/512 + 11: the 512-way partial sums and the
                    reduction.  8: the kernel multiplies by a rounded 1/7 where the oracle divides (one more
                    rounding on each of the five means) and may contract multiply-adds; a numpy emulation
                    of the kernel's formula came to at most 3.1 x the oracle's case maximum, single spectra
                    scatter to 7 x, hence case maxima.  The error is relative, and absolute where the exact
                    SSIM is below 1e-9 in magnitude (rounding noise over the variance: a constant clean).
The families and the measured distances (oracle, device, ratio) are printed per case; DESIGN.md's parity
section holds the table.
"""
import numpy as np
import pytest
import torch

from conftest import golden_state_dict
from metrics_exact import (FAMILY_NAMES, _ratio, acc_words, exact_per_spectrum, exact_total, family_table, rel_err,
                           ssim_err)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _lib():
    from raman_mi355x import _lib
    return _lib


def _expected_acc(per):
    return acc_words(per)


def _oor(acc):
    """The four out-of-range words of an accumulator."""
    L = _lib()
    return [int(acc[k * L.ACC_STRIDE + L.ACC_LIMBS]) for k in range(4)]


def _truncated_sum(values):
    """What rdn_acc_value reports for in-range values: the exact sum of the values truncated toward zero
    at 2^-128, rounded once."""
    total = 0
    for v in values:
        n, d = float(v).as_integer_ratio()
        total += (abs(n) << 128) // d * (1 if n >= 0 else -1)
    return _ratio(total, 1 << 128)


def _gpu(y, clean, acc=True):
    """(per (n, 4), sums (5,), acc words list) of the standalone metrics kernel."""
    from raman_mi355x import engine
    yt, ct = torch.tensor(y).cuda(), torch.tensor(clean).cuda()          # copies: the shared tables are read-only
    a = engine.new_acc(yt.device) if acc else None
    per, sums = engine.metrics(yt, ct, acc=a)
    torch.cuda.synchronize()
    return per.cpu().numpy(), sums.cpu().numpy(), (a.cpu() if acc else None)


def _ssim_bar(orc, exact, L):
    return 8 * ssim_err(orc[:, 1], exact[:, 1]).max() + (64 + L / 512 + 11) * U


# ---- 2. device against the arbiter --------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_device_against_arbiter(name, f64):
    y, clean, exact, orc = family_table(f64)[name]
    n, L = y.shape
    per, sums, acc = _gpu(y, clean)
    e = rel_err(per, exact)
    dev, ora = ssim_err(per[:, 1], exact[:, 1]).max(), ssim_err(orc[:, 1], exact[:, 1]).max()
    print(f"\n| {name} | {L} | {'fp64' if f64 else 'fp32'} | {e[:, 0].max():.1e} | {e[:, 2].max():.1e} | {ora:.1e} | "
          f"{dev:.1e} | {dev / ora if ora else float('nan'):.2f} |")
    assert e[:, 0].max() <= (L + 4) * U, ("MSE", e[:, 0])
    assert e[:, 2].max() <= (L + 4) * U, ("Smoothness", e[:, 2])
    assert np.array_equal(per[:, 3], exact[:, 3]), ("Peak2Peak", per[:, 3], exact[:, 3])
    assert np.array_equal(np.isnan(per[:, 1]), np.isnan(exact[:, 1])), ("SSIM NaN", per[:, 1], exact[:, 1])
    assert dev <= _ssim_bar(orc, exact, L), ("SSIM", dev, ora, per[:, 1], exact[:, 1])
    if name == "anti-correlated":
        assert (exact[:, 1] < 0).all() and (per[:, 1] < 0).all()
    if name == "all zero":
        assert np.isnan(per[:, 1]).all()
    # the accumulator took exactly these values (negative SSIM and the NaN rows' out-of-range words included)
    assert acc.tolist() == _expected_acc(per)
    assert sums[4] == n
    fin = np.isfinite(exact).all(axis=0)
    for k in (0, 2, 3):
        tot = exact_total(exact[:, k])
        assert abs(sums[k] - tot) <= (n + 4) * U * tot, (k, sums[k], tot)
    assert np.isnan(sums[1]) == (not fin[1])


# ---- 3. non-finite values -----------------------------------------------------------------------------------
NF_L = 1100
NF_POS = (0, 64, 700, NF_L - 1)


def _nf_base(n):
    rng = np.random.default_rng(77)
    c = rng.uniform(0, 1, (n, NF_L)).astype(np.float32)
    return (c + rng.normal(0, 0.05, c.shape)).astype(np.float32), c


def _nf_case(kind):
    """(y, clean, rows that hold a non-finite value): finite rows before, between and after them."""
    if kind == "clean nan / all-nan y":
        y, c = _nf_base(4)
        c[1, 64] = np.nan
        y[2, :] = np.nan
        return y, c, [1, 2]
    y, c = _nf_base(7)
    bad = [1, 2, 4, 5]
    for r, p in zip(bad, NF_POS):
        if kind == "nan":
            y[r, p] = np.nan
        elif kind == "+inf":
            y[r, p] = np.inf
        else:
            y[r, p], y[r, (p + 300) % NF_L] = np.inf, -np.inf
    return y, c, bad


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("kind", ["nan", "+inf", "+inf and -inf", "clean nan / all-nan y"])
def test_nonfinite_rows(kind, f64):
    """per_spectrum has the arbiter's class per metric (NaN / +inf / -inf / the finite value), acc exactly the
    out-of-range counts and nothing in those values' limbs, rdn_acc_value NaN for them and the exact sum for
    the others, and the finite rows of the batch the bits they have alone."""
    from raman_mi355x import engine
    y, c, bad = _nf_case(kind)
    if f64:
        c = c.astype(np.float64) + 1e-9 * np.random.default_rng(5).uniform(0, 1, c.shape)
    n = len(y)
    good = [i for i in range(n) if i not in bad]
    exact = exact_per_spectrum(y, c)
    per, sums, acc = _gpu(y, c)
    print(f"\n{kind}: device\n{per[bad]}\narbiter\n{exact[bad]}")
    nonfin = ~np.isfinite(exact)
    assert nonfin[bad].any(axis=1).all() and not nonfin[good].any()
    assert np.array_equal(per[nonfin], exact[nonfin], equal_nan=True), (per[bad], exact[bad])
    assert np.isfinite(per[~nonfin]).all()
    e = rel_err(per, exact)                                   # 0 where the classes agree
    assert e[:, 0].max() <= (NF_L + 4) * U and e[:, 2].max() <= (NF_L + 4) * U, e
    assert np.array_equal(per[:, 3], exact[:, 3], equal_nan=True)
    if kind == "nan":
        assert np.isnan(per[bad]).all()                       # a NaN in y: all four metrics
    per_good, _, _ = _gpu(y[good], c[good], acc=False)
    assert np.array_equal(per[good].view(np.int64), per_good.view(np.int64))
    assert _oor(acc) == nonfin.sum(axis=0).tolist()
    assert acc.tolist() == _expected_acc(per)
    val = engine.acc_value(acc).numpy()
    for k in range(4):
        if nonfin[:, k].any():
            assert np.isnan(val[k]) and not np.isfinite(sums[k]), (k, val, sums)
        else:
            assert val[k] == _truncated_sum(per[:, k]), (k, val[k])
    assert val[4] == n


def test_nan_peak2peak_reaches_the_snr_report():
    """Downstream: a spectrum with a NaN Peak2Peak raises the Peak2Peak out-of-range word of its report row."""
    from raman_mi355x import engine
    L_ = _lib()
    y, c, bad = _nf_case("nan")
    n = len(y)
    yt, ct = torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda()
    per, _ = engine.metrics(yt, ct)
    bins = (20.0, 20.0 + n, n)
    key = torch.arange(n, dtype=torch.float32, device="cuda") + 20.5
    _, report = engine.snr(ct, yt, ct, key=key, bins=bins, per4=per)
    rep = report.cpu().view(-1, L_.REPORT_ROW_WORDS)
    for i in range(n):
        row = engine.report_bin(20.5 + i, bins)
        assert row == 1 + i
        assert int(rep[row, 3 * L_.ACC_STRIDE + L_.ACC_LIMBS]) == (1 if i in bad else 0), i
        assert int(rep[row, L_.REPORT_COUNT4]) == 1
    vals = engine.report_value(report, n).numpy()
    assert np.isnan(vals[-1, 4]) and all(np.isnan(vals[1 + i, 4]) == (i in bad) for i in range(n))


def _saturating_model(dtype):
    """test_range_gpu.py test_walk_saturation_nans_rest_of_spectrum's recipe: the right branch's convs x 1.55."""
    import raman_mi355x as R
    sd = {k: v.clone() for k, v in golden_state_dict("RRCDNet", "synth").items()}
    for k in sd:
        if k.startswith("right_net.") and k.endswith(".0.weight") and sd[k].shape[1] == 64:
            sd[k] *= 1.55
    m = R.RRCDNet()
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval().set_engine_dtype(dtype)


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("dtype", ["f16", "f16-plain"])
def test_epilogue_meters_nonfinite_y_like_the_metrics_kernel(dtype, f64, monkeypatch):
    """Saturated spectra through the walk kernels' metric epilogue (built with -fno-honor-nans): per-spectrum
    values NaN-equal and acc word-equal to the standalone kernel on the same y.  'f16' is
    rrcdnet_hybrid_walk, whose saturated tiles NaN the rest of their spectra: those spectra have four NaN
    metrics and the status word still reports RangeError.  'f16-plain' runs the same weights on the fused16
    walk (the other LDS size and translation unit, no range bit): whatever y comes out is metered alike
    (measured: y stays finite there and the status word 0, so a NaN in clean is what brings non-finite values
    into that kernel's epilogue, below)."""
    from raman_mi355x import _lib as L_, engine
    monkeypatch.setenv("RDN_WALK", "1")
    monkeypatch.setenv("RDN_SHORT_TILES", "0")
    m = _saturating_model(dtype)
    n, L = 4, 6000
    p = np.arange(L, dtype=np.float32) / L
    x = np.zeros((n, L), np.float32)
    x[0] = 0.05 * np.sin(p * 40)                      # stays in range
    x[1] = 1.25 * p                                   # ramp: saturates part-way along
    x[2] = 1.25 * p[::-1]                             # ramp down: saturates from the first tiles
    x[3] = 0.5 + 0.0 * p                              # stays in range
    xs = torch.from_numpy(x).unsqueeze(1).cuda()
    clean = torch.from_numpy(x.astype(np.float64) + 1e-9 * p if f64 else x).cuda()
    ws = engine.Workspace("RRCDNet", m.engine_code, n, L, xs.device)
    acc1 = engine.new_acc(xs.device)
    y, per1, sums1, fused = engine.forward_metrics("RRCDNet", m.engine_code, m.packed_weights(xs.device), xs, clean,
                                                   per_spectrum=True, acc=acc1, check=False, workspace=ws)
    torch.cuda.synchronize()
    assert fused
    acc0 = engine.new_acc(xs.device)
    per0, sums0 = engine.metrics(y.view(n, L), clean, acc=acc0)
    per0, per1 = per0.cpu().numpy(), per1.cpu().numpy()
    bad = ~np.isfinite(y.view(n, L).cpu().numpy())
    print(f"\n{dtype}: non-finite y values per spectrum {bad.sum(axis=1).tolist()}, NaN {np.isnan(y.cpu().numpy()).sum()}\n"
          f"epilogue\n{per1}\nkernel\n{per0}")
    assert np.array_equal(per1, per0, equal_nan=True)
    assert np.array_equal(per1[np.isfinite(per1)].view(np.int64), per0[np.isfinite(per0)].view(np.int64))
    assert torch.equal(acc0, acc1), (acc0.tolist(), acc1.tolist())
    assert acc1.cpu().tolist() == _expected_acc(per1)
    assert np.array_equal(np.isnan(sums1.cpu().numpy()), np.isnan(sums0.cpu().numpy()))
    nan_rows = np.isnan(y.view(n, L).cpu().numpy()).any(axis=1)
    assert np.isnan(per1[nan_rows]).all() and np.isfinite(per1[~bad.any(axis=1)]).all()
    if dtype == "f16":
        assert nan_rows.tolist() == [False, True, True, False]
        assert _oor(acc1.cpu()) == [2, 2, 2, 2]
        with pytest.raises(L_.RangeError):
            ws.check()
    else:
        print(f"f16-plain status flags {ws.check():#x}")
    # a NaN in clean (a caller's input, so it reaches either kernel's epilogue whatever y is): the data range,
    # hence SSIM, and MSE are NaN; Smoothness and Peak2Peak of the finite rows keep their bits
    cn = clean.clone()
    cn[0, 64] = cn[3, L - 1] = float("nan")
    acc3 = engine.new_acc(xs.device)
    y3, per3, _, fused = engine.forward_metrics("RRCDNet", m.engine_code, m.packed_weights(xs.device), xs, cn,
                                                per_spectrum=True, acc=acc3, check=False, workspace=ws)
    acc2 = engine.new_acc(xs.device)
    per2, _ = engine.metrics(y3.view(n, L), cn, acc=acc2)
    per2, per3 = per2.cpu().numpy(), per3.cpu().numpy()
    assert fused and torch.equal(y3.view(torch.int32), y.view(torch.int32))    # NaN and all
    assert np.array_equal(per3, per2, equal_nan=True) and torch.equal(acc2, acc3)
    for r in (0, 3):
        assert np.isnan(per3[r, :2]).all() and np.array_equal(per3[r, 2:], per1[r, 2:]), per3[r]
    assert np.array_equal(per3[1:3], per1[1:3], equal_nan=True)


# ---- 4. the device accumulator over its domain -------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


ACC_V = [0.0, 2.0 ** -149, 2.0 ** -140, 2.0 ** -128 - 2.0 ** -149, 2.0 ** -128, 2.0 ** -128 * (1 + 2.0 ** -10),
         2.0 ** -126, 1.0, -1.0, 2.0 ** 32 - 2.0 ** 9, 2.0 ** 32 + 2.0 ** 9, 2.0 ** 64 - 2.0 ** 40, 2.0 ** 64, float(np.float32(3e38)),
         float("inf")]
ACC_K = [-149, -75, -63, -62, 0, 16, 33, 34, 63, 127]     # MSE = 2^(2k - 3): 2^-129 is truncated away, 2^65 out of range


def _acc_rows():
    """L = 8, clean zero.  Rows y[0] = v: Peak2Peak = |v|, MSE = v^2 / 8, Smoothness = |v| / 7.  Rows
    y[3] = 2^k: MSE = 2^(2k) / 8, Smoothness = 2^(k+1) / 7, Peak2Peak = 2^k.  SSIM is NaN in the first kind
    (window 1 is all zero: 0/0) and 0 in the second (both windows hold the value)."""
    rows = []
    for v in ACC_V:
        assert _f32(v) == v                                   # every value is an fp32
        r = np.zeros(8, np.float32)
        r[0] = v
        rows.append(r)
    for k in ACC_K:
        r = np.zeros(8, np.float32)
        r[3] = 2.0 ** k
        rows.append(r)
    return np.stack(rows)


def test_accumulator_over_its_domain():
    """to_limbs on the device: zero, fp32 subnormals (they arrive as their values, not flushed), the
    truncation at 2^-128, the 2^64 limit, finite values beyond it and inf.  Every row's metrics are exact in
    fp64 (one or two non-zero terms), so per_spectrum is the arbiter's bits and every word of acc -- limbs,
    out-of-range counts, spectrum count -- is the host restatement's applied to the arbiter's values."""
    from raman_mi355x import engine
    y = _acc_rows()
    c = np.zeros_like(y)
    exact = exact_per_spectrum(y, c)
    assert exact[1, 3] == 2.0 ** -149 and exact[1, 0] == 2.0 ** -301 and exact[len(ACC_V), 0] == 2.0 ** -301
    for f64 in (False, True):
        cc = c.astype(np.float64) if f64 else c
        per, sums, acc = _gpu(y, cc)
        assert np.array_equal(per, exact, equal_nan=True), (per, exact)     # subnormals included
        assert acc.tolist() == _expected_acc(exact)
        inr = np.abs(y).max(axis=1) <= 2.0 ** 32 + 2.0 ** 9                   # all four metrics in range or NaN
        per_i, sums_i, acc_i = _gpu(y[inr], cc[inr])
        assert acc_i.tolist() == _expected_acc(exact[inr])
        assert _oor(acc_i) == [0, len(ACC_V) - 4, 0, 0]                       # SSIM: the in-range y[0] = v rows
        val = engine.acc_value(acc_i).numpy()
        assert np.isnan(val[1]) and val[4] == inr.sum()
        for k in (0, 2, 3):
            assert val[k] == _truncated_sum(exact[inr, k]), (k, val[k])
            tot = exact_total(exact[inr, k])
            assert abs(sums_i[k] - tot) <= (inr.sum() + 4) * U * tot, (k, sums_i[k], tot)
        val = engine.acc_value(acc).numpy()
        assert np.isnan(val[:4]).all() and val[4] == len(y)
        assert _oor(acc) == [4 + 3, len(ACC_V), 2 + 1, 3 + 1]   # e.g. Peak2Peak: 2^64, 3e38, inf and 2^127


def test_accumulator_contention_and_split():
    """2000 spectra of L = 8 into one accumulator in one launch, then split 1 / 1999: the same words, equal to
    the integer sums.  y and clean are one-hot at different positions, so MSE, Smoothness and Peak2Peak are
    exact in fp64 (the arbiter's bits); SSIM is finite, of both signs, and held to the arbiter at the SSIM bar."""
    from oracle.metrics import per_spectrum
    from raman_mi355x import engine
    n, L = 2000, 8
    rng = np.random.default_rng(2000)
    y, c = np.zeros((n, L), np.float32), np.zeros((n, L), np.float32)
    i = np.arange(n)
    mag = lambda: (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-60, 31, n)).astype(np.float32)
    y[i, 1 + i % 6] = mag() * rng.choice([-1.0, 1.0], n).astype(np.float32)
    c[i, 1 + (i + 1 + i // 6 % 5) % 6] = mag()
    exact = exact_per_spectrum(y, c)
    per, sums, acc = _gpu(y, c)
    assert np.array_equal(per[:, [0, 2, 3]], exact[:, [0, 2, 3]])
    orc = per_spectrum(y, c)
    dev, ora = ssim_err(per[:, 1], exact[:, 1]).max(), ssim_err(orc[:, 1], exact[:, 1]).max()
    print(f"\nL = 8 one-hot pairs: SSIM in [{exact[:, 1].min():.3g}, {exact[:, 1].max():.3g}], oracle {ora:.1e}, "
          f"device {dev:.1e}")
    assert dev <= _ssim_bar(orc, exact, L)
    mixed = exact.copy()
    mixed[:, 1] = per[:, 1]                                   # SSIM's limbs are of the device's own values
    want = _expected_acc(mixed)
    assert acc.tolist() == want and _oor(acc) == [0, 0, 0, 0]
    yt, ct = torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda()
    acc2 = engine.new_acc(yt.device)
    engine.metrics(yt[:1], ct[:1], acc=acc2, per_spectrum=False)
    engine.metrics(yt[1:], ct[1:], acc=acc2, per_spectrum=False)
    assert acc2.cpu().tolist() == want
    val = engine.acc_value(acc).numpy()
    for k in range(4):
        assert val[k] == _truncated_sum(mixed[:, k]), k
    for k in (0, 2, 3):
        tot = exact_total(exact[:, k])
        assert abs(sums[k] - tot) <= (n + 4) * U * tot, (k, sums[k], tot)
    assert abs(sums[1] - exact_total(per[:, 1])) <= (n + 4) * U * np.abs(per[:, 1]).sum()
    assert sums[4] == n
