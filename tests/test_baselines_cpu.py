"""The classical baseline filters without a device: the ABI's argument checks, the coefficient builders, the
numpy oracle (tests/baselines_oracle.py) and the modules' eager path against scipy's outputs
(tests/golden/baselines.npz, make_baselines_golden.py), and write_comparison.

Bars against the goldens.  The oracle's sequential fp64 sum and scipy's own float64 filters differ by at most
about 1e-12 (w products of at most a few units, each summed with 2^-53 relative error, and scipy's different
order); rounding both to fp32 then lands on the same value or -- where the float64 values straddle a rounding
boundary, which piecewise-constant data makes common -- on neighbours: <= 1 fp32 ulp.  The median picks an
input sample: equal bits."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import baselines_oracle as O
from baselines_oracle import G, check_against_golden, golden_cases, oracle_of
from conftest import GOLDEN

LENGTHS = (21, 22, 255, 256, 1000)
SAVGOL = ((3, 0), (5, 2), (21, 3), (21, 0), (11, 5), (255, 3))


def test_fixture_is_what_the_issue_lists():
    assert all(G[f"x_{L}"].shape == (3, L) and G[f"x_{L}"].dtype == np.float32 for L in LENGTHS)
    want = {f"x_{L}" for L in LENGTHS}
    for L in LENGTHS:
        want |= {f"savgol_{w}_{p}_{m}_{L}" for w, p in SAVGOL if w <= L for m in ("interp", "mirror")}
        want |= {f"uniform_9_{L}", f"gauss_1.0_{L}", f"gauss_2.5_{L}"}
        want |= {f"median_{w}_{L}" for w in (3, 21, 101) if w <= L}
    assert set(G.files) == want
    assert os.path.getsize(os.path.join(GOLDEN, "baselines.npz")) < 1_000_000


def test_abi_symbols_version_and_constants():
    from raman_mi355x import _lib, engine
    lib = _lib.lib()
    assert hasattr(lib, "rdn_fir") and hasattr(lib, "rdn_median") and lib.rdn_version() == 6
    assert {"rdn_fir", "rdn_median"} <= set(_lib.EXPORTED)
    with open(_lib.HEADER) as fh:
        header = fh.read()
    consts = dict(re.findall(r"^#define (RDN_FILTER_\w+) (\d+)", header, re.M))
    assert int(consts["RDN_FILTER_MAX_WINDOW"]) == _lib.FILTER_MAX_WINDOW == engine.FILTER_MAX_WINDOW == 255
    assert int(consts["RDN_FILTER_TILE"]) == _lib.FILTER_TILE == engine.FILTER_TILE


def test_argument_checks_need_no_device():
    """Every RDN_EINVAL case of rdn_fir / rdn_median, for n = 0 too, through ctypes with host pointers: the
    checks come before any device call (this test runs without a GPU)."""
    from raman_mi355x import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 128)()
    taps = (ctypes.c_double * 256)()
    base = ctypes.addressof(buf)
    x, y, t = base, base + 64 * 4, ctypes.addressof(taps)
    EINVAL = -1                                                                # RDN_EINVAL

    def fir(x=x, y=y, n=1, L=16, t=t, w=5):
        return lib.rdn_fir(x, y, n, L, t, w, None, None)

    def med(x=x, y=y, n=1, L=16, w=5):
        return lib.rdn_median(x, y, n, L, w, None)

    for n in (1, 0):
        assert fir(n=n, t=None) == EINVAL                                      # a null pointer
        assert b"null" in lib.rdn_last_error()
        for call in (fir, med):
            for w in (4, 0, -1, 256, 257):                                     # even, < 1, > 255
                assert call(n=n, L=1000 if w > 16 else 16, w=w) == EINVAL, (call.__name__, n, w)
            assert call(n=n, L=4) == EINVAL                                    # L < w
            assert call(n=n, L=2 ** 31) == EINVAL                              # L >= 2^31
            assert call(n=-1) == EINVAL
    for call in (fir, med):
        assert call(x=None) == EINVAL and call(y=None) == EINVAL
        assert call(y=x) == EINVAL and call(y=x + 15 * 4) == EINVAL            # x and y overlapping
        assert b"overlap" in lib.rdn_last_error()
        assert call(x=y, y=x + 49 * 4) == EINVAL                               # ... from the other side
        # n = 0 launches nothing and accepts NULL data pointers
        assert call(x=None, y=None, n=0) == _lib.RDN_OK
        assert call(x=None, y=None, n=0, L=2 ** 31 - 1, w=255) == _lib.RDN_OK


def test_engine_refuses_host_and_malformed_inputs():
    from raman_mi355x import engine
    x = torch.zeros(2, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.fir(x, np.full(3, 1 / 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.median(x, 3)


@pytest.mark.parametrize("w,p", SAVGOL + ((1, 0), (7, 5)))
def test_savgol_taps_match_scipy(w, p):
    """The centre taps against scipy's (which solves on the unscaled abscissa: beyond these cases, e.g. at
    (101, 4), scipy itself is 3e-11 from the exact rational solution that the next test compares with)."""
    sig = pytest.importorskip("scipy.signal")
    from raman_mi355x.baselines import savgol_taps
    taps, edge = savgol_taps(w, p)
    h = (w - 1) // 2
    assert taps.dtype == np.float64 and taps.shape == (w,) and edge.shape == (w - 1, w)
    np.testing.assert_allclose(taps, sig.savgol_coeffs(w, p, use="dot"), rtol=0, atol=1e-12)
    assert h == 0 or abs(taps.sum() - 1) <= 1e-14 and np.abs(edge.sum(axis=1) - 1).max() <= 1e-13   # constants pass


@pytest.mark.parametrize("w,p", ((3, 0), (5, 2), (21, 3), (21, 0), (11, 5), (7, 5), (41, 4)))
def test_savgol_edge_rows_match_exact_least_squares(w, p):
    """Row i of [edge_taps[:h], taps, edge_taps[h:]] evaluates the window's least-squares polynomial at
    position i: v_i^T (A^T A)^-1 A^T, here in exact rational arithmetic on the integer abscissa.  (scipy's
    savgol_coeffs(pos=i) solves the same system unscaled in float64 and is itself 1e-11 off at (11, 5), so it
    is no reference for 1e-12 away from the centre; the goldens hold the edges end to end.)"""
    from fractions import Fraction
    from raman_mi355x.baselines import savgol_taps
    h, n = (w - 1) // 2, p + 1
    A = [[Fraction(k - h) ** q for q in range(n)] for k in range(w)]
    M = [[sum(A[k][a] * A[k][b] for k in range(w)) for b in range(n)] + [Fraction(int(a == b)) for b in range(n)]
         for a in range(n)]
    for c in range(n):                                                # Gauss-Jordan: M = [I | (A^T A)^-1]
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    inv = [row[n:] for row in M]
    rows = np.array([[float(sum(A[i][a] * inv[a][b] * A[k][b] for a in range(n) for b in range(n))) for k in range(w)]
                     for i in range(w)])
    taps, edge = savgol_taps(w, p)
    np.testing.assert_allclose(np.concatenate([edge[:h], taps[None], edge[h:]]), rows, rtol=0, atol=1e-12)


@pytest.mark.parametrize("sigma,truncate", [(1.0, 4.0), (2.5, 4.0), (0.3, 4.0), (7.0, 3.0), (31.0, 4.0)])
def test_gaussian_taps_match_scipy(sigma, truncate):
    ndi = pytest.importorskip("scipy.ndimage")
    from raman_mi355x.baselines import gaussian_taps
    taps = gaussian_taps(sigma, truncate)
    r = int(truncate * sigma + 0.5)
    assert taps.shape == (2 * r + 1,) and abs(taps.sum() - 1) <= 1e-15
    impulse = np.zeros(4 * r + 3)
    impulse[2 * r + 1] = 1.0                                         # scipy's kernel as its impulse response
    got = ndi.gaussian_filter1d(impulse, sigma, truncate=truncate, mode="constant")[r + 1:3 * r + 2]
    np.testing.assert_allclose(taps, got, rtol=0, atol=1e-12)


def test_builders_refuse_bad_arguments():
    from raman_mi355x import baselines as B
    for bad in ((4, 2), (5, 5), (5, 6), (257, 3), (0, 0), (5, -1), (5.5, 2)):
        with pytest.raises(ValueError):
            B.savgol_taps(*bad)
    for bad in ((0.0, 4.0), (-1.0, 4.0), (float("nan"), 4.0), (40.0, 4.0)):
        with pytest.raises(ValueError):
            B.gaussian_taps(*bad)
    for cls, args in ((B.MovingAverage, (4,)), (B.MedianFilter, (0,)), (B.MedianFilter, (257,)), (B.MedianFilter, (True,)),
                      (B.SavitzkyGolay, (5, 2, "nearest"))):
        with pytest.raises(ValueError):
            cls(*args)


@pytest.mark.parametrize("key", [k for k in G.files if not k.startswith("x_")])
def test_oracle_and_eager_module_match_golden(key):
    _, x, make = next(c for c in golden_cases() if c[0] == key)
    m = make()
    ref = oracle_of(m, x)
    check_against_golden(key, ref)
    with torch.no_grad():
        y = m(torch.from_numpy(x).unsqueeze(1))
    assert y.shape == (3, 1, x.shape[1]) and y.dtype == torch.float32
    y = y.squeeze(1).numpy()
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))            # the eager path is the contract too
    check_against_golden(key, y)


def test_modules_have_no_state_and_move_with_to():
    from raman_mi355x import baselines as B
    mods = [B.MovingAverage(5), B.SavitzkyGolay(21, 3), B.SavitzkyGolay(21, 3, "mirror"), B.GaussianSmooth(1.0),
            B.MedianFilter(3)]
    for m in mods:
        assert len(m.state_dict()) == 0 and list(m.parameters()) == []
        m.load_state_dict({}, strict=True)
        assert not m.uses_engine(torch.zeros(1, 1, 64)) and m.window % 2 == 1
    sg = mods[1]
    assert sg.taps.dtype == torch.float64 and tuple(sg.edge_taps.shape) == (20, 21) and mods[2].edge_taps is None
    assert {n for n, _ in sg.named_buffers()} == {"taps", "edge_taps"}
    assert sg.to("meta").taps.device.type == "meta"                           # .to(device) moves the buffers
    with pytest.raises(TypeError, match="float64"):
        B.MovingAverage(3).float()(torch.zeros(1, 1, 8))
    # training mode changes nothing; the eager path carries a gradient
    x = torch.linspace(0, 1, 40).reshape(1, 1, 40).requires_grad_()
    for m in (B.MovingAverage(5).train(), B.MedianFilter(5).train()):
        y = m(x)
        y.sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all() and abs(float(x.grad.sum()) - 40) < 1e-5
        x.grad = None


def test_eager_special_values_match_oracle():
    """NaN, the infinities, signed zeros and subnormals through the eager path: the oracle's bits (a NaN
    compares as a NaN, whatever its payload)."""
    from raman_mi355x import baselines as B
    x = np.linspace(-1, 1, 64, dtype=np.float32).reshape(1, 64).repeat(2, 0)
    x[0, 10], x[0, 30], x[0, 31], x[0, 50] = np.nan, np.inf, -np.inf, 1e-41
    x[1, 19:25] = [0.5, -0.0, 0.0, -0.0, -0.0, 0.5]
    x[1, 40] = -1e-45
    for m in (B.MedianFilter(3), B.MedianFilter(9), B.MovingAverage(3), B.SavitzkyGolay(7, 2)):
        ref = oracle_of(m, x)
        with torch.no_grad():
            y = m(torch.from_numpy(x).unsqueeze(1)).squeeze(1).numpy()
        assert np.array_equal(np.isnan(y), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.array_equal(y.view(np.uint32)[ok], ref.view(np.uint32)[ok])
    med = O.median(x, 3)
    assert np.array_equal(np.flatnonzero(np.isnan(med[0])), [9, 10, 11])       # exactly the windows that hold it
    assert med.view(np.uint32)[0, 10] == 0x7FC00000
    assert np.signbit(med[1, 21]) and not np.signbit(med[1, 20]) and np.signbit(med[1, 22])    # -0 < +0


def test_registry_and_exports():
    import raman_mi355x as R
    from raman_mi355x import baselines as B
    assert R.BASELINES is B.BASELINES
    assert B.BASELINES == {"MovingAverage": B.MovingAverage, "SavitzkyGolay": B.SavitzkyGolay,
                           "GaussianSmooth": B.GaussianSmooth, "MedianFilter": B.MedianFilter}
    assert not set(B.BASELINES) & set(R.MODELS)
    for name in ("BASELINES", "MovingAverage", "SavitzkyGolay", "GaussianSmooth", "MedianFilter", "savgol_taps",
                 "gaussian_taps", "write_comparison"):
        assert name in R.__all__ and hasattr(R, name), name
    assert isinstance(B.BASELINES["MedianFilter"](3), torch.nn.Module)


def test_write_comparison(tmp_path):
    from raman_mi355x.evaluate import KEYS, write_comparison
    means = {k: 0.1 * (i + 1) for i, k in enumerate(KEYS)}
    synthetic = {"cnn": {"means": means, "acc": [0], "spectra": 4, "seconds": 1.0, "spectra_per_s": 4.0,
                         "SNR_in": 28.5, "SNR_out": 27.0, "SNR_gain": -1.5, "by_snr": [], "report": [0]},
                 "med3": {"means": dict(means, MSE=0.05), "acc": [0], "spectra": 4, "seconds": 1.0, "spectra_per_s": 4.0}}
    root = write_comparison(synthetic, str(tmp_path / "a"))
    table = json.load(open(os.path.join(root, "comparison.json")))
    assert list(table) == ["cnn", "med3"]
    assert table["cnn"] == dict(means, SNR_in=28.5, SNR_out=27.0, SNR_gain=-1.5) and table["med3"] == dict(means, MSE=0.05)
    lines = open(os.path.join(root, "comparison.txt")).read().splitlines()
    assert lines[0].split() == ["model", *KEYS, "SNR_in", "SNR_out", "SNR_gain"] and len(lines) == 3
    assert lines[1].split()[0] == "cnn" and float(lines[1].split()[-1]) == -1.5 and lines[2].split()[-3:] == ["-"] * 3
    # a dict name -> evaluate() result (the means at the top level)
    root = write_comparison({"net": dict(means, SNR_in=1.0, SNR_out=2.0, SNR_gain=1.0, by_snr=[]), "flt": dict(means)},
                            str(tmp_path / "b"))
    table = json.load(open(os.path.join(root, "comparison.json")))
    assert table["flt"] == means and table["net"]["SNR_gain"] == 1.0
