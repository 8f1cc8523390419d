"""PhysicsAwareLoss gradient, the parts that need no GPU: the entry point exists (ABI v6, detected by
symbol), argument checking, the numpy oracle (tests/physics_grad_oracle.py) against the reference class's
recorded autograd (tests/golden/physics_grad.npz, make_physics_grad_golden.py), and the
PhysicsAwareLoss(fused_backward=True) module on CPU tensors, where it is the eager path."""
import ctypes
import os

import numpy as np
import pytest
import torch

import physics_grad_oracle as G
from conftest import GOLDEN


@pytest.fixture(scope="module")
def lib():
    from raman_mi355x import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    d = dict(np.load(os.path.join(GOLDEN, "physics.npz")))
    d.update({"g_" + k: v for k, v in np.load(os.path.join(GOLDEN, "physics_grad.npz")).items()})
    return d


def test_entry_point_present_without_a_version_bump(lib):
    from raman_mi355x import _lib, engine
    assert hasattr(lib, "rdn_physics_grad") and "rdn_physics_grad" in _lib.EXPORTED
    assert lib.rdn_version() == 6 and _lib.ABI_VERSION == 6
    assert callable(engine.physics_grad)


def test_argument_errors_need_no_device(lib):
    fake = [ctypes.c_void_p((i + 1) << 32) for i in range(5)]        # addresses that are never read
    x, y, c, per, g = fake
    nan, inf = float("nan"), float("inf")

    def grad(x=x, y=y, c=c, f64=0, n=4, L=100, w=(0.1, 0.05, 0.01), scale=0.25, per=per, g=g):
        return lib.rdn_physics_grad(x, y, c, f64, n, L, w[0], w[1], w[2], scale, per, g, None)

    bad = [dict(L=2), dict(L=0), dict(L=1 << 31), dict(n=-1), dict(f64=2), dict(y=None), dict(c=None), dict(g=None),
           dict(x=None)]                                              # NULL x with a per_spectrum6
    for v in (nan, inf, -inf):
        bad += [dict(w=(v, 0.05, 0.01)), dict(w=(0.1, v, 0.01)), dict(w=(0.1, 0.05, v)), dict(scale=v)]
    # grad overlapping each of x, y and clean: the same address, its last element on their first, and the reverse
    rows = 4 * 100
    for name, a, elt in (("x", x, 4), ("y", y, 4), ("c", c, 4), ("c", c, 8)):
        f64 = {"f64": 1} if elt == 8 else {}
        bad += [dict(g=a, **f64), dict(g=ctypes.c_void_p(a.value - rows * 4 + 4), **f64),
                dict(g=ctypes.c_void_p(a.value + rows * elt - 4), **f64)]
    for kw in bad:
        assert grad(**kw) == -1, kw
        assert lib.rdn_last_error() != b"", kw
    assert b"L" in (grad(L=2), lib.rdn_last_error())[1]
    assert b"overlap" in (grad(g=y), lib.rdn_last_error())[1]
    # fp64 clean is twice as long: a grad that starts where an fp32 clean would end overlaps it
    assert b"overlap" in (grad(g=ctypes.c_void_p(c.value + rows * 4), f64=1), lib.rdn_last_error())[1]
    # n = 0 launches nothing and accepts NULL data, but still checks L, the weights and scale
    none = dict(n=0, x=None, y=None, c=None, per=None, g=None)
    assert grad(**none) == 0
    assert grad(**none, L=3) == 0
    assert grad(**none, L=2) == -1
    assert grad(**none, w=(0.1, nan, 0.01)) == -1
    assert grad(**none, scale=inf) == -1


def test_oracle_meets_the_bar_against_every_recorded_float64_gradient(gold):
    pred, clean = gold["pred"], gold["clean"]
    w = tuple(gold["g_weights"])
    assert w == (0.3, 0.7, 2.0) and gold["g_grad64"].shape == pred.shape == (8, 2000)
    cases = [("default", pred, clean, G.WEIGHTS, gold["g_grad64"]), ("weights", pred, clean, w, gold["g_grad64_w"]),
             ("clean64", pred[:2], gold["clean64"], G.WEIGHTS, gold["g_grad64_clean64"])]
    cases += [(f"L{L}", pred[:3, :L], clean[:3, :L], G.WEIGHTS, gold[f"g_grad64_L{L}"]) for L in (3, 4, 7)]
    for name, p, c, wt, ref in cases:
        assert ref.dtype == np.float64 and ref.shape == p.shape and np.abs(ref).max() > 0, name
        print(name, end=": ")
        G.assert_meets_bar(G.physics_grad(p, c, wt), ref, G.magnitude(p, c, wt))
    # the two weightings differ far beyond the bar: a mis-weighted term fails it
    assert np.abs(gold["g_grad64_w"] - gold["g_grad64"]).max() > 1e-3 * np.abs(gold["g_grad64"]).max()
    # the recorded gradient of the first fixture (two spectra cut to 64 samples) as well
    ref = gold["grad64"]
    G.assert_meets_bar(G.physics_grad(pred[:2, :64], clean[:2, :64]), ref, G.magnitude(pred[:2, :64], clean[:2, :64]))


def test_oracle_rounds_to_the_references_fp32_on_the_whole_batch(gold):
    got = G.physics_grad(gold["pred"], gold["clean"])
    assert np.array_equal(got.astype(np.float32), gold["g_grad64"].astype(np.float32))
    # the reference's own float32 run is within the recorded distance of its float64 run
    assert gold["g_grad32"].dtype == np.float32
    assert np.abs(gold["g_grad32"].astype(np.float64) - gold["g_grad64"]).max() == gold["g_d32"] < 1e-9


def test_oracle_non_finite_positions_equal_the_references(gold):
    pp, at, ref = gold["g_planted_pred"], gold["g_planted_at"], gold["g_planted_grad64"]
    assert pp.shape == ref.shape == (2, 64) and at.tolist()[3:] == [[1, 0], [1, 63]]
    planted = [pp[r, i] for r, i in at]
    assert np.isnan(planted[0]) and planted[1] == np.inf and np.isnan(planted[2]) and planted[3] == -np.inf and planted[4] == np.inf
    mask = G.peak_mask(gold["clean"][:2, :64])
    assert not mask[0, at[0, 1] - 1] and not mask[0, at[1, 1] - 1] and mask[1, at[2, 1] - 1]
    # the reference: NaN where a NaN was planted and at the unmasked +inf (0 * inf), -inf / +inf at the row's ends
    bad = np.argwhere(~np.isfinite(ref)).tolist()
    assert sorted(bad) == sorted(at.tolist())
    assert np.isnan(ref[0, at[0, 1]]) and np.isnan(ref[0, at[1, 1]]) and np.isnan(ref[1, at[2, 1]])
    assert ref[1, 0] == -np.inf and ref[1, 63] == np.inf
    got = G.physics_grad(pp, gold["clean"][:2, :64])
    G.assert_same_nonfinite(got, ref)
    G.assert_meets_bar(got, ref, G.magnitude(pp, gold["clean"][:2, :64]))


def _t(a, dt=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dt).unsqueeze(1)


def test_module_with_fused_backward_is_the_eager_path_on_cpu_tensors(gold):
    from raman_mi355x import PhysicsAwareLoss
    plain, fused = PhysicsAwareLoss(), PhysicsAwareLoss(fused_backward=True)
    assert plain.fused_backward is False and fused.fused_backward is True
    assert (fused.alpha, fused.beta, fused.gamma) == (0.1, 0.05, 0.01)
    w = PhysicsAwareLoss(0.3, 0.7, 2.0, True)
    assert (w.alpha, w.beta, w.gamma, w.fused_backward) == (0.3, 0.7, 2.0, True)
    clean, noisy = _t(gold["clean"]), _t(gold["noisy"])
    res = []
    for crit in (plain, fused):
        pred = _t(gold["pred"]).requires_grad_(True)
        assert not crit.uses_fused_backward(pred, clean, noisy) and not crit.uses_engine(pred, clean, noisy)
        loss = crit(pred, clean, noisy)
        loss.backward()
        res.append((loss.detach(), pred.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0
    # uses_engine answers as it always has: never on CPU tensors, with or without a gradient
    pred = _t(gold["pred"])
    with torch.no_grad():
        for crit in (plain, fused):
            assert not crit.uses_engine(pred, clean, noisy) and not crit.uses_fused_backward(pred, clean, noisy)
            assert torch.equal(crit(pred, clean, noisy), res[0][0])
    # the float64 eager gradient of the fused module is the reference's recorded one
    p64 = _t(gold["pred"], torch.float64).requires_grad_(True)
    fused(p64, _t(gold["clean"], torch.float64), _t(gold["noisy"], torch.float64)).backward()
    np.testing.assert_allclose(p64.grad.squeeze(1).numpy(), gold["g_grad64"], rtol=1e-10, atol=0)


def test_engine_physics_grad_refuses_cpu_tensors():
    from raman_mi355x import engine
    t = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.physics_grad(t, t, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        engine.physics_grad(None, t, t, per_spectrum=False)
    with pytest.raises(ValueError, match="per_spectrum=False"):
        engine.physics_grad(None, t, t)
