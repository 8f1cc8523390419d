"""PhysicsAwareLoss value and gradient from one launch (rdn_physics_grad / engine.physics_grad, the
PhysicsAwareLoss(fused_backward=True) module) against the numpy oracle (tests/physics_grad_oracle.py) and the
reference class's recorded autograd (tests/golden/physics_grad.npz).

The bar is the oracle module's, derived there: |got - ref| <= 2^-24 |ref| + 2^-48 M_i, one rounding to fp32
plus the fp64 operations of both sides.  Against the reference's own float32 run the bound is the triangle
inequality with the recorded distance d32 between its float32 and float64 runs.  The per-spectrum values are
held to the bits of engine.physics, and the gradient to the same bits whether or not the values are computed
beside it and however the batch is split."""
import os

import numpy as np
import pytest
import torch

import physics_grad_oracle as G
from conftest import GOLDEN, golden_state_dict

pytestmark = pytest.mark.gpu

W = G.WEIGHTS


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spectra(n, L, seed, seg=7, f64=False):
    """The spectra of test_physics_gpu.py: piecewise-constant clean in [0, 1] (segments of ``seg`` samples; 1:
    every sample its own level), noisy x at about 25 dB and a denoised y that keeps a third of the noise.
    ``f64``: clean in float64 with values that are not float32-representable."""
    rng = np.random.default_rng(seed)
    c = np.repeat(rng.uniform(0.05, 1, (n, L // seg + 1)), seg, axis=1)[:, :L].astype(np.float32)
    std = np.sqrt(np.mean(c.astype(np.float64) ** 2, axis=1) / 10 ** 2.5)
    noise = rng.normal(0, 1, c.shape) * std[:, None]
    x = (c + noise).astype(np.float32)
    y = (c + noise / 3 + rng.normal(0, 1, c.shape) * std[:, None] / 10).astype(np.float32)
    if f64:
        c = c.astype(np.float64) + rng.uniform(0, 1e-9, c.shape)
        assert not np.array_equal(c, c.astype(np.float32))
    return x, y, c


def _assert_eager_fp32(got, ref, M):
    """The eager path's float32 autograd against the float64 oracle: at most eight float32-rounded operations
    on partial results no larger than M_i, 2^-24 each, doubled once: 2^-20 M_i."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(f"eager float32 gradient: largest error / bar {(err / (2.0 ** -20 * M)).max():.3f}")
    assert np.all(err <= 2.0 ** -20 * M)


def _grad(x, y, c, **kw):
    """engine.physics_grad on numpy rows: (per as numpy or None, grad as numpy)."""
    from raman_mi355x import engine
    per, g = engine.physics_grad(None if x is None else _cuda(x), _cuda(y), _cuda(c), **kw)
    assert g.dtype == torch.float32 and g.shape == y.shape and g.is_contiguous()
    return per, g


# the ends of the L - 1 and L - 2 stencils (3, 4, 7), both sides of the 512-thread partition, its
# unrolled-by-4 loop with a remainder (1025)
@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("L", [3, 4, 7, 511, 512, 513, 1025])
def test_gradient_and_values_on_the_grid(L, n, f64):
    from raman_mi355x import engine
    x, y, c = _spectra(n, L, 1000 * L + n, f64=f64)
    per, g = _grad(x, y, c)
    G.assert_meets_bar(g.cpu().numpy(), G.physics_grad(y, c), G.magnitude(y, c))
    # the values: the bits of rdn_physics
    ref_per, _ = engine.physics(_cuda(x), _cuda(y), _cuda(c))
    assert per.dtype == torch.float64 and per.shape == (n, 6) and torch.equal(per, ref_per)
    # the gradient alone: the same bits, without x
    none, g_only = _grad(None, y, c, per_spectrum=False)
    assert none is None and torch.equal(g_only, g)
    _, g_x = _grad(x, y, c, per_spectrum=False)
    assert torch.equal(g_x, g)


@pytest.mark.parametrize("f64", [False, True], ids=["clean32", "clean64"])
@pytest.mark.parametrize("case", ["unit_segments", "other_weights", "zero_weights", "scale_0.37", "scale_-2", "y_is_clean"])
def test_gradient_special_cases(case, f64):
    """Unit-length segments (a mask that changes at every position), other weights, weights (0, 0, 0) -- the
    plain MSE gradient, the loss the other four networks train on --, other scales of either sign, and
    y == clean: every gradient exactly 0.  (N, 1, L) inputs give the rows of (N, L)."""
    from raman_mi355x import engine
    n, L = 3, 1025
    x, y, c = _spectra(n, L, 77, seg=1 if case == "unit_segments" else 7, f64=f64)
    w = {"other_weights": (0.3, 0.7, 2.0), "zero_weights": (0.0, 0.0, 0.0)}.get(case, W)
    scale = {"scale_0.37": 0.37, "scale_-2": -2.0}.get(case)
    if case == "y_is_clean":
        y = c.astype(np.float32)
        c = y.astype(c.dtype)                                         # float64 clean: the float32 values, so y == clean
    if case == "unit_segments":
        assert np.all(G.peak_mask(c).sum(axis=1) > L // 4)
    per, g = _grad(x, y, c, weights=w, scale=scale)
    got = g.cpu().numpy()
    ref = G.physics_grad(y, c, w, scale)
    if case == "y_is_clean":
        assert np.all(got == 0) and np.all(ref == 0)
    else:
        G.assert_meets_bar(got, ref, G.magnitude(y, c, w, scale))
    if case == "zero_weights":
        assert np.array_equal(ref, (1.0 / n) * (2.0 * (y.astype(np.float64) - c.astype(np.float64)) / L))
    assert torch.equal(per, engine.physics(_cuda(x), _cuda(y), _cuda(c), weights=w)[0])
    per3, g3 = engine.physics_grad(_cuda(x).unsqueeze(1), _cuda(y).unsqueeze(1), _cuda(c).unsqueeze(1), weights=w, scale=scale)
    assert g3.shape == (n, 1, L) and torch.equal(g3.squeeze(1), g) and torch.equal(per3, per)


@pytest.mark.parametrize("k", [1, 4])
def test_gradient_is_independent_of_the_batch_split(k):
    """With one scale, the gradient of rows [0, k) and [k, n) from two calls is the rows of one call."""
    n, L = 5, 1025
    x, y, c = _spectra(n, L, 5)
    for kw in (dict(), dict(per_spectrum=False)):
        _, whole = _grad(x, y, c, scale=1.0 / n, **kw)
        _, a = _grad(x[:k], y[:k], c[:k], scale=1.0 / n, **kw)
        _, b = _grad(x[k:], y[k:], c[k:], scale=1.0 / n, **kw)
        assert torch.equal(torch.cat([a, b]), whole)
    # scale = None is 1 / n of the call
    assert torch.equal(_grad(x, y, c)[1], whole)


def test_wrapper_checks_on_device_tensors():
    from raman_mi355x import engine
    from raman_mi355x._lib import EngineError
    x, y, c = (_cuda(a) for a in _spectra(3, 100, 1))
    with pytest.raises(ValueError, match="per_spectrum=False"):
        engine.physics_grad(None, y, c)
    with pytest.raises(ValueError, match="mismatch"):
        engine.physics_grad(x[:2], y, c)
    with pytest.raises(TypeError):
        engine.physics_grad(x, y.double(), c)
    with pytest.raises(ValueError, match="three samples"):
        engine.physics_grad(x[:, :2], y[:, :2], c[:, :2])
    with pytest.raises(ValueError, match="finite"):
        engine.physics_grad(x, y, c, weights=(0.1, float("nan"), 0.01))
    with pytest.raises(ValueError, match="finite"):
        engine.physics_grad(x, y, c, scale=float("inf"))
    with pytest.raises(ValueError, match="shape"):
        engine.physics_grad(x, y, c, out=torch.empty(3, 1, 100, device="cuda"))
    with pytest.raises(TypeError):
        engine.physics_grad(x, y, c, out=torch.empty(3, 100, device="cuda", dtype=torch.float64))
    with pytest.raises(EngineError, match="overlap"):
        engine.physics_grad(x, y, c, out=y)
    out = torch.empty(3, 100, device="cuda")
    per, g = engine.physics_grad(x, y, c, out=out)
    assert g is out and torch.equal(out, engine.physics_grad(x, y, c)[1])


# ---- the reference's recorded autograd ---------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    d = dict(np.load(os.path.join(GOLDEN, "physics.npz")))
    d.update({"g_" + k: v for k, v in np.load(os.path.join(GOLDEN, "physics_grad.npz")).items()})
    return d


def test_fixture_against_the_reference(gold):
    pred, clean, noisy = gold["pred"], gold["clean"], gold["noisy"]
    _, g = _grad(noisy, pred, clean)
    got = g.cpu().numpy()
    M = G.magnitude(pred, clean)
    G.assert_meets_bar(got, gold["g_grad64"], M)
    # the reference's own float32 run: the triangle inequality with its recorded distance to the float64 run
    d32 = float(gold["g_d32"])
    G.assert_meets_bar(got, gold["g_grad32"].astype(np.float64), M, extra=d32 + 2.0 ** -24 * d32)
    # other weights; the generator's float64 clean
    w = tuple(gold["g_weights"])
    _, gw = _grad(noisy, pred, clean, weights=w)
    G.assert_meets_bar(gw.cpu().numpy(), gold["g_grad64_w"], G.magnitude(pred, clean, w))
    _, g64 = _grad(noisy[:2], pred[:2], gold["clean64"])
    G.assert_meets_bar(g64.cpu().numpy(), gold["g_grad64_clean64"], G.magnitude(pred[:2], gold["clean64"]))
    for L in (3, 4, 7):
        _, gs = _grad(noisy[:3, :L], pred[:3, :L], clean[:3, :L])
        G.assert_meets_bar(gs.cpu().numpy(), gold[f"g_grad64_L{L}"], G.magnitude(pred[:3, :L], clean[:3, :L]))


def test_planted_non_finite_values_against_the_reference(gold):
    """A NaN at an unmasked and at a masked centre position, +inf at an unmasked one (0 * inf: NaN), -inf and
    +inf at a row's ends: NaN and +-inf where the reference has them and nowhere else."""
    pp, ref = gold["g_planted_pred"], gold["g_planted_grad64"]
    c, x = gold["clean"][:2, :64], gold["noisy"][:2, :64]
    assert int((~np.isfinite(ref)).sum()) == 5
    for kw in (dict(), dict(per_spectrum=False)):
        _, g = _grad(x, pp, c, **kw)
        got = g.cpu().numpy()
        G.assert_same_nonfinite(got, ref)
        G.assert_meets_bar(got, ref, G.magnitude(pp, c))


# ---- the module ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim3", [True, False], ids=["N1L", "NL"])
def test_loss_module_fused_backward(gold, dim3):
    from raman_mi355x import PhysicsAwareLoss
    crit = PhysicsAwareLoss(fused_backward=True)
    pred, clean, noisy = (_cuda(gold[k]).unsqueeze(1) if dim3 else _cuda(gold[k]) for k in ("pred", "clean", "noisy"))
    with torch.no_grad():
        value = PhysicsAwareLoss()(pred, clean, noisy)                # the engine path
    pred.requires_grad_(True)
    assert crit.uses_fused_backward(pred, clean, noisy) and not crit.uses_engine(pred, clean, noisy)
    assert not PhysicsAwareLoss().uses_fused_backward(pred, clean, noisy)
    with torch.no_grad():
        assert not crit.uses_fused_backward(pred, clean, noisy) and crit.uses_engine(pred, clean, noisy)
    loss = crit(pred, clean, noisy)
    assert loss.requires_grad and loss.dtype == torch.float32 and loss.dim() == 0 and torch.equal(loss.detach(), value)
    loss.backward()
    g = pred.grad.clone()
    assert g.shape == pred.shape and clean.grad is None and noisy.grad is None
    G.assert_meets_bar(g.reshape(8, 2000).cpu().numpy(), gold["g_grad64"], G.magnitude(gold["pred"], gold["clean"]))
    # grad_output reaches the gradient: exactly the fp32 product
    pred.grad = None
    (3 * crit(pred, clean, noisy)).backward()
    assert torch.equal(pred.grad, 3 * g)
    # float64 clean, and other weights, reach the kernel
    pred.grad = None
    crit(pred, clean.double(), noisy).backward()
    G.assert_meets_bar(pred.grad.reshape(8, 2000).cpu().numpy(), gold["g_grad64"], G.magnitude(gold["pred"], gold["clean"]))
    w = tuple(gold["g_weights"])
    pred.grad = None
    PhysicsAwareLoss(*w, fused_backward=True)(pred, clean, noisy).backward()
    G.assert_meets_bar(pred.grad.reshape(8, 2000).cpu().numpy(), gold["g_grad64_w"], G.magnitude(gold["pred"], gold["clean"], w))


def test_loss_module_falls_back_to_eager(gold):
    """A non-contiguous view, float64 pred, or a clean that wants a gradient: the eager path, with gradients."""
    from raman_mi355x import PhysicsAwareLoss
    crit = PhysicsAwareLoss(fused_backward=True)
    pred, clean, noisy = (_cuda(gold[k]).unsqueeze(1) for k in ("pred", "clean", "noisy"))
    pred.requires_grad_(True)
    ref = G.physics_grad(gold["pred"][:, ::2], gold["clean"][:, ::2])
    M = G.magnitude(gold["pred"], gold["clean"])

    def run(p, c, x):
        assert not crit.uses_fused_backward(p, c, x) and not crit.uses_engine(p, c, x)
        pred.grad = None
        loss = crit(p, c, x)
        assert loss.requires_grad
        loss.backward()

    run(pred[:, :, ::2], clean[:, :, ::2], noisy[:, :, ::2])
    _assert_eager_fp32(pred.grad[:, 0, ::2].cpu().numpy(), ref, G.magnitude(gold["pred"][:, ::2], gold["clean"][:, ::2]))
    assert not bool(pred.grad[:, 0, 1::2].any())
    p64 = pred.detach().double().requires_grad_(True)
    assert not crit.uses_fused_backward(p64, clean.double(), noisy.double())
    crit(p64, clean.double(), noisy.double()).backward()
    np.testing.assert_allclose(p64.grad[:, 0].cpu().numpy(), gold["g_grad64"], rtol=1e-10, atol=0)
    cg = clean.clone().requires_grad_(True)
    run(pred, cg, noisy)
    assert cg.grad is not None and bool(torch.isfinite(cg.grad).all()) and float(cg.grad.abs().max()) > 0
    _assert_eager_fp32(pred.grad[:, 0].cpu().numpy(), gold["g_grad64"], M)


# ---- end to end ----------------------------------------------------------------------------------------
def test_training_step_on_pidn():
    """The reference's training step: PIDN in train() mode (its eager GPU forward), the fused loss, backward."""
    import raman_mi355x as R
    from oracle.refgen import generate_signals
    np.random.seed(20250412)
    n, L = 2, 64
    clean, noisy, _, _ = generate_signals(n, signal_length=L)
    model = R.MODELS["PIDN"]()
    model.load_state_dict(golden_state_dict("PIDN", "trained"), strict=True)
    model = model.cuda().train()
    crit = R.PhysicsAwareLoss(fused_backward=True)
    x = torch.tensor(noisy, dtype=torch.float32).unsqueeze(1).cuda()
    c = torch.tensor(clean, dtype=torch.float32).unsqueeze(1).cuda()
    out = model(x)
    out.retain_grad()
    assert out.requires_grad and crit.uses_fused_backward(out, c, x)
    crit(out, c, x).backward()
    y32, c32 = out.detach().cpu().numpy()[:, 0], c.cpu().numpy()[:, 0]
    G.assert_meets_bar(out.grad.cpu().numpy()[:, 0], G.physics_grad(y32, c32), G.magnitude(y32, c32))
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
