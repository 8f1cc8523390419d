"""Writes tests/golden/physics_grad.npz: the gradient the REFERENCE loss class (PIDN/train.py:109-146
PhysicsAwareLoss, loaded through _refload without running the script) gives by autograd on the input
arrays of tests/golden/physics.npz (make_physics_golden.py: clean, clean64, noisy, pred).  Run in the build
container only (it reads the reference); tests read the .npz, which holds recorded data only.

Every gradient is d loss / d pred of the reference class for (N, 1, L) inputs, loss.backward(), so each
carries the 1 / N of the mean over the batch it was computed on.  Stored:
  grad64            float64 run (inputs cast to float64), the whole 8 x 2000 batch, default weights
  grad64_w, weights the same with weights (0.3, 0.7, 2.0)
  grad64_clean64    float64 run, the first two spectra against clean64 (a batch of two)
  grad32, d32       the reference's own float32 run on the whole batch, and max |grad32 - grad64|
  grad64_L3, _L4, _L7   float64 run, the first three spectra cut to L = 3, 4 and 7 (batches of three)
  planted_pred, planted_grad64, planted_at   a 2 x 64 cut of pred (float32) with a NaN at an unmasked centre
                    position and +inf at another (row 0), a NaN at a masked centre position, -inf at index 0
                    and +inf at index L - 1 (row 1); the float64 gradient the reference gives for it against
                    the same cut of clean and noisy; and the (row, index) of the five planted values in that
                    order."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

WEIGHTS = (0.3, 0.7, 2.0)
N64 = 2
SHORT = (3, 4, 7)
PLANT_N, PLANT_L = 2, 64


def main():
    ns = _refload._exec_nodes(os.path.join(_refload.REF, "PIDN", "train.py"),
                              lambda n: isinstance(n, ast.ClassDef) and n.name == "PhysicsAwareLoss")
    cls = ns["PhysicsAwareLoss"]
    gold = np.load(os.path.join(HERE, "physics.npz"))
    clean, clean64, noisy, pred = (gold[k] for k in ("clean", "clean64", "noisy", "pred"))
    assert clean.dtype == noisy.dtype == pred.dtype == np.float32 and clean64.dtype == np.float64

    def t(a, dt):
        return torch.tensor(a, dtype=dt).unsqueeze(1)

    def grad(p, c, x, dt, cdt=None, crit=cls()):
        pt = t(p, dt).requires_grad_(True)
        crit(pt, t(c, cdt or dt), t(x, dt)).backward()
        assert pt.grad.dtype == dt
        return pt.grad.squeeze(1).numpy()

    f64, f32 = torch.float64, torch.float32
    out = dict(grad64=grad(pred, clean, noisy, f64), grad64_w=grad(pred, clean, noisy, f64, crit=cls(*WEIGHTS)),
               weights=np.array(WEIGHTS), grad64_clean64=grad(pred[:N64], clean64, noisy[:N64], f64),
               grad32=grad(pred, clean, noisy, f32))
    out["d32"] = np.float64(np.abs(out["grad32"].astype(np.float64) - out["grad64"]).max())
    for L in SHORT:
        out[f"grad64_L{L}"] = grad(pred[:3, :L], clean[:3, :L], noisy[:3, :L], f64)

    # the planted array: positions chosen by the mask of the cut (torch.diff(clean, n=2) < 0 in float32)
    pc, px = clean[:PLANT_N, :PLANT_L], noisy[:PLANT_N, :PLANT_L]
    mask = (torch.diff(torch.tensor(pc), n=2, dim=-1) < 0).numpy()
    un0, ma1 = 1 + np.flatnonzero(~mask[0]), 1 + np.flatnonzero(mask[1])
    nan_un = int(un0[un0 >= 8][0])
    inf_un = int(un0[un0 >= nan_un + 8][0])
    nan_ma = int(ma1[ma1 >= 8][0])
    assert inf_un < PLANT_L - 8 and nan_ma < PLANT_L - 8
    at = np.array([[0, nan_un], [0, inf_un], [1, nan_ma], [1, 0], [1, PLANT_L - 1]], dtype=np.int64)
    pp = pred[:PLANT_N, :PLANT_L].copy()
    for (r, i), v in zip(at, (np.nan, np.inf, np.nan, -np.inf, np.inf)):
        pp[r, i] = v
    out.update(planted_pred=pp, planted_at=at, planted_grad64=grad(pp, pc, px, f64))

    g = out["planted_grad64"]
    print("planted at", at.tolist(), "non-finite gradient at", np.argwhere(~np.isfinite(g)).tolist(),
          [g[r, i] for r, i in np.argwhere(~np.isfinite(g))])
    print("d32", out["d32"], "max |grad64|", np.abs(out["grad64"]).max())
    np.savez_compressed(os.path.join(HERE, "physics_grad.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "physics_grad.npz")), "bytes")


if __name__ == "__main__":
    main()
