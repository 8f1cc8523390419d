"""Writes tests/golden/physics.npz: 8 spectra of the REFERENCE generator (数据集产生.py:5-64), L = 2000,
extreme_noise_prob = 0.5, a deterministic stand-in for a denoised output, and what the REFERENCE loss
class (PIDN/train.py:109-146 PhysicsAwareLoss, loaded through _refload without running the script) gives
on them.  Run in the build container only (it reads the reference); tests read the .npz, which holds
recorded data only.

Stored: clean (float32), clean64 (the generator's float64 clean of the first two spectra), noisy
(float32), pred (float32: clean + 0.3 noise + 0.01 sin(i / 50)); of the reference class on the float32
arrays: ref64_batch (inputs cast to float64, whole batch), ref64_each (float64, one spectrum per batch),
ref32_batch (float32 inputs, whole batch), d32 = |ref32 - ref64| / |ref64|; ref64_each_clean64 (float64,
the first two spectra against clean64); counts / counts64: the number of positions where
torch.diff(clean, n=2) < 0 for clean / clean64; grad64: d loss / d pred in float64 for the first two
spectra cut to 64 samples."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

SEED = 20250412
N, L = 8, 2000
N64 = 2
GRAD_N, GRAD_L = 2, 64


def main():
    gen = _refload.load_generate_signals()
    ns = _refload._exec_nodes(os.path.join(_refload.REF, "PIDN", "train.py"),
                              lambda n: isinstance(n, ast.ClassDef) and n.name == "PhysicsAwareLoss")
    crit = ns["PhysicsAwareLoss"]()
    np.random.seed(SEED)
    clean, noisy, _, _ = gen(N, signal_length=L, extreme_noise_prob=0.5)
    assert clean.dtype == np.float64 and clean.shape == (N, L)
    pred = clean + 0.3 * (noisy - clean) + 0.01 * np.sin(np.arange(L) / 50.0)
    clean32, noisy32, pred32 = (a.astype(np.float32) for a in (clean, noisy, pred))
    clean64 = clean[:N64].copy()
    assert not np.array_equal(clean64, clean32[:N64].astype(np.float64))

    def t(a, dt):
        return torch.tensor(a, dtype=dt).unsqueeze(1)

    def loss(p, c, x, dt, cdt=None):
        return crit(t(p, dt), t(c, cdt or dt), t(x, dt))

    with torch.no_grad():
        ref64 = loss(pred32, clean32, noisy32, torch.float64).item()
        each = [loss(pred32[i:i + 1], clean32[i:i + 1], noisy32[i:i + 1], torch.float64).item() for i in range(N)]
        each64 = [loss(pred32[i:i + 1], clean64[i:i + 1], noisy32[i:i + 1], torch.float64).item() for i in range(N64)]
        r32 = loss(pred32, clean32, noisy32, torch.float32)
        assert r32.dtype == torch.float32
        ref32 = float(r32.item())
        counts = (torch.diff(torch.tensor(clean32), n=2, dim=-1) < 0).sum(-1).numpy()
        counts64 = (torch.diff(torch.tensor(clean64), n=2, dim=-1) < 0).sum(-1).numpy()
    d32 = abs(ref32 - ref64) / abs(ref64)
    p = t(pred32[:GRAD_N, :GRAD_L], torch.float64).requires_grad_(True)
    crit(p, t(clean32[:GRAD_N, :GRAD_L], torch.float64), t(noisy32[:GRAD_N, :GRAD_L], torch.float64)).backward()
    grad = p.grad.squeeze(1).numpy()
    print(f"ref64 {ref64!r}\nref32 {ref32!r}  d32 {d32:.3e}\neach {each}\neach64 {each64}\ncounts {counts} {counts64}")
    print("mean of each - batch:", abs(np.mean(each) - ref64) / ref64)
    np.savez_compressed(os.path.join(HERE, "physics.npz"), clean=clean32, clean64=clean64, noisy=noisy32, pred=pred32,
                        ref64_batch=np.float64(ref64), ref64_each=np.array(each), ref32_batch=np.float64(ref32),
                        d32=np.float64(d32), ref64_each_clean64=np.array(each64), counts=counts.astype(np.int64),
                        counts64=counts64.astype(np.int64), grad64=grad, seed=np.int64(SEED))


if __name__ == "__main__":
    main()
