"""A plain bench.py run (no --full): the headline leg alone, and --dump-outputs writing what the timed
path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_headline_only_and_dumps_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at a small shape: one JSON line whose
    headline keys are consistent (value = spectra / timed seconds, ms_per_step = timed seconds / K), no
    other leg run (their keys null / empty / absent), and DIR/y.npy the float32 (B, L) outputs of the
    timed path -- bit-identical to engine.forward on the same simulator spectra and the same
    random-init weights (torch.manual_seed(1234)) in this process."""
    import raman_mi355x as R
    from raman_mi355x import engine
    B, L, K = 64, 2000, 3
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
           "--batch", str(B), "--L", str(L), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == K and rec["n_gpus"] == 1 and rec["dtype"] == "f16" and rec["unit"] == "spectra/s"
    assert rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    assert abs(rec["value"] - B / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert rec["variants"] == {} and "cpu_baseline" not in rec
    for k in ("trained_weights", "pipeline", "sustained", "configs", "batch1"):
        assert rec[k] is None, k
    assert sorted(os.listdir(tmp_path / "out")) == ["y.npy"]
    got = np.load(tmp_path / "out" / "y.npy")
    assert got.dtype == np.float32 and got.shape == (B, L) and np.isfinite(got).all()

    dev = torch.device("cuda")
    torch.manual_seed(1234)
    m = R.RRCDNet().to(dev).eval().set_engine_dtype("f16")
    _, noisy, _, _ = engine.generate(B, 20250410, first_index=0, signal_length=L, device=dev)
    y = engine.forward("RRCDNet", m.engine_code, m.packed_weights(dev), noisy.view(B, 1, L))
    np.testing.assert_array_equal(got, y.view(B, L).cpu().numpy())
