"""The walk kernels' metric epilogue (csrc/metrics.hpp walk_metrics) at the lengths where it changes path.

On the walk geometry rdn_forward_metrics meters each spectrum inside the forward kernel: the spectrum's
y row and its clean row are staged into the kernel's dynamic LDS when

    384 + round16(4 L) + L * sizeof(clean)  <=  the LDS the kernel is launched with

and are read straight from memory otherwise.  Two launch sizes exist: rrcdnet_hybrid_walk (RRCDNet
'f16') has 163840 B, the fused16 walk kernels (DenoiseCNN / PIDN / DSDN 'f16', RRCDNet 'f16-plain')
2 * (4 + 576) * 128 + 88 * 128 = 159744 B.  The cases below sit on both sides of every staging limit,
on stage_row's 4096-value passes, on the 512-thread partition of short spectra, on rows that share
cache lines, on spiked spectra (the tiled fallback inside the walk kernel) and on evaluate().

Every case: the epilogue ran (fused), y is the bits of rdn_forward, per-spectrum values and the exact
accumulator are the bits of the standalone metrics kernel on that y, and from L = 100 on the values
also match the numpy oracle at the suite's metric bar (rtol 1e-10, atol 1e-12).  Below L = 100 the
simulator's clean range over a handful of samples is tiny and SSIM's constants are badly conditioned,
so only the bitwise comparison is made there (test_metrics_gpu.py pins the standalone kernel to the
oracle at L = 7 and 8).
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG_DIR, golden_state_dict

pytestmark = pytest.mark.gpu

SEED = 20250410

HYBRID = ("RRCDNet", "f16")                      # rrcdnet_hybrid_walk
K2 = [("DenoiseCNN", "f16"), HYBRID]             # one kernel of each LDS size
K5 = [HYBRID, ("RRCDNet", "f16-plain"), ("DenoiseCNN", "f16"), ("PIDN", "f16"), ("DSDN", "f16")]
K5_REST = [k for k in K5 if k not in K2]

HYBRID_LDS = 163840                              # the whole LDS of a CU
RED_BYTES = 6 * (512 // 64) * 8                  # metrics.hpp RED_DOUBLES doubles


@functools.lru_cache(maxsize=None)
def _fused16_walk_lds():
    """fused16.hpp LDS_BYTES of the walk instantiation, from the build's walk tile (common.hpp)."""
    with open(os.path.join(PKG_DIR, "csrc", "common.hpp")) as f:
        rows = int(re.search(r"#define RDN_WALK_ROWS (\d+)", f.read()).group(1))
    return 2 * (4 + rows) * 128 + 88 * 128


def _lds(arch, dtype):
    return HYBRID_LDS if (arch, dtype) == HYBRID else _fused16_walk_lds()


def _staged(L, f64, lds):
    """metrics.hpp walk_metrics_t's decision: reduction scratch + y row (16-byte rounded) + clean row."""
    return RED_BYTES + ((4 * L + 15) & ~15) + L * (8 if f64 else 4) <= lds


@functools.lru_cache(maxsize=None)
def _model(arch, dtype):
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(golden_state_dict(arch, "trained" if arch == "RRCDNet" else "synth"), strict=True)
    return m.cuda().eval().set_engine_dtype(dtype)


def _walk(monkeypatch):
    monkeypatch.setenv("RDN_WALK", "1")
    monkeypatch.setenv("RDN_SHORT_TILES", "0")


def _inputs(n, L, first, f64, spikes=()):
    """Simulator spectra; an fp64 clean holds bits no fp32 has (a path reading it as fp32 would differ)."""
    from raman_mi355x import engine
    clean, noisy, _, _ = engine.generate(n, SEED, first_index=first, signal_length=L, device="cuda")
    for i, lo, hi in spikes:
        noisy[i, lo:hi] += 2.0                   # beyond the hybrid's window [-0.3, 1.3], inside the gate (4)
    if f64:
        u = torch.rand((n, L), dtype=torch.float64, generator=torch.Generator().manual_seed(first + L))
        clean = clean.double() + 1e-9 * u.cuda()
    return noisy.view(n, 1, L), clean


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check(arch, dtype, x, clean, out=None):
    """forward_metrics against forward + the metrics kernel (bitwise) and, from L = 100, the oracle."""
    from oracle.metrics import per_spectrum
    from raman_mi355x import engine
    m = _model(arch, dtype)
    dev = x.device
    packed = m.packed_weights(dev)
    n, L = x.shape[0], x.shape[-1]
    y0 = engine.forward(arch, m.engine_code, packed, x)
    acc0 = engine.new_acc(dev)
    per0, sums0 = engine.metrics(y0.view(n, L), clean, acc=acc0)
    acc1 = engine.new_acc(dev)
    y1, per1, sums1, fused = engine.forward_metrics(arch, m.engine_code, packed, x, clean, out=out, per_spectrum=True,
                                                    acc=acc1)
    assert fused                                  # the epilogue ran
    assert torch.equal(y0, y1)
    assert torch.equal(_bits(per0), _bits(per1)), (per0 - per1).abs().max(dim=0).values.tolist()
    assert torch.equal(acc0, acc1)
    s0, s1 = sums0.cpu().numpy(), sums1.cpu().numpy()
    assert s1[4] == n
    np.testing.assert_allclose(s1[:4], s0[:4], rtol=1e-14)
    if L >= 100:
        ref = per_spectrum(y1.view(n, L).cpu().numpy(), clean.cpu().numpy())
        np.testing.assert_allclose(per1.cpu().numpy(), ref, rtol=1e-10, atol=1e-12)
    return per1


def _run(monkeypatch, arch, dtype, n, L, f64, first, spikes=()):
    _walk(monkeypatch)
    x, clean = _inputs(n, L, first, f64, spikes)
    return _check(arch, dtype, x, clean)


# A. the staging limits: the last staged and the first direct length of both LDS sizes
LIMITS = {True: (13280, 13620), False: (19920, 20432)}       # clean fp64 / fp32: (fused16 walk, hybrid)
A_CASES = [(L, f64) for f64, lim in LIMITS.items() for last in lim for L in (last, last + 1)]


def test_limit_lengths_are_the_staging_boundaries():
    """The lengths of group A are where each kernel stops staging (a changed walk tile moves them)."""
    assert _fused16_walk_lds() == 159744
    for f64, (last16, lasth) in LIMITS.items():
        for last, lds in ((last16, _fused16_walk_lds()), (lasth, HYBRID_LDS)):
            assert _staged(last, f64, lds) and not _staged(last + 1, f64, lds), (f64, last, lds)
        # between the two limits the hybrid stages and the fused16 walks must not
        assert all(_staged(L, f64, HYBRID_LDS) and not _staged(L, f64, _fused16_walk_lds()) for L in (last16 + 1, lasth))


@pytest.mark.parametrize("L,f64", A_CASES)
@pytest.mark.parametrize("arch,dtype", K2)
def test_staging_limits(arch, dtype, L, f64, monkeypatch):
    _run(monkeypatch, arch, dtype, 3, L, f64, first=1000 + L)


@pytest.mark.parametrize("L,f64", [(13620, True), (20432, False)])
@pytest.mark.parametrize("arch,dtype", K5_REST)
def test_staging_limits_largest_hybrid_length_on_the_fused16_walks(arch, dtype, L, f64, monkeypatch):
    """The longest spectra the hybrid stages: the fused16 walks (4096 B less LDS) read them from memory."""
    assert _staged(L, f64, HYBRID_LDS) and not _staged(L, f64, _lds(arch, dtype))
    _run(monkeypatch, arch, dtype, 3, L, f64, first=2000 + L)


# B. stage_row's passes of 8 x 512 values
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("L", [4095, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("arch,dtype", K2)
def test_stage_row_pass_edges(arch, dtype, L, f64, monkeypatch):
    assert _staged(L, f64, _lds(arch, dtype))
    _run(monkeypatch, arch, dtype, 3, L, f64, first=3000 + L)


# C. short spectra: one 512-thread workgroup, L - 6 SSIM windows
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("L", [7, 8, 13, 511, 512, 513, 518, 519])
@pytest.mark.parametrize("arch,dtype", K2)
def test_short_spectra_and_partition_edges(arch, dtype, L, f64, monkeypatch):
    _run(monkeypatch, arch, dtype, 3, L, f64, first=4000 + L)


@pytest.mark.parametrize("arch,dtype", K5)
def test_fp64_clean_is_read_as_fp64(arch, dtype, monkeypatch):
    """The same y against an fp64 clean and against its fp32 rounding: the values differ."""
    _walk(monkeypatch)
    n, L = 3, 513
    x, c64 = _inputs(n, L, 5000, True)
    per64 = _check(arch, dtype, x, c64)
    per32 = _check(arch, dtype, x, c64.float())
    assert not torch.equal(per64, per32)


# D. rows of neighbouring spectra share 128-byte lines, several spectra per CU, a reused output buffer
@pytest.mark.parametrize("L", [37, 7])
@pytest.mark.parametrize("arch,dtype", K2)
def test_rows_sharing_cache_lines_reused_output(arch, dtype, L, monkeypatch):
    """The epilogue reads y back through L1-bypassing loads: a second launch into the same buffer must
    meter its own outputs, not lines a CU kept from the first."""
    _walk(monkeypatch)
    n = 1024
    out = torch.empty((n, 1, L), dtype=torch.float32, device="cuda")
    pers = []
    for first in (6000, 60000):
        x, clean = _inputs(n, L, first, False)
        pers.append(_check(arch, dtype, x, clean, out=out))
    assert not torch.equal(pers[0], pers[1])      # two different batches


# E. spiked spectra (the tiled hybrid inside the walk kernel) metered at the limits
@pytest.mark.parametrize("L,f64", [(13620, True), (20433, False)])
def test_spiked_spectra_at_the_limits(L, f64, monkeypatch):
    assert _staged(L, f64, HYBRID_LDS) == (L == 13620)
    spikes = [(1, 100, 140), (3, L - 60, L - 20)]             # the second inside the spectrum's last tile
    _run(monkeypatch, "RRCDNet", "f16", 4, L, f64, first=7000, spikes=spikes)


# F. evaluate(): fp64 clean of a length the fused16 walk cannot stage, a ragged last batch
def test_evaluate_fp64_clean_beyond_the_fused16_staging_limit(monkeypatch):
    from oracle.metrics import per_spectrum
    from raman_mi355x import engine
    from raman_mi355x.evaluate import KEYS, evaluate
    _walk(monkeypatch)
    arch, dtype, n, L = "DenoiseCNN", "f16", 4, 13620
    m = _model(arch, dtype)
    x, c64 = _inputs(n, L, 8000, True)
    noisy, clean = x.view(n, L).cpu().numpy(), c64.cpu().numpy()
    assert clean.dtype == np.float64
    means = evaluate(m, noisy, clean, batch_size=3)
    y = engine.forward(arch, m.engine_code, m.packed_weights(x.device), x).view(n, L).cpu().numpy()
    ref = per_spectrum(y, clean).mean(axis=0)
    np.testing.assert_allclose([means[k] for k in KEYS], ref, rtol=1e-10)
    for b0, b1 in ((0, 3), (3, 4)):               # evaluate's two batches took the epilogue
        _check(arch, dtype, x[b0:b1], c64[b0:b1])


# G. the workload's long length (config 5): fp32 clean staged, fp64 clean direct
@pytest.mark.parametrize("f64", [False, True])
def test_config5_length(f64, monkeypatch):
    assert _staged(16384, f64, _fused16_walk_lds()) == (not f64)
    _run(monkeypatch, "PIDN", "f16", 2, 16384, f64, first=9000)
