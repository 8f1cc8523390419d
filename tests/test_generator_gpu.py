"""On-device simulator vs the numpy restatement (same Philox draws) and vs reference statistics."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED = 20250410


def _gpu(n, first=0, L=10000, **kw):
    from raman_mi355x import engine
    c, x, s, sd = engine.generate(n, SEED, first_index=first, signal_length=L, **kw)
    torch.cuda.synchronize()
    return c.cpu().numpy(), x.cpu().numpy(), s.cpu().numpy(), sd.cpu().numpy()


@pytest.mark.parametrize("L", [10000, 16384, 1000, 101, 7])
def test_matches_numpy_restatement(L):
    from oracle.generator import generate
    n = 6
    kw = dict(extreme_noise_prob=0.5)            # exercise the spike path often
    c, x, s, sd = _gpu(n, first=123, L=L, **kw)
    oc, ox, os_, osd, outs = generate(SEED, 123, n, L, **kw)
    assert np.array_equal(s, os_), "SNR draws differ"
    np.testing.assert_allclose(sd, osd, rtol=2e-6)
    # clean: identical segment structure; values equal up to division rounding
    np.testing.assert_allclose(c, oc, rtol=0, atol=1e-6)
    assert np.array_equal(np.diff(c, axis=1) != 0, np.diff(oc, axis=1) != 0)
    # noisy: logf/sincosf differ from numpy by a few ulp, scaled by sigma (<0.1)
    np.testing.assert_allclose(x, ox, rtol=0, atol=2e-6)


# --- the whole seed, index and parameter domain ------------------------------------------------------
SEED64 = 0x9E3779B97F4A7C15                      # both key words non-zero
MAX_REPEAT_L1000 = (2 ** 31 - 1 - 1000) // 256   # the largest rdn_generate admits at L = 1000 (raman_mi355x.h)


def _case(row, seed=SEED64, first=7, n=4, L=1000, **kw):
    name = f"{row}:seed={seed:#x},first={first:#x},n={n},L={L}" + "".join(f",{k}={v}" for k, v in kw.items())
    return pytest.param(row, seed, first, n, L, kw, id=name)


DOMAIN = (
    [_case("upper-seed-word", seed=s, first=123, extreme_noise_prob=0.5) for s in (SEED64, 1 << 32, 2 ** 64 - 1)]
    # ilo wraps and ihi steps inside one launch
    + [_case("batch-crossing-2^32", first=2 ** 32 - 3, n=6)]
    + [_case("high-index", first=f) for f in (2 ** 63 + 5, 2 ** 64 - 4)]
    # one segment per position: 1, 1, 2 and 3 passes of phase A's 256-segment scan
    + [_case("scan-pass-edges", first=2 ** 32, n=3, L=L, max_repeat=1) for L in (255, 256, 257, 513)]
    + [_case("short-segments", n=3, L=1025, max_repeat=m) for m in (2, 3)]
    + [_case("few-or-one-segment", max_repeat=m) for m in (300, MAX_REPEAT_L1000)]
    # phase C takes 4 * 256 positions per pass
    + [_case("phase-C-edges", n=3, L=L) for L in (1, 2, 3, 5, 1023, 1024, 1025, 1027, 2049)]
    # spike widths are U{20..99}: below L = 21 every width clamps to L, up to L = 99 some do
    + [_case("spike-clamp-zone", n=8, L=L, extreme_noise_prob=1.0) for L in (20, 21, 60, 99, 100, 101)]
    + [_case("snr-range", snr_range=r) for r in ((0.0, 64.0), (5.0, 5.0), (20.0, 64.0))]
)


def _readback_expected(seed, index):
    """The 24 bits the SNR draw of spectrum ``index`` is made of: word 0 of the TAG_SCALAR block."""
    from oracle.generator import TAG_SCALAR, philox4x32
    x = philox4x32(np.uint32(0), np.uint32(TAG_SCALAR), np.uint32(index & 0xFFFFFFFF), np.uint32(index >> 32), seed)
    return int(x[0]) >> 8


@pytest.mark.parametrize("row,seed,first,n,L,kw", DOMAIN)
def test_matches_numpy_restatement_over_the_domain(row, seed, first, n, L, kw):
    """test_matches_numpy_restatement's assertions at 64-bit seeds and indices, at the sweep boundaries of
    the kernel's phases, in the spike clamp zone and over the SNR range.  The noisy bar is the 2e-6 written
    for σ < 0.1, scaled by σ where a low SNR makes σ larger: 2e-6 · max(1, σ/0.1) per spectrum."""
    from oracle.generator import generate
    from raman_mi355x import engine
    c, x, s, sd = (t.cpu().numpy() for t in engine.generate(n, seed, first_index=first, signal_length=L, **kw))
    oc, ox, os_, osd, outs = generate(seed, first, n, L, **kw)
    err_c = np.abs(c.astype(np.float64) - oc).max()
    err_x = np.abs(x.astype(np.float64) - ox).max(axis=1)
    bar_x = 2e-6 * np.maximum(1.0, osd.astype(np.float64) / 0.1)
    print(f"DOMAIN {row} seed={seed:#x} first={first:#x} n={n} L={L} {kw}: max|clean-oracle| {err_c:.3e}, "
          f"max|noisy-oracle| {err_x.max():.3e} (worst err/bar {np.max(err_x / bar_x):.3f}), sigma max {osd.max():.3e}")
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(x)) and np.all(np.isfinite(sd))
    assert np.array_equal(s, os_), "SNR draws differ"
    np.testing.assert_allclose(sd, osd, rtol=2e-6)
    np.testing.assert_allclose(c, oc, rtol=0, atol=1e-6)
    assert np.array_equal(np.diff(c, axis=1) != 0, np.diff(oc, axis=1) != 0)
    assert np.all(err_x <= bar_x), (err_x, bar_x)
    if row == "spike-clamp-zone":
        widths = [w for o in outs for (_, w, _) in o["spikes"]]
        assert all(o["extreme"] for o in outs) and (L > 20 or all(w == L for w in widths))
        assert L > 60 or any(w == L for w in widths), "no clamped width among the oracle's spikes"
        assert L < 60 or any(w < L for w in widths), "no fitting width among the oracle's spikes"
    if kw.get("max_repeat") == MAX_REPEAT_L1000:       # one segment: min = max, so clean = 0 and σ = 0
        assert all(o["seg_lens"].size == 1 for o in outs)
        assert not c.any() and not x.any() and not sd.any()
    if kw.get("snr_range") == (0.0, 64.0):             # snr = 64 · (draw >> 8) · 2^-24, exact in float32
        assert [float(v) * 2 ** 18 for v in s] == [_readback_expected(seed, first + i) for i in range(n)]
    if kw.get("snr_range") == (5.0, 5.0):
        assert np.all(s == 5.0)


@pytest.mark.parametrize("index", [2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1],
                         ids=["2^32-1", "2^32", "2^63+5", "2^64-1"])
def test_snr_draw_reads_back_exactly(index):
    """The device's SNR at snr_range = (0, 64) is the first word of the spectrum's TAG_SCALAR block."""
    from raman_mi355x import engine
    _, _, s, _ = engine.generate(1, SEED64, first_index=index, signal_length=64, snr_range=(0.0, 64.0))
    assert float(s.cpu()[0]) * 2 ** 18 == _readback_expected(SEED64, index)


def test_index_ranges_are_independent_of_batching_across_2_32():
    from raman_mi355x import engine
    first = 2 ** 32 - 8
    c_all, x_all, s_all, _ = engine.generate(16, SEED64, first_index=first)
    c_sub, x_sub, s_sub, _ = engine.generate(4, SEED64, first_index=first + 10)      # 2^32 + 2: after the crossing
    assert torch.equal(c_all[10:14], c_sub) and torch.equal(x_all[10:14], x_sub) and torch.equal(s_all[10:14], s_sub)
    assert len(set(s_all.cpu().tolist())) == 16


@pytest.mark.parametrize("first", [2 ** 32 - 100, 2 ** 63 + 12345], ids=["first=2^32-100", "first=2^63+12345"])
def test_device_noise_is_standard_normal_and_independent(first):
    """tests/noise_stats.py on 200 spike-free device spectra of L = 10000: the bounds the oracle is held
    to in tests/test_generator_cpu.py (sampling theory, not measured)."""
    from noise_stats import check, collect
    from raman_mi355x import engine
    c, x, s, sd = (t.cpu().numpy() for t in engine.generate(200, SEED64, first_index=first, extreme_noise_prob=0.0))
    st = collect(c, x, sd)
    print(f"NOISE device first={first:#x}: {st}")
    check(st)


def test_index_ranges_are_independent_of_batching():
    c_all, x_all, _, _ = _gpu(16, first=0)
    c_sub, x_sub, _, _ = _gpu(4, first=10)
    assert np.array_equal(c_all[10:14], c_sub) and np.array_equal(x_all[10:14], x_sub)


def test_statistics_match_reference():
    """χ²/range checks against the distributional contract and reference-generated statistics."""
    with open(os.path.join(GOLDEN, "generator_stats.json")) as fh:
        ref = json.load(fh)
    n = 2000
    c, x, s, sd = _gpu(n)
    # per-row normalisation (数据集产生.py:38-40)
    assert np.all(c.min(axis=1) == 0.0)
    assert np.all(c.max(axis=1) > 0.9999)
    # segment lengths: U{1..40}, last (truncated) run excluded
    counts = np.zeros(41)
    for row in c:
        b = np.concatenate([[0], np.flatnonzero(np.diff(row) != 0) + 1, [row.size]])
        runs = np.diff(b)[:-1]
        np.add.at(counts, runs[runs <= 40], 1)
    obs = counts[1:]
    exp = np.full(40, obs.sum() / 40)
    chi2 = ((obs - exp) ** 2 / exp).sum()
    assert chi2 < 80.0, f"segment-length chi2 {chi2:.1f} (39 dof, p~1e-4 at 80)"
    ref_obs = np.array(ref["seg_len_counts"], float)
    ref_exp = ref_obs.sum() * obs / obs.sum()
    chi2_ref = ((ref_obs - ref_exp) ** 2 / np.maximum(ref_exp, 1)).sum()
    assert chi2_ref < 90.0, f"segment lengths vs reference chi2 {chi2_ref:.1f}"
    # SNR ~ U[20, 37): 17 equal bins
    h, _ = np.histogram(s, bins=17, range=(20, 37))
    chi2_snr = ((h - n / 17) ** 2 / (n / 17)).sum()
    assert s.min() >= 20 and s.max() < 37 and chi2_snr < 45, f"snr chi2 {chi2_snr:.1f}"
    # noise std range and signal power like the reference
    q = np.quantile(sd, [0.1, 0.5, 0.9])
    rq = np.array(ref["noise_std_quantiles"])[[1, 2, 3]]
    assert np.all(np.abs(q - rq) / rq < 0.1), (q, rq)
    power = np.mean(c.astype(np.float64) ** 2, axis=1).mean()
    assert abs(power - ref["power_mean"]) < 0.01
    # spiked fraction ~ Binomial(n, 0.05): detect >= 20 consecutive points beyond 4 sigma
    spiked = 0
    for r, sig in zip(x - c, sd):
        big = (np.abs(r) > 4 * sig).astype(np.int32)
        spiked += bool((np.convolve(big, np.ones(20, np.int32), "valid") == 20).any())
    frac = spiked / n
    assert abs(frac - 0.05) < 4 * np.sqrt(0.05 * 0.95 / n) + 0.005, frac
    assert abs(frac - ref["spiked_fraction"]) < 0.03


def test_spike_process_matches_reference():
    """The spike process (数据集产生.py:50-62) on the device simulator with every spectrum spiked
    (extreme_noise_prob = 1): spike count U{1,2,3}, width U{20..99}, start U{0..L-W-1}, amplitude/σ
    U[5,15), sign Bernoulli(0.5) — χ² against the uniform contract (p = 0.001 bounds) and two-sample
    χ² against the same statistics of 1000 reference-generated spectra (generator_stats.json
    "spikes", make_golden.py --spikes), both recovered by tests/spike_stats.py."""
    from spike_stats import chi2_two_sample, chi2_uniform, collect
    with open(os.path.join(GOLDEN, "generator_stats.json")) as fh:
        ref = json.load(fh)["spikes"]
    n = 2000
    c, x, s, sd = _gpu(n, first=5000, extreme_noise_prob=1.0)
    st = collect(c, x, sd)
    print({k: v for k, v in st.items()})
    # every spectrum carries 1..3 spikes (a count outside means two edges coincided: rare)
    assert st["count_hist"][0] + st["count_hist"][4] <= n // 200, st["count_hist"]
    assert st["overlapped_spectra"] < 0.08 * n
    bounds = {"count_hist": 13.8, "width_hist": 24.3, "amp_hist": 27.9, "start_hist": 27.9}   # chi2(dof) at p=1e-3
    for key, bound in bounds.items():
        h = st[key][1:4] if key == "count_hist" else st[key]
        r = ref[key][1:4] if key == "count_hist" else ref[key]
        u, t = chi2_uniform(h), chi2_two_sample(h, r)
        print(f"{key}: chi2 vs uniform {u:.1f}, vs reference {t:.1f} (bound {bound})")
        assert u < bound, (key, u)
        assert t < bound, (key, t)
    assert 20 <= st["width_min_max"][0] and st["width_min_max"][1] <= 99
    p = st["sign_pos"] / st["sign_n"]
    assert abs(p - 0.5) < 4 * np.sqrt(0.25 / st["sign_n"]), p
    pr = ref["sign_pos"] / ref["sign_n"]
    assert abs(p - pr) < 4 * np.sqrt(0.25 / st["sign_n"] + 0.25 / ref["sign_n"])
