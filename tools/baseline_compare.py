"""The networks beside the classical filters, from one evaluate_synthetic call, and each filter's throughput
(DESIGN.md §5).

Part 1 meters the six trained-fixture networks (tests/golden, 'trained' weights, 'f16') and a small grid of
baseline filters (linear smoothers, running medians, translation-invariant Haar shrinkage, the exact
piecewise-constant fit, the Bayesian change-point smoother) over the same
on-device simulator spectra with snr_bins = (20, 37, 17), and writes the table
to profiles/baselines/comparison.json / comparison.txt (raman_mi355x.write_comparison).  The last row,
true_segmentation, is the ceiling of every piecewise-constant estimate: the run means of the noisy input under the
clean signal's own runs (plain torch ops on the device; it needs the clean twin, which no denoiser has).

Part 2 times each filter alone at L = 10 000, batch 8192, with HIP events on the launch stream, the filters
interleaved round by round (round 0 warms up), and writes spectra/s and GB/s (80 KB of HBM traffic per
spectrum: 40 KB read, 40 KB written) beside the HBM-bound time into profiles/baselines/throughput.json.  The
piecewise-constant fit is timed as engine.potts alone, with its buffers preallocated and gamma computed before
the clock starts, and the change-point smoother as engine.bayes_steps alone, likewise; their noise estimate is the
leg noise_mad.

    python tools/baseline_compare.py [--total 8192] [--L 10000] [--batch 2048] [--rounds 12] [--out profiles/baselines]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "data-simulation-and-noise-reduction-of-distributed-fiber-raman-intensity_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.29e12          # bytes/s, float4 copy on the MI355X (8.0e12 spec)
BYTES_PER_SAMPLE = 8              # one fp32 read, one fp32 written


def true_segmentation(seed, L):
    """A module for evaluate_synthetic that returns the run means of its input under the CLEAN signal's own runs.
    The clean twin of a batch is regenerated from (seed, index of the batch's first spectrum): the module counts
    the spectra it has seen, and checks that the regenerated noisy batch is the one it was given."""
    import torch
    from raman_mi355x import engine

    class TrueSegmentation(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.seen = 0

        def forward(self, x):
            n = x.shape[0]
            clean, noisy, _, _ = engine.generate(n, seed, first_index=self.seen, signal_length=L, device=x.device)
            assert torch.equal(noisy, x.view(n, L)), "the batch is not the simulator's next one"
            self.seen += n
            idx = torch.arange(L + 1, device=x.device).expand(n, L + 1)
            cut = torch.ones((n, L + 1), dtype=torch.bool, device=x.device)      # boundaries 0 .. L
            cut[:, 1:L] = clean[:, 1:] != clean[:, :-1]
            start = torch.where(cut, idx, torch.zeros_like(idx))[:, :L].cummax(dim=-1).values
            end = torch.where(cut, idx, torch.full_like(idx, L + 1))[:, 1:].flip(-1).cummin(dim=-1).values.flip(-1)
            S = torch.zeros((n, L + 1), dtype=torch.float64, device=x.device)
            S[:, 1:] = noisy.double().cumsum(dim=-1)
            mean = (S.gather(1, end) - S.gather(1, start)) / (end - start).double()
            return mean.float().view(n, 1, L)

    return TrueSegmentation()


def baseline_grid():
    from raman_mi355x import baselines as B
    from raman_mi355x.bayes import BayesSteps
    from raman_mi355x.potts import PottsFit
    from raman_mi355x.wavelets import HaarShrink
    return {"potts8": PottsFit(8.0), "potts10": PottsFit(10.0), "potts12": PottsFit(), "potts16": PottsFit(16.0),
            "potts_bic": PottsFit("bic"), "BayesSteps": BayesSteps(), "haar4_3h": HaarShrink(), "haar3_1.5s": HaarShrink(3, 1.5, "soft"), "haar4_uni_h": HaarShrink(4, "universal"),
            "ma3": B.MovingAverage(3), "ma5": B.MovingAverage(5), "sg5_2": B.SavitzkyGolay(5, 2),
            "sg21_3": B.SavitzkyGolay(21, 3), "gauss1": B.GaussianSmooth(1.0), "gauss2.5": B.GaussianSmooth(2.5),
            "med3": B.MedianFilter(3), "med5": B.MedianFilter(5), "med7": B.MedianFilter(7), "med21": B.MedianFilter(21)}


def main():
    import torch
    import raman_mi355x as R
    from conftest import golden_state_dict
    from raman_mi355x import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=8192)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--time-batch", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baselines"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    filters = {k: m.to(dev) for k, m in baseline_grid().items()}

    models = {}
    for arch in R.MODELS:
        m = R.MODELS[arch]()
        m.load_state_dict(golden_state_dict(arch, "trained"), strict=True)
        models[arch] = m.to(dev).eval().set_engine_dtype("f16")
    models.update(filters)
    seed = 20250410
    models["true_segmentation"] = true_segmentation(seed, a.L)
    res = R.evaluate_synthetic(models, a.total, seed=seed, signal_length=a.L, batch_size=a.batch, device=dev,
                               snr_bins=(20, 37, 17))
    R.write_comparison(res, a.out)
    print(open(os.path.join(a.out, "comparison.txt")).read(), flush=True)

    n, L = a.time_batch, a.L
    _, noisy, _, _ = engine.generate(n, 1, signal_length=L, device=dev)
    x = noisy.view(n, 1, L)
    y = torch.empty_like(x)
    med_buf = torch.empty(n, dtype=torch.float64, device=dev)
    legs = {k: ((lambda m=m: engine.median(x, m.window, out=y)) if isinstance(m, R.MedianFilter) else
                (lambda m=m: engine.haar_shrink(x, m.factors(L), m.mode, out=y, med=med_buf)) if isinstance(m, R.HaarShrink) else
                (lambda m=m: engine.fir(x, m.taps, edge_taps=m.edge_taps, out=y))) for k, m in filters.items()
            if not isinstance(m, (R.PottsFit, R.BayesSteps))}
    gamma = filters["potts12"].gamma(x)                                 # once, outside the timed region
    nseg_buf = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(n * L, dtype=torch.uint8, device=dev)
    legs["potts12"] = lambda: engine.potts(x, gamma, filters["potts12"].max_len, out=y, nseg=nseg_buf, work=work)
    bayes = filters["BayesSteps"]
    sigma = bayes.noise_std(x)                                          # likewise
    jump_buf, logz_buf = torch.empty_like(x), torch.empty(n, dtype=torch.float64, device=dev)
    work64 = torch.empty(n * (L + 1), dtype=torch.float64, device=dev)
    legs["BayesSteps"] = lambda: engine.bayes_steps(x, sigma, bayes.max_len, bayes.level_range, out=y, jump=jump_buf,
                                                    logz=logz_buf, work=work64)
    legs["noise_mad"] = lambda: engine.noise_mad(x, out=med_buf)
    legs["haar7_3h"] = lambda m=R.HaarShrink(7): engine.haar_shrink(x, m.factors(L), m.mode, out=y, med=med_buf)
    for w in (11, 25, 27, 101):                                         # sorting networks up to 25, then the radix select
        legs[f"med{w}"] = lambda w=w: engine.median(x, w, out=y)
    legs["sg255_3"] = (lambda m=R.SavitzkyGolay(255, 3).to(dev): engine.fir(x, m.taps, edge_taps=m.edge_taps, out=y))
    legs["copy"] = lambda: y.copy_(x)                                   # the HBM-bound yardstick, measured
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):
        for name, leg in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            leg()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1))
    nbytes = n * L * BYTES_PER_SAMPLE
    bound_ms = nbytes / HBM_ACHIEVABLE * 1e3
    table = {"batch": n, "L": L, "rounds": a.rounds, "bytes": nbytes, "hbm_bound_ms": bound_ms, "filters": {}}
    print(f"B={n} L={L}: {nbytes / 1e6:.1f} MB per call, HBM-bound {bound_ms:.3f} ms at {HBM_ACHIEVABLE / 1e12:.2f} TB/s")
    for name, t in times.items():
        med = statistics.median(t)
        table["filters"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spectra_per_s": n / med * 1e3,
                                  "GB_per_s": nbytes / med / 1e6, "times_hbm_bound": med / bound_ms}
        print(f"{name:11s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  {n / med * 1e3:12.0f} spectra/s  "
              f"{nbytes / med / 1e6:8.1f} GB/s  {med / bound_ms:7.1f} x HBM-bound", flush=True)
    with open(os.path.join(a.out, "throughput.json"), "w") as f:
        json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
