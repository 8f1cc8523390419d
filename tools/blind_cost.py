"""Cost of the blind residual pass, and the blind table of the networks and baselines beside their true SNR gain
(DESIGN.md §3 and §5).

Part 1 times, interleaved round by round with HIP events on the launch stream, on on-device simulator spectra:
  A  engine.forward_metrics alone (RRCDNet 'f16', exact accumulator: the metered forward)
  B  engine.snr alone, with a report
  C  engine.blind alone, with a report, sigma precomputed
  D  engine.blind with sigma=None: C plus engine.noise_mad and the scaling of its result
and writes the medians and the ratios C / A, C / B, D / A, D / B to <out>/cost.json.

Part 2 meters the trained-fixture networks (tests/golden, 'trained' weights, 'f16'), MedianFilter(3), HaarShrink,
PottsFit and BayesSteps over the same simulator spectra with evaluate_synthetic(snr_bins=..., blind=True) and writes, per
model, the true SNR_in / SNR_gain beside the blind means and the flagged share to <out>/comparison.txt (and .json).

    python tools/blind_cost.py [--batch 8192] [--L 10000] [--rounds 12] [--lags 16] [--total 2048] [--out profiles/blind]
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

TABLE_KEYS = ("SNR_in", "SNR_gain", "SNR_est", "Ratio", "Rho1", "RhoMax", "Q", "flagged_fraction")


def cost(a, dev):
    import torch
    import raman_mi355x as R
    from raman_mi355x import engine
    n, L, bins = a.batch, a.L, (20.0, 37.0, 17)
    clean, noisy, snr_db, _ = engine.generate(n, 1, signal_length=L, device=dev)
    x = noisy.view(n, 1, L)
    torch.manual_seed(0)
    arch, dtype = "RRCDNet", "f16"
    code = engine.resolve_dtype(arch, dtype)
    packed = engine.pack(arch, R.MODELS[arch]().state_dict(), dtype, dev)
    y = torch.empty_like(x)
    acc, report, blind_rep = engine.new_acc(dev), engine.new_report(bins[2], dev), engine.new_blind_report(bins[2], dev)
    engine.forward_metrics(arch, code, packed, x, clean, out=y, acc=acc, check=False)
    sigma = engine.noise_mad(noisy) * (2.0 ** 0.5 / 0.6744897501960817)
    q_crit = engine.blind_q_crit(a.lags)
    legs = {
        "A forward_metrics": lambda: engine.forward_metrics(arch, code, packed, x, clean, out=y, acc=acc, check=False),
        "B snr": lambda: engine.snr(noisy, y, clean, key=snr_db, bins=bins, report=report, per_spectrum=False),
        "C blind": lambda: engine.blind(noisy, y, sigma=sigma, lags=a.lags, q_crit=q_crit, key=snr_db, bins=bins,
                                        report=blind_rep, per_spectrum=False),
        "D blind + noise_mad": lambda: engine.blind(noisy, y, lags=a.lags, q_crit=q_crit, key=snr_db, bins=bins,
                                                    report=blind_rep, per_spectrum=False),
    }
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):                 # round 0 warms up
        for name, leg in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            leg()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1))
    v = engine.blind_value(blind_rep, bins[2])
    print(f"{arch} {dtype} B={n} L={L} lags={a.lags} rounds={a.rounds}: the blind report holds {int(v[-1, 0])} spectra, "
          f"mean Q {float(v[-1, 6] / v[-1, 0]):.2f}, flagged {float(v[-1, 8] / v[-1, 0]):.4f}")
    med = {k: statistics.median(t) for k, t in times.items()}
    for name, t in times.items():
        print(f"{name:22s} median {med[name]:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}", flush=True)
    out = {"batch": n, "L": L, "lags": a.lags, "rounds": a.rounds,
           "median_ms": med, "min_ms": {k: min(t) for k, t in times.items()}, "max_ms": {k: max(t) for k, t in times.items()},
           "blind_over_forward": med["C blind"] / med["A forward_metrics"], "blind_over_snr": med["C blind"] / med["B snr"],
           "blind_with_noise_mad_over_forward": med["D blind + noise_mad"] / med["A forward_metrics"],
           "blind_with_noise_mad_over_snr": med["D blind + noise_mad"] / med["B snr"]}
    print(f"blind / forward {out['blind_over_forward']:.3f}, blind / snr {out['blind_over_snr']:.2f}; with noise_mad "
          f"{out['blind_with_noise_mad_over_forward']:.3f}, {out['blind_with_noise_mad_over_snr']:.2f}", flush=True)
    with open(os.path.join(a.out, "cost.json"), "w") as f:
        json.dump(out, f, indent=1)


def comparison(a, dev):
    import raman_mi355x as R
    from conftest import golden_state_dict
    models = {}
    for arch in R.MODELS:
        m = R.MODELS[arch]()
        m.load_state_dict(golden_state_dict(arch, "trained"), strict=True)
        models[arch] = m.to(dev).eval().set_engine_dtype("f16")
    models.update({"med3": R.MedianFilter(3).to(dev), "haar4_3h": R.HaarShrink().to(dev), "potts12": R.PottsFit().to(dev),
                   "BayesSteps": R.BayesSteps().to(dev)})
    res = R.evaluate_synthetic(models, a.total, signal_length=a.L, batch_size=min(a.total, 1024), device=dev,
                               snr_bins=(20, 37, 17), blind={"lags": a.lags})
    table = {name: dict({k: r[k] for k in TABLE_KEYS[:2]}, **{k: r["blind"][k] for k in TABLE_KEYS[2:]})
             for name, r in res.items()}
    e = next(iter(res.values()))["blind"]
    head = f"# {a.total} simulator spectra, L = {a.L}, lags = {e['lags']}, alpha = {e['alpha']:g}, q_crit = {e['q_crit']:.3f}"
    with open(os.path.join(a.out, "comparison.json"), "w") as f:
        json.dump({"spectra": a.total, "L": a.L, "lags": e["lags"], "alpha": e["alpha"], "q_crit": e["q_crit"],
                   "models": table}, f, indent=1)
    with open(os.path.join(a.out, "comparison.txt"), "w") as f:
        f.write(head + "\n" + "model " + " ".join(TABLE_KEYS) + "\n")
        for name, row in table.items():
            f.write(name + " " + " ".join(format(row[k], ".4f") for k in TABLE_KEYS) + "\n")
    print(open(os.path.join(a.out, "comparison.txt")).read(), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--lags", type=int, default=16)
    ap.add_argument("--total", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blind"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    cost(a, dev)
    comparison(a, dev)


if __name__ == "__main__":
    main()
