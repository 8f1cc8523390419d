"""Cost of the PhysicsAwareLoss pass beside the SNR pass, in one process on one GPU.

Times, interleaved round by round with HIP events on the launch stream, on the same on-device simulator
spectra (x noisy, clean, and y = a stand-in denoised output):
  A  engine.snr      with a report (one pass over x, y and clean)
  B  engine.physics  with a report (the same three rows, their neighbours, and the two noise passes)
and prints the median, minimum and maximum of each over the rounds, and the ratio of the medians.

    python tools/physics_cost.py [--batch 8192] [--L 10000] [--rounds 24] [--bins 17] [--f64]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "data-simulation-and-noise-reduction-of-distributed-fiber-raman-intensity_amd"))


def main():
    import torch
    from raman_mi355x import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--bins", type=int, default=17)
    ap.add_argument("--f64", action="store_true", help="clean in float64")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, L, bins = a.batch, a.L, (20.0, 37.0, a.bins)
    clean, noisy, snr_db, _ = engine.generate(n, 1, signal_length=L, device=dev)
    y = (clean + 0.3 * (noisy - clean)).contiguous()
    if a.f64:
        clean = clean.double()
    srep, prep = engine.new_report(a.bins, dev), engine.new_physics_report(a.bins, dev)
    legs = {"A snr": lambda: engine.snr(noisy, y, clean, key=snr_db, bins=bins, report=srep, per_spectrum=False),
            "B physics": lambda: engine.physics(noisy, y, clean, key=snr_db, bins=bins, report=prep, per_spectrum=False)}
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
    v = engine.physics_value(prep, a.bins)
    print(f"B={n} L={L} clean {'fp64' if a.f64 else 'fp32'} bins={a.bins} rounds={a.rounds}: report holds {int(v[-1, 0])} "
          f"spectra, mean Total {float(v[-1, 5] / v[-1, 0]):.6e}")
    for name, t in times.items():
        print(f"{name:10s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
              f"stdev {statistics.stdev(t):.3f}", flush=True)
    print(f"B / A (medians) {statistics.median(times['B physics']) / statistics.median(times['A snr']):.2f}")


if __name__ == "__main__":
    main()
