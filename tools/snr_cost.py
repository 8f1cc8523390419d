"""Cost of the SNR pass beside the metered forward, in one process on one GPU.

Times, interleaved round by round with HIP events on the launch stream, on on-device simulator spectra:
  A  engine.forward_metrics alone (exact accumulator; what evaluate_synthetic runs without snr_bins)
  B  engine.forward_metrics with per-spectrum metrics + engine.snr with a report (what snr_bins adds)
  C  engine.snr alone (the same call as in B)
and prints the median, minimum and maximum of each over the rounds.

    python tools/snr_cost.py [--batch 8192] [--L 10000] [--rounds 24] [--bins 17] [net:dtype]   (default RRCDNet:f16)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "data-simulation-and-noise-reduction-of-distributed-fiber-raman-intensity_amd"))


def main():
    import torch
    import raman_mi355x as R
    from raman_mi355x import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--bins", type=int, default=17)
    ap.add_argument("spec", nargs="?", default="RRCDNet:f16")
    a = ap.parse_args()
    dev = torch.device("cuda")
    arch, dtype = a.spec.split(":")
    n, L, bins = a.batch, a.L, (20.0, 37.0, a.bins)
    clean, noisy, snr_db, _ = engine.generate(n, 1, signal_length=L, device=dev)
    x = noisy.view(n, 1, L)
    torch.manual_seed(0)
    model = R.MODELS[arch]()
    code = engine.resolve_dtype(arch, dtype)
    packed = engine.pack(arch, model.state_dict(), dtype, dev)
    ws = None                                       # unchecked launches, as the benchmark's
    y = torch.empty_like(x)
    acc, report = engine.new_acc(dev), engine.new_report(a.bins, dev)

    def leg_a():
        engine.forward_metrics(arch, code, packed, x, clean, out=y, acc=acc, check=False, workspace=ws)

    def leg_b():
        _, per, _, _ = engine.forward_metrics(arch, code, packed, x, clean, out=y, acc=acc, per_spectrum=True, check=False,
                                              workspace=ws)
        engine.snr(noisy, y, clean, key=snr_db, bins=bins, per4=per, report=report, per_spectrum=False)

    per4 = engine.forward_metrics(arch, code, packed, x, clean, out=y, per_spectrum=True, check=False, workspace=ws)[1]

    def leg_c():
        engine.snr(noisy, y, clean, key=snr_db, bins=bins, per4=per4, report=report, per_spectrum=False)

    legs = {"A forward_metrics": leg_a, "B forward_metrics + snr": leg_b, "C snr alone": leg_c}
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
    v = engine.report_value(report, a.bins)
    print(f"{arch} {dtype} B={n} L={L} bins={a.bins} rounds={a.rounds}: report holds {int(v[-1, 0])} spectra, "
          f"mean SNR_in {float(v[-1, 5] / v[-1, 0]):.3f} dB")
    for name, t in times.items():
        print(f"{name:26s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
              f"stdev {statistics.stdev(t):.3f}", flush=True)
    d = [b - a_ for a_, b in zip(times["A forward_metrics"], times["B forward_metrics + snr"])]
    print(f"B - A per round            median {statistics.median(d):8.3f} ms  min {min(d):8.3f}  max {max(d):8.3f}")


if __name__ == "__main__":
    main()
