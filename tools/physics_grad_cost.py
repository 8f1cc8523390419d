"""Cost of a PhysicsAwareLoss training step's loss -- forward plus backward -- on torch ops and from one
device launch, in one process on one GPU.

Times, interleaved round by round with HIP events on the launch stream, on the same on-device simulator
spectra (noisy, clean, and pred = a stand-in denoised output that wants a gradient):
  A  PhysicsAwareLoss()                      forward + backward on torch ops (the eager path)
  B  PhysicsAwareLoss(fused_backward=True)   forward + backward: one launch, the mean and grad_output * grad
  C  engine.physics                          rdn_physics alone: the per-spectrum values
  D  engine.physics_grad                     rdn_physics_grad alone: the values and the gradient
  E  engine.physics_grad(per_spectrum=False) the gradient alone
and prints the median, minimum, maximum and spread of each over the rounds, the ratios of the medians to
A's, and the peak device memory legs A and B allocate above what is resident before them.

    python tools/physics_grad_cost.py [--batch 16] [--L 10000] [--rounds 50] [--f64]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "data-simulation-and-noise-reduction-of-distributed-fiber-raman-intensity_amd"))


def main():
    import torch
    from raman_mi355x import PhysicsAwareLoss, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--f64", action="store_true", help="clean in float64")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, L = a.batch, a.L
    clean, noisy, _, _ = engine.generate(n, 1, signal_length=L, device=dev)
    clean, noisy = clean.reshape(n, 1, L), noisy.reshape(n, 1, L)        # the reference's training batch shape
    pred = (clean + 0.3 * (noisy - clean)).contiguous().requires_grad_(True)
    if a.f64:
        clean = clean.double()
    eager, fused = PhysicsAwareLoss(), PhysicsAwareLoss(fused_backward=True)
    assert fused.uses_fused_backward(pred, clean, noisy) and not eager.uses_fused_backward(pred, clean, noisy)
    grad_out = torch.empty_like(pred)

    def step(crit):
        pred.grad = None
        crit(pred, clean, noisy).backward()

    y = pred.detach()
    legs = {"A eager fwd+bwd": lambda: step(eager), "B fused fwd+bwd": lambda: step(fused),
            "C rdn_physics": lambda: engine.physics(noisy, y, clean),
            "D rdn_physics_grad": lambda: engine.physics_grad(noisy, y, clean, out=grad_out),
            "E gradient alone": lambda: engine.physics_grad(None, y, clean, per_spectrum=False, out=grad_out)}
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
    # peak memory of one step above what is resident before it (pred.grad released first)
    peak = {}
    for name, crit in (("A", eager), ("B", fused)):
        pred.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step(crit)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - base
    step(eager)
    g_eager = pred.grad.clone()
    step(fused)
    print(f"B={n} L={L} clean {'fp64' if a.f64 else 'fp32'} rounds={a.rounds}: max |fused - eager gradient| "
          f"{float((pred.grad - g_eager).abs().max()):.3e} of max |gradient| {float(g_eager.abs().max()):.3e}")
    med = {k: statistics.median(t) for k, t in times.items()}
    for name, t in times.items():
        print(f"{name:20s} median {med[name] * 1e3:9.1f} us  min {min(t) * 1e3:9.1f}  max {max(t) * 1e3:9.1f}  "
              f"stdev {statistics.stdev(t) * 1e3:7.1f}  / A {med[name] / med['A eager fwd+bwd']:.3f}", flush=True)
    print(f"peak memory above the resident tensors: A {peak['A'] / 2 ** 20:.2f} MiB, B {peak['B'] / 2 ** 20:.2f} MiB, "
          f"A - B {(peak['A'] - peak['B']) / 2 ** 20:.2f} MiB (one (N, 1, L) float32: {n * L * 4 / 2 ** 20:.2f} MiB)")


if __name__ == "__main__":
    main()
