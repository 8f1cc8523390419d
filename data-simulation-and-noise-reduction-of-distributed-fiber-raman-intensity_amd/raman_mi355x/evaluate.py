"""Batched, on-device replacements of the reference evaluation harness (*/evaulate.py).

``evaluate(model, noisy_data, clean_data)`` returns the same dict as evaulate.py:25-39
({MSE, SSIM, Smoothness, Peak2Peak} averaged over spectra) but runs the forward in batches and the
metrics in the fp64 device kernel instead of a batch-1 loop with a host sync per spectrum.  The
clean reference stays float64 (evaulate.py:34-35 compares against the float64 test.npz arrays).

``evaluate_synthetic(models, total, ...)`` is the config-4 driver: a fixed total of
N simulator spectra, rank r of W owning indices [r·N/W, (r+1)·N/W), chunked generate -> forward ->
metric sums per network, one all-reduce at the end.  The simulator is counter-based and the sums
are exact integer accumulators (rdn_metrics_ex), so the four means are the same bits for any W,
batch size or atomics order.

Under torch.distributed each rank evaluates its contiguous shard and the metric accumulators are
all-reduced (RCCL over xGMI for CUDA tensors).  The CBAM networks' hand-off status is checked once
per network at the end (engine.Workspace), not per batch.  ``write_metrics`` produces
evaulate.py:78-80's ``metrics.txt`` format.
"""
import os
import sys
import time
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, engine
from .distributed import shard, world

KEYS = ("MSE", "SSIM", "Smoothness", "Peak2Peak")


def _as_rows(a):
    if torch.is_tensor(a):
        return a.reshape(a.shape[0], -1)
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1)


def _all_reduce_acc(acc):
    """SUM all-reduce of an exact accumulator (int64, exact under any reduction order)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if dist.get_backend() == "gloo" and acc.is_cuda:        # gloo reduces host tensors
            h = acc.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            acc.copy_(h)
        else:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
    return acc


def means_from_acc(acc):
    """{MSE, SSIM, Smoothness, Peak2Peak} means of an exact accumulator (evaulate.py:39)."""
    s = engine.acc_value(acc).tolist()
    if s[4] <= 0:
        raise ValueError("no spectra were evaluated")
    return {k: s[i] / s[4] for i, k in enumerate(KEYS)}


SNR_KEYS = ("SNR_in", "SNR_out", "SNR_gain")
# what snr_bins adds to a result (write_metrics leaves them to write_snr_report)
_SNR_RESULT_KEYS = SNR_KEYS + ("by_snr", "snr_under", "snr_over")


def _bin_rows(v, bins):
    """(row, lo, hi) of a *_value table ``v`` for the underflow row, each bin with its edges, the overflow row."""
    lo, hi, nbins = engine._bins(bins)
    edges = [float("-inf")] + np.linspace(np.float64(lo), np.float64(hi), nbins + 1).tolist() + [float("inf")]
    return [(v[r], edges[r], edges[r + 1]) for r in range(nbins + 2)]


def snr_summary(report, bins):
    """What ``snr_bins`` adds to a result, from an (all-reduced) report: the means of SNR_in, SNR_out and
    SNR_gain over all spectra (dB), and ``by_snr``: one entry per bin with its edges ``lo`` / ``hi``, its
    ``count`` and -- unless the bin is empty -- the seven means (the four metrics only where per-spectrum
    metrics were supplied).  ``snr_under`` / ``snr_over`` are the same entries for keys below ``lo`` and
    at or above ``hi`` (or NaN).  A mean over values that include a non-finite one is NaN."""
    nbins = engine._bins(bins)[2]
    v = engine.report_value(report, nbins).tolist()

    def entry(row, e_lo, e_hi):
        count, count4 = int(row[0]), int(row[_lib.REPORT_VALUES - 1])
        e = {"lo": e_lo, "hi": e_hi, "count": count}
        for i, k in enumerate(engine.REPORT_QUANTITIES):
            c = count4 if i < 4 else count
            if c > 0:
                e[k] = row[1 + i] / c
        return e

    total = entry(v[nbins + 2], float("-inf"), float("inf"))
    if total["count"] <= 0:
        raise ValueError("no spectra were evaluated")
    out = {k: total[k] for k in SNR_KEYS}
    rows = [entry(*r) for r in _bin_rows(v, bins)]
    out["by_snr"], out["snr_under"], out["snr_over"] = rows[1:-1], rows[0], rows[-1]
    return out


PHYS_KEYS = engine.PHYS_QUANTITIES
# keys of a result that write_metrics leaves to write_snr_report / write_physics_report
_EXTRA_RESULT_KEYS = _SNR_RESULT_KEYS + ("physics", "blind")


def _physics_weights(physics):
    """``physics`` of evaluate(): None / False -> None, True -> the reference's default weights,
    (alpha, beta, gamma) -> those."""
    if physics is None or physics is False:
        return None
    return engine._weights(engine.PHYS_WEIGHTS if physics is True else physics)


def physics_summary(report, weights, L, bins=None):
    """The ``"physics"`` entry of a result, from an (all-reduced) PhysicsAwareLoss report of spectra of
    length ``L``: the ``weights``, the ``count`` of spectra, the means of MSE, Smooth, Peak, Noise, Total
    and PeakCount over all of them (the mean of Total is the reference's loss over the whole set, each
    term's mean the reference's term), and ``PeakMasked`` = ΣPeak (L - 2) / ΣPeakCount, the squared error
    per masked position (Peak itself is a mean over all L - 2 positions; NaN when nothing is masked).
    With ``bins`` = (lo, hi, nbins): ``by_snr``, one such entry per bin with its edges ``lo`` / ``hi``
    (the means only where the bin is not empty), and ``under`` / ``over`` for keys below ``lo`` and at or
    above ``hi`` (or NaN).  A mean over values that include a non-finite one is NaN."""
    nbins = engine._bins(bins)[2] if bins is not None else 1
    v = engine.physics_value(report, nbins).tolist()

    def entry(row, head):
        count = int(row[0])
        e = dict(head, count=count)
        if count > 0:
            for i, k in enumerate(PHYS_KEYS):
                e[k] = row[1 + i] / count
            e["PeakMasked"] = row[3] * (L - 2) / row[6] if row[6] > 0 else float("nan")
        return e

    out = entry(v[nbins + 2], {"weights": list(weights)})
    if out["count"] <= 0:
        raise ValueError("no spectra were evaluated")
    if bins is not None:
        rows = [entry(row, {"lo": e_lo, "hi": e_hi}) for row, e_lo, e_hi in _bin_rows(v, bins)]
        out["by_snr"], out["under"], out["over"] = rows[1:-1], rows[0], rows[-1]
    return out


BLIND_KEYS = engine.BLIND_QUANTITIES
blind_q_crit = engine.blind_q_crit


def _blind_options(blind):
    """``blind`` of evaluate(): None / False -> None, True -> 16 lags at alpha = 0.01, a dict with ``lags``
    and / or ``alpha`` -> those.  Returns (lags, alpha, q_crit) or None."""
    if blind is None or blind is False:
        return None
    opts = {} if blind is True else dict(blind)
    unknown = set(opts) - {"lags", "alpha"}
    if unknown:
        raise ValueError(f"blind takes 'lags' and 'alpha', got {sorted(unknown)}")
    lags, alpha = opts.get("lags", 16), opts.get("alpha", 0.01)
    return int(lags), float(alpha), blind_q_crit(lags, alpha)


def blind_summary(report, options, bins=None):
    """The ``"blind"`` entry of a result, from an (all-reduced) blind report (engine.blind) and ``options`` =
    (lags, alpha, q_crit): those three, the ``count`` of spectra, the means of Mean, RMS, Ratio, Rho1, RhoMax,
    Q and SNR_est over all of them and ``flagged_fraction``, the share whose Q exceeded q_crit.  If the
    denoised output is the signal, Mean is 0, Ratio about 1 (0.95 against the blind noise estimate on the
    simulator), Q about ``lags`` and flagged_fraction about alpha plus the share of spiked spectra.  With
    ``bins`` = (lo, hi, nbins): ``by_snr``, one such entry per bin with its edges ``lo`` / ``hi`` (the means
    only where the bin is not empty), and ``under`` / ``over`` for keys below ``lo`` and at or above ``hi``
    (or NaN).  A mean over values that include a non-finite one is NaN."""
    nbins = engine._bins(bins)[2] if bins is not None else 1
    v = engine.blind_value(report, nbins).tolist()

    def entry(row, head):
        count = int(row[0])
        e = dict(head, count=count)
        if count > 0:
            for i, k in enumerate(BLIND_KEYS):
                e[k] = row[1 + i] / count
            e["flagged_fraction"] = row[_lib.BLIND_VALUES - 1] / count
        return e

    out = entry(v[nbins + 2], {"lags": options[0], "alpha": options[1], "q_crit": options[2]})
    if out["count"] <= 0:
        raise ValueError("no spectra were evaluated")
    if bins is not None:
        rows = [entry(row, {"lo": e_lo, "hi": e_hi}) for row, e_lo, e_hi in _bin_rows(v, bins)]
        out["by_snr"], out["under"], out["over"] = rows[1:-1], rows[0], rows[-1]
    return out


def _engine_module(model):
    """A raman_mi355x network whose own forward is the engine (not a subclass overriding forward)."""
    from .models import _EngineNet
    return isinstance(model, _EngineNet) and type(model).forward is _EngineNet.forward


def _finish(model, ws):
    """One status read after all of a network's batches (rdn_forward_status_ex: the sticky words of every
    forward since): raises on a timed-out CBAM hand-off or a saturated tile, and RangeError when a 16-bit
    forward saw an input beyond the gate (the kernels' stems raise it, fused and CBAM networks alike)."""
    from .models import INPUT_GATE
    flags = ws.check() if ws is not None else 0
    if flags & engine.STATUS_GATE and model.engine_code != 0:
        raise _lib.RangeError(f"evaluate: |input| beyond the 16-bit modes' domain ({INPUT_GATE}, normalised "
                              f"intensity); evaluate this data in 'fp32'")


def _module_device(model):
    """Where a module lives: its first parameter's device, else (a parameter-free baseline filter) its first
    buffer's, else the current CUDA device."""
    for t in model.parameters():
        return t.device
    for t in model.buffers():
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _workspace(model, n, L, device):
    if (not _engine_module(model) or not engine.needs_workspace(model.ARCH, model.engine_code)
            or torch.device(device).type != "cuda"):
        return None
    return engine.Workspace(model.ARCH, model.engine_code, n, L, device)


class _Meters:
    """One model's exact accumulator and its optional SNR, PhysicsAwareLoss and blind reports: the forward +
    metrics of each batch go into ``acc`` (``per_spectrum``: the SNR report wants their per-spectrum
    output), add() runs the batch's report passes, summary() all-reduces and summarises."""

    def __init__(self, device, snr_bins, weights, blind=None):
        self.snr_bins, self.weights, self.blind = snr_bins, weights, blind
        self.phys_bins = snr_bins if snr_bins is not None else (0.0, 1.0, 1)      # unbinned: one bin, no key
        self.acc = engine.new_acc(device)
        self.report = engine.new_report(engine._bins(snr_bins)[2], device) if snr_bins is not None else None
        self.phys_rep = (engine.new_physics_report(engine._bins(self.phys_bins)[2], device)
                         if weights is not None else None)
        self.blind_rep = (engine.new_blind_report(engine._bins(self.phys_bins)[2], device)
                          if blind is not None else None)
        self.per_spectrum = self.report is not None

    def add(self, x, y, clean, per, key):
        """The SNR pass, then the physics pass, then the blind pass, of a batch (``per``: its per-spectrum
        metrics; ``key``: its nominal SNRs or None, which bins by the measured SNR_in)."""
        if self.report is None:
            key = None
        else:
            # without nominal SNRs the physics and blind reports need the key rdn_snr bins by: its SNR_in in fp32
            keyed = self.phys_rep is not None or self.blind_rep is not None
            per3, _ = engine.snr(x, y, clean, key=key, bins=self.snr_bins, per4=per, report=self.report,
                                 per_spectrum=keyed and key is None)
            if per3 is not None:
                key = per3[:, 0].to(torch.float32).contiguous()
        if self.phys_rep is not None:
            engine.physics(x, y, clean, weights=self.weights, key=key, bins=self.phys_bins, report=self.phys_rep,
                           per_spectrum=False)
        if self.blind_rep is not None:
            # unbinned (no snr_bins): the one-bin report's rows split by SNR_est, only their total is read
            engine.blind(x, y, lags=self.blind[0], q_crit=self.blind[2], key=key, bins=self.phys_bins,
                         report=self.blind_rep, per_spectrum=False)

    def summary(self, L, words=False):
        """All-reduce the accumulator and the reports: (means, what snr_bins / physics add to a result --
        with ``words`` the all-reduced report words too)."""
        means = means_from_acc(_all_reduce_acc(self.acc))
        extra = {}
        if self.report is not None:
            extra.update(snr_summary(_all_reduce_acc(self.report), self.snr_bins))
            if words:
                extra["report"] = self.report.cpu().tolist()
        if self.phys_rep is not None:
            extra["physics"] = physics_summary(_all_reduce_acc(self.phys_rep), self.weights, L, self.snr_bins)
            if words:
                extra["physics"]["report"] = self.phys_rep.cpu().tolist()
        if self.blind_rep is not None:
            extra["blind"] = blind_summary(_all_reduce_acc(self.blind_rep), self.blind, self.snr_bins)
            if words:
                extra["blind"]["report"] = self.blind_rep.cpu().tolist()
        return means, extra


def evaluate(model, noisy_data, clean_data, batch_size=1024, device=None, snr_bins=None, snrs=None, physics=None,
             blind=None):
    """evaulate.py:25-39 batched on the device.  Inputs beyond the 16-bit modes' domain (|x| > 4) or
    activations beyond the e4m3 planes' range raise RangeError after the run (one check at the end,
    no per-batch wait) -- unlike the module's own forward, which re-runs such a batch in fp32: evaluate
    such data with the module in 'fp32'.

    ``snr_bins`` = (lo, hi, nbins) additionally runs the SNR pass on every batch (engine.snr) and adds
    snr_summary's keys to the result: the mean SNR_in, SNR_out and SNR_gain in dB and ``by_snr``, the
    seven means per bin of ``snrs`` -- the dataset's nominal SNR per spectrum (the ``snrs`` array of a
    test.npz), or, when None, the measured SNR_in.  The report is all-reduced like the accumulator.

    ``physics`` = True (the reference's weights 0.1, 0.05, 0.01) or (alpha, beta, gamma) additionally runs
    the PhysicsAwareLoss pass on every batch (engine.physics) and adds one key, ``"physics"``
    (physics_summary): the terms PIDN / APIDN were trained against, their weighted total and -- with
    ``snr_bins`` -- the same per bin of the key the SNR report bins by.

    ``blind`` = True (16 lags, alpha = 0.01) or {"lags": ..., "alpha": ...} additionally runs the blind
    residual pass on every batch (engine.blind with its own noise estimate) and adds one key, ``"blind"``
    (blind_summary), binned like the physics entry: the numbers evaluate_blind gives without ``clean``,
    here beside the true SNR gain that calibrates them."""
    model.eval()
    if device is None:
        device = _module_device(model)
    device = torch.device(device)
    noisy = _as_rows(noisy_data)
    clean = _as_rows(clean_data)
    if noisy.shape != clean.shape:
        raise ValueError(f"noisy {tuple(noisy.shape)} vs clean {tuple(clean.shape)}")
    lo, hi = shard(noisy.shape[0])
    L = noisy.shape[1]
    if device.type != "cuda":
        raise RuntimeError("raman_mi355x.evaluate runs its metrics on the GPU; on a CPU device use the module "
                           "itself in the reference's evaulate.py loop (its forward falls back to eager PyTorch)")
    m = _Meters(device, snr_bins, _physics_weights(physics), _blind_options(blind))
    if snrs is not None:
        if snr_bins is None:
            raise ValueError("snrs is the binning key of the SNR report: pass snr_bins=(lo, hi, nbins)")
        snrs = torch.as_tensor(np.asarray(snrs.cpu() if torch.is_tensor(snrs) else snrs), dtype=torch.float32).reshape(-1)
        if snrs.numel() != noisy.shape[0]:
            raise ValueError(f"snrs has {snrs.numel()} values for {noisy.shape[0]} spectra")
    ws = _workspace(model, min(batch_size, max(hi - lo, 1)), L, device)
    # fp64 clean stays fp64 (the metrics compare against the same float64 values as evaulate.py)
    cdt = torch.float64 if (clean.dtype == torch.float64 if torch.is_tensor(clean) else clean.dtype == np.float64) \
        else torch.float32
    with torch.no_grad():
        for b0 in range(lo, hi, batch_size):
            b1 = min(hi, b0 + batch_size)
            x = torch.as_tensor(noisy[b0:b1], dtype=torch.float32).to(device).unsqueeze(1)
            c = torch.as_tensor(clean[b0:b1], dtype=cdt).to(device)
            if _engine_module(model) and model.uses_engine(x):
                # the engine's forward + metric sums (fused into the forward kernel on the walk geometry)
                y, per, _, _ = engine.forward_metrics(model.ARCH, model.engine_code, model.packed_weights(x.device), x, c,
                                                      acc=m.acc, per_spectrum=m.per_spectrum, check=False, workspace=ws)
            else:
                y = model(x)
                per, _ = engine.metrics(y.squeeze(1), c, per_spectrum=m.per_spectrum, acc=m.acc)
            m.add(x, y, c, per, snrs[b0:b1].to(device) if snrs is not None else None)
    _finish(model, ws)
    means, extra = m.summary(L)
    means.update(extra)
    return means


def evaluate_synthetic(models, total, seed=20250410, signal_length=10000, batch_size=8192, device=None,
                       first_index=0, gen_kwargs=None, log_every_s=0.0, fused_metrics=True, snr_bins=None,
                       physics=None, blind=None):
    """Config 4: ``total`` simulator spectra [first_index, first_index + total),
    sharded over the ranks as [r·N/W, (r+1)·N/W), each chunk generated on the device, denoised by
    every model in ``models`` (name -> module) and metered into that model's exact accumulator.  A module
    that is not one of the engine's networks (a baseline filter of baselines.py, any ``nn.Module`` mapping
    (N, 1, L) to (N, 1, L) on the device) runs its own forward and then the metrics kernel; it feeds the same
    accumulator and reports, so its entry has a network's guarantees as far as its forward is deterministic.
    Returns {name: {"means", "spectra", "seconds", "spectra_per_s"}} with the all-reduced means
    (identical for any world size) and the max-over-ranks wall time of the loop.  ``log_every_s`` > 0
    prints progress to stderr about that often (the loop then waits for the device every 64 chunks,
    so the printed count is what the GPU has finished).  ``fused_metrics=False`` meters with the separate
    metrics kernel after each forward (the A/B of the metric epilogue; the same bits).
    ``snr_bins`` = (lo, hi, nbins) additionally runs the SNR pass on every chunk, binned by the
    generator's nominal SNR (its ``snr_db``), and adds snr_summary's keys (SNR_in, SNR_out, SNR_gain,
    by_snr, ...) and the all-reduced ``report`` words to each model's entry -- the same bits for any world
    size or batch size, like the means.
    ``physics`` = True or (alpha, beta, gamma) additionally runs the PhysicsAwareLoss pass on every chunk
    (binned by the nominal SNR when ``snr_bins`` is given) and adds ``"physics"`` (physics_summary, with
    the all-reduced ``report`` words) to each model's entry -- exact accumulators, the same bits likewise.
    ``blind`` = True or {"lags": ..., "alpha": ...} additionally runs the blind residual pass on every chunk
    (binned by the nominal SNR when ``snr_bins`` is given) and adds ``"blind"`` (blind_summary, with the
    all-reduced ``report`` words) to each model's entry, likewise."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    gen_kwargs = gen_kwargs or {}
    weights = _physics_weights(physics)
    blind = _blind_options(blind)
    rank, W = world()
    lo, hi = shard(total, rank, W)
    L = int(signal_length)
    B = max(1, min(batch_size, hi - lo)) if hi > lo else 1
    clean = torch.empty((B, L), dtype=torch.float32, device=device)
    noisy = torch.empty((B, L), dtype=torch.float32, device=device)
    y = torch.empty((B, 1, L), dtype=torch.float32, device=device)
    out = {}
    with torch.no_grad():
        for name, model in models.items():
            model.eval()
            m = _Meters(device, snr_bins, weights, blind)
            ws = _workspace(model, B, L, device)
            eng = _engine_module(model)          # any other module (baselines.py) runs its own forward
            packed = model.packed_weights(device) if eng else None
            if dist.is_available() and dist.is_initialized():
                dist.barrier()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            t_log = t0
            for i, b0 in enumerate(range(lo, hi, B)):
                if log_every_s > 0 and i % 64 == 63:
                    torch.cuda.synchronize(device)
                    if time.perf_counter() - t_log >= log_every_s:
                        t_log = time.perf_counter()
                        print(f"[evaluate_synthetic rank {rank}] {name}: {b0 - lo} / {hi - lo} spectra, "
                              f"{t_log - t0:.1f} s", file=sys.stderr, flush=True)
                nb = min(B, hi - b0)
                _, _, snr_db, _ = engine.generate(nb, seed, first_index=first_index + b0, signal_length=L, device=device,
                                                  out=(clean[:nb], noisy[:nb]), **gen_kwargs)
                if not eng:
                    yb = model(noisy[:nb].view(nb, 1, L))
                    per, _ = engine.metrics(yb.reshape(nb, L), clean[:nb], per_spectrum=m.per_spectrum, acc=m.acc)
                    m.add(noisy[:nb], yb, clean[:nb], per, snr_db)
                    continue
                # forward + metric sums in one call: on the walk geometry the forward kernel meters each
                # spectrum itself (no second pass over y); otherwise the metrics kernel follows it
                if fused_metrics:
                    _, per, _, _ = engine.forward_metrics(model.ARCH, model.engine_code, packed, noisy[:nb].view(nb, 1, L),
                                                          clean[:nb], out=y[:nb], acc=m.acc, per_spectrum=m.per_spectrum,
                                                          check=False, workspace=ws)
                else:
                    engine.forward(model.ARCH, model.engine_code, packed, noisy[:nb].view(nb, 1, L), out=y[:nb],
                                   check=False, workspace=ws)
                    per, _ = engine.metrics(y[:nb].view(nb, L), clean[:nb], per_spectrum=m.per_spectrum, acc=m.acc)
                m.add(noisy[:nb], y[:nb], clean[:nb], per, snr_db)       # binned by the generator's nominal SNR
            _finish(model, ws)              # waits for the stream; raises on a timed-out hand-off / range / gate
            torch.cuda.synchronize(device)
            el = time.perf_counter() - t0
            t = torch.tensor([el], dtype=torch.float64)
            if dist.is_available() and dist.is_initialized() and W > 1:
                tt = t.to(device) if dist.get_backend() != "gloo" else t
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                t = tt.cpu()
            means, extra = m.summary(L, words=True)
            el = float(t.item())
            out[name] = {"means": means, "acc": m.acc.cpu().tolist(), "spectra": int(total),
                         "seconds": el, "spectra_per_s": total / el if el > 0 else None, **extra}
    return out


def evaluate_blind(model, noisy_data, batch_size=1024, device=None, lags=16, alpha=0.01, bins=None, sigma=None):
    """What can be said about ``model``'s output on spectra that have no clean reference (measured traces):
    the residual analysis of engine.blind over ``noisy_data`` (N, L) or (N, 1, L), in batches on the device.
    Returns blind_summary's entry: ``lags``, ``alpha``, ``q_crit`` = blind_q_crit(lags, alpha), ``count``, the
    means of Mean, RMS, Ratio, Rho1, RhoMax, Q and SNR_est and ``flagged_fraction``; with ``bins`` = (lo, hi,
    nbins) also ``by_snr`` / ``under`` / ``over``, the same per bin of the estimated input SNR (SNR_est, dB).
    ``sigma``: None, each spectrum's own blind estimate (noise_mad(x) sqrt(2) / 0.6745); a float for all
    spectra; or N values, one per spectrum.  Under torch.distributed each rank evaluates its shard and the
    report is all-reduced: exact accumulators, the same bits for any batch size or world size."""
    model.eval()
    if device is None:
        device = _module_device(model)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("raman_mi355x.evaluate_blind runs its residual analysis on the GPU")
    options = _blind_options({"lags": lags, "alpha": alpha})
    noisy = _as_rows(noisy_data)
    lo, hi = shard(noisy.shape[0])
    if sigma is not None and not isinstance(sigma, (int, float)):
        sigma = torch.as_tensor(np.asarray(sigma.cpu() if torch.is_tensor(sigma) else sigma), dtype=torch.float64).reshape(-1)
        if sigma.numel() != noisy.shape[0]:
            raise ValueError(f"sigma has {sigma.numel()} values for {noisy.shape[0]} spectra")
    rep_bins = bins if bins is not None else (0.0, 1.0, 1)      # unbinned: only the totals are read
    report = engine.new_blind_report(engine._bins(rep_bins)[2], device)
    with torch.no_grad():
        for b0 in range(lo, hi, batch_size):
            b1 = min(hi, b0 + batch_size)
            x = torch.as_tensor(noisy[b0:b1], dtype=torch.float32).to(device).unsqueeze(1).contiguous()
            y = model(x)
            s = sigma[b0:b1].to(device) if torch.is_tensor(sigma) else sigma
            engine.blind(x, y.contiguous(), sigma=s, lags=options[0], q_crit=options[2], bins=rep_bins, report=report,
                         per_spectrum=False)
    return blind_summary(_all_reduce_acc(report), options, bins)


def write_metrics(metrics, root="eval_results"):
    """evaulate.py:78-80's metrics.txt; what ``snr_bins`` / ``physics`` added to a result goes to
    write_snr_report / write_physics_report."""
    save_dir = os.path.join(root, datetime.now().strftime("%Y%m%d_%H%M%S"))
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "metrics.txt"), "w") as f:
        for k, v in metrics.items():
            if k not in _EXTRA_RESULT_KEYS:
                f.write(f"{k}: {v:.6f}\n")
    return save_dir


def _write_table(f, cols, entries, fmt):
    """One line per entry (a summary's under / by_snr / over): its edges, its count and ``cols`` ('-' for a
    mean an empty bin does not have)."""
    f.write("lo hi count " + " ".join(cols) + "\n")
    for e in entries:
        f.write(f"{e['lo']:.4f} {e['hi']:.4f} {e['count']} "
                + " ".join(format(e[k], fmt) if k in e else "-" for k in cols) + "\n")


def write_snr_report(result, root):
    """Write the SNR part of an ``evaluate(..., snr_bins=...)`` result into the directory ``root`` (e.g.
    the one write_metrics returned, beside its metrics.txt): ``snr_report.json`` (the SNR keys as they
    are) and ``snr_report.txt``, a table with one line per bin."""
    import json
    if "by_snr" not in result:
        raise ValueError("the result has no SNR report: evaluate with snr_bins=(lo, hi, nbins)")
    os.makedirs(root, exist_ok=True)
    part = {k: result[k] for k in _SNR_RESULT_KEYS}
    with open(os.path.join(root, "snr_report.json"), "w") as f:
        json.dump(part, f, indent=1)
    cols = engine.REPORT_QUANTITIES
    with open(os.path.join(root, "snr_report.txt"), "w") as f:
        for k in SNR_KEYS:
            f.write(f"{k}: {result[k]:.6f}\n")
        _write_table(f, cols, [result["snr_under"]] + list(result["by_snr"]) + [result["snr_over"]], ".6f")
    return root


def write_physics_report(result, root):
    """Write the ``"physics"`` entry of an ``evaluate(..., physics=...)`` result into the directory ``root``
    (e.g. the one write_metrics returned): ``physics_report.json`` (the entry as it is) and
    ``physics_report.txt`` -- the weights, the means, and with ``snr_bins`` a table with one line per bin."""
    import json
    if "physics" not in result:
        raise ValueError("the result has no physics report: evaluate with physics=True or (alpha, beta, gamma)")
    os.makedirs(root, exist_ok=True)
    part = result["physics"]
    with open(os.path.join(root, "physics_report.json"), "w") as f:
        json.dump(part, f, indent=1)
    cols = PHYS_KEYS + ("PeakMasked",)
    with open(os.path.join(root, "physics_report.txt"), "w") as f:
        f.write("weights: " + " ".join(f"{w:g}" for w in part["weights"]) + "\n")
        f.write(f"count: {part['count']}\n")
        for k in cols:
            f.write(f"{k}: {part[k]:.6e}\n")
        if "by_snr" in part:
            _write_table(f, cols, [part["under"]] + list(part["by_snr"]) + [part["over"]], ".6e")
    return root


def write_blind_report(result, root):
    """Write an ``evaluate_blind`` result, or the ``"blind"`` entry of an ``evaluate(..., blind=...)`` result,
    into the directory ``root``: ``blind_report.json`` (the entry as it is) and ``blind_report.txt`` -- the
    lags, alpha and q_crit, the means and the flagged share, and with bins a table with one line per bin."""
    import json
    part = result.get("blind", result)
    if not isinstance(part, dict) or "flagged_fraction" not in part:
        raise ValueError("the result has no blind report: use evaluate_blind, or evaluate with blind=True")
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "blind_report.json"), "w") as f:
        json.dump(part, f, indent=1)
    cols = BLIND_KEYS + ("flagged_fraction",)
    with open(os.path.join(root, "blind_report.txt"), "w") as f:
        f.write(f"lags: {part['lags']}\nalpha: {part['alpha']:g}\nq_crit: {part['q_crit']:.6f}\n")
        f.write(f"count: {part['count']}\n")
        for k in cols:
            f.write(f"{k}: {part[k]:.6e}\n")
        if "by_snr" in part:
            _write_table(f, cols, [part["under"]] + list(part["by_snr"]) + [part["over"]], ".6e")
    return root


COMPARISON_KEYS = KEYS + SNR_KEYS


def write_comparison(results, root):
    """One line per model of an ``evaluate_synthetic`` result -- or of a dict name -> ``evaluate`` result --
    into the directory ``root``: ``comparison.json`` (name -> its four means and, where the run had
    ``snr_bins``, SNR_in, SNR_out and SNR_gain) and ``comparison.txt``, the same as a table ('-' where a run
    had no SNR report).  Networks and baseline filters (baselines.py) evaluated by one call stand side by
    side."""
    import json
    table = {}
    for name, r in results.items():
        means = r["means"] if "means" in r else r
        row = {k: float(means[k]) for k in KEYS}
        row.update({k: float(r[k]) for k in SNR_KEYS if k in r})
        table[name] = row
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "comparison.json"), "w") as f:
        json.dump(table, f, indent=1)
    with open(os.path.join(root, "comparison.txt"), "w") as f:
        f.write("model " + " ".join(COMPARISON_KEYS) + "\n")
        for name, row in table.items():
            f.write(name + " " + " ".join(format(row[k], ".6e" if k in KEYS else ".4f") if k in row else "-"
                                          for k in COMPARISON_KEYS) + "\n")
    return root
