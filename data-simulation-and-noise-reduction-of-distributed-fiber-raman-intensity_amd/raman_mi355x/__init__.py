"""raman_mi355x — MI355X-native (gfx950) batched inference engine for the Raman denoising networks
of 223qyc/Data-simulation-and-noise-reduction-of-distributed-fiber-Raman-intensity.

Drop-in surfaces (reference file:line):
  DenoiseCNN, RRCDNet, DSDN, ADSDN, PIDN, APIDN   */train.py model classes (models.py)
  generate_signals                                数据集产生.py:5-64 (simulator.py, on-device)
  evaluate, compute_*                             */evaulate.py:14-39 (evaluate.py, batched, on-device)
  evaluate(..., snr_bins=), write_snr_report      SNR_in / SNR_out / gain and the metrics by SNR bin (engine.snr)
  PhysicsAwareLoss                                PIDN|APIDN/train.py loss class (physics.py: value on device; gradient eager,
                                                  or from the same launch with fused_backward=True: engine.physics_grad)
  evaluate(..., physics=), write_physics_report   the loss's terms over a test set, by SNR bin (engine.physics)
  MovingAverage, SavitzkyGolay, GaussianSmooth,   the classical filters a result is compared with, on the device
  MedianFilter, write_comparison                  (baselines.py, engine.fir / engine.median; no reference counterpart)
  HaarShrink, haar_thresholds                     translation-invariant Haar wavelet shrinkage with a blind per-spectrum
                                                  noise estimate (wavelets.py, engine.haar_shrink; no reference counterpart)
  evaluate_blind, evaluate(..., blind=),          residual analysis of spectra WITHOUT a clean reference (measured traces):
  write_blind_report, blind_q_crit                residual RMS against the noise estimate, autocorrelation, Ljung-Box Q
                                                  (engine.blind; no reference counterpart)
  PottsFit                                        the exact piecewise-constant (jump-penalised least-squares) fit with the same
                                                  noise estimate (potts.py, engine.potts; no reference counterpart)
  BayesSteps                                      the posterior mean under the simulator's own signal model, the jump
                                                  probability of every sample and the log evidence (bayes.py,
                                                  engine.bayes_steps; no reference counterpart)
"""
from . import engine
from .bayes import BayesSteps
from .baselines import (BASELINES, GaussianSmooth, MedianFilter, MovingAverage, SavitzkyGolay, gaussian_taps,
                        savgol_taps)
from ._lib import EngineError, RangeError
from .dataset import load_dataset, save_dataset
from .distributed import all_reduce_sums, shard
from .evaluate import (blind_q_crit, evaluate, evaluate_blind, evaluate_synthetic, write_blind_report, write_comparison,
                       write_metrics, write_physics_report, write_snr_report)
from .models import ADSDN, APIDN, DSDN, MODELS, PIDN, DenoiseCNN, RRCDNet
from .physics import PhysicsAwareLoss
from .potts import PottsFit
from .simulator import generate, generate_signals
from .wavelets import HaarShrink, haar_thresholds

__all__ = ["engine", "DenoiseCNN", "RRCDNet", "DSDN", "ADSDN", "PIDN", "APIDN", "MODELS", "generate",
           "generate_signals", "evaluate", "write_metrics", "write_snr_report", "load_dataset", "save_dataset", "shard",
           "all_reduce_sums", "EngineError", "RangeError", "PhysicsAwareLoss", "write_physics_report", "evaluate_synthetic",
           "write_comparison", "BASELINES", "MovingAverage", "SavitzkyGolay", "GaussianSmooth", "MedianFilter", "savgol_taps",
           "gaussian_taps", "HaarShrink", "haar_thresholds", "PottsFit", "BayesSteps", "evaluate_blind", "blind_q_crit",
           "write_blind_report"]
