// PhysicsAwareLoss report and gradient: what the host (abi.cpp) and the kernel (physics.hip) share -- the
// arguments of a launch.  Definitions and report layout: include/raman_mi355x.h (rdn_physics,
// rdn_physics_grad).
//
// Reference: PIDN/train.py:109-146 (APIDN/train.py:162-199 is the same class): the loss PIDN and APIDN
// are trained against, MSE + alpha * smoothness + beta * peak retention + gamma * noise model.
#pragma once
#include "common.hpp"
#include "report.hpp"

namespace rdn {
namespace phys {

// where a launch's results go (per6 / report / grad may be NULL; key only with a report).  The values
// (per6, report) and the gradient are separate parts of the kernel, each compiled out when not asked for.
struct PhysOut {
  double* per6;          // fp64 [n][6] {MSE, Smooth, Peak, Noise, Total, PeakCount}
  const float* key;      // fp32 [n] binning key, NULL: every spectrum into row 1
  long long* report;     // RDN_PHYS_WORDS(bins.nbins) int64, accumulated
  Bins bins;
  double alpha, beta, gamma;
  float* grad;           // fp32 [n][L] scale * d Total / d y, written (rdn_physics_grad)
  double scale;          // of the gradient: one value per call, whatever the launch chunks
};

}  // namespace phys
}  // namespace rdn
