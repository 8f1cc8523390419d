// SNR report: what the host (abi.cpp) and the kernel (snr.hip) share -- the bin formula and the
// arguments of a launch.  Definitions and report layout: include/raman_mi355x.h (rdn_snr).
//
// Reference: 数据集产生.py:43-45 (signal_power = mean(clean^2), noise_std = sqrt(power / 10^(snr/10))):
// SNR_in measured with P = mean(clean^2) estimates the `snrs` the generator drew.
#pragma once
#include "common.hpp"

namespace rdn {
namespace snr {

// uniform bins of [lo, hi): scale = (float)nbins / (hi - lo), computed once on the host
struct Bins {
  float lo, hi, scale;
  int nbins;
};
inline Bins make_bins(float lo, float hi, int nbins) { return Bins{lo, hi, (float)nbins / (hi - lo), nbins}; }

// Report row of a key (raman_mi355x.h): every operation is one IEEE fp32 operation -- a subtraction and
// a multiplication, which no contraction can fuse -- so a numpy float32 restatement gives the same row.
__host__ __device__ inline int bin_row(float key, const Bins& b) {
  if (key != key) return b.nbins + 1;
  if (key < b.lo) return 0;
  if (key >= b.hi) return b.nbins + 1;
  const int i = (int)((key - b.lo) * b.scale);
  return 1 + (i < b.nbins - 1 ? i : b.nbins - 1);
}

// where a launch's results go (per3 / report may be NULL; key and per4 only with a report)
struct SnrOut {
  double* per3;          // fp64 [n][3] {SNR_in, SNR_out, SNR_gain}
  const float* key;      // fp32 [n] binning key, NULL: the measured SNR_in rounded to fp32
  const double* per4;    // fp64 [n][4] {MSE, SSIM, Smoothness, Peak2Peak} of the same spectra
  long long* report;     // RDN_REPORT_WORDS(bins.nbins) int64, accumulated
  Bins bins;
};

}  // namespace snr
}  // namespace rdn
