// SNR report: what the host (abi.cpp) and the kernel (snr.hip) share -- the arguments of a launch.
// Definitions and report layout: include/raman_mi355x.h (rdn_snr); the bin formula: report.hpp.
//
// Reference: 数据集产生.py:43-45 (signal_power = mean(clean^2), noise_std = sqrt(power / 10^(snr/10))):
// SNR_in measured with P = mean(clean^2) estimates the `snrs` the generator drew.
#pragma once
#include "common.hpp"
#include "report.hpp"

namespace rdn {
namespace snr {

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
