// Blind residual report: what the host (abi.cpp) and the kernel (blind.hip) share -- the arguments of a
// launch and the LDS staging limit.  Definitions, report layout: include/raman_mi355x.h (rdn_blind); the
// bin formula: report.hpp; the design: DESIGN.md §3.
#pragma once
#include "common.hpp"
#include "report.hpp"

namespace rdn {
namespace blind {

constexpr int MAX_LAGS = RDN_BLIND_MAX_LAGS;
// the longest spectrum whose residual is staged in LDS as fp64: 160000 B of dynamic LDS, beside the 64 B of
// reduction scratch, out of the 163840 B of a CU
constexpr int LDS_L = RDN_BLIND_LDS_L;
constexpr unsigned LDS_MAX_BYTES = (unsigned)LDS_L * 8u;
static_assert(LDS_MAX_BYTES + 64u <= 163840u, "the staged residual and the reduction scratch fit one CU's LDS");

// where a launch's results go (per7 / rho / report may each be NULL; key only with a report)
struct BlindOut {
  double* per7;          // fp64 [n][7] {Mean, RMS, Ratio, Rho1, RhoMax, Q, SNR_est}
  double* rho;           // fp64 [n][lags] {rho_1 .. rho_K}
  const float* key;      // fp32 [n] binning key, NULL: SNR_est rounded to fp32
  long long* report;     // RDN_BLIND_WORDS(bins.nbins) int64, accumulated
  Bins bins;
  double q_crit;         // flagged = Q > q_crit
  int lags;              // K
};

}  // namespace blind

hipError_t launch_blind(const float* x, const float* y, const double* sigma, int64_t n, int L,
                        const blind::BlindOut& bo, hipStream_t s);

}  // namespace rdn
