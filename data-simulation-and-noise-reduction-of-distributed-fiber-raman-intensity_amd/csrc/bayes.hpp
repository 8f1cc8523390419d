// The Bayesian change-point smoother: what the host (abi.cpp) and the kernel (bayes.hip) share.
// The arithmetic contract: include/raman_mi355x.h (rdn_bayes_steps); the design: DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/raman_mi355x.h"

namespace rdn {
namespace bayes {

constexpr int THREADS = 256;                                  // 4 independent waves, a spectrum each
constexpr int WAVES = THREADS / 64;
constexpr int MAX_LEN = RDN_BAYES_MAX_LEN;                    // the longest run: one candidate per lane

static_assert(MAX_LEN == 64, "lane j of a wave holds the one open candidate whose boundary is j mod 64");

}  // namespace bayes

hipError_t launch_bayes_steps(const float* x, float* y, float* jump, double* logz, const double* sigma, int64_t n,
                              int L, int max_len, double level_range, double* work, hipStream_t s);

}  // namespace rdn
