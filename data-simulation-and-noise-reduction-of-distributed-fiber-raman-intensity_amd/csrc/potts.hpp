// The exact piecewise-constant (Potts) fit: what the host (abi.cpp) and the kernel (potts.hip) share.
// The arithmetic contract: include/raman_mi355x.h (rdn_potts); the design: DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/raman_mi355x.h"

namespace rdn {
namespace potts {

constexpr int THREADS = 256;                                  // 4 independent waves, a spectrum each
constexpr int WAVES = THREADS / 64;
constexpr int MAX_LEN = RDN_POTTS_MAX_LEN;                    // the longest segment: one candidate per lane

static_assert(MAX_LEN == 64, "lane j of a wave holds the one open candidate whose start is j mod 64");

}  // namespace potts

hipError_t launch_potts(const float* x, float* y, int32_t* nseg, const double* gamma, int64_t n, int L, int max_len,
                        uint8_t* work, hipStream_t s);

}  // namespace rdn
