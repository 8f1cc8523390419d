// Classical baseline filters (FIR with an optional edge table, running median): what the host (abi.cpp)
// and the kernels (filters.hip) share -- the tile geometry, the LDS layout and the launchers.
// The arithmetic contract: include/raman_mi355x.h (rdn_fir, rdn_median); the design: DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/raman_mi355x.h"

namespace rdn {
namespace filt {

constexpr int THREADS = 256;                                  // 4 waves
constexpr int PER_LANE = 8;                                   // consecutive outputs of one lane
constexpr int TILE = THREADS * PER_LANE;                      // outputs of one workgroup
constexpr int MAX_W = RDN_FILTER_MAX_WINDOW;
constexpr int MAX_H = (MAX_W - 1) / 2;
// staged samples: the tile, a halo of h on each side, and the PER_LANE samples the last lane's register
// window loads past its last tap (never used)
constexpr int STAGE = TILE + 2 * MAX_H + PER_LANE;
// A lane reads sample PER_LANE * lane + c: with one pad dword per 32 the 32 lanes of a read's lane group
// fall on 32 different banks (8 l + c + floor((8 l + c) / 32) mod 32 = 8 (l mod 4) + floor(l / 4) + c'),
// and a staging store of 32 consecutive samples meets one bank at most twice.
__host__ __device__ constexpr int lds_at(int i) { return i + (i >> 5); }
constexpr int STAGE_WORDS = lds_at(STAGE) + 1;

static_assert(TILE == RDN_FILTER_TILE, "the header's tile is the kernel's");
static_assert(MAX_W % 2 == 1 && MAX_H < TILE, "a spectrum's first h outputs lie in its first tile");

}  // namespace filt

hipError_t launch_fir(const float* x, float* y, int64_t n, int L, const double* taps, int w, const double* edge_taps,
                      hipStream_t s);
hipError_t launch_median(const float* x, float* y, int64_t n, int L, int w, hipStream_t s);

}  // namespace rdn
