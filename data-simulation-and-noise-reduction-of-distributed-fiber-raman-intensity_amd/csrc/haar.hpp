// Translation-invariant Haar shrinkage: what the host (abi.cpp) and the kernels (haar.hip) share -- the tile
// geometry, the LDS sizes and the launcher.
// The arithmetic contract: include/raman_mi355x.h (rdn_haar_shrink); the design: DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/raman_mi355x.h"

namespace rdn {
namespace haar {

constexpr int THREADS = 256;                                  // 4 waves
constexpr int TILE = RDN_HAAR_TILE;                           // outputs of one shrink workgroup
constexpr int MAX_LEVELS = RDN_HAAR_MAX_LEVELS;
constexpr int MAX_H = (1 << MAX_LEVELS) - 1;                  // the widest halo, each side
constexpr int SELECT_LDS_L = RDN_HAAR_SELECT_LDS_L;           // the longest row the select kernel keeps in LDS

// the thresholds' factors, as kernel arguments (entries past `levels` are 0)
struct Factors {
  double k[MAX_LEVELS];
};

// staged samples of a shrink tile at J levels: the tile and a halo of 2^J - 1 on each side
__host__ __device__ constexpr int staged(int levels) { return TILE + 2 * ((1 << levels) - 1); }
// dynamic LDS of the shrink kernel: two ping-pong planes for a / b and one plane per level for e, fp64
__host__ __device__ constexpr int shrink_lds_bytes(int levels) { return (levels + 2) * staged(levels) * (int)sizeof(double); }

static_assert(shrink_lds_bytes(MAX_LEVELS) <= 64 * 1024, "the shrink kernel's planes fit the default dynamic LDS limit");
static_assert(SELECT_LDS_L * sizeof(float) <= 48 * 1024, "the select kernel's row is static LDS");
static_assert(MAX_H < TILE, "a halo is shorter than a tile");

}  // namespace haar

hipError_t launch_haar_shrink(const float* x, float* y, double* med, int64_t n, int L, int levels,
                              const haar::Factors& k, int mode, hipStream_t s);
// the median |d_1| of each spectrum alone: the select kernel of launch_haar_shrink, any L >= 1
hipError_t launch_noise_mad(const float* x, double* med, int64_t n, int L, hipStream_t s);

}  // namespace rdn
