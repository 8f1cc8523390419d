// Binned reports: the bin formula that the host (abi.cpp) and the kernels of every binned report
// (snr.hip, physics.hip) share.  Report rows: include/raman_mi355x.h (rdn_snr).
#pragma once
#include "common.hpp"

namespace rdn {

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

}  // namespace rdn
