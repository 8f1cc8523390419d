// Which tile geometry a fused network's forward runs on (abi.cpp forward_impl): a pure function of the
// launch, tested without a device (host_check.cpp).  The tile sizes stay with the kernels (common.hpp).
#pragma once
#include "common.hpp"

namespace rdn {

enum class Geometry { Tiled, Short, Walk };

// cus: compute units of the launch's device (<= 0: unknown, Tiled); short_override / walk_override: the
// RDN_SHORT_TILES / RDN_WALK knobs, 0 or 1 forcing either answer (tests compare the geometries), else none.
// Only RDN_F16 and RDN_F16MIX leave Tiled.  Short, the latency geometry: a launch whose 640-row tiles would
// occupy at most half the CUs (the reference's evaulate.py calls the model one spectrum at a time: 18
// workgroups at L = 10,000) runs on 256-row tiles instead (2.8x the workgroups, each layer ~0.4x as long).
// Walk (one workgroup walks a whole spectrum, no halo recompute: fused16_walk.hip for RDN_F16 on the networks
// with a walk_shift, rrcdnet_hybrid_walk.hpp for RDN_F16MIX RRCDNet, both in 576-row tiles) when its predicted
// time -- rounds of the CUs x tiles per spectrum x rows per tile -- is below that of the 640-row tiles
// (rounds x 640 rows): large batches.
inline Geometry forward_geometry(int arch, int dtype, int64_t n, int64_t L, int64_t cus, int short_override, int walk_override) {
  if (dtype != RDN_F16 && dtype != RDN_F16MIX) return Geometry::Tiled;
  const int64_t T = H16_WB - 2 * fused_halo(arch), tiles = (L + T - 1) / T;
  if (short_override == 1 || (short_override != 0 && cus > 0 && 2 * n * tiles <= cus)) return Geometry::Short;
  if (!walk_shift(arch)) return Geometry::Tiled;
  if (walk_override == 0 || walk_override == 1) return walk_override == 1 ? Geometry::Walk : Geometry::Tiled;
  if (cus <= 0) return Geometry::Tiled;
  const int64_t rows = dtype == RDN_F16MIX ? RDN_WALK_ROWS_MIX : H16_WALK_ROWS;
  const int64_t wt = (L + walk_shift(arch) + rows - 1) / rows;
  const int64_t walk_rows = (n + cus - 1) / cus * wt * rows;
  const int64_t tile_rows = (n * tiles + cus - 1) / cus * H16_WB;
  return walk_rows < tile_rows ? Geometry::Walk : Geometry::Tiled;
}

}  // namespace rdn
