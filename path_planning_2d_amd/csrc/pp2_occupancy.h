// pp2_occupancy.h -- shared between the forward occupancy's kernels
// (pp2_occupancy.hip) and their host side (pp2_occupancy.cpp).  The definition
// of D, V and the curve is in include/pp2.h ("occupancy"); DESIGN.md §2.5.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pp2_internal.h"
#include "pp2_policy.h"

namespace pp2 {

// The tile of the PP2_OCC_TILES route: the evaluator's geometry (lane = region
// column, the region at most one wavefront wide) and its class bytes
// (launch_policy_classes: kPolicyClsOff / kPolicyClsGoal are the two pinned
// classes, whose gather weights are all +0).
constexpr int kOccTileRows = 32;
constexpr int kOccTileCols = 48;
constexpr int kOccThreads = 256;
constexpr int kOccMaxBlock = 8;
// steps per launch when the caller passes block = 0 (DESIGN.md §2.5:
// profiles/occupancy/occupancy_timing.json)
constexpr int kOccDefaultBlock = 8;
static_assert(kOccTileCols + 2 * kOccMaxBlock == 64, "lane = region column");

__host__ __device__ inline int occ_tiles_x(const Geom& g) { return (g.width + kOccTileCols - 1) / kOccTileCols; }
__host__ __device__ inline int occ_tiles_y(const Geom& g) { return (g.rows + kOccTileRows - 1) / kOccTileRows; }
size_t occ_tile_lds_bytes(int block);

// One side of the ping-pong: [rows][width] each, row stride g.width.
struct OccPlanes {
  float* D;
  float* V;
};

// All launchers are asynchronous on `st`; unsharded geometries only.  pi is
// the action table, row stride pis (entries <= 8); curve has horizon + 1
// floats, zeroed by the caller (no goal on the grid: nothing writes it).
// The start planes: D = b0 (canonical already), V = +0, curve[0] = D(goal).
hipError_t launch_occ_init(hipStream_t st, const Geom& g, int gx, int gy, const float* b0,
                           OccPlanes out, float* curve);
// The nine gather-weight planes of an evaluation, wts[i][y] =
// T[y - off_i][pi[y - off_i]][i], +0 where the source is off the grid or the goal.
hipError_t launch_occ_weights(hipStream_t st, const Geom& g, PlaneSet T, const uint8_t* pi, int pis,
                              int gx, int gy, float* wts);
// Step k from the weight planes; the goal's thread writes curve[k].
hipError_t launch_occ_step(hipStream_t st, const Geom& g, const float* wts, int gx, int gy, int k,
                           OccPlanes in, OccPlanes out, float* curve);
// `steps` <= block <= kOccMaxBlock steps of every tile in one launch, the ring
// `block` cells deep; steps k0 + 1 .. k0 + steps of the curve.
hipError_t launch_occ_tiles(hipStream_t st, const Geom& g, const float* rfact, const uint8_t* cls,
                            int block, int steps, int k0, OccPlanes in, OccPlanes out,
                            float* curve);

}  // namespace pp2
