// pp2_policy.h -- shared between the policy evaluator's kernels
// (pp2_policy.hip) and their host side (pp2_policy.cpp).  The definition of
// the outcome fields is in include/pp2.h ("policy evaluation"); DESIGN.md §2.4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pp2_internal.h"

namespace pp2 {

// The tile of the PP2_POLICY_TILES route.  A workgroup's LDS region is the
// tile plus a ring `block` cells deep; lane = region column, so the region is
// at most one wavefront wide: kPolicyTileCols + 2 * kPolicyMaxBlock = 64.
constexpr int kPolicyTileRows = 32;
constexpr int kPolicyTileCols = 48;
constexpr int kPolicyThreads = 256;
constexpr int kPolicyMaxBlock = 8;
// steps per launch when the caller passes block = 0 (DESIGN.md §2.4:
// profiles/policy/policy_eval_timing.json)
constexpr int kPolicyDefaultBlock = 4;
static_assert(kPolicyTileCols + 2 * kPolicyMaxBlock == 64, "lane = region column");

// Per-cell class byte of the TILES route: 16 * u + (pair class of the cell's
// dictionary entry for u = pi[x]) addresses the factored tables QT / CT (sweep
// rows) and QR (class tables) of pp2_internal.h; two more for the pinned cells.
constexpr int kPolicyClsOff = 9 * kFactK;       // off the grid: G = P = N = +0
constexpr int kPolicyClsGoal = 9 * kFactK + 1;  // the goal: G = +0, P = 1, N = +0
constexpr int kPolicyClasses = 9 * kFactK + 2;

__host__ __device__ inline int policy_tiles_x(const Geom& g) { return (g.width + kPolicyTileCols - 1) / kPolicyTileCols; }
__host__ __device__ inline int policy_tiles_y(const Geom& g) { return (g.rows + kPolicyTileRows - 1) / kPolicyTileRows; }
size_t policy_tile_lds_bytes(int block);

// The three planes of one side of the ping-pong: [rows][width] each, row
// stride g.width (no halo, no pads: a neighbour off the grid reads +0).
struct PolicyPlanes {
  float* G;
  float* P;
  float* N;
};

// All launchers are asynchronous on `st`; unsharded geometries only.  pi is
// the action table, row stride pis (entries <= 8).
// The start planes: +0 everywhere, P = 1 at a goal on the grid.
hipError_t launch_policy_init(hipStream_t st, const Geom& g, int gx, int gy, PolicyPlanes out);
// One step from the dense planes T (81) and C (9) of the world.
hipError_t launch_policy_step(hipStream_t st, const Geom& g, float gamma, PlaneSet T, PlaneSet C,
                              const uint8_t* pi, int pis, int gx, int gy, PolicyPlanes in,
                              PolicyPlanes out);
// cls[y * width + x] of the world's coded model (code plane at (row 0, x 0),
// factored sweep rows) under pi; kPolicyClsGoal at the goal.
hipError_t launch_policy_classes(hipStream_t st, const Geom& g, const uint16_t* code,
                                 const float* rows, const uint8_t* pi, int pis, int gx, int gy,
                                 uint8_t* cls);
// `steps` <= block <= kPolicyMaxBlock steps of every tile in one launch, the
// ring `block` cells deep.
hipError_t launch_policy_tiles(hipStream_t st, const Geom& g, const float* rows,
                               const float* rfact, const uint8_t* cls, int block, int steps,
                               PolicyPlanes in, PolicyPlanes out);

}  // namespace pp2
