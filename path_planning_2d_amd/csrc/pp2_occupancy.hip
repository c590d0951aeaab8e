// pp2_occupancy.hip -- gfx950 kernels of the forward occupancy (include/pp2.h
// "occupancy"): H steps that push a start distribution through
// the chain of an action table.  The adjoint of the policy evaluator's step:
// a destination cell y gathers from its nine sources x = y - off_i, each with
// the T row of its own action, entry i -- the transposed per-cell rows.
//
// Every step is a pure function of the previous planes, so how the cells of a
// step are spread over launches and workgroups cannot change a bit.  Two
// schedules:
//  * k_occ_step (PP2_OCC_PLANES): the nine gather weights of every cell are
//    fixed for the evaluation, so k_occ_weights materialises them once into
//    nine [H*W] planes (coalesced reads afterwards); then one launch per step,
//    one thread per cell;
//  * k_occ_tiles (PP2_OCC_TILES): `steps` <= block steps per launch.  A
//    workgroup keeps its kOccTileRows x kOccTileCols tile of D plus a ring
//    `block` cells deep in LDS (two sides, ping-pong) and steps the whole
//    region; what the region's outermost cells miss moves inwards one cell per
//    step and does not reach the tile (pp2_policy.hip has the same argument).
//    It reads the world's coded model through the evaluator's class bytes:
//    each workgroup expands the raw T support quads (QR) into a dense
//    nine-entry row per class in LDS, and each thread derives the nine gather
//    weights of its region cells once per launch and keeps them in registers
//    across the steps, next to V of its cells.  The two pinned classes (off
//    the grid, the goal) have all-zero rows, so a source off the grid and the
//    goal as a source need no branch; the goal as a destination starts its
//    chain from its own value.  A weight that is +0 contributes
//    fmaf(+0, v, acc) == acc: every v is finite and >= +0 under the route's
//    admission and no accumulator is -0.
// Flush-to-zero is the definition's, in code (pp2_device.h: ftz, fma_ftz; this
// file is built with IEEE subnormals): the model's entries are flushed where
// they are read, every result after its rounding; b0 arrives flushed.
//
// Lane = region column, row stride kS = 66 words: the nine LDS reads of a step
// are at the same nine offsets for all 64 lanes of a wave, so each is 64
// consecutive words -- a 32-lane half touches 32 distinct banks, no conflict
// (the evaluator's reads go where each lane's support points).  Wave w =
// region rows w, w + 4, ...  Every loop is bounded by a constant.
#include <hip/hip_runtime.h>

#include "pp2_device.h"
#include "pp2_occupancy.h"

namespace pp2 {
namespace {

constexpr int kTR = kOccTileRows, kTC = kOccTileCols;
constexpr int kS = 66;                               // LDS row stride of D (words)
constexpr int kCS = 68;                              // ... of the class bytes
constexpr int kMaxRH = kTR + 2 * kOccMaxBlock;       // region rows, at most
constexpr int kRowsPerWave = (kMaxRH + 3) / 4;
constexpr int kRowFloats = (9 * kPolicyClasses + 3) & ~3;  // dense rows, [class][9]
static_assert(kOccThreads == 256 && kPolicyClasses <= 256, "one staging pass, a class per byte");
static_assert(kOccTileRows == kPolicyTileRows && kOccTileCols == kPolicyTileCols, "one geometry");
static_assert(kCS % 4 == 0 && kCS >= 66, "class rows are filled as words");

__constant__ unsigned char cOccSupN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
__constant__ unsigned char cOccSup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5},
                                            {0, 3, 4, 6}, {4, 0, 0, 0}, {2, 4, 5, 8},
                                            {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};

__device__ __forceinline__ int plane_floats(int rh) { return (rh + 2) * kS; }

__global__ __launch_bounds__(kOccThreads) void k_occ_init(Geom g, int gx, int gy,
                                                          const float* __restrict__ b0,
                                                          OccPlanes out, float* __restrict__ curve) {
  const long long n = (long long)g.rows * g.width;
  const long long i = (long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (i >= n) return;
  const bool goal = gx >= 0 && gx < g.width && gy >= 0 && gy < g.rows &&
                    i == (long long)gy * g.width + gx;
  const float d = b0[i];
  out.D[i] = d;
  out.V[i] = 0.0f;
  if (goal) curve[0] = d;
}

__global__ __launch_bounds__(kOccThreads) void k_occ_weights(Geom g, PlaneSet T,
                                                             const uint8_t* __restrict__ pi,
                                                             int pis, int gx, int gy,
                                                             float* __restrict__ wts) {
  const int H = g.rows, W = g.width;
  const long long n = (long long)H * W;
  const long long cell = (long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (cell >= n) return;
  const int y = (int)(cell / W), x = (int)(cell % W);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int yy = y - (i / 3 - 1), xx = x - (i % 3 - 1);  // the source whose neighbour i is y
    const bool src = yy >= 0 && yy < H && xx >= 0 && xx < W && !(xx == gx && yy == gy);
    float w = 0.0f;
    if (src) {
      const int u = pi[(long long)yy * pis + xx];
      w = ftz(T.p[(long long)yy * T.rs + (long long)(9 * u + i) * T.ps + xx]);
    }
    wts[(long long)i * n + cell] = w;
  }
}

__global__ __launch_bounds__(kOccThreads) void k_occ_step(Geom g, const float* __restrict__ wts,
                                                          int gx, int gy, int k, OccPlanes in,
                                                          OccPlanes out,
                                                          float* __restrict__ curve) {
  const int H = g.rows, W = g.width;
  const long long n = (long long)H * W;
  const long long cell = (long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (cell >= n) return;
  const int y = (int)(cell / W), x = (int)(cell % W);
  const bool goal = x == gx && y == gy;
  const float dc = in.D[cell];
  float d = goal ? dc : 0.0f;
  out.V[cell] = ftz(in.V[cell] + (goal ? 0.0f : dc));
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int yy = y - (i / 3 - 1), xx = x - (i % 3 - 1);
    const bool src = yy >= 0 && yy < H && xx >= 0 && xx < W && !(xx == gx && yy == gy);
    const float s = src ? in.D[(long long)yy * W + xx] : 0.0f;
    d = fma_ftz(wts[(long long)i * n + cell], s, d);
  }
  out.D[cell] = d;
  if (goal) curve[k] = d;
}

__global__ __launch_bounds__(kOccThreads) void k_occ_tiles(
    Geom g, const float* __restrict__ rfact, const uint8_t* __restrict__ cls, int block, int steps,
    int k0, OccPlanes in, OccPlanes out, float* __restrict__ curve) {
  extern __shared__ float lds[];
  const int H = g.rows, W = g.width;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntx = occ_tiles_x(g);
  const int y0 = (blockIdx.x / ntx) * kTR - block, x0 = (blockIdx.x % ntx) * kTC - block;
  const int rh = kTR + 2 * block, cw = kTC + 2 * block;  // the region (cw <= 64 lanes)
  const int pl = plane_floats(rh);
  float* sRow = lds;                // [class][9]: the dense T row of the class's action
  float* sD = lds + kRowFloats;     // [side][rh + 2][kS], region cell (0, 0) at kS + 1
  uint8_t* sCls = reinterpret_cast<uint8_t*>(sD + 2 * pl);  // [rh + 2][kCS], (0, 0) at kCS + 1

  // the dense rows: +0, then raw T on the action's support; the pinned classes stay +0
  if (tid < kPolicyClasses) {
#pragma unroll
    for (int i = 0; i < 9; ++i) sRow[9 * tid + i] = 0.0f;
    if (tid < 9 * kFactK) {
      const int u = tid / kFactK;
      const f4a r = *reinterpret_cast<const f4a*>(rfact + kResQR + 4 * tid);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cOccSupN[u]) sRow[9 * tid + cOccSup[u][j]] = ftz(r[j]);
    }
  }
  // both sides +0 and every class byte "off the grid": the pads, and the lanes
  // past the region, stay that way
  for (int i = tid; i < 2 * pl; i += kOccThreads) sD[i] = 0.0f;
  for (int i = tid; i < (rh + 2) * (kCS / 4); i += kOccThreads)
    reinterpret_cast<uint32_t*>(sCls)[i] = 0x01010101u * (uint32_t)kPolicyClsOff;
  __syncthreads();

  const int x = x0 + lane;
  const bool col_on = lane < cw && x >= 0 && x < W;
  const bool col_tile = lane >= block && lane < block + kTC && x < W;
  float v[kRowsPerWave];
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = wave + 4 * k;
    const int y = y0 + r;
    v[k] = 0.0f;
    if (r < rh && col_on && y >= 0 && y < H) {
      const long long at = (long long)y * W + x;
      sD[(r + 1) * kS + lane + 1] = in.D[at];
      sCls[(r + 1) * kCS + lane + 1] = cls[at];
      if (col_tile && r >= block && r < block + kTR) v[k] = in.V[at];
    }
  }
  __syncthreads();

  // the gather weights of this thread's cells: entry i of the source's row
  float w[kRowsPerWave][9];
  uint32_t goal_m = 0;  // bit k: the cell is the goal
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = wave + 4 * k;
    const bool live = r < rh && lane < cw;
    const int ci = (r + 1) * kCS + lane + 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int c = live ? sCls[ci - (i / 3 - 1) * kCS - (i % 3 - 1)] : kPolicyClsOff;
      w[k][i] = sRow[9 * c + i];
      if (i == 4 && c == kPolicyClsGoal) goal_m |= 1u << k;
    }
  }

#pragma unroll 1
  for (int s = 0; s < kOccMaxBlock; ++s) {
    if (s >= steps) break;
    const float* vi = sD + (s & 1) * pl;
    float* vo = sD + ((s & 1) ^ 1) * pl;
    if (lane < cw) {
#pragma unroll
      for (int k = 0; k < kRowsPerWave; ++k) {
        const int r = wave + 4 * k;
        if (r < rh) {
          const int li = (r + 1) * kS + lane + 1;
          const bool goal = (goal_m >> k) & 1u;
          const float dc = vi[li];
          float d = goal ? dc : 0.0f;
          v[k] = ftz(v[k] + (goal ? 0.0f : dc));
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            const float sv = i == 4 ? dc : vi[li - (i / 3 - 1) * kS - (i % 3 - 1)];
            d = fma_ftz(w[k][i], sv, d);
          }
          vo[li] = d;
          // the goal's owner: the workgroup whose tile holds it
          if (goal && col_tile && r >= block && r < block + kTR) curve[k0 + s + 1] = d;
        }
      }
    }
    __syncthreads();
  }

  // the tile's cells of the last side written, and their V
  const float* vf = sD + (steps & 1) * pl;
  if (col_tile) {
#pragma unroll
    for (int k = 0; k < kRowsPerWave; ++k) {
      const int r = wave + 4 * k;
      const int y = y0 + r;
      if (r >= block && r < block + kTR && y < H) {
        const long long at = (long long)y * W + x;
        out.D[at] = vf[(r + 1) * kS + lane + 1];
        out.V[at] = v[k];
      }
    }
  }
}

inline unsigned cell_blocks(const Geom& g) {
  return (unsigned)(((long long)g.rows * g.width + kOccThreads - 1) / kOccThreads);
}

}  // namespace

size_t occ_tile_lds_bytes(int block) {
  const int rh = kTR + 2 * block;
  return (size_t)(kRowFloats + 2 * (rh + 2) * kS) * sizeof(float) + (size_t)(rh + 2) * kCS;
}

hipError_t launch_occ_init(hipStream_t st, const Geom& g, int gx, int gy, const float* b0,
                           OccPlanes out, float* curve) {
  hipLaunchKernelGGL(k_occ_init, dim3(cell_blocks(g)), dim3(kOccThreads), 0, st, g, gx, gy, b0, out,
                     curve);
  return hipGetLastError();
}

hipError_t launch_occ_weights(hipStream_t st, const Geom& g, PlaneSet T, const uint8_t* pi, int pis,
                              int gx, int gy, float* wts) {
  hipLaunchKernelGGL(k_occ_weights, dim3(cell_blocks(g)), dim3(kOccThreads), 0, st, g, T, pi, pis,
                     gx, gy, wts);
  return hipGetLastError();
}

hipError_t launch_occ_step(hipStream_t st, const Geom& g, const float* wts, int gx, int gy, int k,
                           OccPlanes in, OccPlanes out, float* curve) {
  hipLaunchKernelGGL(k_occ_step, dim3(cell_blocks(g)), dim3(kOccThreads), 0, st, g, wts, gx, gy, k,
                     in, out, curve);
  return hipGetLastError();
}

hipError_t launch_occ_tiles(hipStream_t st, const Geom& g, const float* rfact, const uint8_t* cls,
                            int block, int steps, int k0, OccPlanes in, OccPlanes out,
                            float* curve) {
  if (block < 1 || block > kOccMaxBlock || steps < 1 || steps > block || k0 < 0)
    return hipErrorInvalidValue;
  static unsigned long long attr = 0;
  allow_lds(reinterpret_cast<const void*>(&k_occ_tiles), attr);
  const unsigned tiles = (unsigned)(occ_tiles_x(g) * occ_tiles_y(g));
  hipLaunchKernelGGL(k_occ_tiles, dim3(tiles), dim3(kOccThreads), occ_tile_lds_bytes(block), st, g,
                     rfact, cls, block, steps, k0, in, out, curve);
  return hipGetLastError();
}

}  // namespace pp2
