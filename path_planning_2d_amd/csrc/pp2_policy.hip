// pp2_policy.hip -- gfx950 kernels of the policy evaluator (include/pp2.h
// "policy evaluation"): H steps of a 9-point stencil whose
// weights are the world's T row of the one action the table names per cell.
//
// Every step is a pure function of the previous three planes, so how the
// cells of a step are spread over launches and workgroups cannot change a
// bit.  Two schedules:
//  * k_policy_step (PP2_POLICY_PLANES): one launch per step, one thread per
//    cell, the nine T entries and C of the cell's action from the dense planes;
//  * k_policy_tiles (PP2_POLICY_TILES): `steps` <= block steps per launch.  A
//    workgroup keeps its kPolicyTileRows x kPolicyTileCols tile of G, P and N
//    plus a ring `block` cells deep in LDS (two sides, ping-pong) and steps the
//    whole region: what a region's outermost cells miss -- their neighbours
//    outside it read +0 from the pad -- moves inwards one cell per step and
//    after `block` steps has reached the ring's innermost cells, not the
//    tile.  Only the tile is written back.  The launch boundary is the only
//    ordering between workgroups.
// A tile cell's row comes from the world's coded model by class: one byte per
// cell (k_policy_classes, once per evaluation) names the record {fl(gamma T)
// on the action's support, raw T on it, C}, staged in LDS from the factored
// sweep rows and the class tables.  The terms off the support are the dense
// chain's fmaf(+0, v, acc) == acc (pp2_dict_props.h: every v finite and
// >= +0, no accumulator -0); on it the products and their ascending order
// are the dense ones.  Cells off the grid and the goal are classes too: all
// weights +0 and the start values {+0, +0, +0} / {+0, 1, +0}, so they hold
// their pinned values through the same arithmetic as every other cell.
// Flush-to-zero is the definition's, in code (pp2_device.h: ftz, fma_ftz; this
// file is built with IEEE subnormals): the model's entries are flushed where
// they are read, every result after its rounding.
//
// Lane = region column (row stride kS = 66 words: a row access of the 64
// lanes hits 64 banks, and columns -1 and 64 are the pad), wave w = region
// rows w, w + 4, ...  Every loop is bounded by a constant.
#include <hip/hip_runtime.h>

#include "pp2_device.h"
#include "pp2_policy.h"

namespace pp2 {
namespace {

constexpr int kTR = kPolicyTileRows, kTC = kPolicyTileCols;
constexpr int kS = 66;                                      // LDS row stride (words)
constexpr int kMaxRH = kTR + 2 * kPolicyMaxBlock;           // region rows, at most
constexpr int kRowsPerWave = (kMaxRH + 3) / 4;
constexpr int kTabFloats = 3 * 4 * kPolicyClasses;          // QT, QR, CN records
static_assert(kPolicyThreads == 256 && kPolicyClasses <= 256, "one staging pass, a class per byte");
static_assert(kS + 1 <= 127, "a support offset is a signed byte");

__constant__ unsigned char cPolSupN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
__constant__ unsigned char cPolSup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5},
                                            {0, 3, 4, 6}, {4, 0, 0, 0}, {2, 4, 5, 8},
                                            {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};

__device__ __forceinline__ int plane_floats(int rh) { return (rh + 2) * kS; }

__global__ __launch_bounds__(kPolicyThreads) void k_policy_init(Geom g, int gx, int gy,
                                                                PolicyPlanes out) {
  const long long n = (long long)g.rows * g.width;
  const long long i = (long long)blockIdx.x * kPolicyThreads + threadIdx.x;
  if (i >= n) return;
  const bool goal = gx >= 0 && gx < g.width && gy >= 0 && gy < g.rows &&
                    i == (long long)gy * g.width + gx;
  out.G[i] = 0.0f;
  out.P[i] = goal ? 1.0f : 0.0f;
  out.N[i] = 0.0f;
}

__global__ __launch_bounds__(kPolicyThreads) void k_policy_step(
    Geom g, float gamma, PlaneSet T, PlaneSet C, const uint8_t* __restrict__ pi, int pis, int gx,
    int gy, PolicyPlanes in, PolicyPlanes out) {
  const int H = g.rows, W = g.width;
  const long long cell = (long long)blockIdx.x * kPolicyThreads + threadIdx.x;
  if (cell >= (long long)H * W) return;
  const int y = (int)(cell / W), x = (int)(cell % W);
  if (x == gx && y == gy) {  // absorbing
    out.G[cell] = 0.0f;
    out.P[cell] = 1.0f;
    out.N[cell] = 0.0f;
    return;
  }
  const int u = pi[(long long)y * pis + x];
  const float* tp = T.p + (long long)y * T.rs + (long long)(9 * u) * T.ps + x;
  float gv = ftz(C.p[(long long)y * C.rs + (long long)u * C.ps + x]);
  float pv = 0.0f, nv = 1.0f;
  gamma = ftz(gamma);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int yy = y + i / 3 - 1, xx = x + i % 3 - 1;
    const bool on = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const long long at = on ? (long long)yy * W + xx : cell;
    const float t = ftz(tp[(long long)i * T.ps]);
    const float gt = ftz(gamma * t);
    const float gn = on ? in.G[at] : 0.0f;
    const float pn = on ? in.P[at] : 0.0f;
    const float nn = on ? in.N[at] : 0.0f;
    gv = fma_ftz(gt, gn, gv);
    pv = fma_ftz(t, pn, pv);
    nv = fma_ftz(t, nn, nv);
  }
  out.G[cell] = gv;
  out.P[cell] = pv;
  out.N[cell] = nv;
}

__global__ __launch_bounds__(kPolicyThreads) void k_policy_classes(
    Geom g, const uint16_t* __restrict__ code, const float* __restrict__ rows,
    const uint8_t* __restrict__ pi, int pis, int gx, int gy, uint8_t* __restrict__ cls) {
  const int H = g.rows, W = g.width;
  const long long cell = (long long)blockIdx.x * kPolicyThreads + threadIdx.x;
  if (cell >= (long long)H * W) return;
  const int y = (int)(cell / W), x = (int)(cell % W);
  const uint32_t e = code[(long long)y * g.wp + x];
  const uint32_t u = pi[(long long)y * pis + x];
  // byte u of the entry's IW record = 16 * (its pair class for action u)
  const uint32_t w = reinterpret_cast<const uint32_t*>(rows + kFactIW)[4 * e + (u >> 2)];
  const uint32_t k = ((w >> (8 * (u & 3))) & 0xffu) >> 4;
  cls[cell] = x == gx && y == gy ? (uint8_t)kPolicyClsGoal : (uint8_t)(u * kFactK + k);
}

__global__ __launch_bounds__(kPolicyThreads) void k_policy_tiles(
    Geom g, const float* __restrict__ rows, const float* __restrict__ rfact,
    const uint8_t* __restrict__ cls, int block, int steps, PolicyPlanes in, PolicyPlanes out) {
  extern __shared__ float lds[];
  const int H = g.rows, W = g.width;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntx = policy_tiles_x(g);
  const int y0 = (blockIdx.x / ntx) * kTR - block, x0 = (blockIdx.x % ntx) * kTC - block;
  const int rh = kTR + 2 * block, cw = kTC + 2 * block;  // the region (cw <= 64 lanes)
  const int pl = plane_floats(rh);
  f4a* sQT = reinterpret_cast<f4a*>(lds);
  f4a* sQR = sQT + kPolicyClasses;
  f4a* sCN = sQR + kPolicyClasses;
  float* sV = lds + kTabFloats;  // [side][G, P, N][rh + 2][kS], region cell (0, 0) at kS + 1
  uint8_t* sCls = reinterpret_cast<uint8_t*>(sV + 6 * pl);  // [rh][64]

  // the class records: {gT support quad}, {T support quad}, {C, P start, N start, offsets}
  if (tid < kPolicyClasses) {
    f4a qt = {0.0f, 0.0f, 0.0f, 0.0f}, qr = qt, cn = qt;
    if (tid < 9 * kFactK) {
      const int u = tid / kFactK;
      const f4a t = *reinterpret_cast<const f4a*>(rows + kFactQT + 4 * tid);
      const f4a r = *reinterpret_cast<const f4a*>(rfact + kResQR + 4 * tid);
      uint32_t offs = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in_sup = j < cPolSupN[u];
        qt[j] = in_sup ? ftz(t[j]) : 0.0f;
        qr[j] = in_sup ? ftz(r[j]) : 0.0f;
        const int i = cPolSup[u][j];
        offs |= (uint32_t)(((i / 3 - 1) * kS + i % 3 - 1) & 0xff) << (8 * j);
      }
      cn[0] = ftz(rows[kFactCT + 4 * tid]);
      cn[2] = 1.0f;
      cn[3] = __uint_as_float(offs);
    } else if (tid == kPolicyClsGoal) {
      cn[1] = 1.0f;
    }
    sQT[tid] = qt;
    sQR[tid] = qr;
    sCN[tid] = cn;
  }
  // the pad: rows -1 and rh, columns -1 and 64 of every plane, never written again
  for (int i = tid; i < 2 * kS; i += kPolicyThreads) {
    const int at = (i < kS ? 0 : (rh + 1) * kS) + i % kS;
#pragma unroll
    for (int p = 0; p < 6; ++p) sV[p * pl + at] = 0.0f;
  }
  for (int i = tid; i < 2 * rh; i += kPolicyThreads) {
    const int at = (1 + (i >> 1)) * kS + ((i & 1) ? kS - 1 : 0);
#pragma unroll
    for (int p = 0; p < 6; ++p) sV[p * pl + at] = 0.0f;
  }
  // the region; off the grid: +0 and the pinned class.  Lanes past the region
  // hold +0 on both sides and are never stepped.
#pragma unroll 1
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = wave + 4 * k;
    if (r >= rh) break;
    const int y = y0 + r, x = x0 + lane;
    const bool on = lane < cw && y >= 0 && y < H && x >= 0 && x < W;
    const long long at = on ? (long long)y * W + x : 0;
    const int li = (r + 1) * kS + lane + 1;
    sV[li] = on ? in.G[at] : 0.0f;
    sV[pl + li] = on ? in.P[at] : 0.0f;
    sV[2 * pl + li] = on ? in.N[at] : 0.0f;
    sCls[r * 64 + lane] = on ? cls[at] : (uint8_t)kPolicyClsOff;
    if (lane >= cw) {
      sV[3 * pl + li] = 0.0f;
      sV[4 * pl + li] = 0.0f;
      sV[5 * pl + li] = 0.0f;
    }
  }
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < kPolicyMaxBlock; ++s) {
    if (s >= steps) break;
    const float* vi = sV + (s & 1) * 3 * pl;
    float* vo = sV + ((s & 1) ^ 1) * 3 * pl;
    if (lane < cw) {
#pragma unroll 4
      for (int k = 0; k < kRowsPerWave; ++k) {
        const int r = wave + 4 * k;
        if (r >= rh) break;
        const int li = (r + 1) * kS + lane + 1;
        const int c = sCls[r * 64 + lane];
        const f4a qt = sQT[c], qr = sQR[c], cn = sCN[c];
        const uint32_t offs = __float_as_uint(cn[3]);
        float gv = cn[0], pv = cn[1], nv = cn[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int at = li + (int)(int8_t)(offs >> (8 * j));
          gv = fma_ftz(qt[j], vi[at], gv);
          pv = fma_ftz(qr[j], vi[pl + at], pv);
          nv = fma_ftz(qr[j], vi[2 * pl + at], nv);
        }
        vo[li] = gv;
        vo[pl + li] = pv;
        vo[2 * pl + li] = nv;
      }
    }
    __syncthreads();
  }

  // the tile's cells of the last side written
  const float* vf = sV + (steps & 1) * 3 * pl;
  const int x = x0 + lane;
  if (lane >= block && lane < block + kTC && x < W) {
#pragma unroll 1
    for (int k = 0; k < kTR / 4; ++k) {
      const int tr = wave + 4 * k;
      const int y = y0 + block + tr;
      if (y >= H) break;
      const int li = (block + tr + 1) * kS + lane + 1;
      const long long at = (long long)y * W + x;
      out.G[at] = vf[li];
      out.P[at] = vf[pl + li];
      out.N[at] = vf[2 * pl + li];
    }
  }
}

inline unsigned cell_blocks(const Geom& g) {
  return (unsigned)(((long long)g.rows * g.width + kPolicyThreads - 1) / kPolicyThreads);
}

}  // namespace

size_t policy_tile_lds_bytes(int block) {
  const int rh = kTR + 2 * block;
  return (size_t)(kTabFloats + 6 * (rh + 2) * kS) * sizeof(float) + (size_t)rh * 64;
}

hipError_t launch_policy_init(hipStream_t st, const Geom& g, int gx, int gy, PolicyPlanes out) {
  hipLaunchKernelGGL(k_policy_init, dim3(cell_blocks(g)), dim3(kPolicyThreads), 0, st, g, gx, gy,
                     out);
  return hipGetLastError();
}

hipError_t launch_policy_step(hipStream_t st, const Geom& g, float gamma, PlaneSet T, PlaneSet C,
                              const uint8_t* pi, int pis, int gx, int gy, PolicyPlanes in,
                              PolicyPlanes out) {
  hipLaunchKernelGGL(k_policy_step, dim3(cell_blocks(g)), dim3(kPolicyThreads), 0, st, g, gamma, T,
                     C, pi, pis, gx, gy, in, out);
  return hipGetLastError();
}

hipError_t launch_policy_classes(hipStream_t st, const Geom& g, const uint16_t* code,
                                 const float* rows, const uint8_t* pi, int pis, int gx, int gy,
                                 uint8_t* cls) {
  hipLaunchKernelGGL(k_policy_classes, dim3(cell_blocks(g)), dim3(kPolicyThreads), 0, st, g, code,
                     rows, pi, pis, gx, gy, cls);
  return hipGetLastError();
}

hipError_t launch_policy_tiles(hipStream_t st, const Geom& g, const float* rows,
                               const float* rfact, const uint8_t* cls, int block, int steps,
                               PolicyPlanes in, PolicyPlanes out) {
  if (block < 1 || block > kPolicyMaxBlock || steps < 1 || steps > block)
    return hipErrorInvalidValue;
  static unsigned long long attr = 0;
  allow_lds(reinterpret_cast<const void*>(&k_policy_tiles), attr);
  const unsigned tiles = (unsigned)(policy_tiles_x(g) * policy_tiles_y(g));
  hipLaunchKernelGGL(k_policy_tiles, dim3(tiles), dim3(kPolicyThreads),
                     policy_tile_lds_bytes(block), st, g, rows, rfact, cls, block, steps, in, out);
  return hipGetLastError();
}

}  // namespace pp2
