// pp2_model_dev.h -- device code shared by the full model build and the map
// patch (pp2_kernels.hip, pp2_coded.hip, pp2_map_patch.hip): one cell's
// generated model, and the dictionary's per-cell tuple, hash and comparison.
// One body each, so that a patched cell cannot differ from a generated one.
#pragma once
#include "pp2_device.h"

namespace pp2 {

// ============================================================================
// (a1) model generation -- cudaGenerateModelData, POMDP
// (src/pomdp/model_generation_cuda.cu:161-347) and MDP
// (src/mdp/path_planning_2d_cuda.cu:76-213).  T is identical for both models,
// so one T serves the Bellman sweep and the belief update; R is the POMDP
// stage reward, C the MDP stage cost.  Pad cells and rows outside the global
// grid are written as zeros.
// ============================================================================
__device__ __forceinline__ void base_kernel(int u, float tp[9]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
  switch (u) {
    case 0: tp[0] = 0.7f; tp[1] = 0.1f; tp[3] = 0.1f; tp[4] = 0.1f; break;
    case 1: tp[0] = 0.1f; tp[1] = 0.7f; tp[2] = 0.1f; tp[4] = 0.1f; break;
    case 2: tp[1] = 0.1f; tp[2] = 0.7f; tp[4] = 0.1f; tp[5] = 0.1f; break;
    case 3: tp[0] = 0.1f; tp[3] = 0.7f; tp[4] = 0.1f; tp[6] = 0.1f; break;
    case 4: tp[4] = 1.0f; break;
    case 5: tp[2] = 0.1f; tp[4] = 0.1f; tp[5] = 0.7f; tp[8] = 0.1f; break;
    case 6: tp[3] = 0.1f; tp[4] = 0.1f; tp[6] = 0.7f; tp[7] = 0.1f; break;
    case 7: tp[4] = 0.1f; tp[6] = 0.1f; tp[7] = 0.7f; tp[8] = 0.1f; break;
    default: tp[4] = 0.1f; tp[5] = 0.1f; tp[7] = 0.1f; tp[8] = 0.7f; break;
  }
}

// The model of the cell at column x of local row y (in [-halo, rows + halo)),
// a function of its 3x3 occupancy and of at_goal, into its T/L/R/C words.
__device__ __forceinline__ void model_cell(const Geom& g, const uint8_t* __restrict__ map, int gx,
                                           int gy, const PlaneSet& T, const PlaneSet& L,
                                           const PlaneSet& R, const PlaneSet& C, int x, int y) {
  const int ry = g.row0 + y;          // global row
  const bool valid = x < g.width && ry >= 0 && ry < g.grows;

  uint8_t lm[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int nx = x + i % 3 - 1, ny = ry + i / 3 - 1;
    lm[i] = (!valid || nx < 0 || nx >= g.width || ny < 0 || ny >= g.grows)
                ? 1 : map[(long long)ny * g.width + nx];
  }
  const bool at_goal = (unsigned)x == (unsigned)gx && (unsigned)ry == (unsigned)gy;
  float mr[9], mc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    mr[i] = lm[i] == 1 ? -2.0f : -1.0f;
    mc[i] = lm[i] == 1 ? 2.0f : 1.0f;
  }
  for (int u = 0; u < 9; ++u) {
    float tp[9], nv[9];
    base_kernel(u, tp);
    // POMDP naive = base kernel (copied before the shift, :213-214)
#pragma unroll
    for (int i = 0; i < 9; ++i) nv[i] = tp[i];
    // MDP naive = base kernel after the trap override (:131-137)
    float nm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) nm[i] = (lm[4] == 1) ? (i == 4 ? 1.0f : 0.0f) : tp[i];
    // occupied neighbour -> mass stays (:219-224), in index order
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if (lm[i] == 1 && i != 4) { tp[4] += tp[i]; tp[i] = 0.0f; }
    if (lm[4] == 1) {  // trapped (:230-233)
#pragma unroll
      for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
      tp[4] = 1.0f;
    }
    float r = 0.0f, c = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      r = __builtin_fmaf(mr[i], nv[i], r);  // cudaStageReward :288-291
      c = __builtin_fmaf(mc[i], nm[i], c);  // cudaStageCost   :166-169
    }
    if (u == 4) {
      r = at_goal ? 0.0f : -2.0f;  // :293
      c = at_goal ? 0.0f : 2.0f;   // mdp :171
    }
    const long long rowT = (long long)y * T.rs + x;
#pragma unroll
    for (int i = 0; i < 9; ++i) T.p[rowT + (9 * u + i) * T.ps] = valid ? tp[i] : 0.0f;
    R.p[(long long)y * R.rs + u * R.ps + x] = valid ? r : 0.0f;
    C.p[(long long)y * C.rs + u * C.ps + x] = valid ? c : 0.0f;
  }
  // cudaMeasurementLikelihood (:238-264): m = {up, left, right, down}
  const uint8_t m0 = lm[1], m1 = lm[3], m2 = lm[5], m3 = lm[7];
  for (int i = 0; i < 16; ++i) {
    const float l0 = (((i >> 0) & 1) == m0) ? (float)0.98 : (float)0.02;
    const float l1 = (((i >> 1) & 1) == m1) ? (float)0.98 : (float)0.02;
    const float l2 = (((i >> 2) & 1) == m2) ? (float)0.98 : (float)0.02;
    const float l3 = (((i >> 3) & 1) == m3) ? (float)0.98 : (float)0.02;
    const float l = ((l0 * l1) * l2) * l3;
    L.p[(long long)y * L.rs + i * L.ps + x] = valid ? l : 0.0f;
  }
}

// ---------------------------------------------------------------- dictionary
// value k of a cell's kDictTuple-value tuple: [u][T_u0..T_u8, C_u] | L[16]
__device__ __forceinline__ float tuple_value(const PlaneSet& T, const PlaneSet& C,
                                             const PlaneSet& R, const PlaneSet& L, int y,
                                             int x, int k) {
  if (k < 90) {
    const int u = k / 10, i = k % 10;
    return i < 9 ? T.p[(long long)y * T.rs + (long long)(9 * u + i) * T.ps + x]
                 : C.p[(long long)y * C.rs + (long long)u * C.ps + x];
  }
  if (k < kDictTuple) return L.p[(long long)y * L.rs + (long long)(k - 90) * L.ps + x];
  return 0.0f;
}

__device__ __forceinline__ uint64_t mix64(uint64_t h) {
  h ^= h >> 31;
  h *= 0x7fb5d329728ea185ull;
  h ^= h >> 27;
  h *= 0x81dadef4bc2dd44dull;
  h ^= h >> 33;
  return h;
}

// hash of the tuple of cell (y, x)
__device__ __forceinline__ uint64_t tuple_hash(const PlaneSet& T, const PlaneSet& C,
                                               const PlaneSet& R, const PlaneSet& L, int y, int x) {
  uint64_t h = 0x9e3779b97f4a7c15ull;
  for (int k = 0; k < kDictTuple; ++k) {
    const uint32_t w = __float_as_uint(tuple_value(T, C, R, L, y, x, k));
    h = mix64(h ^ (w + 0x632be59bd9b4e019ull * (uint64_t)(k + 1)));
  }
  return h;
}

// whether the tuple of cell (y, x) differs, as bit patterns, from dictionary row d
__device__ __forceinline__ int tuple_differs(const PlaneSet& T, const PlaneSet& C,
                                             const PlaneSet& R, const PlaneSet& L, int y, int x,
                                             const float* __restrict__ d) {
  int diff = 0;
  for (int k = 0; k < kDictTuple; ++k)
    diff |= __float_as_uint(tuple_value(T, C, R, L, y, x, k)) != __float_as_uint(d[k]);
  return diff;
}

}  // namespace pp2
