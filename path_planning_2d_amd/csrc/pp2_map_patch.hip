// pp2_map_patch.hip -- live map and goal updates (pp2_map_update,
// pp2_goal_set): regenerate the model of the few cells whose
// 3x3 occupancy or at_goal changed and re-code them against the dictionary in
// force, instead of rebuilding 424 B/cell of planes and the dictionary.
//
// k_model_patch: one thread per cell of up to two rectangles (the dilated,
// clipped map rectangle; or the old and the new goal cell).  Each thread
//   1. writes its cell's T/L/R/C words by model_cell -- k_model_gen's body;
//   2. hashes its 106-value tuple as k_dict_hash does;
//   3. probes the open-addressing table hash -> entry built next to the
//      dictionary (keys of 0 are empty slots, linear probing);
//   4. on a hit compares its tuple bitwise with the entry's row, writes the
//      code and raises out[0] on a mismatch (a hash collision);
//   5. on a miss appends {cell, hash} to the miss list (out[1] counts them,
//      also beyond the list's capacity: the host then rebuilds in full).
// Only cells of the grid proper are visited: pad columns and halo rows are
// zeros whatever the map says.  With no table (tab_keys null: a context
// without a dictionary) steps 2 to 5 are skipped.
//
// k_patch_assign: the host numbered the misses' new tuples, gathered their
// rows (k_dict_gather) and now gives every missed cell its code, verified
// bitwise against its row like any other cell.
//
// k_planner_patch: the planner's caches of the model (pp2_tree.cpp: hT / hL on
// the host, the dense R and L rows on the device) follow the journalled
// rectangles of the updates since it last read the model.  One thread per
// (patched cell, value): blockIdx.y is the value -- T plane 0..80, L plane
// 0..15, R plane 0..8 -- and consecutive threads take consecutive cells of a
// rectangle, x fastest, so a wave reads runs of one plane row and writes runs
// of one staging / dense row.  T and L go to the staging buffer as
// [value][patched cell] (the host scatters them into the reference layouts),
// L and R also into the dense rows at cell = y * W + x.  Plain loads and stores.
#include "pp2_model_dev.h"

namespace pp2 {

namespace {

__global__ __launch_bounds__(kBlock) void k_model_patch(
    Geom g, const uint8_t* __restrict__ map, int gx, int gy, PlaneSet T, PlaneSet L, PlaneSet R,
    PlaneSet C, PatchRect r0, PatchRect r1, uint16_t* code, const float* __restrict__ dict,
    const unsigned long long* __restrict__ tab_keys, const int* __restrict__ tab_vals,
    int* __restrict__ out, PatchMiss* __restrict__ miss, int miss_cap) {
  long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long n0 = (long long)r0.w * r0.h, n1 = (long long)r1.w * r1.h;
  if (t >= n0 + n1) return;
  PatchRect r = r0;
  if (t >= n0) {
    r = r1;
    t -= n0;
  }
  const int x = r.x0 + (int)(t % r.w), y = r.y0 + (int)(t / r.w);
  // (the host clips the rectangles; a cell off the grid proper is never written)
  if (x < 0 || x >= g.width || y < 0 || y >= g.rows) return;
  model_cell(g, map, gx, gy, T, L, R, C, x, y);
  if (!tab_keys) return;
  const unsigned long long h = tuple_hash(T, C, R, L, y, x);
  const long long cell = (long long)y * g.wp + x;
  int e = -1;
  if (h != 0ull) {
    unsigned s = (unsigned)h & (kPatchTab - 1);
    for (int probe = 0; probe < kPatchTab; ++probe) {
      const unsigned long long k = tab_keys[s];
      if (k == h) {
        e = tab_vals[s];
        break;
      }
      if (k == 0ull) break;
      s = (s + 1) & (kPatchTab - 1);
    }
  }
  if (e >= 0) {
    if (tuple_differs(T, C, R, L, y, x, dict + (long long)e * kDictRow)) atomicOr(&out[0], 1);
    code[cell] = (uint16_t)e;
    return;
  }
  const int i = atomicAdd(&out[1], 1);
  if (i < miss_cap) {
    miss[i].hash = h;
    miss[i].cell = (int)cell;
    miss[i].code = -1;
  }
}

__global__ __launch_bounds__(kBlock) void k_patch_assign(Geom g, PlaneSet T, PlaneSet C,
                                                         PlaneSet R, PlaneSet L,
                                                         const PatchMiss* __restrict__ miss,
                                                         int n, int E, uint16_t* code,
                                                         const float* __restrict__ dict,
                                                         int* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int cell = miss[i].cell, e = miss[i].code;
  const int y = cell / g.wp, x = cell % g.wp;
  if (e < 0 || e >= E || x >= g.width || y >= g.rows || cell < 0) {
    atomicOr(&out[0], 1);
    return;
  }
  if (tuple_differs(T, C, R, L, y, x, dict + (long long)e * kDictRow)) atomicOr(&out[0], 1);
  code[cell] = (uint16_t)e;
}

__global__ __launch_bounds__(kBlock) void k_planner_patch(
    Geom g, PlaneSet T, PlaneSet L, PlaneSet R, PlannerPatchArgs a, float* __restrict__ stage,
    int cap, float* __restrict__ rrows, float* __restrict__ lrows, int ld) {
  const int j = blockIdx.x * kBlock + threadIdx.x;  // the patched cell's ordinal
  const int v = blockIdx.y;
  if (j >= a.first[kPlannerPatchRects] || j >= cap) return;
  // the rectangle j falls into (constant indices: the arguments stay scalar)
  PatchRect r = a.r[0];
  int base = 0;
#pragma unroll
  for (int i = 1; i < kPlannerPatchRects; ++i)
    if (j >= a.first[i]) {
      r = a.r[i];
      base = a.first[i];
    }
  if (r.w <= 0) return;
  const int t = j - base;
  const int x = r.x0 + t % r.w, y = r.y0 + t / r.w;
  // (the host clips the rectangles; a cell off the grid proper is never touched)
  if (x < 0 || x >= g.width || y < 0 || y >= g.rows || y >= r.y0 + r.h) return;
  const long long cell = (long long)y * g.width + x;
  if (v < kPlannerPatchT) {
    stage[(long long)v * cap + j] = T.p[(long long)y * T.rs + (long long)v * T.ps + x];
  } else if (v < kPlannerPatchT + kPlannerPatchL) {
    const int z = v - kPlannerPatchT;
    const float q = L.p[(long long)y * L.rs + (long long)z * L.ps + x];
    stage[(long long)v * cap + j] = q;
    if (lrows) lrows[(long long)z * ld + cell] = q;
  } else if (rrows && v < kPlannerPatchVals) {
    const int u = v - kPlannerPatchT - kPlannerPatchL;
    rrows[(long long)u * ld + cell] = R.p[(long long)y * R.rs + (long long)u * R.ps + x];
  }
}

}  // namespace

hipError_t launch_planner_patch(hipStream_t st, const Geom& g, PlaneSet T, PlaneSet L, PlaneSet R,
                                const PatchRect* rects, int n, float* stage, int cap,
                                float* rrows, float* lrows, int ld) {
  if (n < 0 || n > kPlannerPatchRects || !stage || cap <= 0) return hipErrorInvalidValue;
  PlannerPatchArgs a;
  int total = 0;
  for (int i = 0; i < kPlannerPatchRects; ++i) {
    a.r[i] = i < n ? rects[i] : PatchRect{0, 0, 0, 0};
    a.first[i] = total;
    if (i < n) {
      const PatchRect& r = rects[i];
      if (r.w <= 0 || r.h <= 0 || r.x0 < 0 || r.y0 < 0 || r.w > g.width - r.x0 ||
          r.h > g.rows - r.y0 || (long long)total + (long long)r.w * r.h > cap)
        return hipErrorInvalidValue;
      total += r.w * r.h;
    }
  }
  a.first[kPlannerPatchRects] = total;
  if (total == 0) return hipSuccess;
  if ((rrows || lrows) && (long long)ld < (long long)g.rows * g.width) return hipErrorInvalidValue;
  // without dense rows (reference_order 0) the R values have no destination
  const int vals = rrows ? kPlannerPatchVals : kPlannerPatchT + kPlannerPatchL;
  hipLaunchKernelGGL(k_planner_patch, dim3((unsigned)((total + kBlock - 1) / kBlock), vals),
                     dim3(kBlock), 0, st, g, T, L, R, a, stage, cap, rrows, lrows, ld);
  return hipGetLastError();
}

hipError_t launch_model_patch(hipStream_t st, const Geom& g, const uint8_t* map, int gx, int gy,
                              PlaneSet T, PlaneSet L, PlaneSet R, PlaneSet C, PatchRect r0,
                              PatchRect r1, uint16_t* code, const float* dict,
                              const unsigned long long* tab_keys, const int* tab_vals, int* out,
                              PatchMiss* miss, int miss_cap) {
  const long long n = (long long)r0.w * r0.h + (long long)r1.w * r1.h;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_model_patch, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, g, map, gx, gy, T, L, R, C, r0, r1, code, dict, tab_keys, tab_vals, out,
                     miss, miss_cap);
  return hipGetLastError();
}

hipError_t launch_patch_assign(hipStream_t st, const Geom& g, PlaneSet T, PlaneSet C, PlaneSet R,
                               PlaneSet L, const PatchMiss* miss, int n, int entries,
                               uint16_t* code, const float* dict, int* out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_patch_assign, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, g, T, C, R, L, miss, n, entries, code, dict, out);
  return hipGetLastError();
}

}  // namespace pp2
