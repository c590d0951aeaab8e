// pp2_control.hip -- on-device control selection (gfx950): the belief's mode
// and the belief-expected Q values of the current MDP values J,
//   S_u = sum_x b(x) Q(x, u),  Q(x, u) = C[x][u] + sum_i fl(gamma T[x][u][i]) J(x + off_i),
// so that a controller reads one 64-byte record instead of the belief and
// action planes (pp2_belief_mode / pp2_mdp_qvalues / pp2_mdp_control).
//
// Q(x, u) is k_mdp_sweep's `cost` of action u, term by term (the same fmaf
// chain, J = 0 outside the grid); the coded kernel reads the same operands
// from the LDS dictionary rows (pp2_coded_dev.h), so both give the same bits.
//
// Reduction order (a function of the geometry alone; no atomics):
//   lane   : its 4 cells in ascending x, acc_u = fmaf(b, Q_u, acc_u) from +0;
//            pad cells (x >= width) and lanes past the last row add nothing;
//   wave   : wave_sum (xor butterfly 32, 16, 8, 4, 2, 1);
//   block  : the 4 waves of a 1024-cell block as ((w0 + w1) + w2) + w3 --
//            blocks are the dense kernels' (cells_grid(g, 4)) in both kernels,
//            whatever the coded kernel's workgroup size and grid;
//   grid   : k_control_finish, per action: 16 threads sum the blocks
//            r = i, i + 16, ... in ascending order, then thread 0 of the 16
//            adds their sums in order i = 0..15; q_u = S_u / mass.
// The mode is a (value, index) maximum under a total order (larger normalised
// value, else smaller index), which any reduction tree evaluates identically.
#include <limits.h>

#include "pp2_coded_dev.h"

namespace pp2 {
namespace {

constexpr int kQ = 9;
constexpr int kFinLanes = 16;  // threads per action in k_control_finish

// ---- expected Q, dense planes ---------------------------------------------
template <bool NT>
__global__ __launch_bounds__(kBlock) void k_control_q(Geom g, float gamma, PlaneSet T, PlaneSet C,
                                                      const float* __restrict__ J,
                                                      const float* __restrict__ b,
                                                      float* __restrict__ partials) {
  constexpr int CPT = 4;
  __shared__ float red[4][kQ];
  const int tpr = g.wp / CPT;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int y = (int)(t / tpr);
  const int x0 = (int)(t % tpr) * CPT;
  float acc[kQ];
#pragma unroll
  for (int u = 0; u < kQ; ++u) acc[u] = 0.0f;
  if (y < g.rows) {
    const bool le = x0 == 0, re = x0 + CPT == g.wp;
    float bv[CPT];
    ldv<CPT, true>(b + (long long)y * g.wp + x0, bv);
    float jn[9][CPT];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int oy = i / 3 - 1, ox = i % 3 - 1;
      const float* jp = J + (long long)(y + oy) * g.wp + x0 + ox;
      if (ox == 0) ldv<CPT, true>(jp, jn[i]);
      else ldv<CPT, false>(jp, jn[i]);
      if (ox < 0 && le) jn[i][0] = 0.0f;
      if (ox > 0 && re) jn[i][CPT - 1] = 0.0f;
    }
    const float* trow = T.p + (long long)y * T.rs + x0;
    const float* crow = C.p + (long long)y * C.rs + x0;
    // k_mdp_sweep's register double-buffering over the actions
    float cb[2][CPT], tb[2][9][CPT];
    ldv_stream<CPT, NT>(crow, cb[0]);
#pragma unroll
    for (int i = 0; i < 9; ++i) ldv_stream<CPT, NT>(trow + (long long)i * T.ps, tb[0][i]);
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
      const int cur = u & 1, nxt = cur ^ 1;
      if (u < 8) {
        ldv_stream<CPT, NT>(crow + (long long)(u + 1) * C.ps, cb[nxt]);
#pragma unroll
        for (int i = 0; i < 9; ++i)
          ldv_stream<CPT, NT>(trow + (long long)(9 * (u + 1) + i) * T.ps, tb[nxt][i]);
      }
      float cost[CPT];
#pragma unroll
      for (int k = 0; k < CPT; ++k) cost[k] = cb[cur][k];
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int k = 0; k < CPT; ++k)
          cost[k] = __builtin_fmaf(gamma * tb[cur][i][k], jn[i][k], cost[k]);
      // pad cells may hold anything in T / C / J (0 * NaN is not 0): skipped
#pragma unroll
      for (int k = 0; k < CPT; ++k)
        if (x0 + k < g.width) acc[u] = __builtin_fmaf(bv[k], cost[k], acc[u]);
    }
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int u = 0; u < kQ; ++u) {
    const float v = wave_sum(acc[u]);
    if ((threadIdx.x & 63) == 0) red[w][u] = v;
  }
  __syncthreads();
  if (threadIdx.x < kQ)
    partials[(long long)blockIdx.x * kQ + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- expected Q, dictionary-coded model -----------------------------------
// One cell's nine costs from its code (sweep_cell_fact / coded_sweep4 without
// the min), each folded into the lane's partial of its action.
template <bool SPARSE>
__device__ __forceinline__ void coded_q_cell(const float* sTC, uint32_t code,
                                             const float (&jn)[9][4], int k, float bk, bool ok,
                                             float (&acc)[kQ]) {
  if constexpr (SPARSE) {
    const uint4 iw = *reinterpret_cast<const uint4*>(sTC + kFactIW + 4 * code);
    const char* qt = reinterpret_cast<const char*>(sTC + kFactQT);
    const char* ct = reinterpret_cast<const char*>(sTC + kFactCT);
#pragma unroll
    for (int a = 0; a < kQ; ++a) {
      const uint32_t w = a < 4 ? iw.x : a < 8 ? iw.y : iw.z;
      const uint32_t off = __builtin_amdgcn_ubfe(w, 8 * (a % 4), 8);
      const int tab = a * kFactK * 16;  // byte offset of action a's table
      float tv[4];
      if (kSupN[a] == 1) {
        tv[0] = *reinterpret_cast<const float*>(qt + tab + off);
      } else {
        const f4a t = *reinterpret_cast<const f4a*>(qt + tab + off);
        tv[0] = t[0]; tv[1] = t[1]; tv[2] = t[2]; tv[3] = t[3];
      }
      float cost = *reinterpret_cast<const float*>(ct + tab + off);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < kSupN[a]) cost = __builtin_fmaf(tv[j], jn[kSup[a][j]][k], cost);
      if (ok) acc[a] = __builtin_fmaf(bk, cost, acc[a]);
    }
  } else {
#pragma unroll
    for (int a = 0; a < kQ; ++a) {
      const f2a* row = reinterpret_cast<const f2a*>(sTC + code * kDictTC + a * 10);
      const f2a t01 = row[0], t23 = row[1], t45 = row[2], t67 = row[3], t8c = row[4];
      const float tv[9] = {t01[0], t01[1], t23[0], t23[1], t45[0], t45[1], t67[0], t67[1], t8c[0]};
      float cost = t8c[1];
#pragma unroll
      for (int i = 0; i < 9; ++i) cost = __builtin_fmaf(tv[i], jn[i][k], cost);
      if (ok) acc[a] = __builtin_fmaf(bk, cost, acc[a]);
      __builtin_amdgcn_sched_barrier(0);  // one action's row reads live at a time
    }
  }
}

// Workgroups of QPB dense blocks (256 threads, 1024 cells each) that stage the
// dictionary rows once and stride over the tiles; quarter q of tile tl is
// dense block QPB * tl + q and writes that block's partials, so the partial
// array is k_control_q's whatever the grid.
template <bool SPARSE, int QPB, int MINB>
__global__ __launch_bounds__(QPB * kBlock, MINB * QPB) void k_control_q_coded(
    Geom g, const uint16_t* __restrict__ code, const float* __restrict__ rows, int E,
    const float* __restrict__ J, const float* __restrict__ b, int dense_blocks,
    float* __restrict__ partials) {
  constexpr int NT = QPB * kBlock;
  extern __shared__ float lds[];
  __shared__ float red[QPB * 4][kQ];
  const int tpr = g.wp / 4;
  const int ntiles = (dense_blocks + QPB - 1) / QPB;
  const int q = threadIdx.x / kBlock, tq = threadIdx.x % kBlock;
  const int w = threadIdx.x >> 6;
  stage_rows(rows, rows_floats(E, SPARSE), lds);
  __syncthreads();
  for (int tile = xcd_remap(blockIdx.x, gridDim.x); tile < ntiles; tile += gridDim.x) {
    const long long t = (long long)tile * NT + threadIdx.x;
    const int y = (int)(t / tpr);
    const int x0 = (int)(t % tpr) * 4;
    float acc[kQ];
#pragma unroll
    for (int u = 0; u < kQ; ++u) acc[u] = 0.0f;
    if (y < g.rows) {
      const long long off = (long long)y * g.wp + x0;
      const uint2 m = *reinterpret_cast<const uint2*>(code + off);
      const uint32_t cc[4] = {m.x & 0xffffu, m.x >> 16, m.y & 0xffffu, m.y >> 16};
      float bv[4];
      ldv<4, true>(b + off, bv);
      float jn[9][4];
      load_jn(J, g.wp, y, x0, x0 == 0, x0 + 4 == g.wp, jn);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        coded_q_cell<SPARSE>(lds, cc[k], jn, k, bv[k], x0 + k < g.width, acc);
        __builtin_amdgcn_sched_barrier(0);  // one cell's table reads live at a time
      }
    }
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
      const float v = wave_sum(acc[u]);
      if ((threadIdx.x & 63) == 0) red[w][u] = v;
    }
    __syncthreads();
    const int d = QPB * tile + q;
    if (tq < kQ && d < dense_blocks)
      partials[(long long)d * kQ + tq] =
          ((red[4 * q][tq] + red[4 * q + 1][tq]) + red[4 * q + 2][tq]) + red[4 * q + 3][tq];
    __syncthreads();  // red is reused by the next tile
  }
}

// ---- belief mode ----------------------------------------------------------
// (v, i) candidates: v the normalised value (k_pack's expression), i the
// host-layout index y * W + x; "none" is (0, INT_MAX), which every cell > 0
// beats and which NaNs never replace (the comparisons are >).
__device__ __forceinline__ void mode_take(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(kBlock) void k_belief_mode(Geom g, const float* __restrict__ b,
                                                        const float* __restrict__ mass,
                                                        float* __restrict__ pv,
                                                        int* __restrict__ pi) {
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int tpr = g.wp / 4;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int y = (int)(t / tpr);
  const int x0 = (int)(t % tpr) * 4;
  float v = 0.0f;
  int idx = INT_MAX;
  if (y < g.rows) {
    float bv[4];
    ldv<4, true>(b + (long long)y * g.wp + x0, bv);
    const float m = *mass;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float n = bv[k] / m;
      if (x0 + k < g.width && n > v) { v = n; idx = y * g.width + x0 + k; }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    mode_take(v, idx, ov, oi);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { rv[w] = v; ri[w] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 1; j < 4; ++j) mode_take(v, idx, rv[j], ri[j]);
    pv[blockIdx.x] = v;
    pi[blockIdx.x] = idx;
  }
}

// ---- finalise: one block folds the partials into the control record -------
// rec (kControlRec words): q[0..8], QMDP action, QMDP value, mode cell, mode
// probability, action and value at the mode.  nq / nm = 0 skips that half
// (its words are left as they are).
__global__ __launch_bounds__(kBlock) void k_control_finish(
    const float* __restrict__ qpart, int nq, const float* __restrict__ mass,
    const float* __restrict__ pv, const int* __restrict__ pi, int nm,
    const float* __restrict__ J, const uint8_t* __restrict__ A, int width, int wp,
    uint32_t* __restrict__ rec) {
  __shared__ float qs[kQ][kFinLanes];
  __shared__ float qv[kQ];
  __shared__ float mv[kBlock];
  __shared__ int mi[kBlock];
  const int tid = threadIdx.x;
  if (nq > 0) {
    const int u = tid / kFinLanes, i = tid % kFinLanes;
    if (u < kQ) {
      // 8 loads in flight ahead of the in-order adds
      float s = 0.0f;
      int r = i;
      for (; r + 7 * kFinLanes < nq; r += 8 * kFinLanes) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = qpart[(long long)(r + j * kFinLanes) * kQ + u];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
      }
      for (; r < nq; r += kFinLanes) s += qpart[(long long)r * kQ + u];
      qs[u][i] = s;
    }
    __syncthreads();
    if (tid < kQ) {
      float s = qs[tid][0];
#pragma unroll
      for (int i = 1; i < kFinLanes; ++i) s += qs[tid][i];
      const float qu = s / *mass;
      qv[tid] = qu;
      rec[tid] = __float_as_uint(qu);
    }
    __syncthreads();
    if (tid == 0) {
      // the sweep's tie rule: first strict minimum
      float best = FLT_MAX;
      uint32_t arg = 0;
#pragma unroll
      for (int u = 0; u < kQ; ++u)
        if (qv[u] < best) { best = qv[u]; arg = (uint32_t)u; }
      rec[kControlRecAction] = arg;
      rec[kControlRecValue] = __float_as_uint(qv[arg]);
    }
  }
  if (nm > 0) {
    float v = 0.0f;
    int idx = INT_MAX;
    for (int r = tid; r < nm; r += kBlock) mode_take(v, idx, pv[r], pi[r]);
    mv[tid] = v;
    mi[tid] = idx;
    __syncthreads();
    for (int s = kBlock / 2; s >= 1; s >>= 1) {
      if (tid < s) {
        mode_take(v, idx, mv[tid + s], mi[tid + s]);
        mv[tid] = v;
        mi[tid] = idx;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int cell = idx == INT_MAX ? 0 : idx;  // no cell > 0: cell 0, probability 0
      const long long at = (long long)(cell / width) * wp + cell % width;
      rec[kControlRecCell] = (uint32_t)cell;
      rec[kControlRecProb] = __float_as_uint(v);
      rec[kControlRecModeAction] = A[at];
      rec[kControlRecModeValue] = __float_as_uint(J[at]);
    }
  }
}

}  // namespace

int control_blocks(const Geom& g) { return cells_grid(g, 4); }

hipError_t launch_control_q(hipStream_t st, const Geom& g, float gamma, PlaneSet T, PlaneSet C,
                            const float* J, const float* b, float* partials, bool nt) {
  const int grid = control_blocks(g);
  if (nt)
    hipLaunchKernelGGL((k_control_q<true>), dim3(grid), dim3(kBlock), 0, st, g, gamma, T, C, J, b,
                       partials);
  else
    hipLaunchKernelGGL((k_control_q<false>), dim3(grid), dim3(kBlock), 0, st, g, gamma, T, C, J,
                       b, partials);
  return hipGetLastError();
}

hipError_t launch_control_q_coded(hipStream_t st, const Geom& g, const uint16_t* code,
                                  const float* rows, int E, bool sparse, const float* J,
                                  const float* b, float* partials, int ncus) {
  const size_t lds = (size_t)lds_span(rows_floats(E, sparse)) * sizeof(float);
  const int dense_blocks = control_blocks(g);
// one 1024-thread workgroup per CU (4 waves per SIMD, <= 128 VGPRs: the nine
// partials and the belief on top of the sweep's registers spill at the sparse
// sweep's 64); full rows take up to ~144 KB of LDS
#define PP2_CTLQ(SP, Q, MB)                                                                    \
  do {                                                                                         \
    if ((lds + Q * 4 * kQ * sizeof(float)) * MB > kDictLdsMaxBytes) return hipErrorInvalidValue; \
    static unsigned long long attr = 0;                                                        \
    allow_lds(reinterpret_cast<const void*>(&k_control_q_coded<SP, Q, MB>), attr);             \
    const int ntiles = (dense_blocks + Q - 1) / Q;                                             \
    const int cap = ncus > 0 ? ncus * MB : ntiles;                                             \
    hipLaunchKernelGGL((k_control_q_coded<SP, Q, MB>), dim3(ntiles < cap ? ntiles : cap),      \
                       dim3(Q * kBlock), lds, st, g, code, rows, E, J, b, dense_blocks,        \
                       partials);                                                              \
  } while (0)
  if (sparse) PP2_CTLQ(true, 4, 1);
  else PP2_CTLQ(false, 4, 1);
#undef PP2_CTLQ
  return hipGetLastError();
}

hipError_t launch_belief_mode(hipStream_t st, const Geom& g, const float* b, const float* mass,
                              float* pv, int* pi) {
  hipLaunchKernelGGL(k_belief_mode, dim3(control_blocks(g)), dim3(kBlock), 0, st, g, b, mass, pv,
                     pi);
  return hipGetLastError();
}

hipError_t launch_control_finish(hipStream_t st, const Geom& g, const float* qpart, int nq,
                                 const float* mass, const float* pv, const int* pi, int nm,
                                 const float* J, const uint8_t* A, uint32_t* rec) {
  hipLaunchKernelGGL(k_control_finish, dim3(1), dim3(kBlock), 0, st, qpart, nq, mass, pv, pi, nm,
                     J, A, g.width, g.wp, rec);
  return hipGetLastError();
}

}  // namespace pp2
