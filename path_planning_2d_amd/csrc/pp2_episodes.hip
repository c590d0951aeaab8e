// pp2_episodes.hip -- batched closed-loop policy episodes on the device
// (gfx950): k_episode_qplanes writes the nine Q planes of the current J
// (k_episode_alpha_planes the planes of the FIB / PBVI alpha vectors), and
// k_episodes runs E independent episodes -- select a control from the belief,
// move the true robot, sample the observation, update the belief -- each
// wholly inside one workgroup whose LDS holds the episode's belief
// (pp2_episodes.h has the LDS layout, include/pp2.h "episodes" the semantics).
// The global placement's instances (k_episodes<POLICY, true>) keep the two
// planes in device memory instead, for grids whose belief does not fit LDS:
// same indexing, same lanes, same arithmetic -- see "global placement" below.
//
// Every quantity is a function of (seed, episode) and the geometry alone:
//  * lane t of the 256 owns the padded plane indices i = 1024 j + 4 t + k
//    (k = 0..3, i < H * wp) for the control reduction, the stencil and the
//    max, so a cell is only ever written by its own lane; the rescale by
//    2^-e2 is not a pass of its own: the plane keeps the raw update and every
//    read multiplies by the step's power of two (exact, the same bits);
//  * the Q dot is acc = acc + fl(b * Q) per lane in ascending i (separate
//    roundings: the file is built with -ffp-contract=off), wave_sum's xor
//    butterfly per wave, then ((w0 + w1) + w2) + w3;
//  * the mode is a (value, index) maximum under a total order, and the belief
//    maximum a plain max: both are exact in any order;
//  * the sampling (counter-based splitmix64 draws, the cumulative scans of the
//    true cell's T row and L row from the class tables) is computed by every
//    lane redundantly from workgroup-uniform values, so a step needs two
//    barriers and no broadcast.
// The belief update is belief_vals' arithmetic (the fmaf chain over the
// action's support in ascending s, then * L_z), gathered by class: raw T of a
// source cell = QR[u][class of its entry for u], L_z = LT[z][L class].
// Off-grid window cells hold b = +0 and code 0, whose finite T adds nothing.
// No atomics, no waits between workgroups, every loop bounded.
#include <limits.h>

#include "pp2_coded_dev.h"
#include "pp2_episodes.h"

namespace pp2 {
namespace {

constexpr int kQ = 9;

// support cells of the actions (kSup / kSupN), indexed at run time
__constant__ unsigned char cSupN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
__constant__ unsigned char cSup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5},
                                         {0, 3, 4, 6}, {4, 0, 0, 0}, {2, 4, 5, 8},
                                         {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};

// ---- Q planes ---------------------------------------------------------------
// k_control_q_coded's structure without the belief: the nine costs of a cell
// (sweep_cell_fact's fmaf chains) stored instead of folded.
__global__ __launch_bounds__(kBlock) void k_episode_qplanes(
    Geom g, const uint16_t* __restrict__ code, const float* __restrict__ rows, int E,
    const float* __restrict__ J, int nblocks, float* __restrict__ Q) {
  extern __shared__ float lds[];
  const int tpr = g.wp / 4;
  const long long np = (long long)g.rows * g.wp;
  stage_rows(rows, rows_floats(E, true), lds);
  __syncthreads();
  const char* qt = reinterpret_cast<const char*>(lds + kFactQT);
  const char* ct = reinterpret_cast<const char*>(lds + kFactCT);
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long long t = (long long)blk * kBlock + threadIdx.x;
    const int y = (int)(t / tpr);
    const int x0 = (int)(t % tpr) * 4;
    if (y >= g.rows) continue;
    const long long off = (long long)y * g.wp + x0;
    const uint2 m = *reinterpret_cast<const uint2*>(code + off);
    const uint32_t cc[4] = {m.x & 0xffffu, m.x >> 16, m.y & 0xffffu, m.y >> 16};
    float jn[9][4];
    load_jn(J, g.wp, y, x0, x0 == 0, x0 + 4 == g.wp, jn);
    float q[kQ][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 iw = *reinterpret_cast<const uint4*>(lds + kFactIW + 4 * cc[k]);
#pragma unroll
      for (int a = 0; a < kQ; ++a) {
        const uint32_t w = a < 4 ? iw.x : a < 8 ? iw.y : iw.z;
        const uint32_t o = __builtin_amdgcn_ubfe(w, 8 * (a % 4), 8);
        const int tab = a * kFactK * 16;
        float tv[4];
        if (kSupN[a] == 1) {
          tv[0] = *reinterpret_cast<const float*>(qt + tab + o);
        } else {
          const f4a tq = *reinterpret_cast<const f4a*>(qt + tab + o);
          tv[0] = tq[0]; tv[1] = tq[1]; tv[2] = tq[2]; tv[3] = tq[3];
        }
        float cost = *reinterpret_cast<const float*>(ct + tab + o);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < kSupN[a]) cost = __builtin_fmaf(tv[j], jn[kSup[a][j]][k], cost);
        q[a][k] = x0 + k < g.width ? cost : 0.0f;  // pad cells: +0
      }
      __builtin_amdgcn_sched_barrier(0);  // one cell's table reads live at a time
    }
#pragma unroll
    for (int a = 0; a < kQ; ++a) store4<false>(Q + a * np + off, q[a]);
  }
}

// ---- alpha planes -----------------------------------------------------------
// out[k][y][x0 .. x0 + 3] of the alpha policy: the FIB plane k of the row
// (fib != null) or PBVI's flat row k at y * W + x; pad cells +0.  One thread
// per quad of one plane.  act_out[k] = acts[k], or k without acts (FIB): the
// run's snapshot of the actions, without a copy call of its own.
__global__ __launch_bounds__(kBlock) void k_episode_alpha_planes(
    Geom g, const float* __restrict__ fib, long long frs, long long fps,
    const float* __restrict__ rows, int ld, int K, float* __restrict__ out,
    const uint8_t* __restrict__ acts, uint8_t* __restrict__ act_out) {
  if (blockIdx.x == 0 && act_out)
    for (int k = threadIdx.x; k < K; k += kBlock) act_out[k] = acts ? acts[k] : (uint8_t)k;
  const int tpr = g.wp / 4;
  const long long qpp = (long long)g.rows * tpr;  // quads per plane
  const long long total = qpp * K;
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < total;
       t += (long long)gridDim.x * kBlock) {
    const int k = (int)(t / qpp);
    const long long r = t - (long long)k * qpp;
    const int y = (int)(r / tpr), x0 = (int)(r % tpr) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0.0f;
      if (x0 + j < g.width)
        v[j] = fib ? fib[(long long)y * frs + (long long)k * fps + x0 + j]
                   : rows[(long long)k * ld + (long long)y * g.width + x0 + j];
    }
    store4<false>(out + ((long long)k * g.rows + y) * g.wp + x0, v);
  }
}

// ---- padded images of a global launch ---------------------------------------
// gcode[i] and gb0[i] for the plane index i = (y + 1) * ps + 4 + x: the code
// and b0 of cell (y, x), +0 / code 0 off the grid (the copies that an LDS
// workgroup makes for itself, made once per run for all workgroups).  ncode
// (a multiple of 8, past the last index a window reads) >= nplane.
__global__ __launch_bounds__(kBlock) void k_episode_pad(Geom g, const uint16_t* __restrict__ code,
                                                        const float* __restrict__ b0, int ncode,
                                                        int nplane, uint16_t* __restrict__ gcode,
                                                        float* __restrict__ gb0) {
  const int ps = g.wp + 4, prows = g.rows + 2;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < ncode; i += gridDim.x * kBlock) {
    const int r = i / ps, c = i - r * ps;
    const int y = r - 1, x = c - 4;
    const bool in = r < prows && y >= 0 && y < g.rows && x >= 0;
    uint16_t cv = 0;
    float bv = 0.0f;
    if (in && x < g.width) cv = code[(long long)y * g.wp + x];
    if (in && x < g.wp) bv = b0[(long long)y * g.wp + x];
    gcode[i] = cv;
    if (i < nplane) gb0[i] = bv;
  }
}

// ---- random numbers ---------------------------------------------------------
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// U(e, d) of the episode with key key_e: 24 bits, [0, 1)
__device__ __forceinline__ float draw(unsigned long long key, unsigned d) {
  const unsigned long long x = mix64(key + kGolden * (unsigned long long)(d + 1u));
  return (float)(unsigned)(x >> 40) * 5.9604644775390625e-08f;  // 2^-24, exact
}

// ---- belief gather of one quad ----------------------------------------------
// cw: the codes of the window (rows y-1 .. y+1, x0-1 .. x0+4), win: its
// beliefs.  p[k] = sum over the support of U, ascending s, of
// T[x + off_s][U][8 - s] * b(x + off_s) (belief_vals' chain).
// cu: the class bytes of action U (4 * class per entry), qr: its QR table.
template <int U>
__device__ __forceinline__ void ep_gather(const uint8_t* cu, const float* qr,
                                          const uint32_t (&cw)[3][6], const float (&win)[3][6],
                                          float (&p)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = 0.0f;
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int sl = sup_slot(U, 8 - s);
    if (sl < 0) continue;
    const int wr = s / 3, wc = s % 3 - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      p[k] = __builtin_fmaf(qr[cu[cw[wr][k + 1 + wc]] + sl], win[wr][k + 1 + wc], p[k]);
  }
}
__device__ __forceinline__ void ep_gather_any(int u, const uint8_t* cu, const float* qr,
                                              const uint32_t (&cw)[3][6],
                                              const float (&win)[3][6], float (&p)[4]) {
  switch (u) {
#define PP2_EG(UU) \
  case UU: ep_gather<UU>(cu, qr, cw, win, p); break;
    PP2_EG(0) PP2_EG(1) PP2_EG(2) PP2_EG(3) PP2_EG(4) PP2_EG(5) PP2_EG(6) PP2_EG(7)
    default: ep_gather<8>(cu, qr, cw, win, p);
#undef PP2_EG
  }
}

__device__ __forceinline__ void mode_take(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// ---- the episodes -----------------------------------------------------------
// The lane's quads in ascending padded index I0 = 4 tid + 1024 j < NP, with
// their row Y and first column X0 stepped instead of divided out (a quad
// never straddles a row: wp is a multiple of 4).
#define PP2_EP_QUADS(I0, Y, X0)                                                   \
  for (int I0 = 4 * tid, Y = qy0, X0 = qx0; I0 < NP; I0 += 4 * kEpThreads, Y += qdy, \
           X0 += qdx, Y += X0 >= wp ? 1 : 0, X0 -= X0 >= wp ? wp : 0)

// ---- control of the alpha-vector policy -------------------------------------
// The lane's partials of NB vectors from k0 on (past K - 1: vector K - 1 again)
// over one pass of the belief: acc[q] = acc[q] + fl(fl(b * sc) * alpha), the
// pinned order.  The plane pointers are formed before the pass, so the NB
// loads of a quad are issued together.
template <int NB>
__device__ __forceinline__ void alpha_dots(const EpisodeRun& a, const float* cur, float sc, int k0,
                                           int tid, int ps, int wp, int NP, int qy0, int qx0,
                                           int qdy, int qdx, float (&acc)[NB]) {
  const float* ap[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    acc[q] = 0.0f;
    ap[q] = a.alpha + (long long)(k0 + q < a.K ? k0 + q : a.K - 1) * NP;
  }
  PP2_EP_QUADS(i0, y, x0) {
    const f4a bv = *reinterpret_cast<const f4a*>(cur + (y + 1) * ps + 4 + x0);
    float bs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bs[j] = bv[j] * sc;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const f4a qv = *reinterpret_cast<const f4a*>(ap[q] + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pr = bs[j] * qv[j];
        acc[q] = acc[q] + pr;
      }
    }
  }
}

// V_k = <stored belief, alpha_k> in the pinned Q-dot order for k = 0 .. K-1;
// best = 0, then for k = 1 .. K-1: if (V_best < V_k) best = k (a NaN sum never
// displaces the incumbent, a NaN V_0 is never displaced).  Returns the action
// of the winner, workgroup-uniform.
//  * K = 9 (FIB): the QMDP control phase -- nine accumulators over one pass of
//    the belief, the per-wave sums in red, one barrier.
//  * else: blocks of kEpAlphaBlock accumulators, so the belief quads are read
//    from LDS (and scaled) once per block; the alpha quads are cached 16-byte
//    loads (every workgroup re-reads the set, from L2).  lane 0 of wave w puts
//    the wave's sum of vector k at asum[buffer][k - c0][w]; one barrier per
//    chunk of kEpAlphaChunk vectors, after which every lane folds the chunk's
//    quads in ascending k.  Two buffers: a wave that writes chunk c + 2 has
//    passed barrier c + 1, which every wave reaches after its reads of chunk c
//    (and a step's belief barrier lies between two steps' chunks).  A tail
//    block re-reads vector K - 1 for its unused accumulators (in bounds, the
//    sums not stored).
// The actions of the vectors at hand (all nine; a chunk's 64) are loaded one
// per lane before the dots and the winner's is read from its lane
// (v_readlane): no global load of action[best] behind the barrier.
__device__ __forceinline__ int alpha_control(const EpisodeRun& a, const EpisodeLds& L, float* lds,
                                             const float* cur, float sc, int k, int e, int qy0,
                                             int qx0, int qdy, int qdx) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wp = a.g.wp, ps = L.ps, K = a.K;
  const int NP = a.g.rows * wp;
  const long long at = (long long)k * a.episodes + e;
  int best = 0, u = 0;
  float vbest = 0.0f;
  if (K == kQ) {
    float* red = lds + L.red;
    // lane l holds the action of vector l: loaded ahead of the dots, so the
    // winner's action is a lane read, not a global load behind the barrier
    const int av = a.alpha_act[lane < kQ ? lane : kQ - 1];
    float acc[kQ];
    alpha_dots<kQ>(a, cur, sc, 0, tid, ps, wp, NP, qy0, qx0, qdy, qdx, acc);
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const float v = wave_sum(acc[q]);
      if (lane == 0) red[wave * kQ + q] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const float sq = ((red[q] + red[kQ + q]) + red[2 * kQ + q]) + red[3 * kQ + q];
      if (q == 0) vbest = sq;
      else if (vbest < sq) { vbest = sq; best = q; }
      if (a.tr_q && tid == q) a.tr_q[at * kQ + q] = sq;
    }
    u = __builtin_amdgcn_readlane(av, __builtin_amdgcn_readfirstlane(best));
  } else {
    float* asum = lds + L.total;
    for (int c0 = 0, buf = 0; c0 < K; c0 += kEpAlphaChunk, buf ^= 1) {
      float* as = asum + buf * (kEpAlphaChunk * 4);
      const int cend = c0 + kEpAlphaChunk < K ? c0 + kEpAlphaChunk : K;
      // lane l holds the action of vector c0 + l (as above)
      const int av = a.alpha_act[c0 + lane < K ? c0 + lane : K - 1];
      for (int kb = c0; kb < cend; kb += kEpAlphaBlock) {
        float acc[kEpAlphaBlock];
        alpha_dots<kEpAlphaBlock>(a, cur, sc, kb, tid, ps, wp, NP, qy0, qx0, qdy, qdx, acc);
#pragma unroll
        for (int q = 0; q < kEpAlphaBlock; ++q) {
          const float v = wave_sum(acc[q]);
          if (lane == 0 && kb + q < cend) as[(kb - c0 + q) * 4 + wave] = v;
        }
      }
      __syncthreads();
      for (int kk = c0; kk < cend; ++kk) {
        const f4a w = *reinterpret_cast<const f4a*>(as + (kk - c0) * 4);
        const float s = ((w[0] + w[1]) + w[2]) + w[3];
        if (kk == 0) vbest = s;
        else if (vbest < s) { vbest = s; best = kk; }
      }
      best = __builtin_amdgcn_readfirstlane(best);
      if (best >= c0) u = __builtin_amdgcn_readlane(av, best - c0);
    }
  }
  if (u > 8) u = 8;  // (the run is refused for more; keeps the tables' bounds)
  if (a.tr_best && tid == 0) {
    a.tr_best[at] = best;
    a.tr_bsum[at] = vbest;
  }
  return u;
}

// ---- control of the one-step lookahead policy -------------------------------
// 64 per-lane values summed across the wave as a reduce-scatter
// (wave_sum_scatter128's scheme, pp2_device.h): every butterfly stage (xor 32,
// 16, 8, 4, 2, 1) halves the values a lane carries, and lane l ends with the
// total of value l -- each total is v_i + v_{i^m} stage by stage from 32 down,
// wave_sum's association, bit for bit.
__device__ __forceinline__ float wave_sum_scatter64(const float (&v)[64]) {
  const int lane = threadIdx.x & 63;
  float v1[32], v2[16], v3[8], v4[4], v5[2], v6[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const auto h = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[j]),
                                                    __float_as_uint(v[32 + j]), false, false);
    v1[j] = __uint_as_float(h[0]) + __uint_as_float(h[1]);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const auto h = __builtin_amdgcn_permlane16_swap(__float_as_uint(v1[j]),
                                                    __float_as_uint(v1[16 + j]), false, false);
    v2[j] = __uint_as_float(h[0]) + __uint_as_float(h[1]);
  }
  auto x8 = [](float x) {
    const float m = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, false));
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x141, 0xf, 0xf, false));
  };
  auto x4 = [](float x) {
    const float m = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, false));
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x1b, 0xf, 0xf, false));
  };
  auto x2 = [](float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4e, 0xf, 0xf, false));
  };
  auto x1 = [](float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xb1, 0xf, 0xf, false));
  };
  // keep the half this lane's xor-group owns, add the partner's copy of it
#define PP2_HALVE(SRC, DST, N, D, XF)                                  \
  {                                                                    \
    const bool h_ = lane & (D);                                        \
    _Pragma("unroll") for (int j = 0; j < (N); ++j) {                  \
      const float keep = h_ ? SRC[(N) + j] : SRC[j];                   \
      const float send = h_ ? SRC[j] : SRC[(N) + j];                   \
      DST[j] = keep + XF(send);                                        \
    }                                                                  \
  }
  PP2_HALVE(v2, v3, 8, 8, x8)
  PP2_HALVE(v3, v4, 4, 4, x4)
  PP2_HALVE(v4, v5, 2, 2, x2)
  PP2_HALVE(v5, v6, 1, 1, x1)
#undef PP2_HALVE
  return v6[0];
}

// One block of the lookahead dots: the lane's partials of the 16 z x NK pairs
// (z, vector kb + q) over one pass of pred = the gather of the stored belief
// for the action at hand, x >= W zeroed: raw_z = fl(pred * L_z) (step 5's
// bits), acc[z][q] = acc[z][q] + fl(raw_z * alpha), the pinned order.  A cell's
// sixteen L_z are four 16-byte reads of the transposed table ltt through its L
// class (the LX byte is 4 * class, so 4 * LX floats in); the pred quad, the
// codes and each alpha quad are read once.  v[4 z + q] = acc[z][q] (q >= NK: 0).
template <int NK>
__device__ __forceinline__ void lookahead_block(const EpisodeRun& a, const float* pred,
                                                const uint16_t* sCode, const uint8_t* sLX,
                                                const float* ltt, int kb, int tid, int ps, int wp,
                                                int NP, int qy0, int qx0, int qdy, int qdx,
                                                float (&v)[64]) {
  float acc[kLaZ][NK];
  const float* ap[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) ap[q] = a.alpha + (long long)(kb + q) * NP;
#pragma unroll
  for (int z = 0; z < kLaZ; ++z)
#pragma unroll
    for (int q = 0; q < NK; ++q) acc[z][q] = 0.0f;
  PP2_EP_QUADS(i0, y, x0) {
    const int at = (y + 1) * ps + 4 + x0;
    const f4a pv = *reinterpret_cast<const f4a*>(pred + at);
    const uint2 cm = *reinterpret_cast<const uint2*>(sCode + at);
    const uint32_t cc[4] = {cm.x & 0xffffu, cm.x >> 16, cm.y & 0xffffu, cm.y >> 16};
    f4a av[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) av[q] = *reinterpret_cast<const f4a*>(ap[q] + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* lc = ltt + 4 * sLX[cc[j]];
#pragma unroll
      for (int zq = 0; zq < kLaZ / 4; ++zq) {
        const f4a lv = *reinterpret_cast<const f4a*>(lc + 4 * zq);
#pragma unroll
        for (int zj = 0; zj < 4; ++zj) {
          const float raw = pv[j] * lv[zj];
#pragma unroll
          for (int q = 0; q < NK; ++q) {
            const float pr = raw * av[q][j];
            acc[4 * zq + zj][q] = acc[4 * zq + zj][q] + pr;
          }
        }
      }
    }
  }
#pragma unroll
  for (int z = 0; z < kLaZ; ++z)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[4 * z + q] = q < NK ? acc[z][q < NK ? q : 0] : 0.0f;
}

// Q_u = <b, R_u> + fl(gamma * sum_z max_k <raw_uz, alpha_k>) for u = 0 .. 8
// (include/pp2.h "Lookahead runs"); returns the first maximum, workgroup-uniform.
// Per action:
//  * one gather of the stored belief (step 5's window and fmaf chain, before
//    * L_z) into the idle plane `pred` -- 9 gathers a step, not 144 -- with the
//    lane's partial of rew[u] on the way; a lane reads back only the quads it
//    wrote, so no barrier lies between the gather and the dots, and only cells
//    that step 5 overwrites are written (halo rows and x pads stay zero);
//  * blocks of 16 z x 4 k accumulators over pred (lookahead_block; a tail
//    block carries only its live vectors), folded per wave by
//    wave_sum_scatter64: lane 4 z + q of wave w puts its total at
//    sums[buffer][4 z + q][w]; one barrier per block, after which lane l folds
//    the quads of z = l % 16 in ascending k into its running (max, index).
//    Two buffers, as alpha_control's chunks.
//  * S_u from the sixteen lanes' maxima in ascending z (lane reads).
// sCode: the instance's code plane (LDS, or a.gcode of a global launch); cur
// and pred are LDS planes or the workgroup's device-memory planes alike.
__device__ __forceinline__ int lookahead_control(const EpisodeRun& a, const EpisodeLds& L,
                                                 float* lds, const uint16_t* sCode,
                                                 const float* cur, float* pred, float sc, int k,
                                                 int e, int qy0, int qx0, int qdy, int qdx) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int W = a.g.width, wp = a.g.wp, ps = L.ps, K = a.K;
  const int NP = a.g.rows * wp;
  const long long at = (long long)k * a.episodes + e;
  float* red = lds + L.red;
  float* sums = lds + L.total;
  const float* ltt = sums + 2 * kLaSums;
  const float* sRf = lds + L.rf;
  const uint8_t* sCls = reinterpret_cast<const uint8_t*>(lds + L.cls);
  const uint8_t* sLX = reinterpret_cast<const uint8_t*>(sRf + kResLX);
  const float* sQR = sRf + kResQR;
  int best = 0, buf = 0;
  float qbest = 0.0f;
  for (int u = 0; u < kQ; ++u) {
    const uint8_t* cu = sCls + u * L.epad;
    const float* qru = sQR + u * kFactK * 4;
    const float* rp = a.rplanes + (long long)u * NP;
    float accr = 0.0f;
    PP2_EP_QUADS(i0, y, x0) {
      float win[3][6];
      uint32_t cw[3][6];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int wa = (y + r) * ps + 4 + x0;
        const f4a mid = *reinterpret_cast<const f4a*>(cur + wa);
        win[r][0] = cur[wa - 1] * sc;
        win[r][1] = mid[0] * sc; win[r][2] = mid[1] * sc;
        win[r][3] = mid[2] * sc; win[r][4] = mid[3] * sc;
        win[r][5] = cur[wa + 4] * sc;
        const uint2 cm = *reinterpret_cast<const uint2*>(sCode + wa);
        cw[r][0] = sCode[wa - 1];
        cw[r][1] = cm.x & 0xffffu; cw[r][2] = cm.x >> 16;
        cw[r][3] = cm.y & 0xffffu; cw[r][4] = cm.y >> 16;
        cw[r][5] = sCode[wa + 4];
      }
      float p[4];
      ep_gather_any(u, cu, qru, cw, win, p);
      const f4a rv = *reinterpret_cast<const f4a*>(rp + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x0 + j >= W) p[j] = 0.0f;
        const float pr = win[1][j + 1] * rv[j];
        accr = accr + pr;
      }
      const f4a out = {p[0], p[1], p[2], p[3]};
      *reinterpret_cast<f4a*>(pred + (y + 1) * ps + 4 + x0) = out;
    }
    accr = wave_sum(accr);
    if (lane == 0) red[wave * kQ + u] = accr;  // read behind the first block's barrier

    float vb = 0.0f;
    int ib = 0;
    for (int kb = 0; kb < K; kb += kLaK, buf ^= 1) {
      float* sb = sums + buf * kLaSums;
      const int nk = K - kb < kLaK ? K - kb : kLaK;
      float v[64];
      switch (nk) {
        case 1: lookahead_block<1>(a, pred, sCode, sLX, ltt, kb, tid, ps, wp, NP, qy0, qx0, qdy, qdx, v); break;
        case 2: lookahead_block<2>(a, pred, sCode, sLX, ltt, kb, tid, ps, wp, NP, qy0, qx0, qdy, qdx, v); break;
        case 3: lookahead_block<3>(a, pred, sCode, sLX, ltt, kb, tid, ps, wp, NP, qy0, qx0, qdy, qdx, v); break;
        default: lookahead_block<4>(a, pred, sCode, sLX, ltt, kb, tid, ps, wp, NP, qy0, qx0, qdy, qdx, v);
      }
      sb[lane * 4 + wave] = wave_sum_scatter64(v);
      __syncthreads();
      const float* sz = sb + (lane & (kLaZ - 1)) * (kLaK * 4);
#pragma unroll
      for (int q = 0; q < kLaK; ++q) {
        if (q < nk) {
          const f4a w = *reinterpret_cast<const f4a*>(sz + 4 * q);
          const float s = ((w[0] + w[1]) + w[2]) + w[3];
          if (kb + q == 0) vb = s;
          else if (vb < s) { vb = s; ib = kb + q; }
        }
      }
    }
    float S = 0.0f;
#pragma unroll
    for (int z = 0; z < kLaZ; ++z)
      S = S + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vb), z));
    const float rew = ((red[u] + red[kQ + u]) + red[2 * kQ + u]) + red[3 * kQ + u];
    const float gs = a.gamma * S;
    const float q = rew + gs;
    if (u == 0) qbest = q;
    else if (qbest < q) { qbest = q; best = u; }
    if (a.tr_q && tid == 0) a.tr_q[at * kQ + u] = q;
    if (a.tr_rew && tid == 0) a.tr_rew[at * kQ + u] = rew;
    if (a.tr_lmax && tid < kLaZ) {
      a.tr_lmax[(at * kQ + u) * kLaZ + tid] = vb;
      a.tr_lidx[(at * kQ + u) * kLaZ + tid] = ib;
    }
  }
  return best;
}

// POLICY: 0 mode, 1 QMDP, 2 the alpha-vector policy (alpha_control), 3 the
// one-step lookahead over the alpha vectors (lookahead_control).
//
// GLOBAL, the global placement (all four policies): the workgroup's two planes are
// its slice of a.gplanes, the code plane is a.gcode (padded like a plane,
// built before the launch, read-only here and shared by all workgroups), and
// step 0 reads the padded b0 image a.gb0 in place of a per-episode copy; the
// tables, red and asum stay in LDS.  The planes were zeroed when they were
// allocated and a step stores the interior quads only, so halo rows and x pads
// hold +0 for good, as the LDS planes' do.  A cell that one wave stores in
// step k is loaded by other waves of the same workgroup in step k + 1, behind
// the step's __syncthreads(): workgroup-scope release / acquire, which orders
// plain vector stores and loads among the waves of one CU (they share its L1;
// the library is not built in threadgroup-split mode).  The plane loads stay
// vector loads (every address is the lane's own), nothing crosses workgroups,
// and there is no agent-scope fence.
//
// The lookahead on global planes (k_episodes<3, true>): sums and ltt sit behind
// episode_lds_global's total, and pred is nxt, the idle plane, as in LDS -- the
// workgroup's plane 0 at step 0 (cur is the shared b0 image, never written),
// afterwards the other of its two planes.  What the LDS instance relies on
// holds here for the same reasons:
//  * the gather stores exactly the quads step 5 stores (PP2_EP_QUADS, cell
//    (y, x0) at (y + 1) * ps + 4 + x0), so the halo rows and x pads of a plane
//    zeroed at allocation stay +0 for the batch's life -- for step 5's window,
//    the workgroup's next episode and later runs of any policy on the batch;
//  * cells x >= W of a quad are stored as +0, as step 5 stores them: whichever
//    of the two wrote a plane last, its cells W <= x < wp hold +0;
//  * a lane reads back only the quads it stored itself: the store and the
//    load are plain C++ accesses of one thread to one address, which the
//    compiler keeps in order (vector store, then vector load behind its
//    s_waitcnt), so no barrier lies between the gather and the dots;
//  * pred is written only while no wave reads it: every wave's window reads
//    of that plane (it was cur one step earlier) precede step 5's barrier of
//    that step, and the episode loop's barrier covers the final belief store.
// The step's two __syncthreads() (and one per block of the dots, on LDS sums)
// remain the only synchronisation.
//
// EXT, the instances of a run with a world attached or of a resumed segment
// (include/pp2.h "The world", "Resumed segments"); a plain run launches the
// EXT = false instances, whose code the flag leaves alone.  Inside it both are
// workgroup-uniform run-time choices:
//  * a.w_code != null, the world: steps 2-4 take the code at s and s', the
//    class byte of (entry, u), the cost, the T support weights, the LX byte and
//    the sixteen L values from the world's own code plane, sweep rows and class
//    tables in device memory -- about two dozen words a step, every lane at
//    the same wave-uniform index (the true cell is made uniform with
//    v_readfirstlane), so each is one L2-resident word that all workgroups
//    share.  No LDS layout grows.  The world's codes index
//    the world's tables only, the believed codes (sCode) the LDS tables only.
//  * a.resume: episode e continues from its stored state -- an episode with
//    status != 0 is left alone altogether; else s = final_cell[e], G = cost[e],
//    d = disc[e], k0 = steps[e] and the stored belief beliefs[e] is the plane,
//    read with sc = 1 (it holds raw * 2^-e2 already).  The LDS instance loads
//    it where a run loads b0; the global instance copies it into the interior
//    quads of its plane 1 (each lane its own quads, the ones step 5 stores:
//    halo rows and x pads stay +0) and works gp1 -> gp0 -> gp1 from there.
//    The draws and the step counts use k0 + j, the traces the local step j.
// Every EXT launch stores the episode's discount in a.disc.
template <int POLICY, bool GLOBAL = false, bool EXT = false>
__global__ __launch_bounds__(kEpThreads) void k_episodes(const EpisodeRun a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Geom g = a.g;
  const EpisodeLds L = GLOBAL ? episode_lds_global(g, a.E) : episode_lds(g, a.E);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int H = g.rows, W = g.width, wp = g.wp, ps = L.ps;
  const int NP = H * wp;
  const int planef = L.prows * ps + 4;
  const int qy0 = 4 * tid / wp, qx0 = 4 * tid - qy0 * wp;          // PP2_EP_QUADS
  const int qdy = 4 * kEpThreads / wp, qdx = 4 * kEpThreads - qdy * wp;
  float* sCT = lds + L.ct;
  float* sRf = lds + L.rf;
  uint8_t* sCls = reinterpret_cast<uint8_t*>(lds + L.cls);
  uint16_t* sCodeL = reinterpret_cast<uint16_t*>(lds + L.code);
  const uint16_t* sCode = GLOBAL ? a.gcode : sCodeL;
  float* red = lds + L.red;  // [4][9] Q partials | 36: mode v[4] | 40: mode i[4] | 44: max[4]
  int* redi = reinterpret_cast<int*>(red);
  const uint8_t* sLX = reinterpret_cast<const uint8_t*>(sRf + kResLX);
  const float* sLT = sRf + kResLT;
  const float* sQR = sRf + kResQR;

  // once per workgroup: the tables and the code plane
  // (plain copies: once per persistent workgroup, and no LDS-DMA slack to pay
  // for in every workgroup's LDS)
  for (int i = tid; i < kEpCtFloats; i += kEpThreads) sCT[i] = a.rows[kFactCT + i];
  for (int i = tid; i < kResTab + ((a.E + 3) >> 2); i += kEpThreads) sRf[i] = a.rfact[i];
  {
    const uint32_t* iw = reinterpret_cast<const uint32_t*>(a.rows + kFactIW);
    for (int i = tid; i < kQ * L.epad; i += kEpThreads) {
      const int q = i / L.epad, en = i - q * L.epad;
      uint32_t cb = 0;  // 16 * class -> 4 * class, the float offset of the class's quad
      if (en < a.E) cb = ((iw[4 * en + (q >> 2)] >> (8 * (q & 3))) & 0xffu) >> 2;
      sCls[i] = (uint8_t)cb;
    }
  }
  if constexpr (!GLOBAL) {
    const int ncode = L.prows * ps + 8;
    for (int i = tid; i < ncode; i += kEpThreads) {
      const int r = i / ps, c = i - r * ps;
      const int y = r - 1, x = c - 4;
      uint16_t v = 0;
      if (r < L.prows && y >= 0 && y < H && x >= 0 && x < W) v = a.code[(long long)y * wp + x];
      sCodeL[i] = v;
    }
  }
  // global placement: the workgroup's planes (64-bit: workgroups x planes pass 2^31 floats)
  float* const gp0 = GLOBAL ? a.gplanes + (long long)blockIdx.x * 2 * a.gstride : nullptr;
  float* const gp1 = GLOBAL ? gp0 + a.gstride : nullptr;
  if constexpr (POLICY == 3) {
    // the L columns transposed, [class][16 z]: a cell's sixteen L_z in one row
    float* ltt = lds + L.total + 2 * kLaSums;
    for (int i = tid; i < kLaZ * kResLK; i += kEpThreads)
      ltt[i] = a.rfact[kResLT + (i & (kLaZ - 1)) * kResLK + (i >> 4)];
  }

  for (int e = blockIdx.x; e < a.episodes; e += gridDim.x) {
    __syncthreads();  // the previous episode's planes are no longer read
    // (global placement: cur is the shared b0 image until the first update,
    // never written through)
    float* cur = GLOBAL ? const_cast<float*>(a.gb0) : lds + L.b0;
    float* nxt = GLOBAL ? gp0 : lds + L.b1;
    const bool resume = EXT && a.resume;
    // (a finished episode of a resumed segment: nothing of it changes)
    if (resume && a.status[e] != 0) continue;
    // the plane an LDS workgroup starts from: b0, or the episode's stored belief
    const float* const bsrc = resume ? a.beliefs + (long long)e * NP : a.b0;
    if constexpr (!GLOBAL) {
      for (int i = tid; i < planef; i += kEpThreads) {
        const int r = i / ps, c = i - r * ps;
        const int y = r - 1, x = c - 4;
        float v = 0.0f;
        if (r < L.prows && y >= 0 && y < H && x >= 0 && x < wp) v = bsrc[(long long)y * wp + x];
        cur[i] = v;
        nxt[i] = 0.0f;
      }
      __syncthreads();
    } else if constexpr (EXT) {
      if (resume) {
        PP2_EP_QUADS(i0, y, x0)
          *reinterpret_cast<f4a*>(gp1 + (y + 1) * ps + 4 + x0) =
              *reinterpret_cast<const f4a*>(bsrc + i0);
        cur = gp1;
        __syncthreads();
      }
    }

    const unsigned long long key = mix64(a.seed + kGolden * (unsigned long long)(e + 1));
    const int s0 = resume ? a.final_cell[e] : a.start[e];
    int sx = s0 % W, sy = s0 / W;
    float G = 0.0f, disc = 1.0f;
    int k0 = 0;  // global step of the segment's first
    if (resume) {
      G = a.cost[e];
      disc = a.disc[e];
      k0 = a.steps[e];
    }
    // The plane holds the last raw update; the stored belief is plane * sc,
    // sc = 2^-e2 of that update, an exact multiply (flush-to-zero) applied
    // wherever the plane is read -- the same bits as a rescaled plane, without
    // a pass over it.
    float sc = 1.0f;
    int steps = k0 + a.horizon, status = 0;
    if (!resume && s0 == a.goal) { steps = 0; status = 1; }

    // k: the segment's own step (the trace row), kg: the episode's
    for (int k = 0; k < a.horizon && status == 0; ++k) {
      const int kg = k0 + k;
      // 1. control: the lane's partials
      int u = 0, mcell = 0;
      if constexpr (POLICY == 3) {
        u = lookahead_control(a, L, lds, sCode, cur, nxt, sc, k, e, qy0, qx0, qdy, qdx);
      } else if constexpr (POLICY == 2) {
        u = alpha_control(a, L, lds, cur, sc, k, e, qy0, qx0, qdy, qdx);
      } else {
      if constexpr (POLICY == 1) {
        float acc[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) acc[q] = 0.0f;
        PP2_EP_QUADS(i0, y, x0) {
          const f4a bv = *reinterpret_cast<const f4a*>(cur + (y + 1) * ps + 4 + x0);
#pragma unroll
          for (int q = 0; q < kQ; ++q) {
            const f4a qv = *reinterpret_cast<const f4a*>(a.Q + (long long)q * NP + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float bs = bv[j] * sc;
              const float pr = bs * qv[j];
              acc[q] = acc[q] + pr;
            }
          }
        }
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const float v = wave_sum(acc[q]);
          if (lane == 0) red[wave * kQ + q] = v;
        }
      } else {
        float v = 0.0f;
        int idx = INT_MAX;
        PP2_EP_QUADS(i0, y, x0) {
          const f4a bv = *reinterpret_cast<const f4a*>(cur + (y + 1) * ps + 4 + x0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
          {
            const float bs = bv[j] * sc;
            if (x0 + j < W && bs > v) { v = bs; idx = y * W + x0 + j; }
          }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const float ov = __shfl_xor(v, o);
          const int oi = __shfl_xor(idx, o);
          mode_take(v, idx, ov, oi);
        }
        if (lane == 0) { red[36 + wave] = v; redi[40 + wave] = idx; }
      }
      __syncthreads();
      if constexpr (POLICY == 1) {
        float best = FLT_MAX;
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const float sq = ((red[q] + red[kQ + q]) + red[2 * kQ + q]) + red[3 * kQ + q];
          if (sq < best) { best = sq; u = q; }
          if (a.tr_q && tid == q) a.tr_q[((long long)k * a.episodes + e) * kQ + q] = sq;
        }
      } else {
        float v = red[36];
        int idx = redi[40];
#pragma unroll
        for (int j = 1; j < 4; ++j) mode_take(v, idx, red[36 + j], redi[40 + j]);
        mcell = idx == INT_MAX ? 0 : idx;
        u = a.A[(long long)(mcell / W) * wp + mcell % W];
        if (u > 8) u = 8;  // (an action plane never holds more; keeps the tables' bounds)
      }
      }
      u = __builtin_amdgcn_readfirstlane(u);

      // 2. cost, 3. motion, 4. observation: every lane, from uniform values
      int z = 15;
      if (EXT && a.w_code) {
        // the world's: its device tables at wave-uniform indices (see EXT
        // above; codes and LX bytes through their aligned dwords)
        const float* __restrict__ const wrows = a.w_rows;
        const float* __restrict__ const wrf = a.w_rfact;
        const uint32_t* __restrict__ const wiw = reinterpret_cast<const uint32_t*>(wrows + kFactIW);
        const uint32_t* __restrict__ const wlx = reinterpret_cast<const uint32_t*>(wrf + kResLX);
        const uint32_t* __restrict__ const wcode = reinterpret_cast<const uint32_t*>(a.w_code);
        sx = __builtin_amdgcn_readfirstlane(sx);
        sy = __builtin_amdgcn_readfirstlane(sy);
        const int ci = sy * wp + sx;  // (< H * wp <= INT_MAX: the planes' own index)
        const uint32_t cs = (wcode[ci >> 1] >> (16 * (ci & 1))) & 0xffffu;
        const uint32_t cls = ((wiw[4 * cs + (u >> 2)] >> (8 * (u & 3))) & 0xffu) >> 2;  // 4 * class
        const float cv = wrows[kFactCT + u * kFactK * 4 + cls];
        const float dc = disc * cv;
        G = G + dc;
        disc = disc * a.gamma;
        const float r = draw(key, 2u * (unsigned)kg);
        const float* __restrict__ const tq = wrf + kResQR + u * kFactK * 4 + cls;
        float c = 0.0f;
        int mv = 4;
        bool found = false;
        const int n = cSupN[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < n) {
            const float t = tq[j];
            c = c + t;
            if (!found && t > 0.0f && r < c) { found = true; mv = cSup[u][j]; }
          }
        }
        mv = __builtin_amdgcn_readfirstlane(mv);
        const int nx = sx + mv % 3 - 1, ny = sy + mv / 3 - 1;
        if (nx >= 0 && nx < W && ny >= 0 && ny < H) { sx = nx; sy = ny; }
        const float r2 = draw(key, 2u * (unsigned)kg + 1u);
        const int ci2 = sy * wp + sx;
        const uint32_t cs2 = (wcode[ci2 >> 1] >> (16 * (ci2 & 1))) & 0xffffu;
        const uint32_t lx = ((wlx[cs2 >> 2] >> (8 * (cs2 & 3))) & 0xffu) >> 2;
        const float* __restrict__ const wlt = wrf + kResLT + lx;
        float c2 = 0.0f;
        bool found2 = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float l = wlt[i * kResLK];
          c2 = c2 + l;
          if (!found2 && l > 0.0f && r2 < c2) { found2 = true; z = i; }
        }
      } else {
      {
        const uint32_t cs = sCode[(sy + 1) * ps + 4 + sx];
        const uint32_t cls = sCls[u * L.epad + cs];  // 4 * class
        const float cv = sCT[u * kFactK * 4 + cls];
        const float dc = disc * cv;
        G = G + dc;
        disc = disc * a.gamma;
        const float r = draw(key, 2u * (unsigned)kg);
        const float* tq = sQR + u * kFactK * 4 + cls;
        float c = 0.0f;
        int mv = 4;
        bool found = false;
        const int n = cSupN[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < n) {
            const float t = tq[j];
            c = c + t;
            if (!found && t > 0.0f && r < c) { found = true; mv = cSup[u][j]; }
          }
        }
        const int nx = sx + mv % 3 - 1, ny = sy + mv / 3 - 1;
        // (a move off the grid is not taken: no generated model has one)
        if (nx >= 0 && nx < W && ny >= 0 && ny < H) { sx = nx; sy = ny; }
      }
      {
        const float r = draw(key, 2u * (unsigned)kg + 1u);
        const uint32_t lx = sLX[sCode[(sy + 1) * ps + 4 + sx]] >> 2;
        float c = 0.0f;
        bool found = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float l = sLT[i * kResLK + lx];
          c = c + l;
          if (!found && l > 0.0f && r < c) { found = true; z = i; }
        }
      }
      }
      z = __builtin_amdgcn_readfirstlane(z);
      if (a.tr_u && tid == 0) {
        const long long at = (long long)k * a.episodes + e;
        a.tr_u[at] = (uint8_t)u;
        a.tr_z[at] = (uint8_t)z;
        a.tr_cell[at] = sy * W + sx;
        if (POLICY == 0) a.tr_mode[at] = mcell;
      }

      // 5. belief: raw update of the lane's quads, and their maximum
      float m = 0.0f;
      const float* lt = sLT + z * kResLK;
      const uint8_t* cu = sCls + u * L.epad;
      const float* qru = sQR + u * kFactK * 4;
      // (two quads' LDS chains -- codes, class bytes, T -- in flight together)
#pragma unroll 2
      PP2_EP_QUADS(i0, y, x0) {
        float win[3][6];
        uint32_t cw[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int at = (y + r) * ps + 4 + x0;
          const f4a mid = *reinterpret_cast<const f4a*>(cur + at);
          win[r][0] = cur[at - 1] * sc;
          win[r][1] = mid[0] * sc; win[r][2] = mid[1] * sc;
          win[r][3] = mid[2] * sc; win[r][4] = mid[3] * sc;
          win[r][5] = cur[at + 4] * sc;
          const uint2 cm = *reinterpret_cast<const uint2*>(sCode + at);
          cw[r][0] = sCode[at - 1];
          cw[r][1] = cm.x & 0xffffu; cw[r][2] = cm.x >> 16;
          cw[r][3] = cm.y & 0xffffu; cw[r][4] = cm.y >> 16;
          cw[r][5] = sCode[at + 4];
        }
        float p[4];
        ep_gather_any(u, cu, qru, cw, win, p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[j] = p[j] * lt[sLX[cw[1][j + 1]] >> 2];
          if (x0 + j >= W) p[j] = 0.0f;
          m = fmaxf(m, p[j]);
        }
        const f4a out = {p[0], p[1], p[2], p[3]};
        *reinterpret_cast<f4a*>(nxt + (y + 1) * ps + 4 + x0) = out;
      }
      m = wave_max(m);
      if (lane == 0) red[44 + wave] = m;
      __syncthreads();
      m = fmaxf(fmaxf(red[44], red[45]), fmaxf(red[46], red[47]));
      if constexpr (GLOBAL) {
        cur = nxt;  // gp0, gp1, gp0, ...: the b0 image is never a target
        nxt = nxt == gp0 ? gp1 : gp0;
      } else {
        float* t = cur;
        cur = nxt;
        nxt = t;
      }
      const uint32_t mb = __float_as_uint(m);
      if (!(m > 0.0f) || mb >= 0x7f800000u) {
        status = 2;  // belief lost: the stored belief stays raw
        steps = kg + 1;
        sc = 1.0f;
      } else {
        int e2 = (int)(mb >> 23) - 127;
        e2 = e2 < -126 ? -126 : e2 > 126 ? 126 : e2;
        sc = __uint_as_float((uint32_t)(127 - e2) << 23);
        // 6. goal
        if (sy * W + sx == a.goal) { status = 1; steps = kg + 1; }
      }
    }

    // the episode's results, and its stored belief (each lane its own quads;
    // an episode that took no step reads the b0 image, behind the barrier above)
    if (tid == 0) {
      a.steps[e] = steps;
      a.status[e] = (uint8_t)status;
      a.cost[e] = G;
      a.final_cell[e] = sy * W + sx;
      if constexpr (EXT) a.disc[e] = disc;
    }
    float* bo = a.beliefs + (long long)e * NP;
    PP2_EP_QUADS(i0, y, x0) {
      f4a v = *reinterpret_cast<const f4a*>(cur + (y + 1) * ps + 4 + x0);
      // (sc = 1: b0 or a raw update, stored as it is -- a multiply would flush
      // b0's subnormals)
      if (sc != 1.0f) { v[0] = v[0] * sc; v[1] = v[1] * sc; v[2] = v[2] * sc; v[3] = v[3] * sc; }
      *reinterpret_cast<f4a*>(bo + i0) = v;
    }
  }
}

#undef PP2_EP_QUADS

}  // namespace

hipError_t launch_episode_qplanes(hipStream_t st, const Geom& g, const uint16_t* code,
                                  const float* rows, int E, const float* J, float* Q, int ncus) {
  const size_t lds = (size_t)lds_span(rows_floats(E, true)) * sizeof(float);
  if (lds > kDictLdsMaxBytes) return hipErrorInvalidValue;
  static unsigned long long attr = 0;
  allow_lds(reinterpret_cast<const void*>(&k_episode_qplanes), attr);
  const int nblocks = cells_grid(g, 4);
  const int cap = ncus > 0 ? 4 * ncus : nblocks;
  hipLaunchKernelGGL(k_episode_qplanes, dim3(nblocks < cap ? nblocks : cap), dim3(kBlock), lds, st,
                     g, code, rows, E, J, nblocks, Q);
  return hipGetLastError();
}

hipError_t launch_episode_alpha_planes(hipStream_t st, const Geom& g, const PlaneSet* fib,
                                       const float* rows, int ld, int K, float* out,
                                       const uint8_t* acts, uint8_t* act_out) {
  if (K < 1 || K > kEpAlphaMax || (!fib && !rows) || (fib && K != 9)) return hipErrorInvalidValue;
  const long long quads = (long long)g.rows * (g.wp / 4) * K;
  const long long nblocks = (quads + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_episode_alpha_planes, dim3((unsigned)(nblocks < 4096 ? nblocks : 4096)),
                     dim3(kBlock), 0, st, g, fib ? fib->p : nullptr, fib ? fib->rs : 0,
                     fib ? fib->ps : 0, rows, ld, K, out, acts, act_out);
  return hipGetLastError();
}

hipError_t launch_episode_pad(hipStream_t st, const Geom& g, const uint16_t* code,
                              const float* b0, uint16_t* gcode, float* gb0) {
  const long long ncode = ep_code_elems(g);
  const long long nplane = ((long long)g.rows + 2) * (g.wp + 4) + 4;
  if (ncode > INT_MAX || !code || !b0 || !gcode || !gb0) return hipErrorInvalidValue;
  const long long nblocks = (ncode + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_episode_pad, dim3((unsigned)(nblocks < 4096 ? nblocks : 4096)),
                     dim3(kBlock), 0, st, g, code, b0, (int)ncode, (int)nplane, gcode, gb0);
  return hipGetLastError();
}

namespace {
// One instance (16 in all: policy x placement x EXT), with its own opt-in to
// the large LDS.
template <int POLICY, bool GLOBAL, bool EXT>
hipError_t launch_instance(hipStream_t st, const EpisodeRun& a, int workgroups, long long bytes) {
  static unsigned long long attr = 0;
  allow_lds(reinterpret_cast<const void*>(&k_episodes<POLICY, GLOBAL, EXT>), attr);
  hipLaunchKernelGGL((k_episodes<POLICY, GLOBAL, EXT>), dim3(workgroups), dim3(kEpThreads),
                     (size_t)bytes, st, a);
  return hipGetLastError();
}
template <bool GLOBAL, bool EXT>
hipError_t launch_policy(hipStream_t st, const EpisodeRun& a, int policy, int workgroups,
                         long long bytes) {
  switch (policy) {
    case 3: return launch_instance<3, GLOBAL, EXT>(st, a, workgroups, bytes);
    case 2: return launch_instance<2, GLOBAL, EXT>(st, a, workgroups, bytes);
    case 1: return launch_instance<1, GLOBAL, EXT>(st, a, workgroups, bytes);
    default: return launch_instance<0, GLOBAL, EXT>(st, a, workgroups, bytes);
  }
}

// disc[e] = the discount after steps[e] steps: d = 1, then d = fl(d * gamma)
// once per step taken -- what an EXT launch stores itself, made up for a plain
// run (whose instances store none) when a resumed segment follows it.
__global__ __launch_bounds__(kBlock) void k_episode_discounts(const int32_t* __restrict__ steps,
                                                              float gamma, int episodes,
                                                              float* __restrict__ disc) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= episodes) return;
  float d = 1.0f;
  for (int k = 0, n = steps[e]; k < n; ++k) d = d * gamma;
  disc[e] = d;
}
}  // namespace

hipError_t launch_episode_discounts(hipStream_t st, const int32_t* steps, float gamma,
                                    int episodes, float* disc) {
  if (!steps || !disc || episodes < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_episode_discounts, dim3((episodes + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     st, steps, gamma, episodes, disc);
  return hipGetLastError();
}

hipError_t launch_episodes(hipStream_t st, const EpisodeRun& a, int policy, int workgroups,
                           bool global, bool ext) {
  if (policy < 0 || policy > 3 || workgroups < 1) return hipErrorInvalidValue;
  if (policy == 3 && (!a.alpha || !a.rplanes || a.K < 1 || a.K > kEpAlphaMax))
    return hipErrorInvalidValue;
  if (policy == 2 && (!a.alpha || !a.alpha_act || a.K < 1 || a.K > kEpAlphaMax))
    return hipErrorInvalidValue;
  // an EXT launch stores the discounts; a world comes with all three tables
  if (ext && (!a.disc || (a.w_code && (!a.w_rows || !a.w_rfact)))) return hipErrorInvalidValue;
  if (!ext && (a.resume || a.w_code)) return hipErrorInvalidValue;
  long long bytes;
  if (global) {
    // tables, red and asum (the lookahead: sums and ltt) in LDS, planes in a.gplanes
    if (!a.gplanes || !a.gb0 || !a.gcode ||
        a.gstride < ((long long)a.g.rows + 2) * (a.g.wp + 4) + 4)
      return hipErrorInvalidValue;
    bytes = episode_global_lds_bytes(a.E, policy == 3   ? ep_lookahead_floats()
                                          : policy == 2 ? ep_alpha_floats(a.K)
                                                        : 0);
  } else {
    bytes = policy == 3   ? episode_lookahead_lds_bytes(a.g, a.E)
            : policy == 2 ? episode_alpha_lds_bytes(a.g, a.E, a.K)
                          : episode_lds_bytes(a.g, a.E);
  }
  if (bytes > (long long)kDictLdsMaxBytes) return hipErrorInvalidValue;
  if (global)
    return ext ? launch_policy<true, true>(st, a, policy, workgroups, bytes)
               : launch_policy<true, false>(st, a, policy, workgroups, bytes);
  return ext ? launch_policy<false, true>(st, a, policy, workgroups, bytes)
             : launch_policy<false, false>(st, a, policy, workgroups, bytes);
}

}  // namespace pp2
