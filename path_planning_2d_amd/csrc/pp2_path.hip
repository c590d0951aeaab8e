// pp2_path.hip -- gfx950 kernels of the shortest-path field (include/pp2.h
// "shortest-path field"): a tiled relaxation from +inf.
//
// One round = one launch of a workgroup per tile.  A clean tile returns at
// once.  A dirty one stages its kPathTileRows x kPathTileCols cells of D plus
// a one-cell ring into LDS (cells off the grid: +inf), relaxes in place for at
// most kPathInnerSweeps sweeps (until one lowers nothing), writes the lowered
// cells back and marks, for the next round, the tiles that see a border cell
// it lowered (the corner tiles too: diagonals cross corners) -- and itself, if
// it ran out of sweeps.  No workgroup waits for another: every loop is bounded
// by a constant or the tile's size, and the round boundary is the kernel
// boundary.  Relaxing from +inf only lowers a value, never below the unique
// solution, so a ring cell read before or after its owner rewrote it, and the
// in-place sweeps' read order, change the path taken but not the bits reached.
//
// Lane = tile column, wave w = tile rows 8w .. 8w + 7: a thread walks its 8
// cells down the column through a sliding three-row window (30 LDS reads a
// sweep; row stride kS = 66 words, so the 64 lanes of a row access hit 64
// banks), stores each cell that fell and hands its new value on to the cell
// below in a register.  fl32(x + c) is monotone in x, so the minimum over the
// four diagonal (axis) neighbours is taken before the one add of their cost:
// the same bits as the minimum of the eight sums, in 2 adds and 5 mins a cell.
// The tile's occupancy is a byte mask per thread: only a tile's own cells are
// tested for it (an occupied ring cell holds +inf).  Of the forms measured
// (profiles/path/ab_sweep_variants.txt: this one, the eight sums, the whole
// window read ahead of the arithmetic) this is the fastest at 256^2 and 1024^2
// and level with the eight sums at 2048^2.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pp2_path.h"

namespace pp2 {
namespace {

constexpr int kTR = kPathTileRows, kTC = kPathTileCols;
constexpr int kS = kTC + 2;              // LDS row stride (words)
constexpr int kRows = kTR / 4;           // rows per wave
constexpr float kAxis = 1.0f;
constexpr float kDiag = 0x1.6a09e6p+0f;  // fp32 sqrt 2
static_assert(kTC == 64 && kPathThreads == 256 && kTR % 4 == 0, "lane = column, 4 waves");

__global__ __launch_bounds__(kPathThreads) void k_path_init(Geom g, const uint8_t* __restrict__ map,
                                                            int gx, int gy, float* __restrict__ D,
                                                            int* __restrict__ words, int nwords) {
  const long long n = (long long)(g.rows + 2) * g.wp;  // rows -1 .. rows
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const bool goal_ok = gx >= 0 && gx < g.width && gy >= 0 && gy < g.rows &&
                       map[(long long)gy * g.width + gx] != 1;
  const long long goal_at = (long long)(gy + 1) * g.wp + gx;
  for (long long i = i0; i < n; i += stride)
    D[i - g.wp] = goal_ok && i == goal_at ? 0.0f : INFINITY;
  // dirty for round 0: every tile that sees the goal, in its cells or in its
  // ring (the goal's own value never falls, so it would mark nobody)
  const int ntx = path_tiles_x(g), nt = ntx * path_tiles_y(g);
  for (long long i = i0; i < nwords; i += stride) {
    const int t = (int)i - kPathWordDirty;
    int v = 0;
    if (goal_ok && t >= 0 && t < nt) {
      const int y0 = (t / ntx) * kTR, x0 = (t % ntx) * kTC;
      v = gx >= x0 - 1 && gx <= x0 + kTC && gy >= y0 - 1 && gy <= y0 + kTR;
    }
    words[i] = v;
  }
}

__global__ __launch_bounds__(kPathThreads) void k_path_round(Geom g, const uint8_t* __restrict__ map,
                                                             float* __restrict__ D,
                                                             int* __restrict__ words, int round,
                                                             int slot) {
  __shared__ float sD[(kTR + 2) * kS];
  __shared__ int s_mark;
  const int ntx = path_tiles_x(g), nty = path_tiles_y(g), nt = ntx * nty;
  const int tile = blockIdx.x;
  if (tile >= nt) return;
  int* cur = words + kPathWordDirty + (round & 1) * nt;
  int* nxt = words + kPathWordDirty + ((round + 1) & 1) * nt;
  if (cur[tile] == 0) return;  // (uniform over the workgroup: nobody writes cur this round)
  const int tid = threadIdx.x;
  const int ty = tile / ntx, tx = tile % ntx;
  const int y0 = ty * kTR, x0 = tx * kTC;
  const int H = g.rows, W = g.width, wp = g.wp;
  if (tid == 0) s_mark = 0;
  // the tile and its ring; off the grid: +inf
  for (int i = tid; i < (kTR + 2) * kS; i += kPathThreads) {
    const int y = y0 - 1 + i / kS, x = x0 - 1 + i % kS;
    sD[i] = y >= 0 && y < H && x >= 0 && x < W ? D[(long long)y * wp + x] : INFINITY;
  }
  const int lane = tid & 63, r0 = (tid >> 6) * kRows;
  const int x = x0 + lane;
  // bit k: cell (r0 + k, lane) is never relaxed (occupied or off the grid)
  unsigned skip = 0;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + r0 + k;
    const bool live = y < H && x < W && map[(long long)y * W + x] != 1;
    skip |= live ? 0u : 1u << k;
  }
  __syncthreads();  // (also orders every thread's read of cur[tile] before the clear below)
  if (tid == 0) atomicAnd(&cur[tile], 0);
  const int base = r0 * kS + lane;  // LDS index of (tile row r0 - 1, tile column lane - 1)
  float orig[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) orig[k] = sD[base + (k + 1) * kS + 1];
  int more = 0;
  for (int s = 0; s < kPathInnerSweeps; ++s) {
    int changed = 0;
    float hu = fminf(sD[base], sD[base + 2]), u1 = sD[base + 1];
    float hm = fminf(sD[base + kS], sD[base + kS + 2]), m1 = sD[base + kS + 1];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int at = base + (k + 2) * kS;
      const float hd = fminf(sD[at], sD[at + 2]), d1 = sD[at + 1];
      if (!((skip >> k) & 1u)) {
        const float best = fminf(fminf(hu, hd) + kDiag, fminf(fminf(u1, d1), hm) + kAxis);
        if (best < m1) {
          m1 = best;
          sD[at - kS + 1] = best;
          changed = 1;
        }
      }
      hu = hm; u1 = m1;
      hm = hd; m1 = d1;
    }
    more = __syncthreads_or((int)changed);
    if (!more) break;
  }
  // write back what fell; border cells that fell mark the tiles that see them
  const int rl = (H - y0 < kTR ? H - y0 : kTR) - 1, cl = (W - x0 < kTC ? W - x0 : kTC) - 1;
  int mark = 0;  // bit (dy + 1) * 3 + (dx + 1): the tile at (ty + dy, tx + dx)
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    if ((skip >> k) & 1u) continue;
    const int r = r0 + k;
    const float v = sD[base + (k + 1) * kS + 1];
    if (!(v < orig[k])) continue;
    D[(long long)(y0 + r) * wp + x] = v;
    // (a one-row or one-column tile's cell is on both borders)
    const bool up = r == 0, down = r == rl, left = lane == 0, right = lane == cl;
    if (up) mark |= 1 << 1;
    if (down) mark |= 1 << 7;
    if (left) mark |= 1 << 3;
    if (right) mark |= 1 << 5;
    if (up && left) mark |= 1 << 0;
    if (up && right) mark |= 1 << 2;
    if (down && left) mark |= 1 << 6;
    if (down && right) mark |= 1 << 8;
  }
  if (more) mark |= 1 << 4;  // out of sweeps: this tile again
  if (mark) atomicOr(&s_mark, mark);
  __syncthreads();
  const int all = s_mark;
  if (tid < 9 && ((all >> tid) & 1)) {
    const int ny = ty + tid / 3 - 1, nx = tx + tid % 3 - 1;
    if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) {
      atomicOr(&nxt[ny * ntx + nx], 1);
      atomicOr(&words[kPathWordMarks + slot], 1);
    }
  }
}

__global__ void k_path_poll(int* __restrict__ words, int n, uint32_t* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int quiet = -1;
  for (int i = 0; i < n; ++i) {
    if (quiet < 0 && words[kPathWordMarks + i] == 0) quiet = i;
    words[kPathWordMarks + i] = 0;
  }
  rec[kPathRecQuiet] = (uint32_t)quiet;
}

__global__ __launch_bounds__(kPathThreads) void k_path_actions(Geom g, int gx, int gy,
                                                               const float* __restrict__ D,
                                                               uint8_t* __restrict__ A,
                                                               int* __restrict__ words) {
  const int H = g.rows, W = g.width, wp = g.wp;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < (long long)H * W;
  bool finite = false;
  if (in) {
    const int y = (int)(i / W), x = (int)(i % W);
    const float d = D[(long long)y * wp + x];
    finite = d < INFINITY;
    int act = 4;
    if (finite && !(x == gx && y == gy)) {
      float best = INFINITY;
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        if (u == 4) continue;
        const int dx = u % 3 - 1, dy = u / 3 - 1;
        const int xx = x + dx, yy = y + dy;
        const float nb = xx >= 0 && xx < W && yy >= 0 && yy < H ? D[(long long)yy * wp + xx]
                                                                 : INFINITY;
        const float cand = nb + (dx != 0 && dy != 0 ? kDiag : kAxis);
        if (cand < best) {
          best = cand;
          act = u;
        }
      }
    }
    A[(long long)y * wp + x] = (uint8_t)act;
  }
  const unsigned long long m = __ballot(finite);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&words[kPathWordReached], (int)__popcll(m));
}

__global__ void k_path_report(const int* __restrict__ words, uint32_t* __restrict__ rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    rec[kPathRecReached] = (uint32_t)words[kPathWordReached];
}

// ---- warm re-solve: seed, raise rounds (DESIGN.md §2.3 "Warm re-solve") ----
//
// The planes hold a converged (D, A) of an earlier map; `map` is the map now.
// The seed pass compares the two on the changed rectangles; the raise rounds
// then throw away every value whose parent chain (by the old A) runs through a
// cell that no longer stands, and k_path_round repairs the hole.  "Parent
// reads +inf" is a monotone operator on the set of raised cells, so as in the
// relaxation the schedule (tile order, in-place sweeps, a ring cell read before
// or after its owner rewrote it) changes the path taken and not the set reached.

__global__ __launch_bounds__(kPathThreads) void k_path_seed(Geom g, const uint8_t* __restrict__ map,
                                                            float* __restrict__ D,
                                                            int* __restrict__ words,
                                                            PathSeedRects R, long long cells) {
  const int H = g.rows, W = g.width, wp = g.wp;
  const int ntx = path_tiles_x(g), nty = path_tiles_y(g), nt = ntx * nty;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool in = i < cells;
  int x = 0, y = 0;
  if (in) {
    int j = 0;
    for (; j < R.n; ++j) {
      const long long a = (long long)R.w[j] * R.h[j];
      if (i < a) break;
      i -= a;
    }
    in = j < R.n;
    if (in) {
      x = R.x0[j] + (int)(i % R.w[j]);
      y = R.y0[j] + (int)(i / R.w[j]);
      in = x >= 0 && x < W && y >= 0 && y < H;
    }
  }
  bool seed = false;
  if (in) {
    const bool occupied = map[(long long)y * W + x] == 1;
    const bool finite = D[(long long)y * wp + x] < INFINITY;
    seed = occupied && finite;
    const int ty = y / kTR, tx = x / kTC;
    if (seed) {
      D[(long long)y * wp + x] = INFINITY;
      // raise-dirty: every tile that sees the seed, in its cells or in its
      // ring (k_path_init's test for the goal)
      int* rd = words + path_word_raise(nt);
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int ny = ty + dy, nx = tx + dx;
          if (ny < 0 || ny >= nty || nx < 0 || nx >= ntx) continue;
          const int y0 = ny * kTR, x0 = nx * kTC;
          if (x >= x0 - 1 && x <= x0 + kTC && y >= y0 - 1 && y <= y0 + kTR)
            atomicOr(&rd[ny * ntx + nx], 1);
        }
    } else if (!occupied && !finite) {
      // freed, or free and unreachable before: the relaxation starts here
      atomicOr(&words[kPathWordDirty + ty * ntx + tx], 1);
    }
  }
  const unsigned long long m = __ballot(seed);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&words[path_word_seeds(nt)], (int)__popcll(m));
}

// The raise counterpart of k_path_round: the same tile, ring, LDS image and
// lane = column layout.  A thread keeps its 8 cells' parents as LDS index
// deltas (0: a cell that is never raised -- occupied, off the grid, the goal,
// or +inf already, whose A is 4).  The parent read is a gather: the 64 lanes
// of one access read row r - 1, r or r + 1 at their own column -1, 0 or +1, so
// at most 3 lanes meet in a bank.
__global__ __launch_bounds__(kPathThreads) void k_path_raise_round(
    Geom g, const uint8_t* __restrict__ map, float* __restrict__ D, const uint8_t* __restrict__ A,
    int* __restrict__ words, int round, int slot) {
  __shared__ float sD[(kTR + 2) * kS];
  __shared__ int s_mark;
  const int ntx = path_tiles_x(g), nty = path_tiles_y(g), nt = ntx * nty;
  const int tile = blockIdx.x;
  if (tile >= nt) return;
  int* cur = words + path_word_raise(nt) + (round & 1) * nt;
  int* nxt = words + path_word_raise(nt) + ((round + 1) & 1) * nt;
  if (cur[tile] == 0) return;  // (uniform over the workgroup: nobody writes cur this round)
  const int tid = threadIdx.x;
  const int ty = tile / ntx, tx = tile % ntx;
  const int y0 = ty * kTR, x0 = tx * kTC;
  const int H = g.rows, W = g.width, wp = g.wp;
  if (tid == 0) s_mark = 0;
  // the tile and its ring; off the grid: +inf
  for (int i = tid; i < (kTR + 2) * kS; i += kPathThreads) {
    const int y = y0 - 1 + i / kS, x = x0 - 1 + i % kS;
    sD[i] = y >= 0 && y < H && x >= 0 && x < W ? D[(long long)y * wp + x] : INFINITY;
  }
  const int lane = tid & 63, r0 = (tid >> 6) * kRows;
  const int x = x0 + lane;
  int par[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + r0 + k;
    const bool live = y < H && x < W && map[(long long)y * W + x] != 1;
    const int u = live ? (int)A[(long long)y * wp + x] : 4;
    par[k] = u < 9 ? (u / 3 - 1) * kS + (u % 3 - 1) : 0;
  }
  __syncthreads();  // (also orders every thread's read of cur[tile] before the clear below)
  if (tid == 0) atomicAnd(&cur[tile], 0);
  const int base = r0 * kS + lane;  // LDS index of (tile row r0 - 1, tile column lane - 1)
  unsigned was = 0;                 // bit k: cell k was finite when the round began
#pragma unroll
  for (int k = 0; k < kRows; ++k)
    was |= sD[base + (k + 1) * kS + 1] < INFINITY ? 1u << k : 0u;
  int more = 0;
  for (int s = 0; s < kPathInnerSweeps; ++s) {
    int changed = 0;
    // top-down and in place: a raise travels down a column within one sweep
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int at = base + (k + 1) * kS + 1;
      if (par[k] != 0 && sD[at] < INFINITY && !(sD[at + par[k]] < INFINITY)) {
        sD[at] = INFINITY;
        changed = 1;
      }
    }
    more = __syncthreads_or(changed);
    if (!more) break;
  }
  // +inf to what was raised; border cells among them mark the tiles that see them
  const int rl = (H - y0 < kTR ? H - y0 : kTR) - 1, cl = (W - x0 < kTC ? W - x0 : kTC) - 1;
  int mark = 0;  // bit (dy + 1) * 3 + (dx + 1): the tile at (ty + dy, tx + dx); bit 9: any raised
  int count = 0;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int r = r0 + k;
    const bool raised = ((was >> k) & 1u) && !(sD[base + (k + 1) * kS + 1] < INFINITY);
    count += (int)__popcll(__ballot(raised));
    if (!raised) continue;
    D[(long long)(y0 + r) * wp + x] = INFINITY;
    mark |= 1 << 9;
    // (a one-row or one-column tile's cell is on both borders)
    const bool up = r == 0, down = r == rl, left = lane == 0, right = lane == cl;
    if (up) mark |= 1 << 1;
    if (down) mark |= 1 << 7;
    if (left) mark |= 1 << 3;
    if (right) mark |= 1 << 5;
    if (up && left) mark |= 1 << 0;
    if (up && right) mark |= 1 << 2;
    if (down && left) mark |= 1 << 6;
    if (down && right) mark |= 1 << 8;
  }
  if (lane == 0 && count) atomicAdd(&words[path_word_raised(nt)], count);
  if (more) mark |= 1 << 4;  // out of sweeps: this tile again
  if (mark) atomicOr(&s_mark, mark);
  __syncthreads();
  const int all = s_mark;
  if (tid < 9 && ((all >> tid) & 1)) {
    const int ny = ty + tid / 3 - 1, nx = tx + tid % 3 - 1;
    if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) {
      atomicOr(&nxt[ny * ntx + nx], 1);
      atomicOr(&words[kPathWordMarks + slot], 1);
    }
  }
  // the relaxation's round 0 repairs what this tile lost
  if (tid == 9 && ((all >> 9) & 1)) atomicOr(&words[kPathWordDirty + tile], 1);
}

__global__ void k_path_resolve_report(const int* __restrict__ words, int nt,
                                      uint32_t* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  rec[kPathRecReached] = (uint32_t)words[kPathWordReached];
  rec[kPathRecRaised] = (uint32_t)words[path_word_raised(nt)];
  rec[kPathRecSeeds] = (uint32_t)words[path_word_seeds(nt)];
}

}  // namespace

hipError_t launch_path_init(hipStream_t st, const Geom& g, const uint8_t* map, int gx, int gy,
                            float* D, int* words) {
  const long long n = (long long)(g.rows + 2) * g.wp;
  long long blocks = (n + kPathThreads - 1) / kPathThreads;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_path_init, dim3((unsigned)blocks), dim3(kPathThreads), 0, st, g, map, gx, gy,
                     D, words, (int)path_words(g));
  return hipGetLastError();
}

hipError_t launch_path_round(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                             int* words, int round, int slot) {
  if (slot < 0 || slot >= kPathBatchMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_path_round, dim3(path_tiles(g)), dim3(kPathThreads), 0, st, g, map, D, words,
                     round, slot);
  return hipGetLastError();
}

hipError_t launch_path_poll(hipStream_t st, int* words, int n, uint32_t* rec) {
  if (n < 1 || n > kPathBatchMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_path_poll, dim3(1), dim3(64), 0, st, words, n, rec);
  return hipGetLastError();
}

hipError_t launch_path_actions(hipStream_t st, const Geom& g, int gx, int gy, const float* D,
                               uint8_t* A, int* words, uint32_t* rec) {
  const long long n = (long long)g.rows * g.width;
  hipLaunchKernelGGL(k_path_actions, dim3((unsigned)((n + kPathThreads - 1) / kPathThreads)),
                     dim3(kPathThreads), 0, st, g, gx, gy, D, A, words);
  hipLaunchKernelGGL(k_path_report, dim3(1), dim3(64), 0, st, words, rec);
  return hipGetLastError();
}

hipError_t launch_path_seed(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                            int* words, const PathSeedRects& rects, long long cells) {
  if (rects.n < 0 || rects.n > kPathSeedRects) return hipErrorInvalidValue;
  long long sum = 0;
  for (int j = 0; j < rects.n; ++j) {
    if (rects.w[j] < 1 || rects.h[j] < 1 || rects.x0[j] < 0 || rects.y0[j] < 0 ||
        rects.w[j] > g.width - rects.x0[j] || rects.h[j] > g.rows - rects.y0[j])
      return hipErrorInvalidValue;
    sum += (long long)rects.w[j] * rects.h[j];
  }
  if (sum != cells) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(words, 0, path_words(g) * sizeof(int), st);
  if (e != hipSuccess) return e;
  if (cells == 0) return hipSuccess;
  hipLaunchKernelGGL(k_path_seed, dim3((unsigned)((cells + kPathThreads - 1) / kPathThreads)),
                     dim3(kPathThreads), 0, st, g, map, D, words, rects, cells);
  return hipGetLastError();
}

hipError_t launch_path_raise_round(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                                   const uint8_t* A, int* words, int round, int slot) {
  if (slot < 0 || slot >= kPathBatchMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_path_raise_round, dim3(path_tiles(g)), dim3(kPathThreads), 0, st, g, map, D,
                     A, words, round, slot);
  return hipGetLastError();
}

hipError_t launch_path_resolve_actions(hipStream_t st, const Geom& g, int gx, int gy,
                                       const float* D, uint8_t* A, int* words, uint32_t* rec) {
  const long long n = (long long)g.rows * g.width;
  hipLaunchKernelGGL(k_path_actions, dim3((unsigned)((n + kPathThreads - 1) / kPathThreads)),
                     dim3(kPathThreads), 0, st, g, gx, gy, D, A, words);
  hipLaunchKernelGGL(k_path_resolve_report, dim3(1), dim3(64), 0, st, words, path_tiles(g), rec);
  return hipGetLastError();
}

}  // namespace pp2
