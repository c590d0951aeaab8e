// pp2_path.h -- shared between the shortest-path field's kernels
// (pp2_path.hip) and their host side (pp2_path.cpp).  The definition of the
// field is in include/pp2.h ("shortest-path field"); DESIGN.md §2.3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pp2_internal.h"

namespace pp2 {

// The relaxation's tile: kPathTileCols = one wavefront, so a tile row is one
// conflict-free LDS access and one 256-B stretch of the plane; kPathTileRows
// = 8 rows for each of the workgroup's 4 waves.
constexpr int kPathTileRows = 32;
constexpr int kPathTileCols = 64;
constexpr int kPathThreads = 256;
// In-LDS sweeps of one tile per round, at most: a value crosses the tile
// along a row (one cell per sweep) and turns into the next lane within one
// round.  The sweeps stop at the first that lowers nothing.
constexpr int kPathInnerSweeps = kPathTileRows + kPathTileCols;
// Rounds enqueued between two polls, at most (the mark words of one batch).
constexpr int kPathBatchMax = 256;

// Device words (int): marks[kPathBatchMax] -- round i of the batch lowered a
// border cell or ran out of inner sweeps --, then the count of finite cells,
// then dirty[2][ntiles] (round r relaxes the tiles of dirty[r & 1] and marks
// into dirty[(r + 1) & 1]).
constexpr int kPathWordMarks = 0;
constexpr int kPathWordReached = kPathBatchMax;
constexpr int kPathWordDirty = kPathBatchMax + 1;
__host__ __device__ inline int path_tiles_x(const Geom& g) { return (g.width + kPathTileCols - 1) / kPathTileCols; }
__host__ __device__ inline int path_tiles_y(const Geom& g) { return (g.rows + kPathTileRows - 1) / kPathTileRows; }
__host__ __device__ inline int path_tiles(const Geom& g) { return path_tiles_x(g) * path_tiles_y(g); }
// The warm re-solve's words follow: raise_dirty[2][ntiles] (the raise rounds'
// ping-pong, as dirty[][] is the relaxation's), the count of raised cells and
// the count of seeds (finite cells found occupied).
__host__ __device__ inline int path_word_raise(int ntiles) { return kPathWordDirty + 2 * ntiles; }
__host__ __device__ inline int path_word_raised(int ntiles) { return kPathWordDirty + 4 * ntiles; }
__host__ __device__ inline int path_word_seeds(int ntiles) { return kPathWordDirty + 4 * ntiles + 1; }
inline size_t path_words(const Geom& g) { return (size_t)kPathWordDirty + 4 * (size_t)path_tiles(g) + 2; }

// The pinned record (4-byte words) the poll and report kernels write.
constexpr int kPathRecQuiet = 0;    // index of the batch's first quiet round, -1: none
constexpr int kPathRecReached = 1;  // cells with finite D
constexpr int kPathRecRaised = 2;   // cells a warm re-solve raised (seeds not counted)
constexpr int kPathRecSeeds = 3;    // finite cells its seed pass found occupied
constexpr int kPathRec = 4;

// The rectangles of a warm re-solve (pp2_path_pending.h), as a kernel argument.
constexpr int kPathSeedRects = 16;
struct PathSeedRects {
  int n;
  int x0[kPathSeedRects], y0[kPathSeedRects], w[kPathSeedRects], h[kPathSeedRects];
};

// map: the context's d_map (row stride g.width, 1 = occupied); D: the plane at
// (row 0, x 0), rows [-1, g.rows], row stride g.wp; A: [g.rows][g.wp].
// All launchers are asynchronous on `st`; unsharded geometries only.
// Cold start: D = +inf everywhere (halo rows and pads too), +0 at a goal that
// is on the grid and free; the tiles that see it (in their cells or their
// ring) start dirty, every other word cleared.
hipError_t launch_path_init(hipStream_t st, const Geom& g, const uint8_t* map, int gx, int gy,
                            float* D, int* words);
// Round `round` (0, 1, ...) of the relaxation, marking into marks[slot].
hipError_t launch_path_round(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                             int* words, int round, int slot);
// rec[kPathRecQuiet] = the first i < n with marks[i] == 0 (-1: none); the
// marks cleared for the next batch.
hipError_t launch_path_poll(hipStream_t st, int* words, int n, uint32_t* rec);
// A_path from the converged D; the finite cells counted into
// rec[kPathRecReached].
hipError_t launch_path_actions(hipStream_t st, const Geom& g, int gx, int gy, const float* D,
                               uint8_t* A, int* words, uint32_t* rec);

// Warm re-solve (DESIGN.md §2.3 "Warm re-solve"), from a converged (D, A) of
// an earlier map and `map` as it is now.
// Seed: every word cleared (enqueued ahead of the kernel); then one thread per
// cell of the rectangles (on the grid, `cells` in all): an occupied cell with
// finite D gets +inf and marks raise_dirty[0] of every tile that sees it; a
// free cell with D = +inf marks its tile in dirty[0].
hipError_t launch_path_seed(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                            int* words, const PathSeedRects& rects, long long cells);
// Round `round` of the raise: a finite cell whose parent by A reads +inf
// becomes +inf; marks into marks[slot], raise_dirty[(round + 1) & 1] and
// dirty[0].  A is the old field's and is only read.
hipError_t launch_path_raise_round(hipStream_t st, const Geom& g, const uint8_t* map, float* D,
                                   const uint8_t* A, int* words, int round, int slot);
// launch_path_actions, reporting the raised cells and the seeds as well.
hipError_t launch_path_resolve_actions(hipStream_t st, const Geom& g, int gx, int gy,
                                       const float* D, uint8_t* A, int* words, uint32_t* rec);

}  // namespace pp2
