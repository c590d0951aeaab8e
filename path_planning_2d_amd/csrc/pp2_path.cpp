// pp2_path.cpp -- C ABI of the shortest-path field (include/pp2.h
// "shortest-path field"): the A* baseline's action for every
// cell at once, from the map and goal the context holds.  Kernels:
// pp2_path.hip.  A solve enqueues its rounds in batches on the context's
// stream; each batch ends in a poll kernel that writes one pinned word, read
// after one synchronise (as pp2_control.cpp reads its record), so the host
// waits once per batch and not once per round.  Rounds enqueued behind the
// one that settled the field find no dirty tile and return at once.
// pp2_path_resolve repairs a converged field after map updates instead of
// starting over: a seed pass over the changed rectangles, raise rounds, then
// the same relaxation rounds (DESIGN.md §2.3 "Warm re-solve").
// pp2_path_control is in pp2_control.cpp, beside the kernels it reuses.
#include <cmath>
#include <cstring>

#include "pp2_ctx.h"
#include "pp2_path.h"

using namespace pp2rt;

namespace {

// batches: 8 rounds, doubling to kPathBatchMax (a small grid settles inside
// the first; a long corridor pays one poll per 256 launches)
constexpr int kFirstBatch = 8;
static_assert(pp2::kPathSeedRects == pp2::kPathPendingCap, "the seed kernel takes the whole list");

int check_path_ctx(pp2_ctx* c, const char* fn) {
  if (c->nranks > 1 || c->group || c->comm || c->g.rows != c->g.grows || c->g.halo != 1)
    return set_err(PP2_ESTATE, "%s runs on an unsharded context", fn);
  return PP2_OK;
}

int check_valid(pp2_ctx* c, const char* fn) {
  CHECK(check_ctx(c));
  CHECK(check_path_ctx(c, fn));
  if (!c->path_valid)
    return set_err(PP2_ESTATE, "%s: no valid shortest-path field (pp2_path_solve; a map or goal "
                   "update invalidates it)", fn);
  return PP2_OK;
}

void path_release(pp2_ctx* c) {
  free_planes(&c->path_D);
  if (c->path_A) (void)hipFree(c->path_A);
  if (c->path_words) (void)hipFree(c->path_words);
  if (c->path_host) (void)hipHostFree(c->path_host);
  c->path_A = nullptr;
  c->path_words = nullptr;
  c->path_host = nullptr;
}

// all or nothing: a failure leaves the context as it was
int path_buffers(pp2_ctx* c) {
  if (c->path_host) return PP2_OK;
  const long long rs = c->g.wp;
  Planes& P = c->path_D;
  P.K = 1;
  P.floats = (size_t)(2 * kGuard) + (size_t)(c->g.rows + 2) * rs;
  const size_t abytes = (size_t)c->g.rows * c->g.wp;
  if (hipMalloc(&P.alloc, P.floats * sizeof(float)) != hipSuccess ||
      hipMalloc(&c->path_A, abytes) != hipSuccess ||
      hipMalloc(&c->path_words, pp2::path_words(c->g) * sizeof(int)) != hipSuccess ||
      hipHostMalloc(&c->path_host, pp2::kPathRec * sizeof(uint32_t), hipHostMallocDefault) !=
          hipSuccess) {
    (void)hipGetLastError();
    path_release(c);
    return set_err(PP2_ENOMEM, "allocating the shortest-path planes (%zu B)",
                   P.floats * sizeof(float) + abytes);
  }
  std::memset(c->path_host, 0, pp2::kPathRec * sizeof(uint32_t));
  P.v.p = P.alloc + kGuard + rs;  // skip the top halo row
  P.v.rs = rs;
  P.v.ps = c->g.wp;
  // the guards and the pads of A_path are never read; defined all the same
  HIPCHK(hipMemsetAsync(P.alloc, 0, P.floats * sizeof(float), c->stream));
  HIPCHK(hipMemsetAsync(c->path_A, 4, abytes, c->stream));
  return PP2_OK;
}

int cache_field(pp2_ctx* c) {
  if (c->path_cached) return PP2_OK;
  const size_t n = owned_cells(c);
  c->h_path_D.resize(n);
  c->h_path_A.resize(n);
  CHECK(download_planes(c, c->path_D, c->h_path_D.data(), nullptr));
  CHECK(ensure_staging(c, n));
  HIPCHK(pp2::launch_pack_u8(c->stream, c->g, c->path_A, (uint8_t*)c->staging));
  HIPCHK(hipMemcpyAsync(c->h_path_A.data(), c->staging, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->path_cached = true;
  return PP2_OK;
}

int check_solvable(pp2_ctx* c, const char* fn, int max_rounds) {
  CHECK(check_ctx(c));
  CHECK(check_path_ctx(c, fn));
  if (max_rounds < 1) return set_err(PP2_EINVAL, "max_rounds = %d (at least 1)", max_rounds);
  if ((long long)c->g.rows * c->g.width > (1ll << 23))
    return set_err(PP2_EINVAL, "a %d x %d grid has more than 2^23 cells: its distances could "
                   "leave the range in which every fp32 add of a move cost is strict",
                   c->g.width, c->g.rows);
  return PP2_OK;
}

// the goal cell is on the grid and free in the map in force
bool goal_free(const pp2_ctx* c) {
  return c->gx >= 0 && c->gx < c->g.width && c->gy >= 0 && c->gy < c->g.rows &&
         c->h_map[(size_t)c->gy * c->g.width + c->gx] != 1;
}

// A solve or resolve begins: no field until it converges, and whatever was
// pending is its to follow.
void begin_solve(pp2_ctx* c) {
  c->path_valid = c->path_field = c->path_cached = false;
  c->path_pending.clear(goal_free(c));
  c->path_rounds = c->path_launches = c->path_polls = 0;
  c->path_warm = c->path_raised = c->path_raise_rounds = c->path_relax_rounds = 0;
  c->path_seed_cells = 0;
}

void end_solve(pp2_ctx* c, int reached) {
  c->path_reached = reached;
  c->path_valid = c->path_field = true;
}

// Rounds 0, 1, ... of one phase (the relaxation or the raise), enqueued in
// batches that each end in a poll, until a round marks nobody or max_rounds
// are done.  launch(round, slot) enqueues one round marking into marks[slot].
template <class Launch>
int run_rounds(pp2_ctx* c, int max_rounds, int* rounds, bool* settled, Launch launch) {
  int done = 0, batch = kFirstBatch;
  *settled = false;
  while (!*settled && done < max_rounds) {
    const int n = batch < max_rounds - done ? batch : max_rounds - done;
    for (int i = 0; i < n; ++i) HIPCHK(launch(done + i, i));
    HIPCHK(pp2::launch_path_poll(c->stream, c->path_words, n, c->path_host));
    c->path_launches += n + 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    ++c->path_polls;
    const int quiet = (int)c->path_host[pp2::kPathRecQuiet];
    if (quiet >= 0 && quiet < n) {
      *settled = true;
      done += quiet + 1;
    } else {
      done += n;
    }
    batch = batch * 2 < pp2::kPathBatchMax ? batch * 2 : pp2::kPathBatchMax;
  }
  *rounds = done;
  return PP2_OK;
}

// pp2_path_solve, and pp2_path_resolve where it cannot run warm
int solve_cold(pp2_ctx* c, int max_rounds, int* rounds, int* converged, int* reached) {
  CHECK(path_buffers(c));
  begin_solve(c);
  float* D = c->path_D.v.p;
  HIPCHK(pp2::launch_path_init(c->stream, c->g, c->d_map, c->gx, c->gy, D, c->path_words));
  ++c->path_launches;
  int done = 0;
  bool settled = false;
  CHECK(run_rounds(c, max_rounds, &done, &settled, [&](int round, int slot) {
    return pp2::launch_path_round(c->stream, c->g, c->d_map, D, c->path_words, round, slot);
  }));
  c->path_rounds = done;
  int cells = 0;
  if (settled) {
    HIPCHK(pp2::launch_path_actions(c->stream, c->g, c->gx, c->gy, D, c->path_A, c->path_words,
                                    c->path_host));
    c->path_launches += 2;
    HIPCHK(hipStreamSynchronize(c->stream));
    ++c->path_polls;
    cells = (int)c->path_host[pp2::kPathRecReached];
    end_solve(c, cells);
  }
  if (rounds) *rounds = done;
  if (converged) *converged = settled ? 1 : 0;
  if (reached) *reached = cells;
  return PP2_OK;
}

}  // namespace

namespace pp2rt {
void path_free(pp2_ctx* c) { path_release(c); }
}  // namespace pp2rt

extern "C" {

int pp2_path_solve(pp2_ctx* c, int max_rounds, int* rounds, int* converged, int* reached) {
  CHECK(check_solvable(c, "pp2_path_solve", max_rounds));
  DeviceGuard dg(c->device);
  return solve_cold(c, max_rounds, rounds, converged, reached);
}

int pp2_path_resolve(pp2_ctx* c, int max_rounds, int* rounds, int* converged, int* reached,
                     int* warm) {
  CHECK(check_solvable(c, "pp2_path_resolve", max_rounds));
  DeviceGuard dg(c->device);
  if (c->path_valid) {  // nothing changed since the field: no launch
    c->path_warm = 1;
    c->path_raised = c->path_raise_rounds = c->path_relax_rounds = c->path_seed_cells = 0;
    if (rounds) *rounds = 0;
    if (converged) *converged = 1;
    if (reached) *reached = c->path_reached;
    if (warm) *warm = 1;
    return PP2_OK;
  }
  if (!c->path_field || !c->path_pending.warm_ok(goal_free(c))) {
    int r = 0;
    CHECK(solve_cold(c, max_rounds, &r, converged, reached));
    c->path_relax_rounds = r;
    if (rounds) *rounds = r;
    if (warm) *warm = 0;
    return PP2_OK;
  }
  const pp2::PathPending pend = c->path_pending;
  begin_solve(c);
  c->path_warm = 1;
  float* D = c->path_D.v.p;
  pp2::PathSeedRects R;
  std::memset(&R, 0, sizeof R);
  R.n = pend.n;
  for (int i = 0; i < pend.n; ++i) {
    R.x0[i] = pend.r[i].x0;
    R.y0[i] = pend.r[i].y0;
    R.w[i] = pend.r[i].w;
    R.h[i] = pend.r[i].h;
  }
  c->path_seed_cells = (int)pend.cells();
  HIPCHK(pp2::launch_path_seed(c->stream, c->g, c->d_map, D, c->path_words, R, pend.cells()));
  ++c->path_launches;
  bool settled = true;
  int raise = 0, relax = 0;
  // no cell went from free to occupied: nothing to raise (a freed-only update
  // costs seed + relax + actions)
  if (pend.any_raised())
    CHECK(run_rounds(c, max_rounds, &raise, &settled, [&](int round, int slot) {
      return pp2::launch_path_raise_round(c->stream, c->g, c->d_map, D, c->path_A, c->path_words,
                                          round, slot);
    }));
  // the relaxation starts once the raise is quiet: a stale value still
  // standing would be copied into a raised neighbour
  if (settled)
    CHECK(run_rounds(c, max_rounds, &relax, &settled, [&](int round, int slot) {
      return pp2::launch_path_round(c->stream, c->g, c->d_map, D, c->path_words, round, slot);
    }));
  int cells = 0;
  if (settled) {
    HIPCHK(pp2::launch_path_resolve_actions(c->stream, c->g, c->gx, c->gy, D, c->path_A,
                                            c->path_words, c->path_host));
    c->path_launches += 2;
    HIPCHK(hipStreamSynchronize(c->stream));
    ++c->path_polls;
    cells = (int)c->path_host[pp2::kPathRecReached];
    c->path_raised = (int)c->path_host[pp2::kPathRecRaised];
    if (c->path_host[pp2::kPathRecSeeds] == 0) raise = 0;  // no finite cell became occupied
    end_solve(c, cells);
  }
  c->path_rounds = raise + relax;
  c->path_raise_rounds = raise;
  c->path_relax_rounds = relax;
  if (rounds) *rounds = raise + relax;
  if (converged) *converged = settled ? 1 : 0;
  if (reached) *reached = cells;
  if (warm) *warm = 1;
  return PP2_OK;
}

int pp2_path_resolve_info(pp2_ctx* c, int* warm, int* raised, int* raise_rounds,
                          int* relax_rounds, int* seed_cells) {
  CHECK(check_ctx(c));
  if (warm) *warm = c->path_warm;
  if (raised) *raised = c->path_raised;
  if (raise_rounds) *raise_rounds = c->path_raise_rounds;
  if (relax_rounds) *relax_rounds = c->path_relax_rounds;
  if (seed_cells) *seed_cells = c->path_seed_cells;
  return PP2_OK;
}

int pp2_path_get(pp2_ctx* c, float* D, uint8_t* A) {
  CHECK(check_valid(c, "pp2_path_get"));
  DeviceGuard dg(c->device);
  CHECK(cache_field(c));
  if (D) std::memcpy(D, c->h_path_D.data(), c->h_path_D.size() * sizeof(float));
  if (A) std::memcpy(A, c->h_path_A.data(), c->h_path_A.size());
  return PP2_OK;
}

int pp2_path_trace(pp2_ctx* c, int32_t start_cell, int32_t* cells, int cap, int* n,
                   float* length) {
  CHECK(check_valid(c, "pp2_path_trace"));
  if (!n) return set_err(PP2_EINVAL, "n is null");
  const int H = c->g.rows, W = c->g.width;
  if (start_cell < 0 || start_cell >= H * W)
    return set_err(PP2_EINVAL, "start_cell = %d outside [0, %d)", start_cell, H * W);
  if (cap < 0 || (cap > 0 && !cells)) return set_err(PP2_EINVAL, "cells is null or cap < 0");
  DeviceGuard dg(c->device);
  CHECK(cache_field(c));
  const float d0 = c->h_path_D[(size_t)start_cell];
  if (length) *length = d0;
  *n = 0;
  if (!(d0 < HUGE_VALF)) return PP2_OK;  // occupied or unreachable: no path
  // D falls strictly along A_path, so the walk ends at the goal (the one
  // finite cell with action 4) within H * W cells
  int count = 0;
  int32_t cell = start_cell;
  for (;;) {
    if (count < cap) cells[count] = cell;
    ++count;
    const int u = c->h_path_A[(size_t)cell];
    if (u == 4 || count > H * W) break;
    cell += (u / 3 - 1) * W + (u % 3 - 1);
  }
  *n = count;
  if (count > cap)
    return set_err(PP2_EINVAL, "the path has %d cells, cells holds %d", count, cap);
  return PP2_OK;
}

int pp2_path_info(pp2_ctx* c, int* valid, int* rounds, int* launches, int* polls, int* tile_rows,
                  int* tile_cols) {
  CHECK(check_ctx(c));
  if (valid) *valid = c->path_valid ? 1 : 0;
  if (rounds) *rounds = c->path_rounds;
  if (launches) *launches = c->path_launches;
  if (polls) *polls = c->path_polls;
  if (tile_rows) *tile_rows = pp2::kPathTileRows;
  if (tile_cols) *tile_cols = pp2::kPathTileCols;
  return PP2_OK;
}

}  // extern "C"
