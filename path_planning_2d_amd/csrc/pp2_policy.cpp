// pp2_policy.cpp -- C ABI of the policy evaluator (include/pp2.h "policy
// evaluation"): the exact expected discounted cost, goal
// probability and expected steps of a robot that knows its cell and follows a
// fixed action table in a given world, for every start cell at once.
// Kernels: pp2_policy.hip.  An evaluation is enqueued whole on the context's
// stream -- the start planes, then one launch per step (PLANES) or per `block`
// steps (TILES) -- and waits for nothing; pp2_policy_get synchronises.
#include <cstring>

#include "pp2_ctx.h"
#include "pp2_policy.h"

using namespace pp2rt;

namespace {

constexpr int kMaxHorizon = 65536;

bool sharded(const pp2_ctx* c) {
  return c->nranks > 1 || c->group || c->comm || c->g.rows != c->g.grows || c->g.halo != 1;
}

// Every T row of the world's dictionary sums to at most 1 + 2^-20
// (pp2_dict_props.h: dict_rows_bounded; generated models: each row is a
// probability distribution).
bool rows_bounded(const pp2_ctx* w) {
  if (w->model_generated) return true;
  if (w->h_dict.size() != (size_t)w->dict_n * pp2::kDictRow) return false;
  return pp2::dict_rows_bounded(w->h_dict.data(), w->dict_n, pp2::kDictRow);
}

// the TILES route's demands on the world: the episodes' (check_episode_world)
bool tiles_ok(const pp2_ctx* w) {
  return coded_active(w) && w->dict_sparse && w->dict_rfact && w->dict_tl_nonneg &&
         rows_bounded(w);
}

void policy_release(pp2_ctx* c) {
  if (c->pol_planes) (void)hipFree(c->pol_planes);
  if (c->pol_cls) (void)hipFree(c->pol_cls);
  c->pol_planes = nullptr;
  c->pol_cls = nullptr;
}

// all or nothing: a failure leaves the context as it was
int policy_buffers(pp2_ctx* c) {
  if (c->pol_planes) return PP2_OK;
  const size_t n = owned_cells(c);
  if (hipMalloc(&c->pol_planes, 6 * n * sizeof(float)) != hipSuccess ||
      hipMalloc(&c->pol_cls, n) != hipSuccess) {
    (void)hipGetLastError();
    policy_release(c);
    return set_err(PP2_ENOMEM, "allocating the policy evaluator's planes (%zu B)",
                   6 * n * sizeof(float) + n);
  }
  return PP2_OK;
}

pp2::PolicyPlanes side(const pp2_ctx* c, int s) {
  const size_t n = owned_cells(c);
  float* p = c->pol_planes + (size_t)s * 3 * n;
  return pp2::PolicyPlanes{p, p + n, p + 2 * n};
}

}  // namespace

namespace pp2rt {
bool policy_sharded(const pp2_ctx* c) { return sharded(c); }
bool policy_tiles_ok(const pp2_ctx* w) { return tiles_ok(w); }

void policy_free(pp2_ctx* c) {
  policy_release(c);
  if (c->pol_user) (void)hipFree(c->pol_user);
  if (c->pol_ev_world) (void)hipEventDestroy(c->pol_ev_world);
  if (c->pol_ev_run) (void)hipEventDestroy(c->pol_ev_run);
  c->pol_user = nullptr;
  c->pol_ev_world = c->pol_ev_run = nullptr;
}
}  // namespace pp2rt

extern "C" {

int pp2_policy_set_table(pp2_ctx* c, const uint8_t* table) {
  CHECK(check_ctx(c));
  if (sharded(c)) return set_err(PP2_ESTATE, "pp2_policy_set_table runs on an unsharded context");
  if (!table) {
    c->pol_user_set = false;
    return PP2_OK;
  }
  const size_t n = owned_cells(c);
  for (size_t i = 0; i < n; ++i)
    if (table[i] > 8)
      return set_err(PP2_EINVAL, "table[%zu] = %d is no action (0 .. 8)", i, (int)table[i]);
  DeviceGuard dg(c->device);
  if (!c->pol_user && hipMalloc(&c->pol_user, n) != hipSuccess) {
    (void)hipGetLastError();
    c->pol_user = nullptr;
    return set_err(PP2_ENOMEM, "allocating the user table (%zu B)", n);
  }
  c->pol_user_set = false;
  HIPCHK(hipMemcpyAsync(c->pol_user, table, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->pol_user_set = true;
  return PP2_OK;
}

int pp2_policy_evaluate(pp2_ctx* c, pp2_ctx* world, int table, int horizon, int route,
                        int block) {
  // settles pending resident launches first: A below is the current one
  CHECK(check_model(c));
  if (sharded(c)) return set_err(PP2_ESTATE, "pp2_policy_evaluate runs on an unsharded context");
  pp2_ctx* w = world ? world : c;
  if (w != c) {
    CHECK(check_ctx(w));
    if (sharded(w))
      return set_err(PP2_ESTATE, "the world context is sharded: the evaluator needs an unsharded world");
    if (!w->model_ready)
      return set_err(PP2_ESTATE, "the world context has no model (not generated or uploaded)");
    if (w->device != c->device)
      return set_err(PP2_EINVAL, "the world context is on device %d, the table's on device %d",
                     w->device, c->device);
    if (w->g.rows != c->g.rows || w->g.width != c->g.width || w->g.wp != c->g.wp)
      return set_err(PP2_EINVAL, "the world is %d x %d, the table %d x %d", w->g.width, w->g.rows,
                     c->g.width, c->g.rows);
    if (std::memcmp(&w->gamma, &c->gamma, sizeof(float)) != 0)
      return set_err(PP2_EINVAL, "the world's gamma (%.9g) is not the context's (%.9g)",
                     (double)w->gamma, (double)c->gamma);
  }
  if (table != PP2_TABLE_MDP && table != PP2_TABLE_PATH && table != PP2_TABLE_USER)
    return set_err(PP2_EINVAL, "unknown action table %d", table);
  if (horizon < 1 || horizon > kMaxHorizon)
    return set_err(PP2_EINVAL, "horizon = %d outside [1, %d]", horizon, kMaxHorizon);
  if (route != PP2_POLICY_AUTO && route != PP2_POLICY_PLANES && route != PP2_POLICY_TILES)
    return set_err(PP2_EINVAL, "unknown route %d", route);
  if (block < 0 || block > pp2::kPolicyMaxBlock)
    return set_err(PP2_EINVAL, "block = %d outside [0, %d]", block, pp2::kPolicyMaxBlock);
  const uint8_t* pi = c->A;
  int pis = c->g.wp;
  if (table == PP2_TABLE_PATH) {
    if (!c->path_valid)
      return set_err(PP2_ESTATE, "no valid shortest-path field (pp2_path_solve; a map or goal "
                     "update invalidates it)");
    pi = c->path_A;
  } else if (table == PP2_TABLE_USER) {
    if (!c->pol_user_set)
      return set_err(PP2_ESTATE, "no user table (pp2_policy_set_table)");
    pi = c->pol_user;
    pis = c->g.width;
  }
  const bool tiles = route == PP2_POLICY_TILES || (route == PP2_POLICY_AUTO && tiles_ok(w));
  if (tiles && !tiles_ok(w))
    return set_err(PP2_ESTATE, "PP2_POLICY_TILES needs the world's dictionary-coded model active "
                   "with factored rows (pp2_model_dict_info) and T rows that sum to at most 1");
  DeviceGuard dg(c->device);
  CHECK(policy_buffers(c));
  const bool cross = w->stream != c->stream;  // the world on a stream of its own
  if (cross && !c->pol_ev_world) {
    HIPCHK(hipEventCreateWithFlags(&c->pol_ev_world, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->pol_ev_run, hipEventDisableTiming));
  }
  c->pol_valid = false;
  // the launches read the world as it stands behind the work already enqueued
  // on the world's stream, and later work there waits for them
  if (cross) {
    HIPCHK(hipEventRecord(c->pol_ev_world, w->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->pol_ev_world, 0));
  }
  const int B = tiles ? (block ? block : pp2::kPolicyDefaultBlock) : 1;
  int launches = 1, cur = 0;
  HIPCHK(pp2::launch_policy_init(c->stream, c->g, w->gx, w->gy, side(c, 0)));
  if (tiles) {
    HIPCHK(pp2::launch_policy_classes(c->stream, c->g, w->d_code, w->d_rows, pi, pis, w->gx, w->gy,
                                      c->pol_cls));
    ++launches;
  }
  for (int done = 0; done < horizon; done += B) {
    const int steps = horizon - done < B ? horizon - done : B;
    if (tiles)
      HIPCHK(pp2::launch_policy_tiles(c->stream, c->g, w->d_rows, w->d_rfact, c->pol_cls, B, steps,
                                      side(c, cur), side(c, cur ^ 1)));
    else
      HIPCHK(pp2::launch_policy_step(c->stream, c->g, w->gamma, w->T.v, w->C.v, pi, pis, w->gx,
                                     w->gy, side(c, cur), side(c, cur ^ 1)));
    cur ^= 1;
    ++launches;
  }
  if (cross) {
    HIPCHK(hipEventRecord(c->pol_ev_run, c->stream));
    HIPCHK(hipStreamWaitEvent(w->stream, c->pol_ev_run, 0));
  }
  c->pol_side = cur;
  c->pol_table = table;
  c->pol_horizon = horizon;
  c->pol_route = tiles ? PP2_POLICY_TILES : PP2_POLICY_PLANES;
  c->pol_block = B;
  c->pol_launches = launches;
  c->pol_valid = true;
  return PP2_OK;
}

int pp2_policy_get(pp2_ctx* c, float* G, float* P, float* N) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (!c->pol_valid) return set_err(PP2_ESTATE, "pp2_policy_get: no evaluation (pp2_policy_evaluate)");
  DeviceGuard dg(c->device);
  const size_t bytes = owned_cells(c) * sizeof(float);
  const pp2::PolicyPlanes r = side(c, c->pol_side);
  if (G) HIPCHK(hipMemcpyAsync(G, r.G, bytes, hipMemcpyDeviceToHost, c->stream));
  if (P) HIPCHK(hipMemcpyAsync(P, r.P, bytes, hipMemcpyDeviceToHost, c->stream));
  if (N) HIPCHK(hipMemcpyAsync(N, r.N, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_policy_info(pp2_ctx* c, int* valid, int* table, int* horizon, int* route_taken, int* block,
                    int* launches, int* tile_rows, int* tile_cols, int* default_block,
                    int* max_block) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (valid) *valid = c->pol_valid ? 1 : 0;
  if (table) *table = c->pol_table;
  if (horizon) *horizon = c->pol_horizon;
  if (route_taken) *route_taken = c->pol_route;
  if (block) *block = c->pol_block;
  if (launches) *launches = c->pol_launches;
  if (tile_rows) *tile_rows = pp2::kPolicyTileRows;
  if (tile_cols) *tile_cols = pp2::kPolicyTileCols;
  if (default_block) *default_block = pp2::kPolicyDefaultBlock;
  if (max_block) *max_block = pp2::kPolicyMaxBlock;
  return PP2_OK;
}

}  // extern "C"
