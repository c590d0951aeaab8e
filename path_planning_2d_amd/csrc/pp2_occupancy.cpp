// pp2_occupancy.cpp -- C ABI of the forward occupancy (include/pp2.h
// "occupancy"): where a robot that knows its cell and follows
// a fixed action table is after `horizon` steps from a start distribution (D),
// how often it has passed through every cell before arriving (V), and the
// mass at the goal after each step (curve).  The adjoint of the policy
// evaluator (pp2_policy.cpp), with the same inputs, checks and stream order.
// Kernels: pp2_occupancy.hip.  An evaluation is enqueued whole on the
// context's stream -- b0 and the start planes, the weight planes (PLANES) or
// class bytes (TILES), then one launch per step (PLANES) or per `block` steps
// (TILES) -- and waits for nothing; pp2_occupancy_get synchronises.
#include <cfloat>
#include <cstring>

#include "pp2_ctx.h"
#include "pp2_occupancy.h"

using namespace pp2rt;

namespace {

constexpr int kMaxHorizon = 65536;

void occ_release(pp2_ctx* c) {
  for (void* p : {(void*)c->occ_planes, (void*)c->occ_wts, (void*)c->occ_cls, (void*)c->occ_b0,
                  (void*)c->occ_curve})
    if (p) (void)hipFree(p);
  c->occ_planes = c->occ_wts = c->occ_b0 = c->occ_curve = nullptr;
  c->occ_cls = nullptr;
  if (c->occ_h_b0) (void)hipHostFree(c->occ_h_b0);
  if (c->occ_ev_b0) (void)hipEventDestroy(c->occ_ev_b0);
  c->occ_h_b0 = nullptr;
  c->occ_ev_b0 = nullptr;
}

// all or nothing per buffer set: a failure leaves the context as it was
int occ_buffers(pp2_ctx* c, bool tiles) {
  const size_t n = owned_cells(c);
  if (!c->occ_planes) {
    float *planes = nullptr, *b0 = nullptr, *curve = nullptr, *h_b0 = nullptr;
    hipEvent_t ev = nullptr;
    if (hipMalloc(&planes, 4 * n * sizeof(float)) != hipSuccess ||
        hipMalloc(&b0, n * sizeof(float)) != hipSuccess ||
        hipMalloc(&curve, (size_t)(kMaxHorizon + 1) * sizeof(float)) != hipSuccess ||
        hipHostMalloc(&h_b0, n * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      for (float* p : {planes, b0, curve})
        if (p) (void)hipFree(p);
      if (h_b0) (void)hipHostFree(h_b0);
      return set_err(PP2_ENOMEM, "allocating the occupancy planes (%zu B)",
                     (5 * n + kMaxHorizon + 1) * sizeof(float));
    }
    c->occ_planes = planes;
    c->occ_b0 = b0;
    c->occ_curve = curve;
    c->occ_h_b0 = h_b0;
    c->occ_ev_b0 = ev;
  }
  if (tiles && !c->occ_cls && hipMalloc(&c->occ_cls, n) != hipSuccess) {
    (void)hipGetLastError();
    c->occ_cls = nullptr;
    return set_err(PP2_ENOMEM, "allocating the occupancy class bytes (%zu B)", n);
  }
  if (!tiles && !c->occ_wts && hipMalloc(&c->occ_wts, 9 * n * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    c->occ_wts = nullptr;
    return set_err(PP2_ENOMEM, "allocating the occupancy weight planes (%zu B)",
                   9 * n * sizeof(float));
  }
  return PP2_OK;
}

pp2::OccPlanes side(const pp2_ctx* c, int s) {
  const size_t n = owned_cells(c);
  float* p = c->occ_planes + (size_t)s * 2 * n;
  return pp2::OccPlanes{p, p + n};
}

}  // namespace

namespace pp2rt {
void occupancy_free(pp2_ctx* c) {
  occ_release(c);
  if (c->occ_ev_world) (void)hipEventDestroy(c->occ_ev_world);
  if (c->occ_ev_run) (void)hipEventDestroy(c->occ_ev_run);
  c->occ_ev_world = c->occ_ev_run = nullptr;
}
}  // namespace pp2rt

extern "C" {

int pp2_occupancy_evaluate(pp2_ctx* c, pp2_ctx* world, int table, const float* b0, int horizon,
                           int route, int block) {
  // settles pending resident launches first: A below is the current one
  CHECK(check_model(c));
  if (policy_sharded(c))
    return set_err(PP2_ESTATE, "pp2_occupancy_evaluate runs on an unsharded context");
  pp2_ctx* w = world ? world : c;
  if (w != c) {
    CHECK(check_ctx(w));
    if (policy_sharded(w))
      return set_err(PP2_ESTATE, "the world context is sharded: the occupancy needs an unsharded world");
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
  if (!b0) return set_err(PP2_EINVAL, "null start distribution");
  if (horizon < 1 || horizon > kMaxHorizon)
    return set_err(PP2_EINVAL, "horizon = %d outside [1, %d]", horizon, kMaxHorizon);
  if (route != PP2_OCC_AUTO && route != PP2_OCC_PLANES && route != PP2_OCC_TILES)
    return set_err(PP2_EINVAL, "unknown route %d", route);
  if (block < 0 || block > pp2::kOccMaxBlock)
    return set_err(PP2_EINVAL, "block = %d outside [0, %d]", block, pp2::kOccMaxBlock);
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
  const bool admitted = policy_tiles_ok(w);
  const bool tiles = route == PP2_OCC_TILES || (route == PP2_OCC_AUTO && admitted);
  if (tiles && !admitted)
    return set_err(PP2_ESTATE, "PP2_OCC_TILES needs the world's dictionary-coded model active "
                   "with factored rows (pp2_model_dict_info) and T rows that sum to at most 1");
  DeviceGuard dg(c->device);
  CHECK(occ_buffers(c, tiles));
  const bool cross = w->stream != c->stream;  // the world on a stream of its own
  if (cross && !c->occ_ev_world) {
    HIPCHK(hipEventCreateWithFlags(&c->occ_ev_world, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->occ_ev_run, hipEventDisableTiming));
  }
  // b0 as the definition reads it, checked and copied in one pass: -0 and
  // subnormals are +0.  The pinned staging copy is reused once the previous
  // evaluation's upload has run; a refusal leaves the result as it was.
  const size_t n = owned_cells(c);
  HIPCHK(hipEventSynchronize(c->occ_ev_b0));
  for (size_t i = 0; i < n; ++i) {
    const float e = b0[i];
    if (!(e >= 0.0f && e <= 1.0f))  // a NaN fails both
      return set_err(PP2_EINVAL, "b0[%zu] = %g is not in [0, 1]", i, (double)e);
    c->occ_h_b0[i] = e < FLT_MIN ? 0.0f : e;
  }
  c->occ_valid = false;
  HIPCHK(hipMemcpyAsync(c->occ_b0, c->occ_h_b0, n * sizeof(float), hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipEventRecord(c->occ_ev_b0, c->stream));
  HIPCHK(hipMemsetAsync(c->occ_curve, 0, (size_t)(horizon + 1) * sizeof(float), c->stream));
  // the launches read the world as it stands behind the work already enqueued
  // on the world's stream, and later work there waits for them
  if (cross) {
    HIPCHK(hipEventRecord(c->occ_ev_world, w->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->occ_ev_world, 0));
  }
  const int B = tiles ? (block ? block : pp2::kOccDefaultBlock) : 1;
  // kernels: the start planes, the class bytes or the weight planes, the steps
  int launches = 2, cur = 0;
  HIPCHK(pp2::launch_occ_init(c->stream, c->g, w->gx, w->gy, c->occ_b0, side(c, 0), c->occ_curve));
  if (tiles)
    HIPCHK(pp2::launch_policy_classes(c->stream, c->g, w->d_code, w->d_rows, pi, pis, w->gx, w->gy,
                                      c->occ_cls));
  else
    HIPCHK(pp2::launch_occ_weights(c->stream, c->g, w->T.v, pi, pis, w->gx, w->gy, c->occ_wts));
  for (int done = 0; done < horizon; done += B) {
    const int steps = horizon - done < B ? horizon - done : B;
    if (tiles)
      HIPCHK(pp2::launch_occ_tiles(c->stream, c->g, w->d_rfact, c->occ_cls, B, steps, done,
                                   side(c, cur), side(c, cur ^ 1), c->occ_curve));
    else
      HIPCHK(pp2::launch_occ_step(c->stream, c->g, c->occ_wts, w->gx, w->gy, done + 1, side(c, cur),
                                  side(c, cur ^ 1), c->occ_curve));
    cur ^= 1;
    ++launches;
  }
  if (cross) {
    HIPCHK(hipEventRecord(c->occ_ev_run, c->stream));
    HIPCHK(hipStreamWaitEvent(w->stream, c->occ_ev_run, 0));
  }
  c->occ_side = cur;
  c->occ_table = table;
  c->occ_horizon = horizon;
  c->occ_route = tiles ? PP2_OCC_TILES : PP2_OCC_PLANES;
  c->occ_block = B;
  c->occ_launches = launches;
  c->occ_valid = true;
  return PP2_OK;
}

int pp2_occupancy_get(pp2_ctx* c, float* D, float* V, float* curve) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (!c->occ_valid)
    return set_err(PP2_ESTATE, "pp2_occupancy_get: no evaluation (pp2_occupancy_evaluate)");
  DeviceGuard dg(c->device);
  const size_t bytes = owned_cells(c) * sizeof(float);
  const pp2::OccPlanes r = side(c, c->occ_side);
  if (D) HIPCHK(hipMemcpyAsync(D, r.D, bytes, hipMemcpyDeviceToHost, c->stream));
  if (V) HIPCHK(hipMemcpyAsync(V, r.V, bytes, hipMemcpyDeviceToHost, c->stream));
  if (curve)
    HIPCHK(hipMemcpyAsync(curve, c->occ_curve, (size_t)(c->occ_horizon + 1) * sizeof(float),
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_occupancy_info(pp2_ctx* c, int* valid, int* table, int* horizon, int* route_taken,
                       int* block, int* launches, int* tile_rows, int* tile_cols,
                       int* default_block, int* max_block) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (valid) *valid = c->occ_valid ? 1 : 0;
  if (table) *table = c->occ_table;
  if (horizon) *horizon = c->occ_horizon;
  if (route_taken) *route_taken = c->occ_route;
  if (block) *block = c->occ_block;
  if (launches) *launches = c->occ_launches;
  if (tile_rows) *tile_rows = pp2::kOccTileRows;
  if (tile_cols) *tile_cols = pp2::kOccTileCols;
  if (default_block) *default_block = pp2::kOccDefaultBlock;
  if (max_block) *max_block = pp2::kOccMaxBlock;
  return PP2_OK;
}

}  // extern "C"
