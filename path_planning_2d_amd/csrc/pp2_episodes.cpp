// pp2_episodes.cpp -- C ABI of the batched closed-loop policy episodes
// (include/pp2.h "episodes").  Kernels: pp2_episodes.hip.  A run enqueues the
// Q planes of the current J and one launch of the persistent episode kernel on
// the context's stream; results, traces and beliefs are copied back on demand.
#include <cstring>
#include <vector>

#include "pp2_ctx.h"
#include "pp2_episodes.h"

using namespace pp2rt;

struct pp2_episodes {
  pp2_ctx* ctx = nullptr;
  int episodes = 0, horizon = 0;
  bool trace = false;
  int H = 0, W = 0, wp = 0;    // the geometry the buffers were sized for
  int policy = -1;             // of the last run (-1: none yet)
  int lds_bytes = 0, workgroups = 0;
  float* d_q = nullptr;        // [9][H][wp]
  float* d_b0 = nullptr;       // [H][wp]
  int32_t* d_start = nullptr;  // [E]
  int32_t* d_steps = nullptr;
  int32_t* d_final = nullptr;
  float* d_cost = nullptr;
  uint8_t* d_status = nullptr;
  float* d_beliefs = nullptr;  // [E][H][wp]
  uint8_t* d_tru = nullptr;    // traces, [horizon][E]
  uint8_t* d_trz = nullptr;
  int32_t* d_trcell = nullptr;
  int32_t* d_trmode = nullptr;
  float* d_trq = nullptr;      // [horizon][E][9]
  std::vector<float> h_b0;     // upload staging (alive until the copies have run)
  std::vector<int32_t> h_start;
};

namespace {

// What a batch needs of its context, at create and again at every run (the
// model may have been replaced in between).
int check_episode_ctx(pp2_ctx* c, const pp2_episodes* ep, long long* lds_bytes) {
  CHECK(check_model(c));
  if (c->nranks > 1 || c->group || c->g.rows != c->g.grows || c->g.halo != 1)
    return set_err(PP2_ESTATE, "episodes run on an unsharded context");
  if (!coded_active(c) || !c->dict_sparse || !c->dict_rfact || !c->dict_tl_nonneg)
    return set_err(PP2_ESTATE,
                   "episodes need an active dictionary-coded model with factored rows "
                   "(pp2_model_dict_info)");
  if (ep && (ep->H != c->g.rows || ep->W != c->g.width || ep->wp != c->g.wp))
    return set_err(PP2_ESTATE, "the context's geometry changed since pp2_episodes_create");
  const long long bytes = pp2::episode_lds_bytes(c->g, c->dict_n);
  if (bytes > (long long)pp2::kDictLdsMaxBytes)
    return set_err(PP2_EINVAL,
                   "a %d x %d belief needs %lld bytes of LDS per episode (at most %zu fit)",
                   c->g.width, c->g.rows, bytes, pp2::kDictLdsMaxBytes);
  if (lds_bytes) *lds_bytes = bytes;
  return PP2_OK;
}

template <typename T>
int dev_alloc(T** p, size_t n, const char* what) {
  if (hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_err(PP2_ENOMEM, "hipMalloc %s (%zu B)", what, n * sizeof(T));
  }
  return PP2_OK;
}

int check_ran(const pp2_episodes* ep, const char* fn) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (ep->policy < 0) return set_err(PP2_ESTATE, "%s before pp2_episodes_run", fn);
  return PP2_OK;
}

template <typename T>
int fetch(pp2_ctx* c, T* dst, const T* src, size_t n) {
  if (dst) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return PP2_OK;
}

}  // namespace

extern "C" {

int pp2_episodes_destroy(pp2_episodes* ep) {
  if (!ep) return PP2_OK;
  DeviceGuard dg(ep->ctx->device);
  (void)hipStreamSynchronize(ep->ctx->stream);
  for (void* p : {(void*)ep->d_q, (void*)ep->d_b0, (void*)ep->d_start, (void*)ep->d_steps,
                  (void*)ep->d_final, (void*)ep->d_cost, (void*)ep->d_status,
                  (void*)ep->d_beliefs, (void*)ep->d_tru, (void*)ep->d_trz, (void*)ep->d_trcell,
                  (void*)ep->d_trmode, (void*)ep->d_trq})
    if (p) (void)hipFree(p);
  delete ep;
  return PP2_OK;
}

int pp2_episodes_create(pp2_episodes** out, pp2_ctx* c, int episodes, int horizon,
                        int record_trace) {
  if (!out) return set_err(PP2_EINVAL, "out is null");
  *out = nullptr;
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (episodes < 1 || episodes > 131072)
    return set_err(PP2_EINVAL, "episodes %d outside 1..131072", episodes);
  if (horizon < 1 || horizon > 4096)
    return set_err(PP2_EINVAL, "horizon %d outside 1..4096", horizon);
  long long lds = 0;
  CHECK(check_episode_ctx(c, nullptr, &lds));
  DeviceGuard dg(c->device);
  pp2_episodes* ep = new pp2_episodes();
  ep->ctx = c;
  ep->episodes = episodes;
  ep->horizon = horizon;
  ep->trace = record_trace != 0;
  ep->H = c->g.rows;
  ep->W = c->g.width;
  ep->wp = c->g.wp;
  ep->lds_bytes = (int)lds;
  // persistent workgroups: as many as the CUs hold at once, at most one per episode
  int per_cu = (int)((long long)pp2::kDictLdsMaxBytes / lds);
  per_cu = per_cu < 1 ? 1 : per_cu > pp2::kEpMaxPerCu ? pp2::kEpMaxPerCu : per_cu;
  const long long cap = (long long)(c->ncus > 0 ? c->ncus : 256) * per_cu;
  ep->workgroups = (int)(episodes < cap ? episodes : cap);
  const size_t np = (size_t)ep->H * ep->wp, E = (size_t)episodes, HE = (size_t)horizon * E;
  auto fail = [&](int s) {
    pp2_episodes_destroy(ep);
    return s;
  };
  int s = PP2_OK;
  if ((s = dev_alloc(&ep->d_q, 9 * np, "Q planes")) != PP2_OK ||
      (s = dev_alloc(&ep->d_b0, np, "root belief")) != PP2_OK ||
      (s = dev_alloc(&ep->d_start, E, "start cells")) != PP2_OK ||
      (s = dev_alloc(&ep->d_steps, E, "steps")) != PP2_OK ||
      (s = dev_alloc(&ep->d_final, E, "final cells")) != PP2_OK ||
      (s = dev_alloc(&ep->d_cost, E, "costs")) != PP2_OK ||
      (s = dev_alloc(&ep->d_status, E, "status")) != PP2_OK ||
      (s = dev_alloc(&ep->d_beliefs, E * np, "episode beliefs")) != PP2_OK)
    return fail(s);
  if (ep->trace &&
      ((s = dev_alloc(&ep->d_tru, HE, "action trace")) != PP2_OK ||
       (s = dev_alloc(&ep->d_trz, HE, "observation trace")) != PP2_OK ||
       (s = dev_alloc(&ep->d_trcell, HE, "cell trace")) != PP2_OK ||
       (s = dev_alloc(&ep->d_trmode, HE, "mode-cell trace")) != PP2_OK ||
       (s = dev_alloc(&ep->d_trq, HE * 9, "Q-sum trace")) != PP2_OK))
    return fail(s);
  ep->h_b0.assign(np, 0.0f);
  ep->h_start.assign(E, 0);
  *out = ep;
  return PP2_OK;
}

int pp2_episodes_run(pp2_episodes* ep, int policy, uint64_t seed, const float* b0,
                     const int32_t* start_cells) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (!b0 || !start_cells) return set_err(PP2_EINVAL, "null argument");
  if (policy != PP2_CONTROL_MODE && policy != PP2_CONTROL_QMDP)
    return set_err(PP2_EINVAL, "unknown control policy %d", policy);
  pp2_ctx* c = ep->ctx;
  // settles pending resident launches first: J and A below are the current ones
  long long lds = 0;
  CHECK(check_episode_ctx(c, ep, &lds));
  ep->lds_bytes = (int)lds;  // (a replaced model may have another dictionary size)
  const int H = ep->H, W = ep->W, wp = ep->wp, E = ep->episodes;
  const size_t hw = (size_t)H * W;
  for (size_t i = 0; i < hw; ++i) {
    uint32_t bits;
    std::memcpy(&bits, &b0[i], 4);
    if (bits >= 0x7f800000u)  // negative (-0 too), infinite or NaN
      return set_err(PP2_EINVAL, "b0[%zu] is not finite and >= +0", i);
  }
  for (int e = 0; e < E; ++e)
    if (start_cells[e] < 0 || (size_t)start_cells[e] >= hw)
      return set_err(PP2_EINVAL, "start_cells[%d] = %d outside [0, %zu)", e, start_cells[e], hw);
  DeviceGuard dg(c->device);
  // the staging vectors may still feed the previous run's copies
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int y = 0; y < H; ++y)
    std::memcpy(&ep->h_b0[(size_t)y * wp], &b0[(size_t)y * W], (size_t)W * sizeof(float));
  std::memcpy(ep->h_start.data(), start_cells, (size_t)E * sizeof(int32_t));
  const size_t np = (size_t)H * wp, HE = (size_t)ep->horizon * E;
  HIPCHK(hipMemcpyAsync(ep->d_b0, ep->h_b0.data(), np * sizeof(float), hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipMemcpyAsync(ep->d_start, ep->h_start.data(), (size_t)E * sizeof(int32_t),
                        hipMemcpyHostToDevice, c->stream));
  if (ep->trace) {
    // steps not taken: 255, 255, -1, 0, -1
    HIPCHK(hipMemsetAsync(ep->d_tru, 0xff, HE, c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trz, 0xff, HE, c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trcell, 0xff, HE * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trmode, 0xff, HE * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trq, 0, HE * 9 * sizeof(float), c->stream));
  }
  HIPCHK(pp2::launch_episode_qplanes(c->stream, c->g, c->d_code, c->d_rows, c->dict_n,
                                     c->J[c->jcur].v.p, ep->d_q, c->ncus));
  pp2::EpisodeRun a{};
  a.g = c->g;
  a.E = c->dict_n;
  a.code = c->d_code;
  a.rows = c->d_rows;
  a.rfact = c->d_rfact;
  a.Q = ep->d_q;
  a.A = c->A;
  a.b0 = ep->d_b0;
  a.start = ep->d_start;
  a.episodes = E;
  a.horizon = ep->horizon;
  a.seed = seed;
  a.gamma = c->gamma;
  a.goal = c->gy * W + c->gx;
  a.steps = ep->d_steps;
  a.status = ep->d_status;
  a.cost = ep->d_cost;
  a.final_cell = ep->d_final;
  a.beliefs = ep->d_beliefs;
  if (ep->trace) {
    a.tr_u = ep->d_tru;
    a.tr_z = ep->d_trz;
    a.tr_cell = ep->d_trcell;
    a.tr_q = policy == PP2_CONTROL_QMDP ? ep->d_trq : nullptr;
    a.tr_mode = ep->d_trmode;
  }
  HIPCHK(pp2::launch_episodes(c->stream, a, policy, ep->workgroups));
  ep->policy = policy;
  return PP2_OK;
}

int pp2_episodes_results(pp2_episodes* ep, int32_t* steps, uint8_t* status, float* cost,
                         int32_t* final_cell) {
  CHECK(check_ran(ep, "pp2_episodes_results"));
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t E = (size_t)ep->episodes;
  CHECK(fetch(c, steps, ep->d_steps, E));
  CHECK(fetch(c, status, ep->d_status, E));
  CHECK(fetch(c, cost, ep->d_cost, E));
  CHECK(fetch(c, final_cell, ep->d_final, E));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_episodes_trace(pp2_episodes* ep, uint8_t* actions, uint8_t* observations, int32_t* cells,
                       float* qsums, int32_t* mode_cells) {
  CHECK(check_ran(ep, "pp2_episodes_trace"));
  if (!ep->trace)
    return set_err(PP2_ESTATE, "the batch was created without record_trace");
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t HE = (size_t)ep->horizon * ep->episodes;
  CHECK(fetch(c, actions, ep->d_tru, HE));
  CHECK(fetch(c, observations, ep->d_trz, HE));
  CHECK(fetch(c, cells, ep->d_trcell, HE));
  CHECK(fetch(c, qsums, ep->d_trq, HE * 9));
  CHECK(fetch(c, mode_cells, ep->d_trmode, HE));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_episodes_get_belief(pp2_episodes* ep, int episode, float* belief) {
  CHECK(check_ran(ep, "pp2_episodes_get_belief"));
  if (!belief) return set_err(PP2_EINVAL, "belief is null");
  if (episode < 0 || episode >= ep->episodes)
    return set_err(PP2_EINVAL, "episode %d outside [0, %d)", episode, ep->episodes);
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t np = (size_t)ep->H * ep->wp;
  HIPCHK(hipMemcpy2DAsync(belief, (size_t)ep->W * sizeof(float), ep->d_beliefs + episode * np,
                          (size_t)ep->wp * sizeof(float), (size_t)ep->W * sizeof(float), ep->H,
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_episodes_get_q(pp2_episodes* ep, float* Q) {
  CHECK(check_ran(ep, "pp2_episodes_get_q"));
  if (!Q) return set_err(PP2_EINVAL, "Q is null");
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t np = (size_t)ep->H * ep->wp;
  std::vector<float> planes(9 * np);
  HIPCHK(hipMemcpyAsync(planes.data(), ep->d_q, planes.size() * sizeof(float),
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int y = 0; y < ep->H; ++y)
    for (int x = 0; x < ep->W; ++x)
      for (int u = 0; u < 9; ++u)
        Q[((size_t)y * ep->W + x) * 9 + u] = planes[u * np + (size_t)y * ep->wp + x];
  return PP2_OK;
}

int pp2_episodes_info(pp2_episodes* ep, int* lds_bytes, int* workgroups, int* threads) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (lds_bytes) *lds_bytes = ep->lds_bytes;
  if (workgroups) *workgroups = ep->workgroups;
  if (threads) *threads = pp2::kEpThreads;
  return PP2_OK;
}

}  // extern "C"
