// pp2_episodes.cpp -- C ABI of the batched closed-loop policy episodes
// (include/pp2.h "episodes").  Kernels: pp2_episodes.hip.  A run enqueues the
// Q planes of the current J -- an alpha run the planes of the current FIB or
// PBVI alpha vectors instead, a lookahead run those and the reward planes --
// and one launch of the persistent episode kernel
// on the context's stream; results, traces and beliefs are copied back on demand.
// A batch created with pp2_episodes_create_placed may keep the belief planes in
// device memory instead of LDS (pp2_episodes.h "Placement"): such a launch is
// preceded by the kernel that pads the code plane and b0, and works in a
// scratch allocated at the first such launch.  Every policy follows the
// placement; the lookahead does so through pp2_episodes_run_lookahead_placed,
// while pp2_episodes_run_lookahead keeps its contract (LDS planes or PP2_EINVAL).
// pp2_episodes_set_world attaches a second context whose model the episodes
// are simulated in, and pp2_episodes_resume continues every episode from the
// batch's stored state: both launch the EXT instance of the run's policy and
// placement (pp2_episodes.hip), a run with neither the plain one.
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
  int policy = -1;             // of the last run (-1: none yet; 2: an alpha run; 3: a lookahead run)
  int alpha_set = -1;          // of the last run, if that was an alpha or a lookahead run
  int lds_bytes = 0, workgroups = 0;  // of the last launch (before any: MODE / QMDP's)
  int base_workgroups = 0;     // of a MODE / QMDP launch from LDS
  int placement = PP2_EPISODES_LDS;  // as requested at create
  int last_placement = -1;     // of the last launch (-1: none yet)
  // the global placement's scratch, from the first global launch on:
  // [scratch_wgs][2] planes of ep_plane_stride floats | padded b0 | padded code
  char* d_scratch = nullptr;
  long long scratch_bytes = 0;
  int scratch_wgs = 0;
  float* d_alpha = nullptr;    // [alpha_cap][H][wp], from the first alpha run on
  uint8_t* d_alpha_act = nullptr;  // [alpha_cap]
  int alpha_cap = 0, alpha_k = 0;  // vectors allocated, vectors of the last alpha run
  int32_t* d_trbest = nullptr;  // alpha traces, [horizon][E]
  float* d_trbsum = nullptr;
  float* d_rplanes = nullptr;  // [9][H][wp] reward planes, from the first lookahead run on
  float* d_larew = nullptr;    // lookahead traces: [horizon][E][9],
  float* d_lamax = nullptr;    // [horizon][E][9][16]
  int32_t* d_laidx = nullptr;
  unsigned acts_ok_version = 0;  // the context's pbvi_version whose actions were found <= 8
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
  // The world (pp2_episodes_set_world; null: the context's own model is the
  // world too) and what a resumed segment continues from besides d_steps,
  // d_status, d_cost, d_final and d_beliefs: the discounts.  An EXT launch
  // stores them; after a plain launch they are made from d_steps when a
  // resume needs them (disc_stale).  The events order a run against a world
  // on another stream, one in each direction; made at the first such run.
  pp2_ctx* world = nullptr;
  float* d_disc = nullptr;     // [E]
  bool disc_stale = false;
  hipEvent_t ev_world = nullptr, ev_run = nullptr;
  // The table a MODE step reads at the belief's mode
  // (pp2_episodes_set_action_table): the MDP's A or the context's A_path.
  int table = PP2_TABLE_MDP;
  std::vector<float> h_b0;     // upload staging (alive until the copies have run)
  std::vector<int32_t> h_start;
};

namespace {

// What a batch needs of its context, at create and again at every run (the
// model may have been replaced in between).
// must_fit: the LDS placement, whose MODE / QMDP layout has to fit.
int check_episode_ctx(pp2_ctx* c, const pp2_episodes* ep, long long* lds_bytes,
                      bool must_fit = true) {
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
  if (must_fit && bytes > (long long)pp2::kDictLdsMaxBytes)
    return set_err(PP2_EINVAL,
                   "a %d x %d belief needs %lld bytes of LDS per episode (at most %zu fit)",
                   c->g.width, c->g.rows, bytes, pp2::kDictLdsMaxBytes);
  if (lds_bytes) *lds_bytes = bytes;
  return PP2_OK;
}

// What a run demands of the attached world, before any launch: everything
// check_episode_ctx demands of the batch's own context but the LDS size (the
// world's tables are read from device memory).  Settles the world's pending
// resident launches first.
int check_episode_world(pp2_ctx* w, const pp2_episodes* ep) {
  CHECK(check_ctx(w));
  if (!w->model_ready)
    return set_err(PP2_ESTATE, "the world context has no model (not generated or uploaded)");
  if (w->nranks > 1 || w->group || w->g.rows != w->g.grows || w->g.halo != 1)
    return set_err(PP2_ESTATE, "the world context is sharded: episodes need an unsharded world");
  if (!coded_active(w) || !w->dict_sparse || !w->dict_rfact || !w->dict_tl_nonneg)
    return set_err(PP2_ESTATE,
                   "the world context needs an active dictionary-coded model with factored rows "
                   "(pp2_model_dict_info)");
  if (ep->H != w->g.rows || ep->W != w->g.width || ep->wp != w->g.wp)
    return set_err(PP2_ESTATE, "the world context's geometry is not the batch's");
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

constexpr int kPolicyAlpha = 2;      // launch_episodes' alpha-vector instance
constexpr int kPolicyLookahead = 3;  // ... and its one-step lookahead instance
// a lookahead workgroup's waves hold two to a SIMD (registers), so two
// workgroups to a CU
constexpr int kLookaheadPerCu = 2;

int check_ran_alpha(const pp2_episodes* ep, const char* fn) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (ep->policy != kPolicyAlpha)
    return set_err(PP2_ESTATE, "%s: the last run was not an alpha run", fn);
  return PP2_OK;
}

// pp2_episodes_get_alpha: the set of an alpha or a lookahead run
int check_ran_alpha_set(const pp2_episodes* ep, const char* fn) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (ep->policy != kPolicyAlpha && ep->policy != kPolicyLookahead)
    return set_err(PP2_ESTATE, "%s: the last run read no alpha set", fn);
  return PP2_OK;
}

// persistent workgroups: as many as the CUs hold at once, at most one per episode
int episode_workgroups(const pp2_ctx* c, int episodes, long long lds,
                       int max_per_cu = pp2::kEpMaxPerCu) {
  int per_cu = (int)((long long)pp2::kDictLdsMaxBytes / lds);
  per_cu = per_cu < 1 ? 1 : per_cu > max_per_cu ? max_per_cu : per_cu;
  const long long cap = (long long)(c->ncus > 0 ? c->ncus : 256) * per_cu;
  return (int)(episodes < cap ? episodes : cap);
}

// The global placement's scratch: bytes of the two planes of a workgroup, of
// the images every workgroup shares, and the workgroups of a launch =
// min(episodes, CUs x kEpGlobalPerCu, what kEpScratchCapBytes holds), at least 1.
struct ScratchPlan {
  long long stride, per_wg, shared, bytes;
  int workgroups;
};
ScratchPlan scratch_plan(const pp2_ctx* c, int episodes) {
  ScratchPlan p;
  p.stride = pp2::ep_plane_stride(c->g);
  p.per_wg = 2 * p.stride * (long long)sizeof(float);
  p.shared = p.stride * (long long)sizeof(float) +
             pp2::ep_code_elems(c->g) * (long long)sizeof(uint16_t);
  long long w = (long long)(c->ncus > 0 ? c->ncus : 256) * pp2::kEpGlobalPerCu;
  const long long fit = (pp2::kEpScratchCapBytes - p.shared) / p.per_wg;
  w = w < episodes ? w : episodes;
  w = w < fit ? w : fit;
  p.workgroups = (int)(w < 1 ? 1 : w);
  p.bytes = p.workgroups * p.per_wg + p.shared;
  return p;
}
// Workgroups of a global lookahead launch: the instance's registers admit
// kEpGlobalLookaheadPerCu per CU, and the launch uses the first plane pairs of
// the batch's scratch (scratch_wgs of them, sized for the other instances).
int global_lookahead_workgroups(const pp2_ctx* c, int episodes, int scratch_wgs) {
  long long w = (long long)(c->ncus > 0 ? c->ncus : 256) * pp2::kEpGlobalLookaheadPerCu;
  w = w < episodes ? w : episodes;
  w = w < scratch_wgs ? w : scratch_wgs;
  return (int)(w < 1 ? 1 : w);
}

// One run.  policy: PP2_CONTROL_MODE / PP2_CONTROL_QMDP, or kPolicyAlpha /
// kPolicyLookahead with alpha_set PP2_ALPHA_FIB / PP2_ALPHA_PBVI (all checked
// by the callers).  lds_only_lookahead: pp2_episodes_run_lookahead's contract,
// which refuses a lookahead launch that would not run from LDS planes;
// pp2_episodes_run_lookahead_placed follows the placement as every other run.
// resume: a resumed segment (pp2_episodes_resume; b0 and start_cells null) --
// every episode continues from what the batch stores.
int run_impl(pp2_episodes* ep, int policy, int alpha_set, uint64_t seed, const float* b0,
             const int32_t* start_cells, bool lds_only_lookahead = false, bool resume = false) {
  pp2_ctx* c = ep->ctx;
  pp2_ctx* w = ep->world;
  const bool ext = w != nullptr || resume;  // the EXT instances
  const bool look = policy == kPolicyLookahead;
  const bool alpha = policy == kPolicyAlpha || look;  // reads an alpha set
  // settles pending resident launches first: J and A below are the current ones
  long long lds = 0;
  CHECK(check_episode_ctx(c, ep, &lds, ep->placement == PP2_EPISODES_LDS));
  if (w && w != c) CHECK(check_episode_world(w, ep));
  const bool path_table = policy == PP2_CONTROL_MODE && ep->table == PP2_TABLE_PATH;
  if (path_table && !c->path_valid)
    return set_err(PP2_ESTATE, "the batch reads the shortest-path table and the context has no "
                   "valid field (pp2_path_solve; a map or goal update invalidates it)");
  const int H = ep->H, W = ep->W, wp = ep->wp, E = ep->episodes;
  const size_t hw = (size_t)H * W;
  // the alpha set: the context's current one
  int K = 0, ld = 0;
  const float* d_rows = nullptr;     // PBVI's flat rows
  const uint8_t* d_acts = nullptr;   // ... and their actions
  if (alpha) {
    if (alpha_set == PP2_ALPHA_FIB) {
      K = 9;
    } else {
      int Sp = 0;
      CHECK(pbvi_alphas(c, &d_rows, &K, &Sp, &ld));
      CHECK(pbvi_actions(c, &d_acts));
      if (K > pp2::kEpAlphaMax)
        return set_err(PP2_EINVAL, "%d alpha vectors (at most %d)", K, pp2::kEpAlphaMax);
    }
    lds = look ? pp2::episode_lookahead_lds_bytes(c->g, c->dict_n)
               : pp2::episode_alpha_lds_bytes(c->g, c->dict_n, K);
  }
  // where this launch's planes live: AUTO takes LDS if this launch's layout fits
  const bool fits = lds <= (long long)pp2::kDictLdsMaxBytes;
  const bool global = ep->placement == PP2_EPISODES_GLOBAL ||
                      (ep->placement == PP2_EPISODES_AUTO && !fits);
  if (lds_only_lookahead && ep->placement == PP2_EPISODES_GLOBAL)
    return set_err(PP2_EINVAL,
                   "pp2_episodes_run_lookahead runs from LDS planes only: the batch was created "
                   "with PP2_EPISODES_GLOBAL (pp2_episodes_run_lookahead_placed follows the "
                   "placement)");
  if (lds_only_lookahead && global)
    return set_err(PP2_EINVAL,
                   "pp2_episodes_run_lookahead runs from LDS planes only, and a %d x %d belief "
                   "with the lookahead scratch needs %lld bytes of LDS per episode (at most %zu "
                   "fit; pp2_episodes_run_lookahead_placed follows the placement)",
                   W, H, lds, pp2::kDictLdsMaxBytes);
  if (!global && !fits)  // (the LDS placement's alpha and lookahead layouts)
    return set_err(PP2_EINVAL,
                   "a %d x %d belief with the %s scratch needs %lld bytes of LDS per "
                   "episode (at most %zu fit)",
                   W, H, look ? "lookahead" : "alpha", lds, pp2::kDictLdsMaxBytes);
  ScratchPlan plan{};
  if (global) {
    lds = pp2::episode_global_lds_bytes(c->dict_n, look    ? pp2::ep_lookahead_floats()
                                                   : alpha ? pp2::ep_alpha_floats(K)
                                                           : 0);
    if (lds > (long long)pp2::kDictLdsMaxBytes)
      return set_err(PP2_EINVAL, "the tables of %d dictionary entries need %lld bytes of LDS",
                     c->dict_n, lds);
    plan = scratch_plan(c, ep->episodes);
  }
  for (size_t i = 0; !resume && i < hw; ++i) {
    uint32_t bits;
    std::memcpy(&bits, &b0[i], 4);
    if (bits >= 0x7f800000u)  // negative (-0 too), infinite or NaN
      return set_err(PP2_EINVAL, "b0[%zu] is not finite and >= +0", i);
  }
  for (int e = 0; !resume && e < E; ++e)
    if (start_cells[e] < 0 || (size_t)start_cells[e] >= hw)
      return set_err(PP2_EINVAL, "start_cells[%d] = %d outside [0, %zu)", e, start_cells[e], hw);
  DeviceGuard dg(c->device);
  // the staging vectors may still feed the previous run's copies
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t np = (size_t)H * wp, HE = (size_t)ep->horizon * E;
  if (global && !ep->d_scratch) {
    // the first global launch: planes zeroed once (halo rows and x pads stay
    // zero, the steps store interior quads only).  A failure leaves the batch
    // as it was.
    CHECK(dev_alloc(&ep->d_scratch, (size_t)plan.bytes, "episode planes"));
    if (hipMemsetAsync(ep->d_scratch, 0, (size_t)plan.bytes, c->stream) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(ep->d_scratch);
      ep->d_scratch = nullptr;
      return set_err(PP2_EHIP, "hipMemsetAsync episode planes");
    }
    ep->scratch_bytes = plan.bytes;
    ep->scratch_wgs = plan.workgroups;
  }
  if (alpha) {
    // a PBVI action the tables have no row for: before any launch.  Checked
    // once per version of the set (a copy to the host and a synchronise), not
    // once per run.
    if (d_acts && ep->acts_ok_version != c->pbvi_version) {
      std::vector<uint8_t> act((size_t)K);
      HIPCHK(hipMemcpyAsync(act.data(), d_acts, (size_t)K, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int k = 0; k < K; ++k)
        if (act[k] > 8)
          return set_err(PP2_EINVAL, "action %u of alpha vector %d out of range", act[k], k);
      ep->acts_ok_version = c->pbvi_version;
    }
    if (K > ep->alpha_cap) {  // (the stream is idle: nothing reads the old planes)
      if (ep->d_alpha) (void)hipFree(ep->d_alpha);
      if (ep->d_alpha_act) (void)hipFree(ep->d_alpha_act);
      ep->d_alpha = nullptr;
      ep->d_alpha_act = nullptr;
      ep->alpha_cap = ep->alpha_k = 0;
      CHECK(dev_alloc(&ep->d_alpha, (size_t)K * np, "alpha planes"));
      CHECK(dev_alloc(&ep->d_alpha_act, (size_t)K, "alpha actions"));
      ep->alpha_cap = K;
    }
    if (!look) {
      if (ep->trace && !ep->d_trbest) CHECK(dev_alloc(&ep->d_trbest, HE, "winner trace"));
      if (ep->trace && !ep->d_trbsum) CHECK(dev_alloc(&ep->d_trbsum, HE, "winning-sum trace"));
    } else {
      if (!ep->d_rplanes) CHECK(dev_alloc(&ep->d_rplanes, 9 * np, "reward planes"));
      if (ep->trace && !ep->d_larew) CHECK(dev_alloc(&ep->d_larew, HE * 9, "reward trace"));
      if (ep->trace && !ep->d_lamax) CHECK(dev_alloc(&ep->d_lamax, HE * 144, "leaf-maximum trace"));
      if (ep->trace && !ep->d_laidx) CHECK(dev_alloc(&ep->d_laidx, HE * 144, "leaf-index trace"));
    }
  }
  if (ext && !ep->d_disc) CHECK(dev_alloc(&ep->d_disc, (size_t)E, "discounts"));
  const bool cross = w && w->stream != c->stream;  // the world on a stream of its own
  if (cross && !ep->ev_world) {
    HIPCHK(hipEventCreateWithFlags(&ep->ev_world, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ep->ev_run, hipEventDisableTiming));
  }
  ep->lds_bytes = (int)lds;  // (a replaced model may have another dictionary size)
  ep->workgroups = global && look ? global_lookahead_workgroups(c, E, ep->scratch_wgs)
                   : global       ? ep->scratch_wgs
                   : look         ? episode_workgroups(c, E, lds, kLookaheadPerCu)
                   : alpha        ? episode_workgroups(c, E, lds)
                                  : ep->base_workgroups;
  if (!resume) {
    for (int y = 0; y < H; ++y)
      std::memcpy(&ep->h_b0[(size_t)y * wp], &b0[(size_t)y * W], (size_t)W * sizeof(float));
    std::memcpy(ep->h_start.data(), start_cells, (size_t)E * sizeof(int32_t));
    HIPCHK(hipMemcpyAsync(ep->d_b0, ep->h_b0.data(), np * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipMemcpyAsync(ep->d_start, ep->h_start.data(), (size_t)E * sizeof(int32_t),
                          hipMemcpyHostToDevice, c->stream));
  } else if (ep->disc_stale) {
    // the last launch was a plain one, which stores no discounts
    HIPCHK(pp2::launch_episode_discounts(c->stream, ep->d_steps, c->gamma, E, ep->d_disc));
    ep->disc_stale = false;
  }
  if (ep->trace) {
    // steps not taken: 255, 255, -1, 0, -1 (alpha runs: winner -1, its sum 0)
    HIPCHK(hipMemsetAsync(ep->d_tru, 0xff, HE, c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trz, 0xff, HE, c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trcell, 0xff, HE * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trmode, 0xff, HE * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(ep->d_trq, 0, HE * 9 * sizeof(float), c->stream));
    if (look) {
      HIPCHK(hipMemsetAsync(ep->d_larew, 0, HE * 9 * sizeof(float), c->stream));
      HIPCHK(hipMemsetAsync(ep->d_lamax, 0, HE * 144 * sizeof(float), c->stream));
      HIPCHK(hipMemsetAsync(ep->d_laidx, 0xff, HE * 144 * sizeof(int32_t), c->stream));
    } else if (alpha) {
      HIPCHK(hipMemsetAsync(ep->d_trbest, 0xff, HE * sizeof(int32_t), c->stream));
      HIPCHK(hipMemsetAsync(ep->d_trbsum, 0, HE * sizeof(float), c->stream));
    }
  }
  if (alpha) {
    // the snapshot of the set: planes and actions, stream-ordered
    const bool fib = alpha_set == PP2_ALPHA_FIB;
    HIPCHK(pp2::launch_episode_alpha_planes(c->stream, c->g, fib ? &c->fib[c->fcur].v : nullptr,
                                            d_rows, ld, K, ep->d_alpha, d_acts, ep->d_alpha_act));
    // ... and of the POMDP stage rewards, R_u[y][x] as nine planes
    if (look)
      HIPCHK(pp2::launch_episode_alpha_planes(c->stream, c->g, &c->R.v, nullptr, 0, 9,
                                              ep->d_rplanes, nullptr, nullptr));
  } else {
    HIPCHK(pp2::launch_episode_qplanes(c->stream, c->g, c->d_code, c->d_rows, c->dict_n,
                                       c->J[c->jcur].v.p, ep->d_q, c->ncus));
  }
  pp2::EpisodeRun a{};
  a.g = c->g;
  a.E = c->dict_n;
  a.code = c->d_code;
  a.rows = c->d_rows;
  a.rfact = c->d_rfact;
  a.Q = ep->d_q;
  a.A = path_table ? c->path_A : c->A;
  if (alpha) {
    a.alpha = ep->d_alpha;
    a.alpha_act = ep->d_alpha_act;
    a.K = K;
    a.rplanes = look ? ep->d_rplanes : nullptr;
  }
  a.b0 = ep->d_b0;
  a.start = ep->d_start;
  a.episodes = E;
  a.horizon = ep->horizon;
  a.seed = seed;
  a.gamma = c->gamma;
  a.goal = c->gy * W + c->gx;
  if (w) {
    // steps 2-4 and the goal tests are the world's; a goal off the grid is none
    a.w_code = w->d_code;
    a.w_rows = w->d_rows;
    a.w_rfact = w->d_rfact;
    a.goal = w->gx >= 0 && w->gx < W && w->gy >= 0 && w->gy < H ? w->gy * W + w->gx : -1;
  }
  a.resume = resume ? 1 : 0;
  a.disc = ext ? ep->d_disc : nullptr;
  a.steps = ep->d_steps;
  a.status = ep->d_status;
  a.cost = ep->d_cost;
  a.final_cell = ep->d_final;
  a.beliefs = ep->d_beliefs;
  if (ep->trace) {
    a.tr_u = ep->d_tru;
    a.tr_z = ep->d_trz;
    a.tr_cell = ep->d_trcell;
    // the nine sums: QMDP's S_u, a FIB run's V_k, a lookahead run's Q_u
    a.tr_q = policy == PP2_CONTROL_QMDP || look || (alpha && alpha_set == PP2_ALPHA_FIB)
                 ? ep->d_trq
                 : nullptr;
    a.tr_mode = ep->d_trmode;
    if (look) {
      a.tr_rew = ep->d_larew;
      a.tr_lmax = ep->d_lamax;
      a.tr_lidx = ep->d_laidx;
    } else if (alpha) {
      a.tr_best = ep->d_trbest;
      a.tr_bsum = ep->d_trbsum;
    }
  }
  if (global) {
    // the padded code plane and b0 image of this run (the model may have been
    // replaced since the last one), then the global instance
    const long long stride = pp2::ep_plane_stride(c->g);
    a.gplanes = reinterpret_cast<float*>(ep->d_scratch);
    a.gstride = stride;
    float* gb0 = a.gplanes + (long long)ep->scratch_wgs * 2 * stride;
    uint16_t* gcode = reinterpret_cast<uint16_t*>(gb0 + stride);
    a.gb0 = gb0;
    a.gcode = gcode;
    HIPCHK(pp2::launch_episode_pad(c->stream, c->g, c->d_code, ep->d_b0, gcode, gb0));
  }
  // the launch reads the world as it stands behind the work already enqueued
  // on the world's stream, and later work there waits for the launch
  if (cross) {
    HIPCHK(hipEventRecord(ep->ev_world, w->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, ep->ev_world, 0));
  }
  HIPCHK(pp2::launch_episodes(c->stream, a, policy, ep->workgroups, global, ext));
  if (cross) {
    HIPCHK(hipEventRecord(ep->ev_run, c->stream));
    HIPCHK(hipStreamWaitEvent(w->stream, ep->ev_run, 0));
  }
  ep->disc_stale = !ext;
  ep->last_placement = global ? PP2_EPISODES_GLOBAL : PP2_EPISODES_LDS;
  ep->policy = policy;
  ep->alpha_set = alpha ? alpha_set : -1;
  if (alpha) ep->alpha_k = K;
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
                  (void*)ep->d_trmode, (void*)ep->d_trq, (void*)ep->d_alpha,
                  (void*)ep->d_alpha_act, (void*)ep->d_trbest, (void*)ep->d_trbsum,
                  (void*)ep->d_rplanes, (void*)ep->d_larew, (void*)ep->d_lamax,
                  (void*)ep->d_laidx, (void*)ep->d_scratch, (void*)ep->d_disc})
    if (p) (void)hipFree(p);
  if (ep->ev_world) (void)hipEventDestroy(ep->ev_world);
  if (ep->ev_run) (void)hipEventDestroy(ep->ev_run);
  delete ep;
  return PP2_OK;
}

int pp2_episodes_create(pp2_episodes** out, pp2_ctx* c, int episodes, int horizon,
                        int record_trace) {
  return pp2_episodes_create_placed(out, c, episodes, horizon, record_trace, PP2_EPISODES_LDS);
}

int pp2_episodes_create_placed(pp2_episodes** out, pp2_ctx* c, int episodes, int horizon,
                               int record_trace, int placement) {
  if (!out) return set_err(PP2_EINVAL, "out is null");
  *out = nullptr;
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (episodes < 1 || episodes > 131072)
    return set_err(PP2_EINVAL, "episodes %d outside 1..131072", episodes);
  if (horizon < 1 || horizon > 4096)
    return set_err(PP2_EINVAL, "horizon %d outside 1..4096", horizon);
  if (placement != PP2_EPISODES_LDS && placement != PP2_EPISODES_GLOBAL &&
      placement != PP2_EPISODES_AUTO)
    return set_err(PP2_EINVAL, "unknown placement %d", placement);
  long long lds = 0;
  CHECK(check_episode_ctx(c, nullptr, &lds, placement == PP2_EPISODES_LDS));
  DeviceGuard dg(c->device);
  pp2_episodes* ep = new pp2_episodes();
  ep->ctx = c;
  ep->placement = placement;
  ep->episodes = episodes;
  ep->horizon = horizon;
  ep->trace = record_trace != 0;
  ep->H = c->g.rows;
  ep->W = c->g.width;
  ep->wp = c->g.wp;
  ep->base_workgroups = episode_workgroups(c, episodes, lds);
  if (placement == PP2_EPISODES_GLOBAL ||
      (placement == PP2_EPISODES_AUTO && lds > (long long)pp2::kDictLdsMaxBytes)) {
    // what a MODE / QMDP launch of this batch will take
    ep->lds_bytes = (int)pp2::episode_global_lds_bytes(c->dict_n, 0);
    ep->workgroups = scratch_plan(c, episodes).workgroups;
  } else {
    ep->lds_bytes = (int)lds;
    ep->workgroups = ep->base_workgroups;
  }
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
  return run_impl(ep, policy, -1, seed, b0, start_cells);
}

int pp2_episodes_run_alpha(pp2_episodes* ep, int alpha_set, uint64_t seed, const float* b0,
                           const int32_t* start_cells) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (!b0 || !start_cells) return set_err(PP2_EINVAL, "null argument");
  if (alpha_set != PP2_ALPHA_FIB && alpha_set != PP2_ALPHA_PBVI)
    return set_err(PP2_EINVAL, "unknown alpha set %d", alpha_set);
  return run_impl(ep, kPolicyAlpha, alpha_set, seed, b0, start_cells);
}

int pp2_episodes_run_lookahead(pp2_episodes* ep, int alpha_set, uint64_t seed, const float* b0,
                               const int32_t* start_cells) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (!b0 || !start_cells) return set_err(PP2_EINVAL, "null argument");
  if (alpha_set != PP2_ALPHA_FIB && alpha_set != PP2_ALPHA_PBVI)
    return set_err(PP2_EINVAL, "unknown alpha set %d", alpha_set);
  return run_impl(ep, kPolicyLookahead, alpha_set, seed, b0, start_cells, true);
}

int pp2_episodes_run_lookahead_placed(pp2_episodes* ep, int alpha_set, uint64_t seed,
                                      const float* b0, const int32_t* start_cells) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (!b0 || !start_cells) return set_err(PP2_EINVAL, "null argument");
  if (alpha_set != PP2_ALPHA_FIB && alpha_set != PP2_ALPHA_PBVI)
    return set_err(PP2_EINVAL, "unknown alpha set %d", alpha_set);
  return run_impl(ep, kPolicyLookahead, alpha_set, seed, b0, start_cells);
}

int pp2_episodes_set_world(pp2_episodes* ep, pp2_ctx* world) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (world) {
    pp2_ctx* c = ep->ctx;
    if (world->nranks > 1 || world->group || world->g.rows != world->g.grows ||
        world->g.halo != 1)
      return set_err(PP2_EINVAL, "the world context is sharded: episodes need an unsharded world");
    if (world->device != c->device)
      return set_err(PP2_EINVAL, "the world context is on device %d, the batch's on device %d",
                     world->device, c->device);
    if (world->g.rows != ep->H || world->g.width != ep->W || world->g.wp != ep->wp)
      return set_err(PP2_EINVAL, "the world is %d x %d, the batch %d x %d", world->g.width,
                     world->g.rows, ep->W, ep->H);
  }
  ep->world = world;
  return PP2_OK;
}

int pp2_episodes_set_action_table(pp2_episodes* ep, int table) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (table != PP2_TABLE_MDP && table != PP2_TABLE_PATH)
    return set_err(PP2_EINVAL, "unknown action table %d", table);
  ep->table = table;
  return PP2_OK;
}

int pp2_episodes_resume(pp2_episodes* ep, int policy, uint64_t seed) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (policy < PP2_EPISODE_MODE || policy > PP2_EPISODE_PBVI_LOOKAHEAD)
    return set_err(PP2_EINVAL, "unknown episode policy %d", policy);
  if (ep->policy < 0) return set_err(PP2_ESTATE, "pp2_episodes_resume before any run of the batch");
  switch (policy) {
    case PP2_EPISODE_MODE:
      return run_impl(ep, PP2_CONTROL_MODE, -1, seed, nullptr, nullptr, false, true);
    case PP2_EPISODE_QMDP:
      return run_impl(ep, PP2_CONTROL_QMDP, -1, seed, nullptr, nullptr, false, true);
    case PP2_EPISODE_FIB:
      return run_impl(ep, kPolicyAlpha, PP2_ALPHA_FIB, seed, nullptr, nullptr, false, true);
    case PP2_EPISODE_PBVI:
      return run_impl(ep, kPolicyAlpha, PP2_ALPHA_PBVI, seed, nullptr, nullptr, false, true);
    case PP2_EPISODE_FIB_LOOKAHEAD:
      return run_impl(ep, kPolicyLookahead, PP2_ALPHA_FIB, seed, nullptr, nullptr, false, true);
    default:
      return run_impl(ep, kPolicyLookahead, PP2_ALPHA_PBVI, seed, nullptr, nullptr, false, true);
  }
}

int pp2_episodes_trace_lookahead(pp2_episodes* ep, float* q, float* rewards, float* leaf_max,
                                 int32_t* leaf_index) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (ep->policy != kPolicyLookahead)
    return set_err(PP2_ESTATE, "pp2_episodes_trace_lookahead: the last run was not a lookahead run");
  if (!ep->trace)
    return set_err(PP2_ESTATE, "the batch was created without record_trace");
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t HE = (size_t)ep->horizon * ep->episodes;
  CHECK(fetch(c, q, ep->d_trq, HE * 9));
  CHECK(fetch(c, rewards, ep->d_larew, HE * 9));
  CHECK(fetch(c, leaf_max, ep->d_lamax, HE * 144));
  CHECK(fetch(c, leaf_index, ep->d_laidx, HE * 144));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_episodes_trace_alpha(pp2_episodes* ep, int32_t* best_index, float* best_sum) {
  CHECK(check_ran_alpha(ep, "pp2_episodes_trace_alpha"));
  if (!ep->trace)
    return set_err(PP2_ESTATE, "the batch was created without record_trace");
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  const size_t HE = (size_t)ep->horizon * ep->episodes;
  CHECK(fetch(c, best_index, ep->d_trbest, HE));
  CHECK(fetch(c, best_sum, ep->d_trbsum, HE));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PP2_OK;
}

int pp2_episodes_get_alpha(pp2_episodes* ep, int* count, float* alphas, uint8_t* actions) {
  CHECK(check_ran_alpha_set(ep, "pp2_episodes_get_alpha"));
  if (ep->alpha_k < 1) return set_err(PP2_ESTATE, "the alpha planes were released");
  pp2_ctx* c = ep->ctx;
  DeviceGuard dg(c->device);
  if (count) *count = ep->alpha_k;
  if (alphas)
    HIPCHK(hipMemcpy2DAsync(alphas, (size_t)ep->W * sizeof(float), ep->d_alpha,
                            (size_t)ep->wp * sizeof(float), (size_t)ep->W * sizeof(float),
                            (size_t)ep->alpha_k * ep->H, hipMemcpyDeviceToHost, c->stream));
  CHECK(fetch(c, actions, ep->d_alpha_act, (size_t)ep->alpha_k));
  HIPCHK(hipStreamSynchronize(c->stream));
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
  if (ep->policy == kPolicyAlpha || ep->policy == kPolicyLookahead)
    return set_err(PP2_ESTATE, "an alpha or a lookahead run builds no Q planes");
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

int pp2_episodes_placement(pp2_episodes* ep, int* requested, int* last, long long* scratch_bytes) {
  if (!ep) return set_err(PP2_EINVAL, "null episode batch");
  if (requested) *requested = ep->placement;
  if (last) *last = ep->last_placement;
  if (scratch_bytes) *scratch_bytes = ep->scratch_bytes;
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
