// pp2_control.cpp -- C ABI of the on-device control selection (include/pp2.h
// "control"): the belief's mode, the belief-expected Q values of the current
// MDP values, and the two policies built on them.  Kernels: pp2_control.hip.
// Every call enqueues on the context's stream and synchronises; the finalise
// kernel writes one kControlRec-word record into pinned host memory (as the
// resident kernels write their status words), so no plane leaves the device
// and no copy is queued behind the kernels.
#include <cstring>

#include "pp2_ctx.h"

using namespace pp2rt;

namespace {

struct ControlBufs {
  float* qpart;   // [blocks][9]
  float* pv;      // [blocks]
  int* pi;        // [blocks]
  uint32_t* rec;  // kControlRec words, pinned host memory
};

int control_bufs(pp2_ctx* c, ControlBufs* o) {
  const int nb = pp2::control_blocks(c->g);
  if (!c->ctl_host) {
    if (hipHostMalloc(&c->ctl_host, pp2::kControlRec * sizeof(uint32_t), hipHostMallocDefault) !=
        hipSuccess) {
      (void)hipGetLastError();
      c->ctl_host = nullptr;
      return set_err(PP2_ENOMEM, "hipHostMalloc control record");
    }
    std::memset(c->ctl_host, 0, pp2::kControlRec * sizeof(uint32_t));
  }
  if (!c->ctl_buf || c->ctl_blocks != nb) {
    if (c->ctl_buf) HIPCHK(hipFree(c->ctl_buf));
    c->ctl_buf = nullptr;
    const size_t words = (size_t)nb * 11;
    if (hipMalloc(&c->ctl_buf, words * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      return set_err(PP2_ENOMEM, "hipMalloc control partials (%zu B)", words * sizeof(float));
    }
    c->ctl_blocks = nb;
  }
  o->qpart = c->ctl_buf;
  o->pv = c->ctl_buf + (size_t)nb * 9;
  o->pi = reinterpret_cast<int*>(c->ctl_buf + (size_t)nb * 10);
  o->rec = c->ctl_host;
  return PP2_OK;
}

// Row shards and shard-group members hold a part of the belief only.
int check_unsharded(pp2_ctx* c, const char* fn) {
  if (c->nranks > 1 || c->group || c->g.rows != c->g.grows || c->g.halo != 1)
    return set_err(PP2_ESTATE, "%s runs on an unsharded context", fn);
  return PP2_OK;
}

int enqueue_q(pp2_ctx* c, const ControlBufs& B) {
  const float* J = c->J[c->jcur].v.p;
  const float* b = c->b[c->bcur].v.p;
  if (coded_active(c))
    HIPCHK(pp2::launch_control_q_coded(c->stream, c->g, c->d_code, c->d_rows, c->dict_n,
                                       c->dict_sparse, J, b, B.qpart, c->ncus));
  else
    HIPCHK(pp2::launch_control_q(c->stream, c->g, c->gamma, c->T.v, c->C.v, J, b, B.qpart,
                                 c->nt_streams));
  return PP2_OK;
}

int enqueue_mode(pp2_ctx* c, const ControlBufs& B) {
  HIPCHK(pp2::launch_belief_mode(c->stream, c->g, c->b[c->bcur].v.p, c->bsum + c->bcur, B.pv,
                                 B.pi));
  return PP2_OK;
}

// values / table: the planes read at the mode (null: the MDP's J and A)
int finish(pp2_ctx* c, const ControlBufs& B, bool q, bool mode, uint32_t (&rec)[pp2::kControlRec],
           const float* values = nullptr, const uint8_t* table = nullptr) {
  const int nb = c->ctl_blocks;
  HIPCHK(pp2::launch_control_finish(c->stream, c->g, B.qpart, q ? nb : 0, c->bsum + c->bcur,
                                    B.pv, B.pi, mode ? nb : 0,
                                    values ? values : c->J[c->jcur].v.p, table ? table : c->A,
                                    B.rec));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(rec, B.rec, sizeof rec);
  return PP2_OK;
}

float word_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, 4);
  return f;
}

}  // namespace

extern "C" {

int pp2_belief_mode(pp2_ctx* c, int32_t* cell, float* prob) {
  CHECK(check_ctx(c));
  CHECK(check_unsharded(c, "pp2_belief_mode"));
  DeviceGuard dg(c->device);
  ControlBufs B;
  CHECK(control_bufs(c, &B));
  CHECK(ensure_mass(c));
  CHECK(enqueue_mode(c, B));
  uint32_t rec[pp2::kControlRec];
  CHECK(finish(c, B, false, true, rec));
  if (cell) *cell = (int32_t)rec[pp2::kControlRecCell];
  if (prob) *prob = word_float(rec[pp2::kControlRecProb]);
  return PP2_OK;
}

int pp2_mdp_qvalues(pp2_ctx* c, float q[9]) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (!q) return set_err(PP2_EINVAL, "q is null");
  CHECK(check_model(c));
  CHECK(check_unsharded(c, "pp2_mdp_qvalues"));
  DeviceGuard dg(c->device);
  ControlBufs B;
  CHECK(control_bufs(c, &B));
  CHECK(ensure_mass(c));
  CHECK(enqueue_q(c, B));
  uint32_t rec[pp2::kControlRec];
  CHECK(finish(c, B, true, false, rec));
  std::memcpy(q, rec, 9 * sizeof(float));
  return PP2_OK;
}

int pp2_mdp_control(pp2_ctx* c, int policy, uint8_t* action, float* value, int32_t* cell) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (!action) return set_err(PP2_EINVAL, "action is null");
  if (policy != PP2_CONTROL_MODE && policy != PP2_CONTROL_QMDP)
    return set_err(PP2_EINVAL, "unknown control policy %d", policy);
  CHECK(check_model(c));
  CHECK(check_unsharded(c, "pp2_mdp_control"));
  DeviceGuard dg(c->device);
  ControlBufs B;
  CHECK(control_bufs(c, &B));
  CHECK(ensure_mass(c));
  const bool qmdp = policy == PP2_CONTROL_QMDP;
  CHECK(qmdp ? enqueue_q(c, B) : enqueue_mode(c, B));
  uint32_t rec[pp2::kControlRec];
  CHECK(finish(c, B, qmdp, !qmdp, rec));
  if (qmdp) {
    *action = (uint8_t)rec[pp2::kControlRecAction];
    if (value) *value = word_float(rec[pp2::kControlRecValue]);
    if (cell) *cell = -1;
  } else {
    *action = (uint8_t)rec[pp2::kControlRecModeAction];
    if (value) *value = word_float(rec[pp2::kControlRecModeValue]);
    if (cell) *cell = (int32_t)rec[pp2::kControlRecCell];
  }
  return PP2_OK;
}

// The A* node's beliefCallback over the shortest-path field (pp2_path.cpp):
// the mode and finish kernels with D and A_path in place of J and A.
int pp2_path_control(pp2_ctx* c, uint8_t* action, float* dist, int32_t* cell) {
  if (!c) return set_err(PP2_EINVAL, "null context");
  if (!action) return set_err(PP2_EINVAL, "action is null");
  CHECK(check_ctx(c));
  CHECK(check_unsharded(c, "pp2_path_control"));
  if (!c->path_valid)
    return set_err(PP2_ESTATE, "pp2_path_control: no valid shortest-path field (pp2_path_solve; "
                   "a map or goal update invalidates it)");
  DeviceGuard dg(c->device);
  ControlBufs B;
  CHECK(control_bufs(c, &B));
  CHECK(ensure_mass(c));
  CHECK(enqueue_mode(c, B));
  uint32_t rec[pp2::kControlRec];
  CHECK(finish(c, B, false, true, rec, c->path_D.v.p, c->path_A));
  *action = (uint8_t)rec[pp2::kControlRecModeAction];
  if (dist) *dist = word_float(rec[pp2::kControlRecModeValue]);
  if (cell) *cell = (int32_t)rec[pp2::kControlRecCell];
  return PP2_OK;
}

}  // extern "C"
