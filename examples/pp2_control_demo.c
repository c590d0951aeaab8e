/*
 * pp2_control_demo.c -- control selection through the C ABI alone
 * (include/pp2.h "control"): create a context from an occupancy grid,
 * generate the model, solve the MDP, set a belief and ask both policies for
 * the next action -- the belief-mode lookup of the MDP node's beliefCallback
 * and the QMDP argmin of the belief-expected Q values.  Each answer is one
 * small record from the device; no plane is downloaded.  Plain C99, linked
 * against libpp2_hip.so.
 *
 *   ./pp2_control_demo      exit status 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pp2.h"

#define CHECK(call)                                                                \
  do {                                                                             \
    int s_ = (call);                                                               \
    if (s_ != PP2_OK) {                                                            \
      fprintf(stderr, "%s: %s: %s\n", #call, pp2_status_string(s_), pp2_last_error()); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(void) {
  const uint32_t H = 40, W = 60;
  uint8_t* map = (uint8_t*)calloc(H * W, 1);
  float* belief = (float*)calloc(H * W, sizeof(float));
  if (!map || !belief) return 1;
  /* a walled room with two pillars; the goal near the far corner */
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x)
      map[y * W + x] = (x == 0 || y == 0 || x == W - 1 || y == H - 1 ||
                        (x >= 20 && x < 23 && y >= 10 && y < 30) ||
                        (x >= 40 && x < 43 && y >= 5 && y < 25));
  /* a belief split between two free regions, the heavier one left of the
   * first pillar: 60 % over a 3x3 patch, 40 % over a 5x5 patch */
  for (uint32_t y = 19; y < 22; ++y)
    for (uint32_t x = 9; x < 12; ++x) belief[y * W + x] = 0.6f / 9.0f;
  for (uint32_t y = 28; y < 33; ++y)
    for (uint32_t x = 30; x < 35; ++x) belief[y * W + x] = 0.4f / 25.0f;

  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx* ctx = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, 55, 35, 0.95f));
  CHECK(pp2_model_generate(ctx));
  int sweeps = 0;
  double norm = 0.0;
  CHECK(pp2_mdp_solve(ctx, 0, &sweeps, &norm));
  CHECK(pp2_belief_set(ctx, belief));

  int32_t cell = -1, mode_cell = -1;
  float prob = 0.0f, q[9], mode_value = 0.0f, qmdp_value = 0.0f;
  uint8_t mode_action = 0, qmdp_action = 0;
  CHECK(pp2_belief_mode(ctx, &cell, &prob));
  CHECK(pp2_mdp_qvalues(ctx, q));
  CHECK(pp2_mdp_control(ctx, PP2_CONTROL_MODE, &mode_action, &mode_value, &mode_cell));
  CHECK(pp2_mdp_control(ctx, PP2_CONTROL_QMDP, &qmdp_action, &qmdp_value, NULL));
  if (mode_cell != cell || mode_action > 8 || qmdp_action > 8 || q[qmdp_action] != qmdp_value)
    return 3;

  printf("pp2_control_demo ok: MDP solved in %d sweeps; belief mode at (x %d, y %d) p %.4f\n",
         sweeps, (int)(cell % (int32_t)W), (int)(cell / (int32_t)W), prob);
  printf("  mode policy: action %u, J(mode) %.4f\n", mode_action, mode_value);
  printf("  QMDP policy: action %u, E_b[Q] %.4f; q =", qmdp_action, qmdp_value);
  for (int u = 0; u < 9; ++u) printf(" %.4f", q[u]);
  printf("\n");
  CHECK(pp2_destroy(ctx));
  free(map);
  free(belief);
  return 0;
}
