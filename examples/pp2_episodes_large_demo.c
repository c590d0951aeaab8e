/*
 * pp2_episodes_large_demo.c -- evaluating control policies on a map whose
 * belief does not fit the LDS of a workgroup, through the C ABI alone
 * (include/pp2.h "episodes", "Placement"): build a 256 x 256 map in the
 * program, solve its MDP and sweep its FIB alphas, then run one batch created
 * with PP2_EPISODES_AUTO -- which keeps the belief planes of such a grid in
 * device memory -- under the belief-mode policy, the QMDP policy and the
 * FIB-greedy policy: the same robots, seed and cost scale, each in one launch.
 * Then the one-step lookahead over the FIB alphas, the reference POMDP node's
 * policy, on the first LOOK_EPISODES of the same robots (its step costs 144
 * dots per alpha vector, so the batch is smaller):
 * pp2_episodes_run_lookahead_placed follows the placement to device memory.
 * Prints success rate, mean steps to the goal and mean discounted cost.
 * pp2_episodes_create refuses this grid (PP2_EINVAL); that is shown first.
 * Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_episodes_large_demo          exit status 0 on success
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

enum { H = 256, W = 256, EPISODES = 1024, HORIZON = 96, FIB_SWEEPS = 30, GX = 200, GY = 180 };
enum { LOOK_EPISODES = 512 };

/* one row of the table: the first n episodes' results */
static int report(const char* name, int n, const int32_t* steps, const uint8_t* status,
                  const float* cost) {
  int reached = 0, lost = 0;
  double sum_steps = 0.0, sum_cost = 0.0;
  for (int e = 0; e < n; ++e) {
    if (status[e] > 2 || steps[e] < 0 || steps[e] > HORIZON) return 3;
    if (status[e] == 1) { ++reached; sum_steps += steps[e]; }
    lost += status[e] == 2;
    sum_cost += cost[e];
  }
  printf("  %s policy: success rate %.3f, mean steps to the goal %.1f, mean discounted cost "
         "%.3f, beliefs lost %d\n", name, (double)reached / n,
         reached ? sum_steps / reached : 0.0, sum_cost / n, lost);
  return 0;
}

/* a small linear congruential generator: the map is the program's own */
static uint32_t lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 8;
}

int main(void) {
  static uint8_t map[H * W], status[EPISODES];
  static float b0[H * W], cost[EPISODES];
  static int32_t start[EPISODES], steps[EPISODES];
  /* 15 % occupied cells, the goal and its neighbours free */
  uint32_t seed = 2024u;
  int nfree = 0;
  for (int i = 0; i < H * W; ++i) map[i] = lcg(&seed) % 100u < 15u;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) map[(GY + dy) * W + GX + dx] = 0;
  for (int i = 0; i < H * W; ++i) nfree += map[i] == 0;
  /* uniform belief over the free cells; start cells within 40 cells of the goal */
  for (int i = 0; i < H * W; ++i) b0[i] = map[i] ? 0.0f : 1.0f / (float)nfree;
  for (int e = 0; e < EPISODES; ++e) {
    int x, y;
    do {
      x = GX - 40 + (int)(lcg(&seed) % 81u);
      y = GY - 40 + (int)(lcg(&seed) % 81u);
    } while (x < 0 || x >= W || y < 0 || y >= H || map[y * W + x]);
    start[e] = y * W + x;
  }

  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx* ctx = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, GX, GY, 0.95f));
  CHECK(pp2_model_generate(ctx));
  int sweeps = 0;
  double norm = 0.0;
  CHECK(pp2_mdp_solve(ctx, 0, &sweeps, &norm));
  CHECK(pp2_fib_sweep(ctx, FIB_SWEEPS));
  pp2_episodes* ep = NULL;
  /* the LDS placement does not hold a 256 x 256 belief ... */
  if (pp2_episodes_create(&ep, ctx, EPISODES, HORIZON, 0) != PP2_EINVAL || ep != NULL) {
    fprintf(stderr, "pp2_episodes_create was expected to refuse a %d x %d grid\n", W, H);
    return 3;
  }
  printf("pp2_episodes_large_demo: pp2_episodes_create: %s\n", pp2_last_error());
  /* ... the automatic one moves it to device memory */
  CHECK(pp2_episodes_create_placed(&ep, ctx, EPISODES, HORIZON, 0, PP2_EPISODES_AUTO));
  const int policies[3] = {PP2_CONTROL_MODE, PP2_CONTROL_QMDP, PP2_ALPHA_FIB};
  const char* names[3] = {"mode", "QMDP", "FIB-greedy"};
  for (int p = 0; p < 3; ++p) {
    if (p < 2)
      CHECK(pp2_episodes_run(ep, policies[p], 2024, b0, start));
    else
      CHECK(pp2_episodes_run_alpha(ep, policies[p], 2024, b0, start));
    CHECK(pp2_episodes_results(ep, steps, status, cost, NULL));
    if (p == 0) {
      int lds = 0, wgs = 0, threads = 0, requested = -1, last = -1;
      long long scratch = 0;
      CHECK(pp2_episodes_info(ep, &lds, &wgs, &threads));
      CHECK(pp2_episodes_placement(ep, &requested, &last, &scratch));
      if (requested != PP2_EPISODES_AUTO || last != PP2_EPISODES_GLOBAL || scratch <= 0) return 3;
      printf("  MDP solved in %d sweeps, FIB swept %d times; %d episodes x %d steps, %d workgroups "
             "of %d threads, %d B of LDS each, planes in %.1f MiB of device memory\n", sweeps,
             FIB_SWEEPS, EPISODES, HORIZON, wgs, threads, lds, (double)scratch / (1024.0 * 1024.0));
    }
    if (report(names[p], EPISODES, steps, status, cost)) return 3;
    if (p == 2 && report("FIB-greedy (the lookahead's episodes)", LOOK_EPISODES, steps, status, cost))
      return 3;
  }
  CHECK(pp2_episodes_destroy(ep));
  /* the one-step lookahead over the same alphas: episode e of a batch depends
   * on (seed, e) alone, so these are the first LOOK_EPISODES robots again.
   * pp2_episodes_run_lookahead would refuse this batch (it runs from LDS planes
   * only); the placed call follows the placement. */
  ep = NULL;
  CHECK(pp2_episodes_create_placed(&ep, ctx, LOOK_EPISODES, HORIZON, 0, PP2_EPISODES_AUTO));
  if (pp2_episodes_run_lookahead(ep, PP2_ALPHA_FIB, 2024, b0, start) != PP2_EINVAL) return 3;
  CHECK(pp2_episodes_run_lookahead_placed(ep, PP2_ALPHA_FIB, 2024, b0, start));
  CHECK(pp2_episodes_results(ep, steps, status, cost, NULL));
  {
    int lds = 0, wgs = 0, threads = 0, last = -1;
    CHECK(pp2_episodes_info(ep, &lds, &wgs, &threads));
    CHECK(pp2_episodes_placement(ep, NULL, &last, NULL));
    if (last != PP2_EPISODES_GLOBAL) return 3;
    printf("  lookahead: %d episodes x %d steps, %d workgroups of %d threads, %d B of LDS each\n",
           LOOK_EPISODES, HORIZON, wgs, threads, lds);
  }
  if (report("FIB-lookahead", LOOK_EPISODES, steps, status, cost)) return 3;
  CHECK(pp2_episodes_destroy(ep));
  CHECK(pp2_destroy(ctx));
  return 0;
}
