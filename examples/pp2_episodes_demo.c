/*
 * pp2_episodes_demo.c -- evaluating the six control policies through the C ABI
 * alone (include/pp2.h "episodes"): solve the MDP, the FIB alphas and a small
 * PBVI set of sparse_map_100x40, then run a batch of simulated closed-loop
 * episodes under the belief-mode policy, the QMDP policy, the FIB-greedy and
 * the PBVI-greedy policy and the one-step lookahead over either alpha set --
 * the same robots, seed and cost scale, each in one launch -- and print success
 * rate, mean steps to the goal and mean discounted cost.  Plain C99, linked
 * against libpp2_hip.so.
 *
 *   ./pp2_episodes_demo [map.npy]     (default tests/golden/maps/sparse_map_100x40.npy,
 *                                      from the repository root); exit status 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pp2.h"

#define CHECK(call)                                                                \
  do {                                                                             \
    int s_ = (call);                                                               \
    if (s_ != PP2_OK) {                                                            \
      fprintf(stderr, "%s: %s: %s\n", #call, pp2_status_string(s_), pp2_last_error()); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

enum { H = 40, W = 100, EPISODES = 2048, HORIZON = 128, PBVI_SET = 32 };

/* the uint8 payload of a version-1 .npy file of H * W bytes */
static int load_map(const char* path, uint8_t* map) {
  unsigned char head[10];
  FILE* f = fopen(path, "rb");
  if (!f) return -1;
  int ok = fread(head, 1, 10, f) == 10 && memcmp(head, "\x93NUMPY", 6) == 0 && head[6] == 1;
  if (ok) ok = fseek(f, (long)(head[8] | (head[9] << 8)), SEEK_CUR) == 0;
  if (ok) ok = fread(map, 1, (size_t)H * W, f) == (size_t)H * W && fgetc(f) == EOF;
  fclose(f);
  return ok ? 0 : -1;
}

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "tests/golden/maps/sparse_map_100x40.npy";
  static uint8_t map[H * W], status[EPISODES];
  static float b0[H * W], cost[EPISODES];
  static int32_t start[EPISODES], steps[EPISODES];
  if (load_map(path, map) != 0) {
    fprintf(stderr, "cannot read a %dx%d uint8 map from %s\n", W, H, path);
    return 2;
  }
  /* uniform belief over the free cells; start cells spread over them */
  int nfree = 0;
  for (int i = 0; i < H * W; ++i) nfree += map[i] == 0;
  if (nfree == 0) return 2;
  for (int i = 0; i < H * W; ++i) b0[i] = map[i] ? 0.0f : 1.0f / (float)nfree;
  for (int e = 0, i = 0; e < EPISODES; ++e) {
    do i = (i + 37) % (H * W); while (map[i]);
    start[e] = i;
  }

  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx* ctx = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, 95, 34, 0.95f));
  CHECK(pp2_model_generate(ctx));
  int sweeps = 0;
  double norm = 0.0;
  CHECK(pp2_mdp_solve(ctx, 0, &sweeps, &norm));
  int fib_sweeps = 0;
  float fib_norm = 0.0f;
  CHECK(pp2_fib_solve(ctx, 0, &fib_sweeps, &fib_norm));
  CHECK(pp2_pbvi_solve(ctx, b0, PBVI_SET, 1, NULL));
  pp2_episodes* ep = NULL;
  CHECK(pp2_episodes_create(&ep, ctx, EPISODES, HORIZON, 0));
  int lds = 0, wgs = 0, threads = 0;
  CHECK(pp2_episodes_info(ep, &lds, &wgs, &threads));
  printf("pp2_episodes_demo: MDP solved in %d sweeps, FIB in %d, PBVI with %d beliefs; %d episodes "
         "x %d steps, %d workgroups of %d threads, %d B of LDS each\n", sweeps, fib_sweeps,
         PBVI_SET, EPISODES, HORIZON, wgs, threads, lds);
  /* mode and QMDP read J and A, the alpha and the lookahead runs the FIB /
   * PBVI vectors */
  const int policies[6] = {PP2_CONTROL_MODE, PP2_CONTROL_QMDP, PP2_ALPHA_FIB,
                           PP2_ALPHA_PBVI,   PP2_ALPHA_FIB,    PP2_ALPHA_PBVI};
  const char* names[6] = {"mode", "QMDP", "FIB-greedy", "PBVI-greedy", "FIB-lookahead",
                          "PBVI-lookahead"};
  for (int p = 0; p < 6; ++p) {
    if (p < 2)
      CHECK(pp2_episodes_run(ep, policies[p], 2024, b0, start));
    else if (p < 4)
      CHECK(pp2_episodes_run_alpha(ep, policies[p], 2024, b0, start));
    else
      CHECK(pp2_episodes_run_lookahead(ep, policies[p], 2024, b0, start));
    CHECK(pp2_episodes_results(ep, steps, status, cost, NULL));
    int reached = 0, lost = 0;
    double sum_steps = 0.0, sum_cost = 0.0;
    for (int e = 0; e < EPISODES; ++e) {
      if (status[e] > 2 || steps[e] < 0 || steps[e] > HORIZON) return 3;
      if (status[e] == 1) { ++reached; sum_steps += steps[e]; }
      lost += status[e] == 2;
      sum_cost += cost[e];
    }
    printf("  %s policy: success rate %.3f, mean steps to the goal %.1f, mean discounted cost "
           "%.3f, beliefs lost %d\n", names[p], (double)reached / EPISODES,
           reached ? sum_steps / reached : 0.0, sum_cost / EPISODES, lost);
  }
  CHECK(pp2_episodes_destroy(ep));
  CHECK(pp2_destroy(ctx));
  return 0;
}
