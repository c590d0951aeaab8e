/*
 * pp2_astar_demo.c -- the A* baseline through the C ABI alone (include/pp2.h
 * "shortest-path field"): solve the MDP and the goal-rooted shortest-path field
 * of sparse_map_100x40, print the path from the launch file's start (11, 6),
 * then run one batch of closed-loop episodes under the belief-mode policy with
 * each action table -- the MDP's A and the field's A_path, the same robots and
 * seed -- and print the two success rates and mean discounted costs.  Plain
 * C99, linked against libpp2_hip.so.
 *
 *   ./pp2_astar_demo [map.npy]     (default tests/golden/maps/sparse_map_100x40.npy,
 *                                   from the repository root); exit status 0 on success
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

enum { H = 40, W = 100, EPISODES = 1024, HORIZON = 160, START_X = 11, START_Y = 6 };

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
  static int32_t start[EPISODES], steps[EPISODES], cells[H * W];
  if (load_map(path, map) != 0) {
    fprintf(stderr, "cannot read a %dx%d uint8 map from %s\n", W, H, path);
    return 2;
  }
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
  int rounds = 0, converged = 0, reached = 0, launches = 0, polls = 0, tr = 0, tc = 0;
  CHECK(pp2_path_solve(ctx, H * W, &rounds, &converged, &reached));
  if (!converged) {
    fprintf(stderr, "the field did not settle in %d rounds\n", rounds);
    return 3;
  }
  CHECK(pp2_path_info(ctx, NULL, NULL, &launches, &polls, &tr, &tc));
  printf("pp2_astar_demo: MDP solved in %d sweeps; shortest-path field in %d rounds of %d x %d "
         "tiles (%d launches, %d polls), %d of %d free cells reach the goal\n", sweeps, rounds, tr,
         tc, launches, polls, reached, nfree);

  int n = 0;
  float length = 0.0f;
  CHECK(pp2_path_trace(ctx, START_Y * W + START_X, cells, H * W, &n, &length));
  if (n < 2 || cells[0] != START_Y * W + START_X || cells[n - 1] != 34 * W + 95) return 3;
  printf("  path from (%d, %d): %d cells, length %.4f:", START_X, START_Y, n, length);
  for (int i = 0; i < n; ++i) printf(" (%d,%d)", (int)(cells[i] % W), (int)(cells[i] / W));
  printf("\n");

  pp2_episodes* ep = NULL;
  CHECK(pp2_episodes_create(&ep, ctx, EPISODES, HORIZON, 0));
  const int tables[2] = {PP2_TABLE_MDP, PP2_TABLE_PATH};
  const char* names[2] = {"mdp", "path"};
  for (int t = 0; t < 2; ++t) {
    CHECK(pp2_episodes_set_action_table(ep, tables[t]));
    CHECK(pp2_episodes_run(ep, PP2_CONTROL_MODE, 2024, b0, start));
    CHECK(pp2_episodes_results(ep, steps, status, cost, NULL));
    int goal = 0;
    double sum_steps = 0.0, sum_cost = 0.0;
    for (int e = 0; e < EPISODES; ++e) {
      if (status[e] > 2 || steps[e] < 0 || steps[e] > HORIZON) return 3;
      if (status[e] == 1) { ++goal; sum_steps += steps[e]; }
      sum_cost += cost[e];
    }
    printf("  mode policy, table %s: success rate %.3f, mean steps to the goal %.1f, mean "
           "discounted cost %.3f\n", names[t], (double)goal / EPISODES,
           goal ? sum_steps / goal : 0.0, sum_cost / EPISODES);
  }
  CHECK(pp2_episodes_destroy(ep));
  CHECK(pp2_destroy(ctx));
  printf("pp2_astar_demo ok\n");
  return 0;
}
