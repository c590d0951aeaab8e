/*
 * pp2_policy_eval_demo.c -- the exact outcome fields of an action table through
 * the C ABI alone (include/pp2.h "policy evaluation").  On sparse_map_100x40:
 * solve the MDP and the shortest-path field, evaluate both tables over 200
 * steps and print, for the launch file's start (11, 6), the expected
 * discounted cost G, the probability P of reaching the goal and the expected
 * steps N -- what the episodes estimate by sampling, here without a sample --
 * and the largest G difference between the two tables over all cells.  Then
 * the price of a stale map: a world with the sense demo's wall at x = 50 that
 * the believed map lacks -- y = 6 .. 25 here, which leaves row 26 as the one
 * way through on this map (down to y = 33 it would cut the goal off) -- and
 * the believed map's table evaluated in that world before and after
 * pp2_map_update + pp2_mdp_resolve.
 * Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_policy_eval_demo [map.npy]  (default tests/golden/maps/sparse_map_100x40.npy,
 *                                      from the repository root); exit status 0 on success
 */
#include <math.h>
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

enum { H = 40, W = 100, HORIZON = 200, START_X = 11, START_Y = 6, GOAL_X = 95, GOAL_Y = 34 };
enum { WALL_X = 50, WALL_Y0 = 6, WALL_H = 20 };

static float G[2][H * W], P[H * W], N[H * W];

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

/* evaluate `table` of ctx in world, print the start cell's line, G into g */
static int evaluate(pp2_ctx* ctx, pp2_ctx* world, int table, const char* label, float* g) {
  const int s = START_Y * W + START_X;
  CHECK(pp2_policy_evaluate(ctx, world, table, HORIZON, PP2_POLICY_AUTO, 0));
  CHECK(pp2_policy_get(ctx, g, P, N));
  printf("  %-22s G %a P %a N %a   (cost %.4f, reaches the goal %.4f, steps %.2f)\n", label,
         (double)g[s], (double)P[s], (double)N[s], (double)g[s], (double)P[s], (double)N[s]);
  return 0;
}

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "tests/golden/maps/sparse_map_100x40.npy";
  static uint8_t map[H * W];
  uint8_t wall[WALL_H];
  if (load_map(path, map) != 0) {
    fprintf(stderr, "cannot read a %dx%d uint8 map from %s\n", W, H, path);
    return 2;
  }
  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx *ctx = NULL, *world = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, GOAL_X, GOAL_Y, 0.95f));
  CHECK(pp2_model_generate(ctx));
  CHECK(pp2_mdp_solve(ctx, 0, NULL, NULL));
  int converged = 0;
  CHECK(pp2_path_solve(ctx, H * W, NULL, &converged, NULL));
  if (!converged) return 3;

  int route = 0, block = 0, launches = 0, tr = 0, tc = 0;
  printf("pp2_policy_eval_demo: start (%d, %d), goal (%d, %d), horizon %d\n", (int)START_X,
         (int)START_Y, (int)GOAL_X, (int)GOAL_Y, (int)HORIZON);
  if (evaluate(ctx, NULL, PP2_TABLE_MDP, "table mdp", G[0])) return 1;
  if (evaluate(ctx, NULL, PP2_TABLE_PATH, "table path", G[1])) return 1;
  CHECK(pp2_policy_info(ctx, NULL, NULL, NULL, &route, &block, &launches, &tr, &tc, NULL, NULL));
  float worst = 0.0f;
  int at = 0;
  for (int i = 0; i < H * W; ++i)
    if (!map[i] && fabsf(G[1][i] - G[0][i]) > worst) {
      worst = fabsf(G[1][i] - G[0][i]);
      at = i;
    }
  printf("  largest |G path - G mdp| over the free cells: %.4f at (%d, %d); route %s, %d steps per "
         "launch, %d launches, %d x %d tiles\n", (double)worst, at % W, at / W,
         route == PP2_POLICY_TILES ? "tiles" : "planes", block, launches, tr, tc);

  /* the world has a wall the believed map lacks */
  for (int i = 0; i < WALL_H; ++i) {
    wall[i] = 1;
    map[(WALL_Y0 + i) * W + WALL_X] = 1;
  }
  CHECK(pp2_create(&world, 0, H, W, map, GOAL_X, GOAL_Y, 0.95f));
  CHECK(pp2_model_generate(world));
  if (evaluate(ctx, world, PP2_TABLE_MDP, "stale map, in the world", G[0])) return 1;
  int warm = 0;
  CHECK(pp2_map_update(ctx, WALL_X, WALL_Y0, 1, WALL_H, wall));
  CHECK(pp2_mdp_resolve(ctx, 0, &warm, NULL));
  if (evaluate(ctx, world, PP2_TABLE_MDP, "updated, in the world", G[1])) return 1;
  printf("  the stale map costs %.4f at the start (warm re-solve: %d sweeps)\n",
         (double)(G[0][START_Y * W + START_X] - G[1][START_Y * W + START_X]), warm);
  CHECK(pp2_destroy(world));
  CHECK(pp2_destroy(ctx));
  printf("pp2_policy_eval_demo ok\n");
  return 0;
}
