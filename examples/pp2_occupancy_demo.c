/*
 * pp2_occupancy_demo.c -- where the robot will be, and when, through the C ABI
 * alone (include/pp2.h "occupancy").  On sparse_map_100x40, from the launch
 * file's start (11, 6) over 200 steps: for the MDP's table and the
 * shortest-path field's, the step at which the arrival curve passes 0.5 and
 * 0.9, the most visited cell of the corridor, and the cells where the two
 * visit fields differ most.  Then the stale map of pp2_policy_eval_demo.c: a
 * world with a wall at x = 50, y = 6 .. 25 that the believed map lacks, and the
 * believed map's table run in that world before and after pp2_map_update +
 * pp2_mdp_resolve -- the cells the stale table sends the robot through, as the
 * difference of the two visit fields.
 * Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_occupancy_demo [map.npy]  (default tests/golden/maps/sparse_map_100x40.npy,
 *                                    from the repository root); exit status 0 on success
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
enum { WALL_X = 50, WALL_Y0 = 6, WALL_H = 20, NDIFF = 3 };

static float b0[H * W], D[H * W], V[2][H * W], curve[HORIZON + 1];

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

/* the first step at which the curve reaches p, -1 if it never does */
static int passes(float p) {
  for (int k = 0; k <= HORIZON; ++k)
    if (curve[k] >= p) return k;
  return -1;
}

/* the occupancy of `table` of ctx in world from the start cell: print its line, V into v */
static int occupancy(pp2_ctx* ctx, pp2_ctx* world, int table, const char* label, float* v) {
  CHECK(pp2_occupancy_evaluate(ctx, world, table, b0, HORIZON, PP2_OCC_AUTO, 0));
  CHECK(pp2_occupancy_get(ctx, D, v, curve));
  int at = 0;
  double visits = 0.0;
  for (int i = 0; i < H * W; ++i) {
    visits += (double)v[i];
    if (i != START_Y * W + START_X && v[i] > v[at]) at = i;
  }
  printf("  %-24s arrived %a (%.4f); curve passes 0.5 at step %d, 0.9 at step %d; expected "
         "steps %.2f; most visited cell after the start (%d, %d), %.4f visits\n", label,
         (double)curve[HORIZON], (double)curve[HORIZON], passes(0.5f), passes(0.9f), visits,
         at % W, at / W, (double)v[at]);
  return 0;
}

/* the NDIFF cells where two visit fields differ most */
static void differ(const char* what, const float* a, const float* b) {
  int taken[NDIFF];
  printf("  %s:", what);
  for (int n = 0; n < NDIFF; ++n) {
    int at = -1;
    for (int i = 0; i < H * W; ++i) {
      int used = 0;
      for (int m = 0; m < n; ++m) used |= taken[m] == i;
      if (!used && (at < 0 || fabsf(a[i] - b[i]) > fabsf(a[at] - b[at]))) at = i;
    }
    taken[n] = at;
    printf(" (%d, %d) %+.4f", at % W, at / W, (double)(a[at] - b[at]));
  }
  printf("\n");
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
  b0[START_Y * W + START_X] = 1.0f;

  int route = 0, block = 0, launches = 0, tr = 0, tc = 0;
  printf("pp2_occupancy_demo: start (%d, %d), goal (%d, %d), horizon %d\n", (int)START_X,
         (int)START_Y, (int)GOAL_X, (int)GOAL_Y, (int)HORIZON);
  if (occupancy(ctx, NULL, PP2_TABLE_MDP, "table mdp", V[0])) return 1;
  if (occupancy(ctx, NULL, PP2_TABLE_PATH, "table path", V[1])) return 1;
  CHECK(pp2_occupancy_info(ctx, NULL, NULL, NULL, &route, &block, &launches, &tr, &tc, NULL, NULL));
  differ("largest V path - V mdp", V[1], V[0]);
  printf("  route %s, %d steps per launch, %d launches, %d x %d tiles\n",
         route == PP2_OCC_TILES ? "tiles" : "planes", block, launches, tr, tc);

  /* the world has a wall the believed map lacks */
  for (int i = 0; i < WALL_H; ++i) {
    wall[i] = 1;
    map[(WALL_Y0 + i) * W + WALL_X] = 1;
  }
  CHECK(pp2_create(&world, 0, H, W, map, GOAL_X, GOAL_Y, 0.95f));
  CHECK(pp2_model_generate(world));
  if (occupancy(ctx, world, PP2_TABLE_MDP, "stale map, in the world", V[0])) return 1;
  int warm = 0;
  CHECK(pp2_map_update(ctx, WALL_X, WALL_Y0, 1, WALL_H, wall));
  CHECK(pp2_mdp_resolve(ctx, 0, &warm, NULL));
  if (occupancy(ctx, world, PP2_TABLE_MDP, "updated, in the world", V[1])) return 1;
  differ("largest V stale - V updated", V[0], V[1]);
  printf("  (warm re-solve: %d sweeps)\n", warm);
  CHECK(pp2_destroy(world));
  CHECK(pp2_destroy(ctx));
  printf("pp2_occupancy_demo ok\n");
  return 0;
}
