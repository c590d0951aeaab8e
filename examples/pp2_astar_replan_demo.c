/*
 * pp2_astar_replan_demo.c -- the A* baseline following a live map update
 * through the C ABI alone (include/pp2.h "shortest-path field"): solve the
 * goal-rooted shortest-path field of sparse_map_100x40, trace the path from
 * the launch file's start (11, 6), drop an obstacle on the middle of that
 * path (pp2_map_update), repair the field warm (pp2_path_resolve: raise what
 * no longer stands, then relax) and trace again.  It needs no model.  Plain
 * C99, linked against libpp2_hip.so.
 *
 *   ./pp2_astar_replan_demo [map.npy]   (default tests/golden/maps/sparse_map_100x40.npy,
 *                                        from the repository root); exit status 0 only
 *                                        if the re-solve ran warm and the new path
 *                                        avoids the obstacle
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

enum { H = 40, W = 100, START_X = 11, START_Y = 6, GOAL_X = 95, GOAL_Y = 34 };

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
  static uint8_t map[H * W];
  static int32_t before[H * W], after[H * W];
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
  pp2_ctx* ctx = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, GOAL_X, GOAL_Y, 0.95f));
  int rounds = 0, converged = 0, reached = 0;
  CHECK(pp2_path_solve(ctx, H * W, &rounds, &converged, &reached));
  if (!converged) {
    fprintf(stderr, "the field did not settle in %d rounds\n", rounds);
    return 3;
  }
  const int32_t start = START_Y * W + START_X;
  int n0 = 0, n1 = 0;
  float len0 = 0.0f, len1 = 0.0f;
  CHECK(pp2_path_trace(ctx, start, before, H * W, &n0, &len0));
  if (n0 < 5 || before[n0 - 1] != GOAL_Y * W + GOAL_X) return 3;
  printf("pp2_astar_replan_demo: cold solve in %d rounds, %d cells reach the goal; path from "
         "(%d, %d): %d cells, length %.4f\n", rounds, reached, START_X, START_Y, n0, len0);

  /* an obstacle on the middle of the path */
  const int32_t mid = before[n0 / 2];
  const uint8_t one = 1;
  CHECK(pp2_map_update(ctx, (uint32_t)(mid % W), (uint32_t)(mid / W), 1, 1, &one));
  int valid = 1;
  CHECK(pp2_path_info(ctx, &valid, NULL, NULL, NULL, NULL, NULL));
  if (valid) return 3; /* the update invalidates the field */

  int warm = 0, raised = 0, raise_rounds = 0, relax_rounds = 0, seed_cells = 0, reached1 = 0;
  CHECK(pp2_path_resolve(ctx, H * W, &rounds, &converged, &reached1, &warm));
  if (!converged) return 3;
  CHECK(pp2_path_resolve_info(ctx, NULL, &raised, &raise_rounds, &relax_rounds, &seed_cells));
  CHECK(pp2_path_trace(ctx, start, after, H * W, &n1, &len1));
  printf("  obstacle at (%d, %d): %s re-solve, %d cells raised in %d raise rounds, %d relax "
         "rounds (%d cells seeded), %d cells reach the goal\n", (int)(mid % W), (int)(mid / W),
         warm ? "warm" : "cold", raised, raise_rounds, relax_rounds, seed_cells, reached1);
  printf("  path before: %d cells, length %.4f; after: %d cells, length %.4f\n", n0, len0, n1,
         len1);
  int avoids = n1 >= 2 && after[0] == start && after[n1 - 1] == GOAL_Y * W + GOAL_X;
  for (int i = 0; i < n1; ++i) avoids = avoids && after[i] != mid;
  CHECK(pp2_destroy(ctx));
  if (!avoids || !warm || !(len1 >= len0)) {
    fprintf(stderr, "the re-solved path does not avoid the obstacle, or the re-solve ran cold\n");
    return 3;
  }
  printf("pp2_astar_replan_demo ok\n");
  return 0;
}
