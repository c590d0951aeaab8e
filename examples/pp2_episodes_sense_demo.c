/*
 * pp2_episodes_sense_demo.c -- simulate robots whose map is stale, through the
 * C ABI alone (include/pp2.h "episodes": "The world", "Resumed segments").
 * Two contexts over a 100 x 40 room: the believed one holds the map the robots
 * plan on, the world one the true map, which has a wall across the greedy path
 * that the believed map lacks.  512 QMDP episodes run in segments of 40 steps
 * (pp2_episodes_run, then pp2_episodes_resume), motion, observations, cost and
 * goal from the world, control and belief update from the believed context:
 *   never updated     the believed map stays stale for all 200 steps
 *   updated at k=40   after the first segment the wall is sensed:
 *                     pp2_map_update on the believed context, a warm
 *                     pp2_mdp_resolve, and the episodes carry on
 *   known from start  the believed map is the true one from step 0
 * Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_episodes_sense_demo      exit status 0 on success
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

enum { H = 40, W = 100, E = 512, SEG = 40, SEGS = 5, SEED = 11 };
/* the wall only the world has at first: x = 50, y = 6 .. 33 */
enum { WALL_X = 50, WALL_Y0 = 6, WALL_H = 28 };

static uint8_t status[E];

/* segments first .. SEGS-1 as resumed ones; *rate = the share that reached the goal */
static int carry_on(pp2_episodes* ep, int first, double* rate, int* lost) {
  for (int k = first; k < SEGS; ++k) CHECK(pp2_episodes_resume(ep, PP2_EPISODE_QMDP, SEED));
  CHECK(pp2_episodes_results(ep, NULL, status, NULL, NULL));
  int ok = 0;
  *lost = 0;
  for (int e = 0; e < E; ++e) {
    ok += status[e] == 1;
    *lost += status[e] == 2;
  }
  *rate = (double)ok / E;
  return 0;
}

int main(void) {
  const int32_t gx = 92, gy = 20;
  uint8_t* map = (uint8_t*)calloc((size_t)H * W, 1);
  float* b0 = (float*)calloc((size_t)H * W, sizeof(float));
  int32_t* starts = (int32_t*)calloc(E, sizeof(int32_t));
  uint8_t wall[WALL_H];
  if (!map || !b0 || !starts) return 1;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) map[y * W + x] = x == 0 || y == 0 || x == W - 1 || y == H - 1;
  /* the robots start in columns 2 .. 9 and know that much: b0 is uniform there */
  int n0 = 0;
  for (int y = 1; y < H - 1; ++y)
    for (int x = 2; x < 10; ++x) ++n0;
  for (int y = 1; y < H - 1; ++y)
    for (int x = 2; x < 10; ++x) b0[y * W + x] = 1.0f / (float)n0;
  for (int e = 0; e < E; ++e) starts[e] = (1 + (e * 7) % (H - 2)) * W + 2 + e % 8;
  for (int i = 0; i < WALL_H; ++i) wall[i] = 1;

  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx *believed = NULL, *world = NULL;
  CHECK(pp2_create(&believed, 0, H, W, map, gx, gy, 0.95f));
  CHECK(pp2_model_generate(believed));
  CHECK(pp2_mdp_solve(believed, 0, NULL, NULL));
  for (int i = 0; i < WALL_H; ++i) map[(WALL_Y0 + i) * W + WALL_X] = 1;
  CHECK(pp2_create(&world, 0, H, W, map, gx, gy, 0.95f));
  CHECK(pp2_model_generate(world));

  pp2_episodes* ep = NULL;
  CHECK(pp2_episodes_create(&ep, believed, E, SEG, 0));
  CHECK(pp2_episodes_set_world(ep, world));
  double never = 0, sensed = 0, known = 0;
  int lost_never = 0, lost_sensed = 0, lost_known = 0, warm = 0;

  /* never updated */
  CHECK(pp2_episodes_run(ep, PP2_CONTROL_QMDP, SEED, b0, starts));
  if (carry_on(ep, 1, &never, &lost_never)) return 1;

  /* updated at k = SEG: sense, patch the believed map, re-solve warm, carry on */
  CHECK(pp2_episodes_run(ep, PP2_CONTROL_QMDP, SEED, b0, starts));
  CHECK(pp2_map_update(believed, WALL_X, WALL_Y0, 1, WALL_H, wall));
  CHECK(pp2_mdp_resolve(believed, 0, &warm, NULL));
  if (carry_on(ep, 1, &sensed, &lost_sensed)) return 1;

  /* known from the start: the believed map is the true one by now */
  CHECK(pp2_episodes_run(ep, PP2_CONTROL_QMDP, SEED, b0, starts));
  if (carry_on(ep, 1, &known, &lost_known)) return 1;

  printf("pp2_episodes_sense_demo ok: %d QMDP episodes, %d steps in segments of %d, a wall at "
         "x %d, y %d..%d that the believed map lacks\n",
         (int)E, SEG * SEGS, (int)SEG, (int)WALL_X, (int)WALL_Y0, WALL_Y0 + WALL_H - 1);
  printf("  never updated     success rate %.3f (%d beliefs lost)\n", never, lost_never);
  printf("  updated at k=%d   success rate %.3f (%d beliefs lost; warm re-solve %d sweeps)\n",
         (int)SEG, sensed, lost_sensed, warm);
  printf("  known from start  success rate %.3f (%d beliefs lost)\n", known, lost_known);
  CHECK(pp2_episodes_destroy(ep));
  CHECK(pp2_destroy(world));
  CHECK(pp2_destroy(believed));
  free(map);
  free(b0);
  free(starts);
  return 0;
}
