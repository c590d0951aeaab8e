/*
 * pp2_pomdp_replan_demo.c -- the POMDP node's replanning sequence through the
 * C ABI alone (include/pp2.h "live updates", pp2_planner_refresh): plan a few
 * steps with the QV-tree planner, drop an obstacle on the cell ahead of the
 * belief's mode with pp2_map_update, re-solve the FIB alphas warm with
 * pp2_fib_resolve and bring the planner up to date with pp2_planner_refresh --
 * it keeps its belief and its rand() stream, only the cells around the obstacle
 * are read again -- then plan on.  Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_pomdp_replan_demo      exit status 0 on success
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
  const int32_t gx = 55, gy = 35;
  uint8_t* map = (uint8_t*)calloc(H * W, 1);
  float* belief = (float*)malloc(sizeof(float) * H * W);
  if (!map || !belief) return 1;
  /* a walled room with two pillars; the goal near the far corner */
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x)
      map[y * W + x] = (x == 0 || y == 0 || x == W - 1 || y == H - 1 ||
                        (x >= 20 && x < 23 && y >= 10 && y < 30) ||
                        (x >= 40 && x < 43 && y >= 5 && y < 25));
  float free_cells = 0.0f;
  for (uint32_t i = 0; i < H * W; ++i) free_cells += 1.0f - map[i];
  for (uint32_t i = 0; i < H * W; ++i) belief[i] = (1.0f - map[i]) / free_cells;

  int ndev = 0;
  CHECK(pp2_device_count(&ndev));
  if (ndev < 1) {
    fprintf(stderr, "no GPU\n");
    return 2;
  }
  pp2_ctx* ctx = NULL;
  CHECK(pp2_create(&ctx, 0, H, W, map, gx, gy, 0.95f));
  CHECK(pp2_model_generate(ctx));
  int cold = 0, warm = 0;
  float fnorm = 0.0f;
  CHECK(pp2_fib_solve(ctx, 0, &cold, &fnorm));

  pp2_planner_params prm;
  CHECK(pp2_planner_default_params(&prm));
  prm.max_search_tree_depth = 5;
  pp2_planner* pl = NULL;
  CHECK(pp2_planner_create(&pl, ctx, &prm));
  uint8_t act = 0, obs = 0;
  float value = 0.0f;
  for (int k = 0; k < 3; ++k) {
    CHECK(pp2_planner_step(pl, act, obs, k == 0 ? belief : NULL, &act, &value));
    if (act > 8) return 3;
    obs = (uint8_t)((k * 5) & 15);
  }
  const float value_before = value;

  /* the belief's mode (first maximum); action a moves to the neighbour
   * (a % 3 - 1, a / 3 - 1): the 3x3 obstacle goes on the cell ahead */
  CHECK(pp2_planner_root_belief(pl, belief));
  uint32_t mode = 0;
  for (uint32_t i = 1; i < H * W; ++i)
    if (belief[i] > belief[mode]) mode = i;
  int32_t x = (int32_t)(mode % W) + act % 3 - 1, y = (int32_t)(mode / W) + act / 3 - 1;
  if (x < 1) x = 1;
  if (y < 1) y = 1;
  if (x > (int32_t)W - 2) x = (int32_t)W - 2;
  if (y > (int32_t)H - 2) y = (int32_t)H - 2;
  uint8_t block[9];
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) block[j * 3 + i] = !(x - 1 + i == gx && y - 1 + j == gy);
  CHECK(pp2_map_update(ctx, (uint32_t)x - 1, (uint32_t)y - 1, 3, 3, block));
  /* the planner caches the model: it refuses to step until it is refreshed */
  if (pp2_planner_step(pl, act, obs, NULL, NULL, NULL) != PP2_ESTATE) return 4;
  CHECK(pp2_fib_resolve(ctx, 0, &warm, &fnorm));
  CHECK(pp2_planner_refresh(pl));

  for (int k = 3; k < 6; ++k) {
    CHECK(pp2_planner_step(pl, act, obs, NULL, &act, &value));
    if (act > 8) return 3;
    obs = (uint8_t)((k * 5) & 15);
  }
  long long refreshes = 0, incremental = 0, full = 0, cells = 0;
  CHECK(pp2_planner_refresh_info(pl, &refreshes, &incremental, &full, &cells));
  uint64_t draws = 0;
  CHECK(pp2_planner_rand_calls(pl, &draws));
  if (refreshes != 1 || incremental + full != 1) return 5;

  printf("pp2_pomdp_replan_demo ok: FIB cold %d sweeps; 3x3 obstacle at (x %d, y %d) ahead of the "
         "belief's mode; FIB warm %d sweeps (norm %.3g)\n", cold, (int)x, (int)y, warm, fnorm);
  printf("  planner refreshes %lld: patch path %lld, full %lld, cells patched %lld; value %.4f "
         "before, %.4f after; %llu rand() draws, one stream\n", refreshes, incremental, full, cells,
         value_before, value, (unsigned long long)draws);
  CHECK(pp2_planner_destroy(pl));
  CHECK(pp2_destroy(ctx));
  free(map);
  free(belief);
  return 0;
}
