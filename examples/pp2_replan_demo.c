/*
 * pp2_replan_demo.c -- a live map update through the C ABI alone
 * (include/pp2.h "live updates"): solve the MDP on an occupancy grid, follow
 * the greedy policy from a start cell, drop an obstacle on that path with
 * pp2_map_update -- only the cells around it are regenerated; values, belief
 * and tuning stay -- and re-solve warm with pp2_mdp_resolve from the previous
 * solution.  Plain C99, linked against libpp2_hip.so.
 *
 *   ./pp2_replan_demo      exit status 0 on success
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
  const int32_t sx = 5, sy = 5, gx = 55, gy = 35;
  uint8_t* map = (uint8_t*)calloc(H * W, 1);
  uint8_t* A = (uint8_t*)calloc(H * W, 1);
  if (!map || !A) return 1;
  /* a walled room with two pillars; start near one corner, goal near the other */
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x)
      map[y * W + x] = (x == 0 || y == 0 || x == W - 1 || y == H - 1 ||
                        (x >= 20 && x < 23 && y >= 10 && y < 30) ||
                        (x >= 40 && x < 43 && y >= 5 && y < 25));

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
  double norm = 0.0;
  CHECK(pp2_mdp_solve(ctx, 0, &cold, &norm));
  CHECK(pp2_mdp_get(ctx, NULL, A));
  const uint8_t first_before = A[sy * W + sx];

  /* the greedy path: action a moves to the neighbour (a % 3 - 1, a / 3 - 1);
   * the obstacle goes 6 moves ahead */
  int32_t x = sx, y = sy;
  for (int k = 0; k < 6 && !(x == gx && y == gy); ++k) {
    const uint8_t a = A[y * W + x];
    x += a % 3 - 1;
    y += a / 3 - 1;
  }
  if (x < 2 || y < 2 || x > (int32_t)W - 3 || y > (int32_t)H - 3) return 3;
  const uint8_t block[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
  CHECK(pp2_map_update(ctx, (uint32_t)x - 1, (uint32_t)y - 1, 3, 3, block));
  long long updates = 0, incremental = 0, rebuilds = 0;
  int added = 0;
  CHECK(pp2_map_update_info(ctx, &updates, &incremental, &rebuilds, &added));
  CHECK(pp2_mdp_resolve(ctx, 0, &warm, &norm));
  CHECK(pp2_mdp_get(ctx, NULL, A));
  const uint8_t first_after = A[sy * W + sx];
  if (updates != 1 || first_before > 8 || first_after > 8) return 4;

  printf("pp2_replan_demo ok: cold solve %d sweeps; 3x3 obstacle at (x %d, y %d) on the greedy "
         "path: %s, %d dictionary rows added; warm re-solve %d sweeps (norm %.3g)\n",
         cold, (int)x, (int)y, incremental ? "patched in place" : "full rebuild", added, warm, norm);
  printf("  first action from (x %d, y %d): %u before, %u after\n", (int)sx, (int)sy, first_before,
         first_after);
  CHECK(pp2_destroy(ctx));
  free(map);
  free(A);
  return 0;
}
