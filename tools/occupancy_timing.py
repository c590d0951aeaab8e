"""Wall time of pp2_occupancy_evaluate + pp2_synchronize per route and block
depth, by tools/policy_eval_timing.py's protocol: a host clock
around a call that ends in a synchronise; 1 warm-up, then 7 timed repetitions,
the variants alternating in one process; min / median / max in microseconds,
and per step.  Two yardsticks run in the same run on the same context:
pp2_policy_evaluate on its TILES route at its default block (the adjoint
operator) and pp2_mdp_sweep(ctx, H) (nine actions per cell on the resident
path).  The occupancy call includes what the evaluator's has not: the check and
upload of b0 (H*W floats) from the host.

Sizes: the bench's 1024^2 synthetic grid at H = 1024 and H = 64, and
sparse_map_100x40 at H = 64.  Variants: PLANES, TILES at block 1 and at each
candidate block.  b0 is uniform on the free cells.

    python tools/occupancy_timing.py [out.json]
        default profiles/occupancy/occupancy_timing.json
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import path_planning_2d_amd as P
from path_planning_2d_amd import _lib, synthetic as S

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "occupancy",
                                                        "occupancy_timing.json")
WARM, REPS = 1, 7
CANDIDATES = (2, 4, 8)
lib = _lib.load()


def case(name, grid, goal, horizon):
    H, W = grid.shape
    res = {"case": name, "rows": H, "cols": W, "horizon": horizon}
    free = grid == 0
    b0 = np.ascontiguousarray(free / np.float32(free.sum()), np.float32)
    b0p = b0.ctypes.data_as(C.POINTER(C.c_float))
    with P.GridContext(grid, goal, gamma=0.95) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        ctx.synchronize()
        h = ctx.handle
        info = ctx.occupancy_info()
        blocks = [b for b in (1,) + CANDIDATES if b <= info["max_block"]]

        def occupancy(route, block):
            def run():
                assert lib.pp2_occupancy_evaluate(h, None, 0, b0p, horizon, route, block) == 0
                assert lib.pp2_synchronize(h) == 0
            return run

        def policy_tiles():
            assert lib.pp2_policy_evaluate(h, None, 0, horizon, 2, 0) == 0
            assert lib.pp2_synchronize(h) == 0

        def sweep():
            assert lib.pp2_mdp_sweep(h, horizon) == 0
            assert lib.pp2_synchronize(h) == 0

        variants = {"mdp_sweep": sweep, "policy_tiles_default": policy_tiles,
                    "planes": occupancy(1, 0)}
        for b in blocks:
            variants[f"tiles_block{b}"] = occupancy(2, b)
        times = {k: [] for k in variants}
        for rep in range(WARM + REPS):  # alternate, so drift hits all alike
            for k, fn in variants.items():
                t = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t) * 1e6
                if rep >= WARM:
                    times[k].append(dt)
        for k, v in times.items():
            res[k] = {"min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1),
                      "max_us": round(max(v), 1),
                      "median_us_per_step": round(statistics.median(v) / horizon, 3)}
        res["tile_rows"], res["tile_cols"] = info["tile_rows"], info["tile_cols"]
        res["default_block"] = info["default_block"]
        res["policy_default_block"] = ctx.policy_info()["default_block"]
        # every variant computed the same bits
        ctx.occupancy_evaluate(horizon, b0, route="planes")
        ref = [a.view(np.uint32).copy() for a in ctx.occupancy_get()]
        for b in blocks:
            ctx.occupancy_evaluate(horizon, b0, route="tiles", block=b)
            assert all(np.array_equal(a.view(np.uint32), r)
                       for a, r in zip(ctx.occupancy_get(), ref))
    return res


big = S.synth_grid(1024, 1024, seed=1024)
small = np.load(os.path.join(ROOT, "tests", "golden", "maps", "sparse_map_100x40.npy"),
                allow_pickle=False)
out = {"method": f"host clock around evaluate + synchronise, {WARM} warm-up, {REPS} timed, "
                 "variants alternating",
       "cases": [case("synthetic_1024", big, S.synth_goal(big), 1024),
                 case("synthetic_1024", big, S.synth_goal(big), 64),
                 case("sparse_map_100x40", small, (95, 34), 64)]}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
