"""Getting the QV-tree planner back after a live map or goal update at 256^2,
reference_order 1, host clock around calls that end in a
device synchronise.  After one 16 x 16 obstacle patch and after one goal move
(the update itself is not timed: tools/map_update_timing.py), each way is timed
  (a) pp2_planner_refresh on the patch path (k_planner_patch over the
      journalled rectangles),
  (b) pp2_planner_refresh with PP2_TUNE_MAP_INCREMENTAL 0 (the caches read
      again in full),
  (c) pp2_planner_destroy + pp2_planner_create: all a planner without the
      refresh call can do, which also loses the belief and the rand() stream,
alternating a, b, c within every repetition after a warm-up round, so that
drift on a shared host hits all three alike; min / median / max are printed.
The planners of (a) and (b) hold a root (one plan step taken), so their refresh
includes the new root's bounds; (c)'s new planner has none.

  python tools/planner_refresh_timing.py [--n 256] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4),
            "max_ms": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import numpy as np
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    N = args.n
    grid = S.synth_grid(N, N, seed=N)
    goal = S.synth_goal(grid)
    x0 = y0 = N // 2 - 8
    orig = grid[y0:y0 + 16, x0:x0 + 16].copy()
    block = np.ones((16, 16), np.uint8)
    free = np.argwhere(grid == 0)
    goal2 = (int(free[len(free) // 3][1]), int(free[len(free) // 3][0]))
    b0 = S.uniform_belief(grid)
    kw = dict(max_search_tree_depth=3, max_online_iteration=2, reference_order=1)

    ctxs, planners = [], []
    for knob in (1, 0, 1):
        c = P.GridContext(grid, goal, gamma=0.95)
        c.model_generate()
        c.set_tuning(c.TUNE_MAP_INCREMENTAL, knob)
        c.fib_solve(max_sweeps=40)
        p = P.QVTreePlanner(c, **kw)
        p.step(0, 0, b0)
        c.synchronize()
        ctxs.append(c)
        planners.append(p)

    def recreate():
        planners[2].close()
        planners[2] = P.QVTreePlanner(ctxs[2], **kw)
        ctxs[2].synchronize()

    out = {"n": N, "reference_order": 1}
    for what in ("patch_16x16", "goal_move"):
        t = {"a": [], "b": [], "c": []}
        for rep in range(args.reps + 1):  # round 0: warm-up
            k = (rep + 1) % 2  # the state to move to: alternates, every call changes the model
            for c in ctxs:
                if what == "patch_16x16":
                    c.map_update(block if k else orig, x0, y0)
                else:
                    c.goal_set(goal2 if k else goal)
                c.synchronize()
            ra = timed(planners[0].refresh)
            rb = timed(planners[1].refresh)
            rc = timed(recreate)
            if rep:
                t["a"].append(ra)
                t["b"].append(rb)
                t["c"].append(rc)
        out[what] = {k: stats(v) for k, v in t.items()}
        out[what]["a_max_below_c_min"] = out[what]["a"]["max_ms"] < out[what]["c"]["min_ms"]
        print(f"{what}: (a) refresh, patch path {out[what]['a']}  (b) refresh, knob 0 "
              f"{out[what]['b']}  (c) destroy + create {out[what]['c']}  (a) max < (c) min: "
              f"{out[what]['a_max_below_c_min']}", flush=True)
    out["refresh_info_a"] = planners[0].refresh_info()
    out["refresh_info_b"] = planners[1].refresh_info()
    assert out["refresh_info_a"][2] == 0 and out["refresh_info_b"][1] == 0, out
    print(json.dumps(out), flush=True)
    for p in planners:
        p.close()
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
