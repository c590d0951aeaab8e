"""Live map and goal updates at 1024^2, host clock around calls
that end in a device synchronise: one 16 x 16 obstacle patch and one goal move,
each timed
  (a) as pp2_map_update / pp2_goal_set on the patch path,
  (b) as the same call with PP2_TUNE_MAP_INCREMENTAL 0 (regenerate + rebuild),
  (c) as what a context without these calls needs for the same effect:
      pp2_destroy + pp2_create + pp2_model_generate on the new map (which also
      loses belief, values, alphas and tuning),
alternating a, b, c within every repetition after a warm-up round, so that
drift on a shared host hits all three alike; min / median / max are printed.
Then a cold pp2_mdp_solve against a warm pp2_mdp_resolve after the patch.

  python tools/map_update_timing.py [--n 1024] [--reps 9] [--solve-reps 3]
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
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--solve-reps", type=int, default=3)
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
    maps = [grid.copy(), grid.copy()]
    maps[1][y0:y0 + 16, x0:x0 + 16] = block
    free = np.argwhere(grid == 0)
    goal2 = (int(free[len(free) // 3][1]), int(free[len(free) // 3][0]))

    def fresh(g, gl):
        c = P.GridContext(g, gl, gamma=0.95)
        c.model_generate()
        c.synchronize()
        return c

    a = fresh(grid, goal)
    b = fresh(grid, goal)
    b.set_tuning(b.TUNE_MAP_INCREMENTAL, 0)
    box = [fresh(grid, goal)]

    def recreate(g, gl):
        box[0].close()
        box[0] = fresh(g, gl)

    out = {"n": N, "dict_entries": a.model_dict_info()[0]}
    for what in ("patch_16x16", "goal_move"):
        t = {"a": [], "b": [], "c": []}
        for rep in range(args.reps + 1):  # round 0: warm-up
            k = (rep + 1) % 2  # the state to move to: alternates, every call changes the model
            if what == "patch_16x16":
                p = block if k else orig
                ra = timed(lambda: a.map_update(p, x0, y0))
                rb = timed(lambda: b.map_update(p, x0, y0))
                rc = timed(lambda: recreate(maps[k], goal))
            else:
                gl = goal2 if k else goal
                ra = timed(lambda: a.goal_set(gl))
                rb = timed(lambda: b.goal_set(gl))
                rc = timed(lambda: recreate(grid, gl))
            if rep:
                t["a"].append(ra)
                t["b"].append(rb)
                t["c"].append(rc)
        out[what] = {k: stats(v) for k, v in t.items()}
        print(f"{what}: (a) patch path {out[what]['a']}  (b) knob 0 {out[what]['b']}  "
              f"(c) destroy + create + generate {out[what]['c']}", flush=True)
    out["update_info_a"] = a.map_update_info()
    out["update_info_b"] = b.map_update_info()
    assert out["update_info_a"][2] == 0 and out["update_info_b"][1] == 0, out

    # cold solve of the patched map against the warm re-solve after the patch
    cold, warm = [], []
    sw = {}
    for rep in range(args.solve_reps + 1):
        a.map_update(orig, x0, y0)
        a.mdp_solve()
        a.map_update(block, x0, y0)
        a.synchronize()
        r = {}
        tw = timed(lambda: r.setdefault("warm", a.mdp_resolve()))
        tc = timed(lambda: r.setdefault("cold", a.mdp_solve()))
        if rep:
            warm.append(tw)
            cold.append(tc)
        sw = {"warm_sweeps": r["warm"][0], "cold_sweeps": r["cold"][0]}
    out["solve"] = {"cold": stats(cold), "warm": stats(warm), **sw}
    print(f"solve after the patch: cold mdp_solve {out['solve']['cold']} ({sw['cold_sweeps']} "
          f"sweeps), warm mdp_resolve {out['solve']['warm']} ({sw['warm_sweeps']} sweeps)",
          flush=True)
    print(json.dumps(out), flush=True)
    for c in (a, b, box[0]):
        c.close()


if __name__ == "__main__":
    main()
