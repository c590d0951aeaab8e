"""Wall time of a warm pp2_path_resolve against a cold pp2_path_solve after the
same map update, on the same context in the same run (DESIGN.md §2.3 "Warm
re-solve"): host clock around the call (each ends in a device synchronise).

Grids: sparse_map_100x40; 256^2 and 1024^2 synthetic at 20 % obstacles; the
1025 x 1024 serpentine.  Updates on each: a 16 x 16 obstacle patch on the traced
path (from (11, 6) on sparse_map_100x40, else from the reachable cell farthest
from the goal), a 1-cell obstacle on it, and a freed 16 x 16 patch around the
occupied cell nearest to the path's middle.  Per update: one warm-up and --reps
timed repetitions of

    map_update(patch), path_resolve   (timed; must run warm)
    map_update(old cells), path_solve (the map and the field restored)
    map_update(patch), path_solve     (timed, cold)
    map_update(old cells), path_solve

min / median / max of each, the rounds of each phase, ``raised``, and the two
fields compared bit for bit once.

  python tools/path_resolve_timing.py [--reps 7] [--out FILE.json] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.path_timing import serpentine, stats, timed  # noqa: E402


def cases():
    import numpy as np
    from path_planning_2d_amd import synthetic as S
    yield "sparse_map_100x40", np.load(os.path.join(ROOT, "tests", "golden", "maps",
                                                    "sparse_map_100x40.npy")), (95, 34), (11, 6)
    for n in (256, 1024):
        g = S.synth_grid(n, n, seed=n)
        yield f"synth_{n}x{n}", g, S.synth_goal(g), None
    yield "serpentine_1025x1024", serpentine(1025, 1024), (0, 0), None


def window(grid, cx, cy, n, keep):
    """(x0, y0, old cells) of the n x n window around (cx, cy), on the grid and
    clear of the cell ``keep`` (the goal)."""
    H, W = grid.shape
    x0 = min(max(cx - n // 2, 0), W - n)
    y0 = min(max(cy - n // 2, 0), H - n)
    if x0 <= keep[0] < x0 + n and y0 <= keep[1] < y0 + n:
        raise ValueError("the window would cover the goal")
    return x0, y0, grid[y0:y0 + n, x0:x0 + n].copy()


def updates(grid, goal, mid):
    """name -> (x0, y0, patch, old cells)."""
    import numpy as np
    H, W = grid.shape
    mx, my = mid % W, mid // W
    x0, y0, old = window(grid, mx, my, 16, goal)
    yield "obstacle_16x16", (x0, y0, np.ones_like(old), old)
    yield "obstacle_1", (mx, my, np.ones((1, 1), np.uint8), grid[my:my + 1, mx:mx + 1].copy())
    ys, xs = np.nonzero(grid == 1)
    k = int(np.argmin(np.maximum(np.abs(xs - mx), np.abs(ys - my))))
    x0, y0, old = window(grid, int(xs[k]), int(ys[k]), 16, goal)
    yield "freed_16x16", (x0, y0, np.zeros_like(old), old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import numpy as np
    import path_planning_2d_amd as P
    out = {}
    for name, grid, goal, start in cases():
        if args.only and args.only != name:
            continue
        H, W = grid.shape
        out[name] = {"H": H, "W": W, "updates": {}}
        with P.GridContext(grid, goal, gamma=0.95) as ctx:
            base = ctx.path_solve()
            assert base[1], f"{name}: the field did not settle"
            D, _ = ctx.path_get()
            if start is None:
                far = int(np.argmax(np.where(np.isfinite(D), D, -1.0)))
                start = (far % W, far // W)
            cells, _ = ctx.path_trace(start)
            mid = int(cells[len(cells) // 2])
            out[name].update(reached=base[2], cold_rounds=base[0], path_cells=len(cells))
            for uname, (x0, y0, patch, old) in updates(grid, goal, mid):
                tw, tc = [], []
                fields = {}
                for rep in range(args.reps + 1):  # round 0: warm-up
                    for which in ("warm", "cold"):
                        ctx.map_update(patch, x0=x0, y0=y0)
                        if which == "warm":
                            ms, res = timed(ctx.path_resolve)
                            assert res[1] and res[3], f"{name} {uname}: not warm"
                            info, rinfo = ctx.path_info(), ctx.path_resolve_info()
                            warm_res = res
                        else:
                            ms, res = timed(ctx.path_solve)
                            assert res[1]
                            cinfo = ctx.path_info()
                        if rep:
                            (tw if which == "warm" else tc).append(ms)
                        else:
                            fields[which] = ctx.path_get()
                        ctx.map_update(old, x0=x0, y0=y0)
                        assert ctx.path_solve()[1]
                same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8))
                           for a, b in zip(fields["warm"], fields["cold"]))
                assert same, f"{name} {uname}: the warm field differs from the cold one"
                r = {"rect": [x0, y0, int(patch.shape[1]), int(patch.shape[0])],
                     "seed_cells": rinfo["seed_cells"], "raised": rinfo["raised"],
                     "raise_rounds": rinfo["raise_rounds"], "relax_rounds": rinfo["relax_rounds"],
                     "reached": warm_res[2], "launches": info["launches"], "polls": info["polls"],
                     "cold_rounds": cinfo["rounds"], "cold_launches": cinfo["launches"],
                     "cold_polls": cinfo["polls"], "bit_equal": bool(same),
                     "path_resolve": stats(tw), "path_solve": stats(tc),
                     "warm_over_cold": round(statistics.median(tw) / statistics.median(tc), 3)}
                out[name]["updates"][uname] = r
                print(name, uname, json.dumps(r), flush=True)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
