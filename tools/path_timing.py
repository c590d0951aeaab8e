"""Wall time of pp2_path_solve, host clock around the call (it
ends in a device synchronise), with its rounds, launches and polls, and next to
it pp2_mdp_solve on the same grid from the same run -- the yardstick a user
would reach for: the field replaces an MDP solve as the per-cell policy.

Grids: sparse_map_100x40; 256^2, 1024^2 and 2048^2 synthetic at 20 %
obstacles; a 1025 x 1024 serpentine, the adversarial case (one corridor of
about half a million cells, so rounds of the order of its length over the tile
edge).  Per grid: one warm-up call, then --reps timed calls of each solve,
alternating; min / median / max are reported.

  python tools/path_timing.py [--reps 7] [--mdp-reps 3] [--out FILE.json] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4),
            "max_ms": round(max(v), 4), "n": len(v)}


def serpentine(H, W):
    import numpy as np
    g = np.zeros((H, W), np.uint8)
    for k, y in enumerate(range(1, H, 2)):
        g[y, :] = 1
        g[y, W - 1 if k % 2 == 0 else 0] = 0
    return g


def cases():
    import numpy as np
    from path_planning_2d_amd import synthetic as S
    yield "sparse_map_100x40", np.load(os.path.join(ROOT, "tests", "golden", "maps",
                                                    "sparse_map_100x40.npy")), (95, 34)
    for n in (256, 1024, 2048):
        g = S.synth_grid(n, n, seed=n)
        yield f"synth_{n}x{n}", g, S.synth_goal(g)
    yield "serpentine_1025x1024", serpentine(1025, 1024), (0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mdp-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import path_planning_2d_amd as P
    out = {}
    for name, grid, goal in cases():
        if args.only and args.only != name:
            continue
        H, W = grid.shape
        with P.GridContext(grid, goal, gamma=0.95) as ctx:
            ctx.model_generate()
            ctx.synchronize()
            tp, tm = [], []
            res, sweeps = None, None
            for rep in range(args.reps + 1):  # round 0: warm-up
                ms, res = timed(ctx.path_solve)
                assert res[1], f"{name}: the field did not settle"
                if rep:
                    tp.append(ms)
                if args.mdp_reps and rep <= args.mdp_reps:
                    ms, sweeps = timed(ctx.mdp_solve)
                    if rep:
                        tm.append(ms)
            info = ctx.path_info()
        ntiles = -(-H // info["tile_rows"]) * -(-W // info["tile_cols"])
        out[name] = {"H": H, "W": W, "free": int((grid != 1).sum()), "reached": res[2],
                     "tiles": ntiles, "rounds": info["rounds"], "launches": info["launches"],
                     "polls": info["polls"], "path_solve": stats(tp),
                     "us_per_launch": round(1e3 * statistics.median(tp) / info["launches"], 3),
                     "mdp_solve": stats(tm) if tm else None,
                     "mdp_sweeps": sweeps[0] if sweeps else None}
        print(name, json.dumps(out[name]), flush=True)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
