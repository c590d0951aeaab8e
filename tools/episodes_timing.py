"""Wall time of batched closed-loop policy episodes (pp2_episodes_*, DESIGN.md
§3.4) on sparse_map_100x40 with the solved J: E = 4096 episodes x horizon 64
under both policies -- pp2_episodes_run + pp2_episodes_results after a warm-up
run, median / min / max of 7 rounds, per episode-step and episodes per second
-- against, in alternating rounds of the same process, the host loop the
library offered before: BeliefMdpController driven by synthetic.closed_loop,
8 episodes of 64 steps, one belief update and one control call per step.
An episode that reaches the goal stops early, so the device's steps are
counted from the results; the host loop always runs its 64.

    python tools/episodes_timing.py [--rounds N] [--no-host] [--out FILE]
        prints one JSON line (and writes it to FILE)

Kernel time comes from a separate run under
    rocprofv3 --kernel-trace --stats -- python tools/episodes_timing.py --rounds 1 --no-host
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import path_planning_2d_amd as P
from path_planning_2d_amd import synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()

E, HORIZON, HOST_EPISODES = 4096, 64, 8
grid = np.load(os.path.join(ROOT, "tests", "golden", "maps", "sparse_map_100x40.npy"),
               allow_pickle=False)
goal = (95, 34)
b0 = S.uniform_belief(grid)
starts = S.sample_cells(b0, E, seed=7)
out = {"map": "sparse_map_100x40", "episodes": E, "horizon": HORIZON, "rounds": args.rounds}


def stats(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd),
            "max": round(max(v), nd)}


with P.GridContext(grid, goal, gamma=0.95) as ctx:
    ctx.model_generate()
    out["mdp_sweeps"] = ctx.mdp_solve()[0]
    with P.EpisodeBatch(ctx, E, HORIZON) as ep:
        out.update(ep.info())
        dev = {p: {"wall_ms": [], "steps": 0} for p in ("mode", "qmdp")}
        host = {p: [] for p in ("mode", "qmdp")}
        for p in dev:  # warm-up
            ep.run(p, b0, starts, seed=1).results()
        for rnd in range(args.rounds):  # alternate, so drift hits all alike
            for p in dev:
                t = time.perf_counter()
                ep.run(p, b0, starts, seed=1)
                res = ep.results()
                dev[p]["wall_ms"].append((time.perf_counter() - t) * 1e3)
                dev[p]["steps"] = int(res["steps"].sum())
                dev[p]["summary"] = ep.summary()
                if not args.no_host:
                    ctl = P.BeliefMdpController(ctx, policy=p)
                    t = time.perf_counter()
                    n = 0
                    for h in range(HOST_EPISODES // args.rounds + 1):
                        ms, _, _ = S.closed_loop(grid, b0, ctl.step, HORIZON,
                                                 seed=100 + rnd * 16 + h)
                        n += len(ms)
                    host[p].append((time.perf_counter() - t) * 1e6 / n)
        for p, d in dev.items():
            w = d["wall_ms"]
            out[p] = {"wall_ms": stats(w), "episode_steps": d["steps"],
                      "us_per_episode_step": stats([x * 1e3 / d["steps"] for x in w], 5),
                      "episodes_per_s": stats([E / (x * 1e-3) for x in w], 0),
                      "summary": d["summary"]}
            if host[p]:
                out[p]["host_loop_us_per_episode_step"] = stats(host[p], 2)
                out[p]["host_loop_over_device"] = round(
                    statistics.median(host[p]) / out[p]["us_per_episode_step"]["median"], 1)
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
