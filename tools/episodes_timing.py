"""Wall time of batched closed-loop policy episodes (pp2_episodes_*, DESIGN.md
§3.4) on sparse_map_100x40 with the solved J: E = 4096 episodes x horizon 64
under every policy -- mode, QMDP, FIB-greedy (the solved FIB alphas; and
"fibq", the FIB policy fed -Q, which takes QMDP's very steps, so the two
kernels are compared on one workload) and PBVI-greedy (pp2_pbvi_solve at every
--set-size) -- pp2_episodes_run[_alpha] +
pp2_episodes_results after a warm-up run, median / min / max of 7 rounds, per
episode-step and episodes per second -- against, in alternating rounds of the
same process, the host loop the library offered before: BeliefMdpController
driven by synthetic.closed_loop for mode and QMDP (one belief update and one
control call per step), and for PBVI one pp2_belief_update, one pp2_belief_get
and one pp2_pbvi_evaluate per step; 14 episodes of 64 steps each.
--placement lds | global | auto places the belief planes (include/pp2.h
"Placement"); --grid HxW times a synthetic.synth_grid(H, W) with cell (0, 0)
freed and the goal there, as the tests build it, in place of the map -- with
"global" or "auto" any size, e.g. 256x256, which LDS does not hold.
--compare-lds also times an LDS batch of the same runs in the same alternating
rounds and reports the ratio (the price of the memory path, where both fit).
An episode that reaches the goal stops early, so the device's steps are
counted from the results; the host loop always runs its 64.  A PBVI entry also
reports the implied alpha read rate, K * NP * 4 bytes per episode-step.
--policies also takes "fib-lookahead" and "pbvi-lookahead" (the latter an entry
per --set-size), the one-step lookahead over the set; they have no host loop.
With --placement global | auto they go through the call that follows the
placement (``placed=True``); the --compare-lds batch runs the plain call.
--episodes / --horizon replace E = 4096 and horizon 64 (a lookahead step on a
large grid costs milliseconds per workgroup).

    python tools/episodes_timing.py [--rounds N] [--no-host] [--out FILE]
                                    [--placement lds|global|auto] [--grid HxW] [--compare-lds]
                                    [--policies mode,qmdp,fib,fibq,pbvi,fib-lookahead,pbvi-lookahead]
                                    [--set-size 21,128,500] [--episodes E] [--horizon N]
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
ap.add_argument("--policies", default="mode,qmdp,fib,fibq,pbvi")
ap.add_argument("--set-size", default="21", help="PBVI belief set sizes, comma separated")
ap.add_argument("--placement", default="lds", choices=("lds", "global", "auto"))
ap.add_argument("--grid", default="", help="HxW: a synthetic grid with goal (0, 0)")
ap.add_argument("--compare-lds", action="store_true",
                help="time an LDS batch too, in the same rounds")
ap.add_argument("--episodes", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=64)
args = ap.parse_args()

E, HORIZON, HOST_EPISODES = args.episodes, args.horizon, 8
LOOKAHEAD = ("fib-lookahead", "pbvi-lookahead")
# a lookahead run follows the placement through the placed call; on an LDS
# batch it is the old call, which the tool then keeps
PLACED = args.placement != "lds"
if args.grid:
    try:
        gh, gw = (int(v) for v in args.grid.lower().split("x"))
    except ValueError:
        sys.exit(f"--grid {args.grid!r}: expected HxW")
    grid = S.synth_grid(gh, gw)
    grid[0, 0] = 0
    goal, name = (0, 0), f"synth_{gh}x{gw}"
else:
    grid = np.load(os.path.join(ROOT, "tests", "golden", "maps", "sparse_map_100x40.npy"),
                   allow_pickle=False)
    goal, name = (95, 34), "sparse_map_100x40"
b0 = S.uniform_belief(grid)
starts = S.sample_cells(b0, E, seed=7)
out = {"map": name, "episodes": E, "horizon": HORIZON, "rounds": args.rounds,
       "placement": args.placement}
policies = [p for p in args.policies.split(",") if p]
for p in policies:
    if p not in ("mode", "qmdp", "fib", "fibq", "pbvi") + LOOKAHEAD:
        sys.exit(f"unknown policy {p!r}")
PBVI = ("pbvi", "pbvi-lookahead")
sizes = [int(s) for s in args.set_size.split(",") if s] if set(PBVI) & set(policies) else []
# the entries timed: a PBVI (or PBVI-lookahead) entry per set size
entries = [p for p in policies if p not in PBVI] + \
    [f"{p}_{s}" for p in PBVI if p in policies for s in sizes]


def stats(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd),
            "max": round(max(v), nd)}


class PbviHostLoop:
    """The PBVI plan step the library offered before: synchronous calls, the
    belief through the host."""

    def __init__(self, ctx):
        self.ctx = ctx

    def step(self, action, observation, belief=None):
        if belief is not None:
            self.ctx.belief_set(belief)
        else:
            self.ctx.belief_update(action, observation)
        v, a = self.ctx.pbvi_evaluate(self.ctx.belief_get())
        return int(a[0]), np.float32(v[0])


with P.GridContext(grid, goal, gamma=0.95) as ctx:
    ctx.model_generate()
    out["mdp_sweeps"] = ctx.mdp_solve()[0]
    fib_sets = {}
    if "fib" in policies or "fib-lookahead" in policies:
        out["fib_sweeps"] = ctx.fib_solve()[0]
        fib_sets["fib"] = fib_sets["fib-lookahead"] = ctx.fib_get()
    sets = {}
    for s in sizes:  # solved once; a round only uploads the set it times
        ctx.pbvi_solve(b0, s)
        sets[s] = ctx.pbvi_get()
    NP = grid.shape[0] * ctx.row_stride

    def prepare(entry):
        """-> the policy to run"""
        if entry.startswith(("pbvi_", "pbvi-lookahead_")):
            pol, size = entry.rsplit("_", 1)
            ctx.pbvi_set(*sets[int(size)])
            return pol
        if entry in fib_sets:
            ctx.fib_set(fib_sets[entry])
            return entry if entry in LOOKAHEAD else "fib"
        return entry

    def run(batch, pol, placed):
        """One run of the policy; ``placed``: a lookahead run through the
        call that follows the batch's placement."""
        return batch.run(pol, b0, starts, seed=1, placed=placed and pol in LOOKAHEAD)

    with P.EpisodeBatch(ctx, E, HORIZON, placement=args.placement) as ep:
        out.update(ep.info())
        dev = {p: {"wall_ms": [], "steps": 0, "lds_wall_ms": []} for p in entries}
        lds_ep = P.EpisodeBatch(ctx, E, HORIZON) if args.compare_lds else None
        host = {p: [] for p in entries}
        if "fibq" in entries:
            fib_sets["fibq"] = -ep.run("qmdp", b0, starts, seed=1).qplanes()
        for p in dev:  # warm-up
            run(ep, prepare(p), PLACED).results()
            dev[p]["info"] = ep.info()
            if lds_ep is not None:
                run(lds_ep, prepare(p), False).results()
            if args.placement != "lds":
                dev[p]["info"].update(ep.placement())
        for rnd in range(args.rounds):  # alternate, so drift hits all alike
            for p in dev:
                pol = prepare(p)
                t = time.perf_counter()
                run(ep, pol, PLACED)
                res = ep.results()
                dev[p]["wall_ms"].append((time.perf_counter() - t) * 1e3)
                dev[p]["steps"] = int(res["steps"].sum())
                dev[p]["summary"] = ep.summary()
                if lds_ep is not None:
                    t = time.perf_counter()
                    run(lds_ep, pol, False)
                    lds_res = lds_ep.results()
                    dev[p]["lds_wall_ms"].append((time.perf_counter() - t) * 1e3)
                    if not all(np.array_equal(res[k], lds_res[k]) for k in res):
                        sys.exit(f"{p}: the two placements disagree")
                if not args.no_host and pol != "fib" and pol not in LOOKAHEAD:
                    ctl = PbviHostLoop(ctx) if pol == "pbvi" else \
                        P.BeliefMdpController(ctx, policy=p)
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
                      "summary": d["summary"], "info": d["info"]}
            if d["lds_wall_ms"]:
                out[p]["lds_wall_ms"] = stats(d["lds_wall_ms"])
                out[p]["over_lds"] = round(statistics.median(w)
                                           / statistics.median(d["lds_wall_ms"]), 3)
            if p.startswith("pbvi_"):
                nbytes = int(p[5:]) * NP * 4
                out[p]["alpha_bytes_per_episode_step"] = nbytes
                out[p]["alpha_read_TB_per_s"] = stats(
                    [nbytes * d["steps"] / (x * 1e-3) / 1e12 for x in w], 3)
            if host[p]:
                out[p]["host_loop_us_per_episode_step"] = stats(host[p], 2)
                out[p]["host_loop_over_device"] = round(
                    statistics.median(host[p]) / out[p]["us_per_episode_step"]["median"], 1)
        if lds_ep is not None:
            lds_ep.close()
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
