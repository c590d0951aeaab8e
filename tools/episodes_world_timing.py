"""What a world costs an episode run (pp2_episodes_set_world):
sparse_map_100x40 with the solved J, E = 4096 episodes x horizon 64, QMDP, LDS
placement; the host clock around pp2_episodes_run + pp2_episodes_results.

    (a) no world, this build
    (b) no world, another build of the library (--parent-lib: the parent
        commit's libpp2_hip.so), which launches the same kernel instance
    (c) world = a second context with the same map, this build

One worker process per case (a library is loaded once per process), each with
its context solved and one warm-up run behind it; the driver then asks them for
one timed run each in turn, a, b, c, a, b, c, ..., so drift hits all alike.

    python tools/episodes_world_timing.py [--parent-lib FILE] [--rounds 9] [--out FILE]
        prints one JSON line (and writes it to FILE)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, HORIZON, SEED = 4096, 64, 1


def worker(case: str) -> None:
    import numpy as np
    sys.path.insert(0, ROOT)
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    grid = np.load(os.path.join(ROOT, "tests", "golden", "maps", "sparse_map_100x40.npy"),
                   allow_pickle=False)
    goal = (95, 34)
    b0 = S.uniform_belief(grid)
    starts = S.sample_cells(b0, E, seed=7)
    with P.GridContext(grid, goal, gamma=0.95) as ctx, \
            P.GridContext(grid, goal, gamma=0.95) as twin:
        ctx.model_generate()
        ctx.mdp_solve()
        with P.EpisodeBatch(ctx, E, HORIZON) as ep:
            if case == "c":
                twin.model_generate()
                ep.set_world(twin)
            ep.run("qmdp", b0, starts, seed=SEED).results()  # warm-up
            print("ready", flush=True)
            for line in sys.stdin:
                if line.strip() != "go":
                    break
                t = time.perf_counter()
                ep.run("qmdp", b0, starts, seed=SEED)
                res = ep.results()
                ms = (time.perf_counter() - t) * 1e3
                print(json.dumps({"ms": ms, "steps": int(res["steps"].sum()),
                                  "reached": int((res["status"] == 1).sum())}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    cases = ["a", "c"] if not args.parent_lib else ["a", "b", "c"]
    procs = {}
    try:
        for c in cases:
            env = dict(os.environ)
            if c == "b":
                env["PP2_LIBRARY"] = os.path.abspath(args.parent_lib)
                env["PP2_ALLOW_PARTIAL_ABI"] = "1"  # the parent lacks the newer entry points
            procs[c] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", c],
                                        stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                        env=env)
        for c, p in procs.items():
            if p.stdout.readline().strip() != "ready":
                sys.exit(f"worker {c} did not start")
        raw = {c: [] for c in cases}
        for _ in range(args.rounds):
            for c in cases:
                procs[c].stdin.write("go\n")
                procs[c].stdin.flush()
                raw[c].append(json.loads(procs[c].stdout.readline()))
    finally:
        for p in procs.values():
            if p.stdin:
                p.stdin.close()
            p.wait(timeout=60)
    out = {"map": "sparse_map_100x40", "episodes": E, "horizon": HORIZON, "policy": "qmdp",
           "placement": "lds", "rounds": args.rounds,
           "cases": {"a": "no world, this build", "b": "no world, the parent build",
                     "c": "world = a second context with the same map, this build"}}
    for c in cases:
        ms = [r["ms"] for r in raw[c]]
        out[c] = {"wall_ms": {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3),
                              "max": round(max(ms), 3)},
                  "raw_ms": [round(v, 3) for v in ms], "episode_steps": raw[c][0]["steps"],
                  "reached": raw[c][0]["reached"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
