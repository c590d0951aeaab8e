"""Wall time per call (synchronise included) of the control selection
(pp2_mdp_qvalues, pp2_belief_mode, pp2_mdp_control) against the yardstick of
one pp2_mdp_sweep(1) + pp2_synchronize, on the coded and the dense path
(DESIGN.md §3.3).  The bench's synthetic grid after pp2_mdp_solve and a
20-step pp2_loop_run; 200 back-to-back calls per figure after 20 warm-up
calls, 7 alternating rounds, median / min / max in microseconds.

    python tools/control_timing.py [size=1024]      prints one JSON line
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS, ROUNDS = 200, 7
grid = S.synth_grid(N, N, seed=N)
goal = S.synth_goal(grid)
us, zs, _ = S.synth_trajectory(grid, 20, seed=42)
lib = _lib.load()
out = {"size": N}
with P.GridContext(grid, goal, gamma=0.95) as ctx:
    ctx.model_generate()
    sweeps, norm = ctx.mdp_solve()
    ctx.belief_set(S.uniform_belief(grid))
    ctx.loop_run(us, zs)
    ctx.synchronize()
    h = ctx.handle
    q = (C.c_float * 9)()
    cell = C.c_int32()
    prob = C.c_float()
    act = C.c_uint8()
    val = C.c_float()

    def t_q():
        assert lib.pp2_mdp_qvalues(h, q) == 0

    def t_mode():
        assert lib.pp2_belief_mode(h, C.byref(cell), C.byref(prob)) == 0

    def t_ctl_q():
        assert lib.pp2_mdp_control(h, 1, C.byref(act), C.byref(val), None) == 0

    def t_ctl_m():
        assert lib.pp2_mdp_control(h, 0, C.byref(act), C.byref(val), C.byref(cell)) == 0

    def t_sweep():
        assert lib.pp2_mdp_sweep(h, 1) == 0
        assert lib.pp2_synchronize(h) == 0

    def t_sync():
        assert lib.pp2_synchronize(h) == 0

    def t_download():
        ctx.belief_get()
        ctx.mdp_get()

    def per_call(fn, reps=REPS):
        for _ in range(20):
            fn()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) / reps * 1e6

    for path, coded in (("coded", 1), ("dense", 0)):
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, coded)
        assert ctx.model_dict_info()[1] == bool(coded)
        res = {k: [] for k in ("qvalues", "belief_mode", "control_qmdp", "control_mode",
                               "sweep1_sync", "sync_only")}
        for _ in range(ROUNDS):  # alternate, so drift hits all alike
            res["qvalues"].append(per_call(t_q))
            res["belief_mode"].append(per_call(t_mode))
            res["control_qmdp"].append(per_call(t_ctl_q))
            res["control_mode"].append(per_call(t_ctl_m))
            res["sweep1_sync"].append(per_call(t_sweep))
            res["sync_only"].append(per_call(t_sync))
        out[path] = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                         "max_us": round(max(v), 2)} for k, v in res.items()}
        out[path]["q"] = [float(x) for x in q]
    ctx.set_tuning(ctx.TUNE_CODED_MODEL, 1)
    out["download_belief_and_mdp_us"] = round(per_call(t_download, 20), 1)
    assert out["coded"]["q"] == out["dense"]["q"]
print(json.dumps(out))
