"""`bench.py`'s plain run, --full and --dump-outputs.

CPU: the options parse, and dump_outputs writes float32 arrays, cuts an
array over its share of the byte limit to the same seeded sample every time
and never writes more than the limit.

GPU: one plain run at 128^2 prints a result line with the headline keys and
none of the --full legs, and the arrays it dumps are what a caller of the
timed path reads back: the same seeded grid, trajectory and initial state run
through GridContext.loop_run in this process give the same values and
actions bit for bit and the same belief (rel 1e-5, the suite's bound for the
belief across launch shapes: the bench runs warm-up and timed steps as two
launches, this test as one).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_rel_close

BENCH = os.path.join(ROOT, "bench.py")
HEAD_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step",
             "steps", "warmup", "n_gpus", "config", "full"}
FULL_KEYS = {"roofline", "kernels", "dense_path", "config4", "plan_step", "pbvi", "rollout",
             "cpu_baseline", "mdp_solve", "fib_sweep", "weak_rank_share"}


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_options_parse():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "some/dir"])
    assert a.full and a.dump_outputs == "some/dir"


def test_dump_outputs_small_arrays_whole(tmp_path):
    bench = _bench()
    b = np.linspace(0, 1, 1000, dtype=np.float32)
    A = (np.arange(1000) % 9).astype(np.uint8)
    n = bench.dump_outputs(str(tmp_path / "o"), {"belief": b, "actions": A})
    assert n == {"belief": 1000, "actions": 1000}
    got_b = np.load(tmp_path / "o" / "belief.npy", allow_pickle=False)
    got_a = np.load(tmp_path / "o" / "actions.npy", allow_pickle=False)
    assert got_b.dtype == np.float32 and got_a.dtype == np.float32
    np.testing.assert_array_equal(got_b, b)
    np.testing.assert_array_equal(got_a, A.astype(np.float32))


def test_dump_outputs_samples_within_the_limit(tmp_path):
    bench = _bench()
    x = np.arange(5000, dtype=np.float32)
    y = np.arange(100, dtype=np.float32)
    limit = 4000  # bytes: 2000 per array = 500 float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y}, limit=limit)
    xa = np.load(tmp_path / "a" / "x.npy")
    xb = np.load(tmp_path / "b" / "x.npy")
    assert xa.size == 500 and np.all(np.diff(xa) > 0)  # a sorted sample without repeats
    np.testing.assert_array_equal(xa, xb)               # the same one every run
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "y.npy"), y)
    assert xa.nbytes + y.nbytes <= limit


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    bench = _bench()
    N, steps, warm = 128, 6, 3
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warm), "--size", str(N), "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert HEAD_KEYS <= set(res) and not (FULL_KEYS & set(res)), sorted(res)
    assert res["full"] is False and res["steps"] == steps and res["belief_mass_ok"] is True
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N * N / (res["ms_per_step"] * 1e-3), rel=1e-9)

    # the bench's inputs, rebuilt here (bench.main: seed = grid height, trajectory seed 42)
    grid = S.synth_grid(N, N, seed=N)
    goal = S.synth_goal(grid)
    us, zs, _ = S.synth_trajectory(grid, warm + steps, seed=42)
    with P.GridContext(grid, goal, gamma=bench.GAMMA, device=0) as ctx:
        ctx.model_generate()
        ctx.belief_set(S.uniform_belief(grid))
        ctx.mdp_reset()
        ctx.loop_run(us, zs)
        b = ctx.belief_get()
        J, A = ctx.mdp_get()
    got = {k: np.load(out / f"{k}.npy", allow_pickle=False)
           for k in ("belief", "values", "actions")}
    assert all(v.dtype == np.float32 and v.shape == (N * N,) for v in got.values())
    np.testing.assert_array_equal(got["values"].view(np.uint32), J.view(np.uint32))
    np.testing.assert_array_equal(got["actions"], A.astype(np.float32))
    assert_rel_close(got["belief"], b, rel=1e-5, msg="dumped belief")
