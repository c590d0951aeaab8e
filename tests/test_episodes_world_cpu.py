"""CPU: the reference of episodes whose world differs from the believed map and
of resumed segments (tests/episodes_world_reference.py), and the ABI and Python
mirror of pp2_episodes_set_world / pp2_episodes_resume -- no GPU.

The case is 9 x 13, all free, the world with a wall at x = 6, y = 2..6, goal
(11, 4), gamma 0.95, seed 7, horizon 40, 16 starts in columns 0..2, QMDP over
fp64 Q planes rounded to fp32.

* with the world being the believed model the reference equals
  ``R.run_batch``, ``AR.run_alpha_batch`` and ``LR.run_lookahead_batch`` bit for
  bit (the lookahead over its own tests' cut: 12 steps, eight starts);
* its own split run, 12 steps and then 28 resumed, equals the 40-step run;
* a stale map costs goals: episodes that reach the goal, out of 16, under
  (believed, world) = (stale, stale) 13, (stale, true) 4, (true, true) 9 with
  these starts -- the test asserts that (stale, true) is below both others;
* include/pp2.h, ``_lib`` and the built library carry the two new entries, the
  ABI version stays 4, and both refuse a null batch.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import episodes_alpha_reference as AR
import episodes_lookahead_reference as LR
import episodes_reference as R
import episodes_world_reference as WR


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {k}")


RESULTS = ("steps", "status", "cost", "final_cell", "beliefs")
TRACES = ("actions", "observations", "cells")


@pytest.fixture(scope="module")
def case(oracle):
    from path_planning_2d_amd import synthetic as S
    c = WR.world_case("9x13", believed_extra=False)
    assert not c["believed"].any() and (c["starts"] % 13 <= 2).all() and len(c["starts"]) == 16
    H, W = c["believed"].shape
    models, solved = {}, {}
    for name, grid in (("stale", c["believed"]), ("true", c["world"])):
        m = R.Model(grid, c["goal"], c["gamma"])
        J, A, _, _ = oracle.mdp_solve(H, W, m.gamma, m.T, m.C)
        models[name] = m
        solved[name] = (R.q_planes_f64(m.T, m.C, J, m.gamma, H, W).astype(np.float32), A)
    return c, models, solved, S.uniform_belief(c["believed"])


def test_own_world_is_the_plain_episode(oracle, case):
    c, models, solved, b0 = case
    m = models["stale"]
    H, W = m.H, m.W
    Q, A = solved["stale"]
    hz, seed, starts = c["horizon"], c["seed"], c["starts"]
    for pol, ctl, key in ((R.QMDP, WR.qmdp_control(m, Q), "qsums"),
                          (R.MODE, WR.mode_control(m, A), "mode_cells")):
        want = R.run_batch(m, Q, A, b0, starts, pol, hz, seed)
        got = WR.run_batch(m, m, ctl, b0, starts, hz, seed)
        assert_same(got, want, RESULTS + TRACES + (key,), f"policy {pol}")
        assert (want["status"] == 1).any() and (want["status"] == 0).any()
    _, _, Rw = oracle.model_pomdp(m.grid, m.goal)
    al, _, _ = oracle.fib_solve(H, W, m.gamma, m.T, m.L, Rw)
    al, act = np.ascontiguousarray(al.T), np.arange(9, dtype=np.uint8)
    want = AR.run_alpha_batch(m, al, act, b0, starts, hz, seed)
    got = WR.run_batch(m, m, WR.alpha_control(m, al, act), b0, starts, hz, seed)
    assert_same(got, want, RESULTS + TRACES + ("qsums", "best_index", "best_sum"), "fib")


def test_own_world_is_the_plain_lookahead_episode(oracle, case):
    """... over the first LR.LOOK_HORIZON = 12 steps of eight starts, the cut the
    lookahead's own tests make: its reference costs 144 belief updates a step."""
    c, models, solved, b0 = case
    m = models["stale"]
    hz, seed, starts = LR.LOOK_HORIZON, c["seed"], c["starts"][:8]
    _, _, Rw = oracle.model_pomdp(m.grid, m.goal)
    al, _, _ = oracle.fib_solve(m.H, m.W, m.gamma, m.T, m.L, Rw)
    al = np.ascontiguousarray(al.T)
    want = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, seed)
    got = WR.run_batch(m, m, WR.look_control(m, Rw, al), b0, starts, hz, seed)
    assert_same(got, want, RESULTS + TRACES + ("qsums", "q", "rewards", "leaf_max", "leaf_index"),
                "fib-lookahead")


def test_split_run_equals_the_long_run(case):
    c, models, solved, b0 = case
    mp, mw = models["stale"], models["true"]
    ctl = WR.qmdp_control(mp, solved["stale"][0])
    whole = WR.run_batch(mp, mw, ctl, b0, c["starts"], 40, c["seed"])
    first = WR.run_batch(mp, mw, ctl, b0, c["starts"], 12, c["seed"])
    second = WR.run_batch_segment(mp, mw, ctl, first["states"], 28, c["seed"])
    assert_same(second, whole, RESULTS, "12 + 28")
    for k in TRACES + ("qsums",):
        both = np.concatenate([first[k], second[k]])
        # rows of a segment that an episode finished before hold the fill values
        np.testing.assert_array_equal(both, whole[k], err_msg=k)
    assert (first["status"] == 0).any() and ((second["steps"] > 12) & (second["status"] == 1)).any()


def test_a_stale_map_costs_goals(case):
    c, models, solved, b0 = case
    reached = {}
    for believed, world in (("stale", "stale"), ("stale", "true"), ("true", "true")):
        mp, mw = models[believed], models[world]
        r = WR.run_batch(mp, mw, WR.qmdp_control(mp, solved[believed][0]), b0, c["starts"],
                         c["horizon"], c["seed"])
        reached[believed, world] = int((r["status"] == 1).sum())
        assert not (r["status"] == 2).any()
    print(reached)
    assert reached["stale", "true"] < reached["stale", "stale"]
    assert reached["stale", "true"] < reached["true", "true"]


def test_world_goal_off_the_grid_is_no_goal(case):
    c, models, solved, b0 = case
    mp = models["stale"]
    mw = R.Model(c["world"], (-1, 4), c["gamma"], T=models["true"].T, L=models["true"].L,
                 C=models["true"].C)
    assert WR.goal_cell(mw) == -1
    r = WR.run_batch(mp, mw, WR.qmdp_control(mp, solved["stale"][0]), b0, c["starts"][:4], 6, 1)
    assert (r["status"] == 0).all() and (r["steps"] == 6).all()


def test_header_mirror_and_library():
    from path_planning_2d_amd import EpisodeBatch, _lib
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    flat = re.sub(r"\s+", " ", text)
    assert "int pp2_episodes_set_world(pp2_episodes* ep, pp2_ctx* world);" in flat
    assert "int pp2_episodes_resume(pp2_episodes* ep, int policy, uint64_t seed);" in flat
    for i, name in enumerate(("MODE", "QMDP", "FIB", "PBVI", "FIB_LOOKAHEAD", "PBVI_LOOKAHEAD")):
        assert re.search(rf"^#define PP2_EPISODE_{name} {i}\b", text, re.M), name
    assert "The world (pp2_episodes_set_world)" in text
    assert "Resumed segments (pp2_episodes_resume)" in text
    assert len(_lib.SIGNATURES["pp2_episodes_set_world"]) == 2
    assert len(_lib.SIGNATURES["pp2_episodes_resume"]) == 3
    assert callable(EpisodeBatch.set_world) and callable(EpisodeBatch.resume)
    path = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "libpp2_hip.so")
    assert os.path.exists(path), "the library is not built"
    lib = C.CDLL(path)
    lib.pp2_episodes_set_world.argtypes = [C.c_void_p, C.c_void_p]
    lib.pp2_episodes_resume.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    assert lib.pp2_abi_version() == 4
    assert lib.pp2_episodes_set_world(None, None) == 1   # PP2_EINVAL
    assert lib.pp2_episodes_resume(None, 1, 0) == 1
    assert _lib.STATUS_NAMES[1] == "PP2_EINVAL"


def test_resume_validates_before_the_library(monkeypatch):
    from path_planning_2d_amd import EpisodeBatch
    from path_planning_2d_amd import episodes as E
    ep = EpisodeBatch.__new__(EpisodeBatch)
    ep._h, ep.cells, ep.episodes = None, 12, 3
    called = []
    monkeypatch.setattr(E, "call", lambda name, *a: called.append((name, a[1])))
    for bad in ("greedy", 1, None, "QMDP"):
        with pytest.raises(ValueError):
            ep.resume(bad)
    with pytest.raises(ValueError):
        ep.resume("qmdp", seed=-1)
    assert not called
    for i, name in enumerate(("mode", "qmdp", "fib", "pbvi", "fib-lookahead", "pbvi-lookahead")):
        assert ep.resume(name, seed=3) is ep
        assert called[-1] == ("pp2_episodes_resume", i)
        assert ep.lookahead == (i >= 4) and (ep.alpha_set is None) == (i < 2)
