"""CPU: the batched closed-loop episodes' reference (tests/episodes_reference.py)
and the argument checks of ``EpisodeBatch`` -- no GPU.

* the counter-based generator is synthetic's SplitMix64 stream of the
  episode's key, cut to 24 bits;
* the pinned Q-dot order agrees with an fp64 dot within the project's parity
  budget (rel 1e-5; every term is >= 0, so there is no cancellation);
* the main parity case of tests/test_gpu_episodes.py exercises every path
  (goal reached, full horizon, an early stop, tied maxima), asserted on the
  reference alone;
* ``EpisodeBatch`` rejects bad arguments before it touches the library.
"""
import numpy as np
import pytest

import episodes_reference as R


def test_uniform_is_the_splitmix_stream_of_the_key():
    from path_planning_2d_amd import synthetic as S
    for seed in (0, 2024, (1 << 64) - 5):
        for e in (0, 1, 599, 131071):
            rng = S.SplitMix64(R.episode_key(seed, e))
            for d in range(6):
                x = int(rng.next())
                want = np.float32(x >> 40) * np.float32(2.0 ** -24)
                got = R.uniform(seed, e, d)
                assert got == want and 0.0 <= got < 1.0, (seed, e, d)
    # mix is synthetic._mix
    with np.errstate(over="ignore"):
        assert R.mix(12345) == int(S._mix(np.uint64(12345)))


@pytest.mark.parametrize("H,W", [(40, 100), (97, 131), (1, 7), (5, 1)])
def test_pinned_qdot_agrees_with_fp64(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    wp = R.row_stride(W)
    b = rng.random(H * W).astype(np.float32) * np.float32(2.0)
    b[rng.random(H * W) < 0.3] = 0
    Q = (rng.random((H * W, 9)) * 40).astype(np.float32)
    S = R.qdot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(Q.T, H, W, wp))
    want = b.astype(np.float64) @ Q.astype(np.float64)
    assert S.dtype == np.float32 and S.shape == (9,)
    assert np.all(np.abs(S - want) <= 1e-5 * np.abs(want)), (S, want)


@pytest.fixture(scope="module")
def main_runs(oracle):
    case = R.main_case()
    grid = case["grid"]
    H, W = grid.shape
    m = R.Model(grid, case["goal"], case["gamma"])
    J, A, _, _ = oracle.mdp_solve(H, W, m.gamma, m.T, m.C)
    Q = R.q_planes_f64(m.T, m.C, J, m.gamma, H, W).astype(np.float32)
    runs = {p: R.run_batch(m, Q, A, case["b0"], case["starts"], p, case["horizon"], case["seed"])
            for p in (R.MODE, R.QMDP)}
    return case, m, runs


def test_main_case_exercises_every_path(main_runs):
    case, m, runs = main_runs
    E, hz = len(case["starts"]), case["horizon"]
    assert E == 32 and case["starts"][0] == 611
    q = runs[R.QMDP]
    reached = int((q["status"] == 1).sum())
    full = int(((q["status"] == 0) & (q["steps"] == hz)).sum())
    print(f"QMDP: {reached} reached, {full} full horizon, earliest stop "
          f"{int(q['steps'][q['status'] == 1].min())}")
    assert reached >= 6 and full >= 6
    assert (q["steps"][q["status"] == 1] < hz).any()          # an early stop
    md = runs[R.MODE]
    print(f"mode: {int((md['status'] == 1).sum())} reached, "
          f"{int((md['status'] == 0).sum())} full horizon, {int(md['ties'].sum())} tie steps")
    assert int(md["ties"].sum()) >= 50
    for r in runs.values():
        assert not (r["status"] == 2).any()
        # steps not taken keep their fill values; steps taken are recorded
        for e in range(E):
            n = int(r["steps"][e])
            assert (r["actions"][:n, e] <= 8).all() and (r["actions"][n:, e] == 255).all()
            assert (r["observations"][:n, e] <= 15).all() and (r["cells"][n:, e] == -1).all()
            if n:
                assert r["cells"][n - 1, e] == r["final_cell"][e]
            top = r["beliefs"][e].max()
            assert n == 0 or 1.0 <= top < 2.0
        assert ((r["final_cell"] == m.goal_cell) == (r["status"] == 1)).all()


def test_reference_edges(oracle):
    """Start on the goal: no step; b0 = 0: the belief is lost at once."""
    case = R.main_case()
    m = R.Model(case["grid"], case["goal"], case["gamma"])
    hw = m.H * m.W
    Q = np.ones((hw, 9), np.float32)
    A = np.full(hw, 4, np.uint8)
    r = R.run_batch(m, Q, A, case["b0"], [m.goal_cell], R.QMDP, 4, 1)
    assert r["steps"][0] == 0 and r["status"][0] == 1 and r["cost"][0] == 0
    assert np.array_equal(r["beliefs"][0], case["b0"])
    r = R.run_batch(m, Q, A, np.zeros(hw, np.float32), [611, 7], R.MODE, 4, 1)
    assert (r["status"] == 2).all() and (r["steps"] == 1).all()
    assert (r["mode_cells"][0] == 0).all() and (r["mode_cells"][1:] == -1).all()


def test_episode_batch_validates_before_the_library():
    from path_planning_2d_amd import EpisodeBatch

    class NoCtx:  # any use of the context would raise AttributeError
        pass

    for ep, hz in ((0, 8), (131073, 8), (4, 0), (4, 4097)):
        with pytest.raises(ValueError):
            EpisodeBatch(NoCtx(), ep, hz)
    ok_b0 = np.full(12, 1 / 12, np.float32)
    check = EpisodeBatch.check_run_args
    pol, b0, st, seed = check(12, 3, "qmdp", ok_b0, [0, 5, 11], 7)
    assert pol == 1 and b0.dtype == np.float32 and st.dtype == np.int32 and seed == 7
    assert check(12, 3, 0, ok_b0, [0, 5, 11], 0)[0] == 0
    bad_neg, bad_nan, bad_m0 = ok_b0.copy(), ok_b0.copy(), ok_b0.copy()
    bad_neg[3], bad_nan[3], bad_m0[3] = -0.1, np.nan, -0.0
    for args in ((12, 3, "greedy", ok_b0, [0, 5, 11], 0),
                 (12, 3, 2, ok_b0, [0, 5, 11], 0),
                 (12, 3, 1, ok_b0[:11], [0, 5, 11], 0),
                 (12, 3, 1, bad_neg, [0, 5, 11], 0),
                 (12, 3, 1, bad_nan, [0, 5, 11], 0),
                 (12, 3, 1, bad_m0, [0, 5, 11], 0),
                 (12, 3, 1, ok_b0, [0, 5, 12], 0),
                 (12, 3, 1, ok_b0, [0, -1, 11], 0),
                 (12, 3, 1, ok_b0, [0, 5], 0),
                 (12, 3, 1, ok_b0, [0.5, 5, 11], 0),
                 (12, 3, 1, ok_b0, [0, 5, 11], -1),
                 (12, 3, 1, ok_b0, [0, 5, 11], 1 << 64)):
        with pytest.raises(ValueError):
            check(*args)


def test_sample_cells_follow_the_belief():
    from path_planning_2d_amd import synthetic as S
    b = np.zeros(50, np.float32)
    b[[3, 17, 40]] = (0.5, 0.25, 0.25)
    c = S.sample_cells(b, 400, seed=9)
    assert c.dtype == np.int32 and set(c.tolist()) == {3, 17, 40}
    assert abs((c == 3).mean() - 0.5) < 0.1
    assert np.array_equal(c, S.sample_cells(b, 400, seed=9))
    with pytest.raises(ValueError):
        S.sample_cells(np.zeros(5, np.float32), 2)
