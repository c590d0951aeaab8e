"""CPU: the lookahead episodes' reference (tests/episodes_lookahead_reference.py),
the C ABI's declarations and the argument checks of
``EpisodeBatch.run_lookahead`` -- no GPU.

* include/pp2.h declares pp2_episodes_run_lookahead / _trace_lookahead and
  ``_lib`` binds them;
* ``run_lookahead`` dispatches and rejects bad arguments before it touches the
  library;
* on the oracle's FIB alphas of the main case, cut to horizon 12 and eight
  starts (``LR.look_case``: the first 8 starts alone reach no goal in 12 steps,
  so two of them are the case's starts near the goal): with a one-vector zero
  set the control is the first argmax of rew; with actions = arange(9) on a
  set that makes gamma * S constant the result is the same; the lookahead
  differs from the greedy FIB policy of ``AR.run_alpha_batch`` in at least one
  step; at least one episode reaches the goal.
"""
import re

import numpy as np
import pytest

import episodes_alpha_reference as AR
import episodes_lookahead_reference as LR
import episodes_reference as R

HORIZON = LR.LOOK_HORIZON
NSTARTS = 8


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_declares_and_lib_binds():
    from path_planning_2d_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    declared = set(re.findall(r"^\s*int\s+(pp2_\w+)\s*\(", text, re.M))
    for name in ("pp2_episodes_run_lookahead", "pp2_episodes_trace_lookahead"):
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["pp2_episodes_run_lookahead"]) == 5
    assert len(_lib.SIGNATURES["pp2_episodes_trace_lookahead"]) == 5
    assert "Lookahead runs (pp2_episodes_run_lookahead)" in text
    assert re.search(r"#define PP2_ABI_VERSION 4\b", text)  # additive: the version stays


def test_run_lookahead_validates_and_dispatches_before_the_library():
    from path_planning_2d_amd import EpisodeBatch

    ep = EpisodeBatch.__new__(EpisodeBatch)  # no context, no library
    ep._h, ep.cells, ep.episodes = None, 12, 3
    seen = []
    ep.run_lookahead = lambda *a, **k: seen.append((a, k)) or ep
    ok_b0 = np.full(12, 1 / 12, np.float32)
    assert ep.run("fib-lookahead", ok_b0, [0, 5, 11], 7) is ep
    assert ep.run("pbvi-lookahead", ok_b0, [0, 5, 11], seed=8) is ep
    assert [s[0][0] for s in seen] == ["fib", "pbvi"] and seen[0][0][3] == 7
    del ep.run_lookahead

    bad_neg, bad_m0 = ok_b0.copy(), ok_b0.copy()
    bad_neg[3], bad_m0[3] = -0.1, -0.0
    for args in (("greedy", ok_b0, [0, 5, 11], 0),
                 ("fib-lookahead", ok_b0, [0, 5, 11], 0),  # run's name, not a set
                 ("qmdp", ok_b0, [0, 5, 11], 0),
                 (2, ok_b0, [0, 5, 11], 0),
                 (-1, ok_b0, [0, 5, 11], 0),
                 (None, ok_b0, [0, 5, 11], 0),
                 (1.0, ok_b0, [0, 5, 11], 0),
                 (True, ok_b0, [0, 5, 11], 0),
                 ("fib", ok_b0[:11], [0, 5, 11], 0),
                 ("fib", bad_neg, [0, 5, 11], 0),
                 (1, bad_m0, [0, 5, 11], 0),
                 ("pbvi", ok_b0, [0, 5, 12], 0),
                 (0, ok_b0, [0, 5], 0),
                 ("fib", ok_b0, [0.5, 5, 11], 0),
                 ("fib", ok_b0, [0, 5, 11], -1),
                 ("pbvi", ok_b0, [0, 5, 11], 1 << 64)):
        with pytest.raises(ValueError):
            ep.run_lookahead(*args)
    with pytest.raises(ValueError):
        ep.run("qmdp-lookahead", ok_b0, [0, 5, 11], 0)


def test_zk_dot_is_the_alpha_dot():
    H, W = 7, 13
    wp = R.row_stride(W)
    rng = np.random.default_rng(2)
    x = rng.random((16, H * W)).astype(np.float32)
    al = rng.normal(size=(11, H * W)).astype(np.float32)
    al[4, 5] = np.inf
    x[:, 5] = 0
    V = LR.adot_pinned_zk(R.pad_plane(x, H, W, wp), R.pad_plane(al, H, W, wp))
    assert V.shape == (16, 11) and np.isnan(V[:, 4]).all()
    for z in range(16):
        want = AR.adot_pinned(R.pad_plane(x[z], H, W, wp), R.pad_plane(al, H, W, wp))
        np.testing.assert_array_equal(bits(V[z]), bits(want))
    np.testing.assert_array_equal(LR.pick_rows(V), [AR.pick(V[z]) for z in range(16)])


@pytest.fixture(scope="module")
def cut_case(oracle):
    case = LR.look_case()
    m, alphas, actions = AR.main_fib_alphas(case)
    _, _, Rw = oracle.model_pomdp(case["grid"], case["goal"])
    starts = case["starts"]
    assert len(starts) == NSTARTS and case["horizon"] == HORIZON
    look = LR.run_lookahead_batch(m, Rw, alphas, case["b0"], starts, HORIZON, case["seed"])
    return case, m, alphas, actions, Rw, starts, look


def test_zero_set_and_constant_tail_pick_the_reward_argmax(cut_case):
    case, m, alphas, actions, Rw, starts, look = cut_case
    H, W = m.H, m.W
    wp = R.row_stride(W)
    hw = H * W
    # stored beliefs of the run, the root first
    beliefs = [np.asarray(case["b0"], np.float32)] + [look["beliefs"][e] for e in range(3)]
    zero = R.pad_plane(np.zeros((1, hw), np.float32), H, W, wp)
    # nine equal vectors: every max over k is the same number whatever the
    # vectors' actions, and gamma * S is what one of them alone gives
    same = R.pad_plane(np.tile(alphas[:1], (9, 1)), H, W, wp)
    one = R.pad_plane(alphas[:1], H, W, wp)
    for b in beliefs:
        u, Q, rew, M, idx = LR.lookahead_control(m, Rw, zero, b)
        assert not M.any() and not idx.any()
        np.testing.assert_array_equal(bits(Q), bits(rew + np.float32(0.0)))
        assert u == AR.pick(rew)
        u9, Q9, rew9, M9, idx9 = LR.lookahead_control(m, Rw, same, b)
        u1, Q1, rew1, M1, _ = LR.lookahead_control(m, Rw, one, b)
        assert not idx9.any()  # the first of equal sums wins
        np.testing.assert_array_equal(bits(M9), bits(M1))
        np.testing.assert_array_equal(bits(Q9), bits(Q1))
        assert u9 == u1
    # gamma * S constant over u: a one-vector set of a constant c gives
    # S_u = c * sum_z p(z | b, u) = c up to rounding; with the tail removed
    # exactly (zeros) the choice is the argmax of rew, asserted above, and a
    # constant set must agree with it wherever rew's top two are well apart
    const = R.pad_plane(np.full((1, hw), np.float32(-3.0)), H, W, wp)
    for b in beliefs:
        u, Q, rew, M, _ = LR.lookahead_control(m, Rw, const, b)
        tail = (Q.astype(np.float64) - rew.astype(np.float64))
        assert np.ptp(tail) <= 1e-4 * np.abs(tail).max(), tail
        top2 = np.sort(rew.astype(np.float64))[-2:]
        if top2[1] - top2[0] > 4 * np.ptp(tail):
            assert u == AR.pick(rew)


def test_cut_main_case_shows_what_the_lookahead_buys(cut_case):
    case, m, alphas, actions, Rw, starts, look = cut_case
    greedy = AR.run_alpha_batch(m, alphas, actions, case["b0"], starts, HORIZON, case["seed"])
    # the first step of every episode sees the same belief under both policies
    n_differ = 0
    for e in range(NSTARTS):
        n = min(int(look["steps"][e]), int(greedy["steps"][e]))
        for k in range(n):
            if look["actions"][k, e] != greedy["actions"][k, e]:
                n_differ += 1
                break  # the beliefs part ways here
    reached = int((look["status"] == 1).sum())
    print(f"lookahead: {reached} of {NSTARTS} reached, {n_differ} episodes leave the greedy "
          f"FIB policy, actions {np.unique(look['actions'][look['actions'] != 255]).tolist()}")
    assert n_differ >= 1
    assert reached >= 1
    assert not (look["status"] == 2).any()
    for e in range(NSTARTS):
        n = int(look["steps"][e])
        taken = look["actions"][:n, e]
        for k in range(n):
            assert taken[k] == AR.pick(look["q"][k, e])
        assert (look["leaf_index"][:n, e] >= 0).all() and (look["leaf_index"][:n, e] < 9).all()
        assert (look["leaf_index"][n:, e] == -1).all() and not look["leaf_max"][n:, e].any()
        assert not look["q"][n:, e].any() and (look["mode_cells"][:, e] == -1).all()
        np.testing.assert_array_equal(bits(look["qsums"][:, e]), bits(look["q"][:, e]))
