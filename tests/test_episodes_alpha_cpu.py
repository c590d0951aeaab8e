"""CPU: the alpha-vector episodes' reference (tests/episodes_alpha_reference.py)
and the argument checks of ``EpisodeBatch.run_alpha`` -- no GPU.

* the pinned alpha dot agrees with an fp64 dot within the project's parity
  budget (rel 1e-5, as test_pinned_qdot_agrees_with_fp64: every term >= 0);
* with alphas = -Q and actions 0..8 an alpha episode is the QMDP episode of
  episodes_reference in every output (negation is exact, so the sums are exact
  negations and "first V_best < V_k" is QMDP's first strict minimum);
* the main FIB case of tests/test_gpu_episodes_alpha.py exercises every path
  (goal and horizon, many actions, near-ties that a wrong summation order
  flips), asserted on the reference alone;
* the NaN rule of the winner;
* ``EpisodeBatch`` dispatches "fib" / "pbvi" and rejects bad arguments before
  it touches the library.
"""
import numpy as np
import pytest

import episodes_alpha_reference as AR
import episodes_reference as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("H,W", [(40, 100), (97, 131)])
def test_pinned_alpha_dot_agrees_with_fp64(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    wp = R.row_stride(W)
    K = 21
    b = rng.random(H * W).astype(np.float32) * np.float32(2.0)
    b[rng.random(H * W) < 0.3] = 0
    al = (rng.random((K, H * W)) * 40).astype(np.float32)
    V = AR.adot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(al, H, W, wp))
    want = al.astype(np.float64) @ b.astype(np.float64)
    assert V.dtype == np.float32 and V.shape == (K,)
    assert np.all(np.abs(V - want) <= 1e-5 * np.abs(want)), (V, want)
    # K = 9 planes: the Q dot itself
    np.testing.assert_array_equal(
        bits(V[:9]), bits(R.qdot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(al[:9], H, W, wp))))


def test_alpha_of_minus_q_is_qmdp(oracle):
    case = R.main_case()
    grid = case["grid"]
    H, W = grid.shape
    m = R.Model(grid, case["goal"], case["gamma"])
    J, A, _, _ = oracle.mdp_solve(H, W, m.gamma, m.T, m.C)
    Q = R.q_planes_f64(m.T, m.C, J, m.gamma, H, W).astype(np.float32)
    starts, hz, seed = case["starts"], case["horizon"], case["seed"]
    q = R.run_batch(m, Q, A, case["b0"], starts, R.QMDP, hz, seed)
    a = AR.run_alpha_batch(m, -Q.T, np.arange(9), case["b0"], starts, hz, seed)
    for k in ("steps", "status", "final_cell", "actions", "observations", "cells"):
        np.testing.assert_array_equal(a[k], q[k], err_msg=k)
    np.testing.assert_array_equal(bits(a["cost"]), bits(q["cost"]))
    np.testing.assert_array_equal(bits(a["beliefs"]), bits(q["beliefs"]))
    # exact negations (a step not taken holds +0 in both)
    taken = q["actions"] != 255
    np.testing.assert_array_equal(bits(a["qsums"][taken]), bits(-q["qsums"][taken]))
    np.testing.assert_array_equal(a["best_index"][taken], q["actions"][taken])
    assert (q["status"] == 1).any() and taken.sum() > 100


def test_main_fib_case_exercises_every_path(oracle):
    case = R.main_case()
    m, alphas, actions = AR.main_fib_alphas(case)
    assert np.isfinite(alphas).all()
    E, hz = len(case["starts"]), case["horizon"]
    r = AR.run_alpha_batch(m, alphas, actions, case["b0"], case["starts"], hz, case["seed"])
    reached = int((r["status"] == 1).sum())
    full = int(((r["status"] == 0) & (r["steps"] == hz)).sum())
    used = np.unique(r["actions"][r["actions"] != 255])
    gaps = []
    for e in range(E):
        for V in r["sums"][e]:
            top2 = np.sort(V.astype(np.float64))[-2:]
            gaps.append((top2[1] - top2[0]) / abs(top2[1]))
    gaps = np.array(gaps)
    print(f"FIB: {reached} reached, {full} full horizon, actions {used.tolist()}, "
          f"smallest relative gap {gaps.min():.3g}, exact ties {(gaps == 0).sum()}")
    assert reached >= 1 and full >= 1 and reached + full == E
    assert len(used) >= 5
    assert gaps.min() < 1e-5
    assert not (r["status"] == 2).any()
    for e in range(E):
        n = int(r["steps"][e])
        assert (r["best_index"][:n, e] == r["actions"][:n, e]).all()  # action of vector k = k
        assert (r["best_index"][n:, e] == -1).all() and (r["best_sum"][n:, e] == 0).all()
        assert (r["mode_cells"][:, e] == -1).all()
        if n:
            assert r["cells"][n - 1, e] == r["final_cell"][e]
            np.testing.assert_array_equal(bits(r["best_sum"][:n, e]),
                                          bits(r["qsums"][:n, e].max(axis=1)))


def test_nan_rule():
    H, W = 5, 7
    wp = R.row_stride(W)
    rng = np.random.default_rng(4)
    b = rng.random(H * W).astype(np.float32)
    b[11] = 0
    al = rng.normal(size=(6, H * W)).astype(np.float32)
    base = AR.adot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(al, H, W, wp))
    want = int(np.argmax(base))
    assert AR.pick(base) == want
    # +inf where b = 0: the product is NaN, the sum is NaN, the vector never wins
    for k in range(1, 6):
        x = al.copy()
        x[k] = 1e6                       # would win by far ...
        x[k, 11] = np.inf                # ... but for the NaN
        V = AR.adot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(x, H, W, wp))
        assert np.isnan(V[k]) and np.isfinite(np.delete(V, k)).all()
        others = base.copy()
        others[k] = -np.inf
        assert AR.pick(V) == int(np.argmax(others)) != k
    # a NaN V_0 keeps winning
    x = al.copy()
    x[0, 11] = np.inf
    x[3] = 1e6
    V = AR.adot_pinned(R.pad_plane(b, H, W, wp), R.pad_plane(x, H, W, wp))
    assert np.isnan(V[0]) and AR.pick(V) == 0
    # ties: the first index
    assert AR.pick(np.array([1.0, 3.0, 3.0, 2.0], np.float32)) == 1
    assert AR.pick(np.array([-0.0, 0.0], np.float32)) == 0


def test_run_alpha_validates_and_dispatches_before_the_library():
    from path_planning_2d_amd import EpisodeBatch, _lib, episodes

    for name in ("pp2_episodes_run_alpha", "pp2_episodes_trace_alpha", "pp2_episodes_get_alpha"):
        assert name in _lib.SIGNATURES
    assert (episodes.ALPHA_FIB, episodes.ALPHA_PBVI) == (0, 1)

    ep = EpisodeBatch.__new__(EpisodeBatch)  # no context, no library
    ep._h, ep.cells, ep.episodes = None, 12, 3
    seen = []
    ep.run_alpha = lambda *a, **k: seen.append((a, k)) or ep
    ok_b0 = np.full(12, 1 / 12, np.float32)
    assert ep.run("fib", ok_b0, [0, 5, 11], 7) is ep
    assert ep.run("pbvi", ok_b0, [0, 5, 11], seed=8) is ep
    assert [s[0][0] for s in seen] == ["fib", "pbvi"] and seen[0][0][3] == 7
    del ep.run_alpha

    bad_neg, bad_m0 = ok_b0.copy(), ok_b0.copy()
    bad_neg[3], bad_m0[3] = -0.1, -0.0
    for args in (("greedy", ok_b0, [0, 5, 11], 0),
                 ("qmdp", ok_b0, [0, 5, 11], 0),
                 (2, ok_b0, [0, 5, 11], 0),
                 (-1, ok_b0, [0, 5, 11], 0),
                 (None, ok_b0, [0, 5, 11], 0),
                 (0.0, ok_b0, [0, 5, 11], 0),
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
            ep.run_alpha(*args)
    # integer 2 and unknown strings still fail in run itself
    for policy in (2, "greedy"):
        with pytest.raises(ValueError):
            ep.run(policy, ok_b0, [0, 5, 11], 0)
