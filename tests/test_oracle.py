"""CPU: the oracle (test infrastructure) against the golden fixtures and
against independent restatements.  The reference ships no tests; these tests
pin the oracle as far as the reference's own data allows -- real glibc rand()
output, the simulator's independent scatter-form filter, and numpy
restatements of the kernels.  test_ref_pin_cpu.py pins the device-kernel
restatements to the reference's own kernels built for the host."""
import ctypes

import numpy as np
import pytest

from conftest import GAMMA, assert_rel_close, golden, golden_map

MAPS = ["map_3x3", "map_5x5", "map_10x10", "map_100x40", "sparse_map_100x40",
        "tile64_sparse_map_100x40"]


@pytest.mark.parametrize("name", MAPS)
def test_model_matches_golden(oracle, name):
    g = golden("model", name)
    grid = golden_map(name)
    T, L, R = oracle.model_pomdp(grid, tuple(g["goal"]))
    T2, C = oracle.model_mdp(grid, tuple(g["goal"]))
    np.testing.assert_array_equal(T, g["T"])
    np.testing.assert_array_equal(T2, g["T"])
    np.testing.assert_array_equal(L, g["L"])
    np.testing.assert_array_equal(R, g["R"])
    np.testing.assert_array_equal(C, g["C"])


def numpy_model(grid, goal):
    """Independent vectorised restatement of cudaGenerateModelData
    (model_generation_cuda.cu:161-347, mdp/path_planning_2d_cuda.cu:76-213)."""
    from path_planning_2d_amd.synthetic import _BASE
    H, W = grid.shape
    pad = np.ones((H + 2, W + 2), np.uint8)
    pad[1:-1, 1:-1] = grid
    lm = np.stack([pad[1 + i // 3 - 1:H + 1 + i // 3 - 1, 1 + i % 3 - 1:W + 1 + i % 3 - 1]
                   for i in range(9)], -1).reshape(H * W, 9)
    occ = lm == 1
    T = np.broadcast_to(_BASE, (H * W, 9, 9)).copy()
    for i in range(9):
        if i == 4:
            continue
        m = occ[:, i]
        T[m, :, 4] = (T[m, :, 4] + T[m, :, i]).astype(np.float32)
        T[m, :, i] = 0
    trap = occ[:, 4]
    T[trap] = 0
    T[trap, :, 4] = 1
    hi, lo = np.float32(0.98), np.float32(0.02)
    z = np.arange(16)
    m4 = lm[:, [1, 3, 5, 7]]
    fac = [np.where(((z[None, :] >> k) & 1) == m4[:, k:k + 1], hi, lo) for k in range(4)]
    L = (((fac[0] * fac[1]).astype(np.float32) * fac[2]).astype(np.float32) * fac[3]).astype(np.float32)
    mr = np.where(occ, np.float32(-2), np.float32(-1))
    R = np.zeros((H * W, 9), np.float32)
    for i in range(9):
        R = (R + mr[:, None, i] * _BASE[None, :, i]).astype(np.float32)
    nm = np.broadcast_to(_BASE, (H * W, 9, 9)).copy()
    nm[trap] = 0
    nm[trap, :, 4] = 1
    mc = np.where(occ, np.float32(2), np.float32(1))
    C = np.zeros((H * W, 9), np.float32)
    for i in range(9):
        C = (C + mc[:, None, i] * nm[:, :, i]).astype(np.float32)
    goal_idx = goal[1] * W + goal[0]
    R[:, 4] = -2
    C[:, 4] = 2
    R[goal_idx, 4] = 0
    C[goal_idx, 4] = 0
    return T, L, R, C


@pytest.mark.parametrize("name", MAPS)
def test_model_matches_numpy_restatement(name):
    g = golden("model", name)
    T, L, R, C = numpy_model(golden_map(name), tuple(g["goal"]))
    np.testing.assert_array_equal(T, g["T"])
    np.testing.assert_array_equal(L, g["L"])
    np.testing.assert_array_equal(R, g["R"])
    np.testing.assert_array_equal(C, g["C"])


@pytest.mark.parametrize("name", ["map_10x10", "sparse_map_100x40",
                                  "tile64_sparse_map_100x40"])
def test_belief_trajectory_golden_and_simulator(oracle, name):
    """Gather-form planner update == golden, and == the simulator's scatter
    filter (dummy_simulator.cpp:671-773) to 1e-5 relative."""
    grid = golden_map(name)
    H, W = grid.shape
    m = golden("model", name)
    bt = golden("belief", name)
    b = bt["b0"].copy()
    bs = bt["b0"].copy()
    for k in range(64):
        b = oracle.belief_step(H, W, m["T"], m["L"], b, bt["us"][k], bt["zs"][k])
        bs = oracle.sim_step(grid, bs, bt["us"][k], bt["zs"][k])
        if f"b{k + 1}" in bt:
            np.testing.assert_array_equal(b, bt[f"b{k + 1}"])
            assert_rel_close(b, bs, rel=1e-5, abs_floor=1e-30,
                             msg=f"{name} step {k + 1} gather vs scatter")


def test_mdp_golden(oracle):
    for name in ["map_10x10", "sparse_map_100x40", "tile64_sparse_map_100x40"]:
        grid = golden_map(name)
        H, W = grid.shape
        m = golden("model", name)
        g = golden("mdp", name)
        J, A, n, nrm = oracle.mdp_solve(H, W, GAMMA, m["T"], m["C"])
        assert n == int(g["sweeps"]) == 300
        np.testing.assert_array_equal(J, g["J"])
        np.testing.assert_array_equal(A, g["A"])


def test_mdp_sweep_matches_numpy(oracle):
    """Independent numpy sweep with the same pinned op order."""
    name = "sparse_map_100x40"
    grid = golden_map(name)
    H, W = grid.shape
    m = golden("model", name)
    T, C = m["T"], m["C"]
    J = np.zeros(H * W, np.float32)
    Jn = J
    for _ in range(7):
        pad = np.zeros((H + 2, W + 2), np.float32)
        pad[1:-1, 1:-1] = Jn.reshape(H, W)
        nb = np.stack([pad[i // 3:i // 3 + H, i % 3:i % 3 + W] for i in range(9)],
                      -1).reshape(H * W, 9)
        cost = C.copy()
        for i in range(9):
            t = (GAMMA * T[:, :, i]).astype(np.float32)
            cost = (np.float64(cost) + np.float64(t) * np.float64(nb[:, i:i + 1])).astype(np.float32)
        Jn = cost.min(1).astype(np.float32)
        A = cost.argmin(1).astype(np.uint8)
    g = golden("mdp", name)
    # fma(t, j, c) == fl(c + t*j) computed in double (single rounding) here
    np.testing.assert_array_equal(Jn, g["J7"])
    np.testing.assert_array_equal(A, g["A7"])


def test_fib_golden(oracle):
    for name in ["map_10x10", "sparse_map_100x40"]:
        grid = golden_map(name)
        H, W = grid.shape
        m = golden("model", name)
        g = golden("fib", name)
        a, n, nrm = oracle.fib_solve(H, W, GAMMA, m["T"], m["L"], m["R"])
        assert n == int(g["sweeps"])
        np.testing.assert_array_equal(a, g["alphas"])


def test_glibc_rand_restatement(oracle):
    """orc_rand_* == real glibc rand() from the reference's (default) seed."""
    ref = np.load(__import__("conftest").GOLDEN + "/glibc_rand.npy")
    lib = oracle.lib()

    class St(ctypes.Structure):
        _fields_ = [("r", ctypes.c_int32 * 34), ("f", ctypes.c_int), ("b", ctypes.c_int)]
    s = St()
    lib.orc_rand_seed(ctypes.byref(s), 1)
    lib.orc_rand_next.restype = ctypes.c_int32
    mine = np.array([lib.orc_rand_next(ctypes.byref(s)) for _ in range(ref.size)], np.int32)
    np.testing.assert_array_equal(mine, ref)


def test_curand_xorwow_subsequence_is_linear_jump(oracle):
    """Subsequence k+1 == 2^67 raw draws after subsequence k is not checkable
    directly; check the GF(2) jump composes: (seq 2) == jump(jump(seq 0))."""
    a = oracle.curand_xorwow(1234, 2, 0, 8)
    b = oracle.curand_xorwow(1234, 2, 0, 8)
    np.testing.assert_array_equal(a, b)
    c = oracle.curand_xorwow(1234, 0, 3, 5)
    d = oracle.curand_xorwow(1234, 0, 0, 8)[3:]
    np.testing.assert_array_equal(c, d)
    u = oracle.curand_uniform(0xFFFFFFFF)
    assert 0.0 < u <= 1.0


def test_product_curand_stream_matches_oracle(oracle):
    """The product's cuRAND XORWOW (rocRAND's precomputed 2^67 jump matrices)
    equals the oracle's independent GF(2) matrix-power jump, for the 50
    subsequences every QNode re-creates (search_tree_cuda.cu:84-92)."""
    from path_planning_2d_amd.planner import curand_uniforms
    u1, u2 = curand_uniforms(1234, 50)
    for i in range(50):
        x = oracle.curand_xorwow(1234, i, 0, 2)
        assert u1[i] == oracle.curand_uniform(x[0])
        assert u2[i] == oracle.curand_uniform(x[1])


def test_oracle_planner_runs(oracle):
    """The reference-semantics tree on the sparse map: depth advances by 2
    per expansion level (QNode::update depth quirk, search_tree_cuda.cu:
    277-283) and 9 QNodes hang under an expanded root."""
    from path_planning_2d_amd import synthetic as S
    name = "sparse_map_100x40"
    g = golden_map(name)
    m = golden("model", name)
    f = golden("fib", name)
    pl = oracle.Planner(g, m["T"], m["L"], m["R"], f["alphas"], max_depth=3,
                        max_iter=15)
    a, v = pl.step(0, 0, S.uniform_belief(g))
    info = pl.info()
    assert info["expansions"] == 2 and info["depth"] == 4
    assert info["n_root_children"] == 9
    assert v == max(info["q_upper_bound"])
    assert a == int(np.argmax(info["q_upper_bound"]))


def test_loop_run_mt_matches_sequence(oracle):
    """The threaded CPU-baseline loop (rows split over threads) = the
    single-thread oracle step sequence: values/actions bit-exact, beliefs to
    rel 1e-5 (it scales by 1/sum instead of dividing)."""
    import numpy as np
    from conftest import GAMMA, assert_rel_close, golden_map
    from path_planning_2d_amd import synthetic as S
    grid = golden_map("sparse_map_100x40")
    H, W = grid.shape
    goal = S.synth_goal(grid)
    T, L, _ = oracle.model_pomdp(grid, goal)
    _, Cc = oracle.model_mdp(grid, goal)
    us, zs, _ = S.synth_trajectory(grid, 6, seed=3)
    b0 = S.uniform_belief(grid)
    lib = oracle.lib()
    b = b0.copy()
    J = np.zeros(H * W, np.float32)
    for k in range(6):
        b = oracle.belief_update(H, W, T, L, b, int(us[k]), int(zs[k]))
        b = (b / np.float32(b.sum(dtype=np.float32))).astype(np.float32)
        J, A = oracle.mdp_sweep(H, W, GAMMA, T, Cc, J)
    bm, bo = b0.copy(), np.empty_like(b0)
    Jm, Jo = np.zeros(H * W, np.float32), np.empty(H * W, np.float32)
    Am = np.zeros(H * W, np.uint8)
    n = lib.orc_loop_run_mt(H, W, np.float32(GAMMA), T, L, Cc, bm, bo, Jm, Jo, Am, 6,
                            np.ascontiguousarray(us[:6], np.uint8),
                            np.ascontiguousarray(zs[:6], np.uint8), 4)
    assert n == 6
    # 6 steps = even number of swaps: results are back in the first buffers
    np.testing.assert_array_equal(Jm, J)
    np.testing.assert_array_equal(Am, A)
    assert_rel_close(bm, b, rel=1e-5, msg="threaded loop belief")


def test_heap_sort_matches_libstdcxx(oracle, tmp_path):
    """orc_heap_sort_desc restates what libstdc++ does for the reference's
    partial_sort(idx.begin(), idx.end(), idx.begin() + 100, comp) call
    (point_based_value_iteration_cuda.cu:264-269: middle and last swapped ->
    make_heap + sort_heap over the whole range); checked against the real
    libstdc++ algorithms, ties included."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = tmp_path / "h.cpp"
    src.write_text(r'''
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>
int main() {
  size_t n; if (scanf("%zu", &n) != 1) return 1;
  std::vector<float> k(n); for (auto& v : k) if (scanf("%f", &v) != 1) return 1;
  std::vector<size_t> idx(n); std::iota(idx.begin(), idx.end(), 0);
  auto comp = [&](size_t a, size_t b) { return k[a] > k[b]; };
  std::make_heap(idx.begin(), idx.end(), comp);
  std::sort_heap(idx.begin(), idx.end(), comp);
  for (size_t i : idx) printf("%zu\n", i);
}
''')
    exe = tmp_path / "h"
    subprocess.run(["g++", "-O2", "-o", str(exe), str(src)], check=True)
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 100, 101, 128, 228, 428):
        key = rng.integers(0, max(2, n // 3), n).astype(np.float32) / 7  # many ties
        inp = f"{n}\n" + "\n".join(f"{v:.9g}" for v in key) + "\n"
        out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True)
        want = np.array(out.stdout.split(), np.uint64)
        got = oracle.heap_sort_desc(key)
        np.testing.assert_array_equal(got.astype(np.uint64), want, err_msg=f"n={n}")


def test_pbvi_oracle_structure(oracle):
    """generateBeliefSet keeps b0 first and only normalised rows; the backup
    runs the reference's iteration count ceil(log(2e-4)/log(0.95)) = 167."""
    from conftest import GAMMA, golden, golden_map
    from path_planning_2d_amd import synthetic as S
    g = golden_map("map_10x10")
    H, W = g.shape
    T, L, R = oracle.model_pomdp(g, tuple(golden("model", "map_10x10")["goal"]))
    b0 = S.uniform_belief(g)
    B, _ = oracle.pbvi_belief_set(H, W, T, L, b0, 12)
    np.testing.assert_array_equal(B[0], b0)
    assert np.allclose(B.sum(1), 1.0, atol=1e-5)
    assert oracle.pbvi_iterations(GAMMA) == 167
    al, act, n = oracle.pbvi_backup(H, W, GAMMA, T, L, R, B, iterations=2)
    assert n == 2 and act.max() <= 8 and np.isfinite(al).all()
    # one backup from zero alphas: alpha_i = R[:, a*] with a* = argmax <b_i, R_a>
    al1, act1, _ = oracle.pbvi_backup(H, W, GAMMA, T, L, R, B, iterations=1)
    for i in range(len(B)):
        np.testing.assert_array_equal(al1[i], R[:, act1[i]])


@pytest.mark.parametrize("name", ["map_10x10", "sparse_map_100x40"])
def test_pbvi_oracle_matches_golden(oracle, name):
    """The oracle's generateBeliefSet + backupAlphaVectors reproduce the
    frozen PBVI fixtures bit for bit (tests/golden/make_golden.py pbvi)."""
    from conftest import GAMMA, golden, golden_map
    from path_planning_2d_amd import synthetic as S
    g = golden_map(name)
    p = golden("pbvi", name)
    T, L, R = oracle.model_pomdp(g, tuple(golden("model", name)["goal"]))
    H, W = g.shape
    B, _ = oracle.pbvi_belief_set(H, W, T, L, S.uniform_belief(g), p["beliefs"].shape[0])
    np.testing.assert_array_equal(B, p["beliefs"])
    al, act, n = oracle.pbvi_backup(H, W, GAMMA, T, L, R, B, iterations=int(p["iterations"]))
    np.testing.assert_array_equal(al, p["alphas"])
    np.testing.assert_array_equal(act, p["actions"])


def test_pbvi_eval_is_the_sequential_chain(oracle):
    """evaluatePbviCpu (point_based_value_iteration_cuda.cu:678-699): the
    oracle walks eight alphas' chains side by side; every dot must still be
    the x-ordered fp32 chain (numpy's float32 cumsum is one sequential
    chain), with the first maximum."""
    rng = np.random.default_rng(3)
    n, S = 1000, 21  # two groups of 8 and a tail of 5
    b = rng.random(n).astype(np.float32)
    b /= b.sum(dtype=np.float32)
    al = -rng.random((S, n)).astype(np.float32) * 40
    al[13] = al[5]  # a tie: the first maximum wins
    act = (np.arange(S) % 9).astype(np.uint8)
    dots = np.array([np.cumsum(b * al[i], dtype=np.float32)[-1] for i in range(S)], np.float32)
    best = 0
    for i in range(1, S):
        if dots[best] < dots[i]:
            best = i
    v, a = oracle.pbvi_eval(b, al, act)
    assert np.float32(v).view(np.uint32) == dots[best].view(np.uint32)
    assert a == act[best]


# ---------------------------------------------------------------- fp16 rollout step
def test_rollout_step_f16_is_the_belief_update(oracle):
    """orc_rollout_step_f16 on a plane of exactly fp16-representable values
    (subnormals included) with max = 1 (so 1/max = 1 and L * inv = L): its
    unrounded v equals orc_belief_update on the same plane bit for bit -- the
    new stencil indexing is the golden-checked update's."""
    name = "tile64_sparse_map_100x40"
    grid = golden_map(name)
    H, W = grid.shape
    m = golden("model", name)
    rng = np.random.default_rng(16)
    # magnitudes 2^-26 .. 1: a third of the cells fp16-subnormal or zero
    plane = (rng.random(H * W) * 2.0 ** -rng.integers(0, 26, H * W)).astype(np.float16)
    plane[grid.reshape(-1) == 1] = 0
    plane[int(np.argmax(plane))] = 1.0
    sub = (plane > 0) & (plane.astype(np.float64) < 2.0 ** -14)
    assert sub.sum() > H * W // 8
    for u, z in ((0, 0), (4, 15), (8, 5), (3, 10), (6, 9)):
        out, v, (s, mx, rd) = oracle.rollout_step_f16(H, W, m["T"], m["L"], m["R"], u, z,
                                                      plane, 1.0)
        want = oracle.belief_update(H, W, m["T"], m["L"], plane.astype(np.float32), u, z)
        np.testing.assert_array_equal(v.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(out, want.astype(np.float16))
        assert s == out.astype(np.float64).sum() and mx == float(out.max())
        assert rd == pytest.approx(float(plane.astype(np.float64) @ m["R"][:, u].astype(np.float64)),
                                   rel=1e-12)
        # the subnormal input cells carry weight: flushing them changes v
        flushed = np.where(sub, np.float16(0), plane)
        _, v0, _ = oracle.rollout_step_f16(H, W, m["T"], m["L"], m["R"], u, z, flushed, 1.0)
        assert (v0 != v).any()


def test_rollout_chain_f16_tracks_fp32_rollout(oracle):
    """The chained exact fp16 reference (depth 4, tile64_sparse_map_100x40)
    stays within the fp16 storage tolerance of tests/test_gpu_rollout.py of an
    fp32 rollout: rewards and likelihoods rel 3e-3, beliefs 5e-3 |b| + 1e-4
    of the copy's peak."""
    from path_planning_2d_amd import synthetic as S
    name = "tile64_sparse_map_100x40"
    grid = golden_map(name)
    H, W = grid.shape
    m = golden("model", name)
    T, L, R = m["T"], m["L"], m["R"]
    copies, depth = 6, 4
    b0 = S.uniform_belief(grid)
    us, zs = S.rollout_trajectories(grid, b0, copies, depth, seed=11)
    for c in range(copies):
        b = b0.astype(np.float32)
        rw, pr = [], []
        for k in range(depth):
            u, z = int(us[k, c]), int(zs[k, c])
            rw.append(float(np.dot(b.astype(np.float64), R[:, u])))
            nb = oracle.belief_update(H, W, T, L, b, u, z)
            p = float(nb.astype(np.float64).sum())
            pr.append(p)
            b = (nb.astype(np.float64) / p).astype(np.float32)
        e = oracle.rollout_chain_f16(H, W, T, L, R, b0, us[:, c], zs[:, c])
        assert np.all(np.abs(e["rewards"] - rw) <= 3e-3 * np.abs(rw) + 1e-7), c
        assert np.all(np.abs(e["obs_prob"] - pr) <= 3e-3 * np.abs(pr) + 1e-7), c
        err = np.abs(e["belief"].astype(np.float64) - b)
        assert np.all(err <= 5e-3 * np.abs(b) + 1e-4 * b.max()), c


def _rollout_cases():
    import rollout_exact_cases as RC
    return RC


@pytest.mark.parametrize("key", list(_rollout_cases().ALL_CASES))
def test_rollout_exact_cases_are_sensitive(oracle, key):
    """Every case of tests/test_gpu_rollout_exact.py, on the emulated planes
    alone, contains what it is meant to exercise, so that no GPU comparison
    passes vacuously: every plane has mass; nonzero stored values in the last
    column, on both sides of a segment boundary (columns 255 | 256) and of a
    band seam (rows 31 | 32); from the uniform root at least 10 % of the
    positive stored cells fp16-subnormal (shares of the 13-copy geometry
    cases, trajectory seed 7: 1x9 8 % -- hence seed 28 there: 16 % --, 2x16
    40 %, 3x300 43 %, 5x264 33 %, 70x260 34 %, 33x64 28 %, 64x256 34 %, 35x512
    32 %, 37x50 34 %; the least of the other cases is 33x64 at depth 1: 11 %); each
    one-hot root reaches its neighbours across the edge it stands at; and
    the model variants change the planes."""
    RC = _rollout_cases()
    case = RC.ALL_CASES[key]
    H, W = case.H, case.W
    inp = RC.inputs(case)
    P = RC.stored_planes(case)
    assert P.shape[0] == len(inp["runs"]) * case.copies * case.depth
    assert np.isfinite(P).all() and (P.reshape(len(P), -1).max(1) > 0).all()
    assert (P[:, :, W - 1] > 0).any()
    if W > 256:
        assert (P[:, :, 255] > 0).any() and (P[:, :, 256] > 0).any()
    if H > 32:
        assert (P[:, 31, :] > 0).any() and (P[:, 32, :] > 0).any()
    U = RC.stored_planes(case, "uniform")
    share = ((U > 0) & (U < RC.F16_MIN_NORMAL)).sum() / (U > 0).sum()
    print(f"{key}: fp16-subnormal share of the positive stored cells {share:.3f}")
    assert share >= 0.10, share
    if case.roots == "all":
        em = RC.emulate(case)
        for name, y, x in RC.hot_cells(H, W):
            # after the first step the mass has crossed to the neighbour
            # columns / rows of the hot cell in at least one copy
            first = np.array([e["planes"][0].astype(np.float32).reshape(H, W) for e in em[name]])
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                if 0 <= yy < H and 0 <= xx < W:
                    assert (first[:, yy, xx] > 0).any(), (name, yy, xx)
    us = np.concatenate([r[2].reshape(-1) for r in inp["runs"]])
    if case.batch == "nine":
        assert set(us.tolist()) == set(range(9))
    if case.model != "gen":
        if case.model == "offsupport":
            # same trajectories but for the forced stay actions: compare on the
            # off-support model's own inputs with the plain T
            from oracle import oracle as O
            g = RC.inputs(case._replace(model="gen"))
            _, b0, us_, zs_ = inp["runs"][0]
            assert (us_ == RC.OFF_ACTION).any()
            oc = RC.off_cell(H, W)
            differs = False
            for c in range(case.copies):
                a = O.rollout_chain_f16(H, W, g["T"], g["L"], g["R"], b0, us_[:, c], zs_[:, c])
                differs |= bool((a["plane"] != RC.emulate(case)["uniform"][c]["plane"]).any())
            assert differs
            assert inp["T"][oc, RC.OFF_ACTION, 0] == np.float32(0.25) and g["T"][oc, RC.OFF_ACTION, 0] == 0
        else:
            assert (RC.stored_planes(case._replace(model="gen")) != P).any()
            tup = inp["T"].reshape(H * W, -1)
            assert len(np.unique(tup, axis=0)) > 400  # more than the dictionary holds
