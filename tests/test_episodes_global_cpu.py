"""CPU: the device-memory belief placement of the batched episodes -- no GPU.

* ``large_case()`` (tests/episodes_global_cases.py), the grid the LDS placement
  refuses, exercises the paths that tests/test_gpu_episodes_global.py compares
  bit for bit: asserted here on the reference alone, with the oracle's MDP
  solve, as tests/test_episodes_cpu.py does for the main case;
* ``EpisodeBatch`` validates the placement before it touches the library;
* include/pp2.h declares the two entry points and the three constants, and the
  ABI version is still 4.
"""
import re

import numpy as np
import pytest

import episodes_global_cases as GC
import episodes_reference as R


@pytest.fixture(scope="module")
def large_runs(oracle):
    case = GC.large_case()
    grid = case["grid"]
    H, W = grid.shape
    m = R.Model(grid, case["goal"], case["gamma"])
    J, A, _, _ = oracle.mdp_solve(H, W, m.gamma, m.T, m.C)
    Q = R.q_planes_f64(m.T, m.C, J, m.gamma, H, W).astype(np.float32)
    runs = {p: R.run_batch(m, Q, A, case["b0"], case["starts"], p, case["horizon"], case["seed"])
            for p in (R.MODE, R.QMDP)}
    return case, m, runs


def test_large_case_is_what_the_tests_assume():
    case = GC.large_case()
    grid, starts = case["grid"], case["starts"]
    H, W = grid.shape
    assert (H, W) == (130, 140) and case["goal"] == (0, 0) and case["horizon"] == 10
    flat = grid.reshape(-1)
    free = np.flatnonzero(flat == 0)
    assert starts.dtype == np.int32 and len(starts) == 7 and starts[0] == 0
    assert (flat[starts] == 0).all()
    assert all(c != 0 and max(c % W, c // W) <= 3 for c in starts[1:5])
    assert list(starts[1:5]) == sorted(starts[1:5]) and len(set(starts[1:5].tolist())) == 4
    assert starts[5] == free[len(free) // 2]
    assert starts[6] == (H * W - 1 if flat[-1] == 0 else free[-1])
    # the LDS placement's layout of this grid (csrc/pp2_episodes.h: two fp32
    # planes and a uint16 code plane of [H + 2][wp + 4]) is past 160 KiB by the
    # planes alone
    wp = R.row_stride(W)
    assert (2 * 4 + 2) * (H + 2) * (wp + 4) > 160 * 1024


def test_large_case_exercises_every_path(large_runs):
    case, m, runs = large_runs
    hz = case["horizon"]
    q = runs[R.QMDP]
    reached_late = int(((q["status"] == 1) & (q["steps"] >= 1)).sum())
    full = int(((q["status"] == 0) & (q["steps"] == hz)).sum())
    md = runs[R.MODE]
    print(f"QMDP: steps {q['steps'].tolist()}, status {q['status'].tolist()}; "
          f"mode: {int(md['ties'].sum())} tie steps in {int((md['ties'] > 0).sum())} episodes")
    assert q["steps"][0] == 0 and q["status"][0] == 1   # the start on the goal
    assert reached_late >= 1
    assert full >= 4
    assert int(md["ties"].sum()) >= 1
    for r in runs.values():
        assert not (r["status"] == 2).any()


def test_placement_validates_before_the_library():
    import path_planning_2d_amd as P
    from path_planning_2d_amd import episodes as E

    class NoCtx:  # any use of the context would raise AttributeError
        pass

    assert (P.EPISODES_LDS, P.EPISODES_GLOBAL, P.EPISODES_AUTO) == (0, 1, 2)
    for name, val in (("lds", 0), ("global", 1), ("auto", 2)):
        assert E.check_placement(name) == val and E.check_placement(val) == val
        assert E.check_placement(np.int32(val)) == val
    for bad in ("LDS", "hbm", "", 3, -1, 1.0, True, None, b"lds"):
        with pytest.raises(ValueError):
            E.check_placement(bad)
        with pytest.raises(ValueError):
            P.EpisodeBatch(NoCtx(), 4, 8, placement=bad)
    # the existing checks come first and keep their order
    with pytest.raises(ValueError, match="episodes"):
        P.EpisodeBatch(NoCtx(), 0, 8)
    with pytest.raises(ValueError, match="episodes"):
        P.EpisodeBatch(NoCtx(), 0, 8, placement="nowhere")
    with pytest.raises(ValueError, match="horizon"):
        P.EpisodeBatch(NoCtx(), 4, 0, placement="nowhere")
    # a valid placement goes on to the context (which NoCtx does not have)
    for ok in ("lds", "global", "auto", 1):
        with pytest.raises(AttributeError):
            P.EpisodeBatch(NoCtx(), 4, 8, placement=ok)


def test_header_declares_the_placement_abi():
    from path_planning_2d_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    for name, val in (("PP2_EPISODES_LDS", 0), ("PP2_EPISODES_GLOBAL", 1),
                      ("PP2_EPISODES_AUTO", 2)):
        assert re.search(rf"^#define {name}\s+{val}\b", text, re.M), name
    flat = re.sub(r"\s+", " ", text)
    assert ("int pp2_episodes_create_placed(pp2_episodes** out, pp2_ctx* ctx, int episodes, "
            "int horizon, int record_trace, int placement);") in flat
    assert ("int pp2_episodes_placement(pp2_episodes* ep, int* requested, int* last, "
            "long long* scratch_bytes);") in flat
    assert len(_lib.SIGNATURES["pp2_episodes_create_placed"]) == 6
    assert len(_lib.SIGNATURES["pp2_episodes_placement"]) == 4
