"""What test_gpu_planner_shapes.py relies on, checked without a GPU:

* the shape table (planner_shape_cases.SHAPES) against the constants the
  planner branches on -- read out of the sources, so a changed constant fails
  here instead of silently moving a shape to the other side of its limit;
* the condition under which the default-order planner may be held to the
  fp64-accumulating oracle: with ONE expansion the reference-arithmetic and
  the fp64-accumulating oracle build trees of identical shape and choose the
  same action (no near-tied choice of the next node to expand exists yet);
* the short_mass belief really runs draws off its cdf (the sampler's clamp);
* every reference-order case small enough runs through the
  reference-arithmetic oracle without error;
* the table of the library's environment switches (planner_shape_cases.
  SWITCHES) names every variable the sources read and where each is held to
  the oracle, and the shapes of test_gpu_planner_switches.py keep as many
  children as its cases count on.
"""
import functools
import os
import re

import numpy as np
import pytest

import planner_shape_cases as PC
from conftest import ROOT

CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")


@functools.lru_cache(maxsize=None)
def host_model(H, W):
    """(T, L, R, FIB alphas after at most 40 sweeps) of a table shape."""
    from oracle import oracle as O
    O.build()
    grid = PC.grid_of(H, W)
    T, L, R = O.model_pomdp(grid, PC.goal_of(H, W))
    alphas, _, _ = O.fib_solve(H, W, PC.GAMMA, T, L, R, max_sweeps=40)
    return T, L, R, alphas


def oracle_planner(oracle, H, W, lb, accurate, max_iter):
    T, L, R, alphas = host_model(H, W)
    pl = oracle.Planner(PC.grid_of(H, W), T, L, R, alphas, max_depth=PC.MAX_DEPTH,
                        max_iter=max_iter, accurate=accurate)
    if lb:
        pl.set_pbvi(*PC.pbvi_of(H, W))
    return pl


@pytest.mark.parametrize("name", sorted(PC.LIMITS))
def test_restated_constants_match_sources(name):
    value, fname, pattern = PC.LIMITS[name]
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, f"{name}: {pattern!r} matches {len(found)} times in {fname}"
    assert int(found[0]) == value, f"{name} is {found[0]} in {fname}, restated as {value}"


def test_shape_table_straddles_limits():
    K = PC.K
    assert K["kSeqChainMax"] == K["kWalkMax"] == 8192
    assert K["kSubCellsMax"] == 16 * K["kSampleSub"] == 65536
    n = {hw: hw[0] * hw[1] for hw in PC.ALL}
    assert set(PC.SHAPE_NOTES) == set(PC.ALL)
    # 1x7: one row, n < 16 < 64, a single (ragged) 16-cell block
    assert n[(1, 7)] == 7 and PC.nsub(7) == 1
    # 5x1: one column
    assert n[(5, 1)] == 5
    # 3x3: the smallest grid with an interior cell
    assert n[(3, 3)] == 9
    # 33x65: walked chains, ragged in every unit
    m = n[(33, 65)]
    assert m == 2145 and m <= K["kSeqChainMax"]
    assert (65 % 4, m % 16, m % 64, m % 256) == (1, 1, 33, 97)
    # 64x128: the last size on the walked chains
    assert n[(64, 128)] == 8192 == K["kSeqChainMax"] == K["kWalkMax"]
    assert PC.branches(8192, 128)["walked_chains"]
    # 63x131: the first sizes on the chain sets, ragged sub block
    m = n[(63, 131)]
    assert m == 8253 and m > 8192 and m > K["kSeqChainMax"] and m % 16 != 0
    assert (131 % 4, m % 16, m % 256) == (3, 13, 61)
    assert not PC.branches(m, 131)["walked_chains"] and PC.branches(m, 131)["d_sub"]
    # 255x257: every LDS slot of the sampler's first search, ragged last block
    m = n[(255, 257)]
    assert (m + 15) // 16 == 4096 == K["kSampleSub"] and m % 16 != 0 and 257 % 4 == 1
    assert m <= K["kSubCellsMax"] and PC.fx_fits(m)
    # 257x257: no d_sub, the plain binary search; the fused sets do not fit
    m = n[(257, 257)]
    assert m > 65536 and m > K["kSubCellsMax"] and not PC.fx_fits(m)
    assert PC.branches(m, 257)["fc_walk"]
    # 513x515: more chunks than k_fc_walk holds, padded plane rows, and no
    # further above that limit than one percent
    m = n[(513, 515)]
    assert (m + 255) // 256 > 1024 and PC.fc_chunks(m) == 1033 > K["kWkEntries"]
    assert 515 % 4 != 0 and m < 1.01 * K["kWkEntries"] * K["kFcChunk"]
    assert not PC.branches(m, 515)["fc_walk"]
    # every other shape stays on k_fc_walk unless a test forces the driver
    assert all(PC.branches(n[hw], hw[1])["fc_walk"] for hw in PC.ALL if hw != PC.LARGEST)


@pytest.mark.parametrize("hw", PC.ALL, ids=PC.shape_id)
def test_grids_are_usable(hw):
    """A free goal, at least three free cells, and for delta_last a last free
    cell inside the last 16-cell block of a ragged grid."""
    grid = PC.grid_of(*hw)
    gx, gy = PC.goal_of(*hw)
    assert grid[gy, gx] == 0
    assert int((grid == 0).sum()) >= 3
    n = grid.size
    assert PC.last_free_cell(grid) // 16 == (n - 1) // 16
    # the hand-made PBVI alphas lie below every FIB alpha (R >= -2, 40 sweeps)
    _, _, R, alphas = host_model(*hw)
    assert R.min() >= -2.0 and alphas.min() > -34.9
    al, act = PC.pbvi_of(*hw)
    mixed = np.arange(n) % 97 == 3
    assert al.shape == (PC.PBVI_S, n) and al[:, ~mixed].max() < -40.0
    assert (al[5, mixed] >= 0).all() and (al[np.arange(PC.PBVI_S) != 5] < 0).all()
    assert act.max() <= 8


def test_case_lists_cover_the_issue():
    ref = PC.REF_CASES
    assert len({PC.ref_case_id(c) for c in ref}) == len(ref)
    plain = [c for c in ref if c[2] == "uniform" and c[3] == 0 and not c[5]]
    assert [(c[0], c[1]) for c in plain] == PC.ALL
    assert all(c[4] == (1 if (c[0], c[1]) == PC.LARGEST else 3) for c in plain)
    for kind in ("delta_last", "short_mass"):
        assert {(c[0], c[1]) for c in ref if c[2] == kind} == {(63, 131), (255, 257), (257, 257)}
    assert {(c[0], c[1]) for c in ref if c[3] == 1} == {(5, 1), (33, 65), (63, 131), (257, 257)}
    assert len(PC.DEFAULT_CASES) == 8 * 2 * 2
    assert PC.LARGEST not in {(c[0], c[1]) for c in PC.DEFAULT_CASES}
    # the switches mean what they are there for
    for H, W, _, _, _, sw in ref:
        n = H * W
        if sw.get("PP2_FX") == "1":
            assert PC.fx_fits(n) and (n > PC.K["kSeqChainMax"] or sw.get("PP2_SEQ_CHAIN_MAX") == "0")
        if "PP2_CHAIN_WALK" in sw:
            assert n <= PC.K["kWalkMax"]
        if sw.get("fc_walk") == 0:
            assert n > PC.K["kSeqChainMax"] and PC.branches(n, W)["fc_walk"]


@pytest.mark.parametrize("case", PC.DEFAULT_CASES, ids=PC.default_case_id)
def test_one_expansion_tree_is_arithmetic_independent(oracle, case):
    """The condition test_gpu_planner_shapes.py's default-order cases rest on."""
    H, W, kind, lb = case
    b0 = PC.belief_of(H, W, kind)
    out = []
    for accurate in (True, False):
        pl = oracle_planner(oracle, H, W, lb, accurate, max_iter=1)
        a, v = pl.step(0, 0, b0)
        out.append((a, v, pl.info()))
        pl.close()
    (a1, v1, i1), (a0, v0, i0) = out
    assert i1["expansions"] == 1 and i1["n_root_children"] == 9
    PC.same_tree_shape(i1, i0, PC.default_case_id(case))
    assert a1 == a0


@pytest.mark.parametrize("hw", [(63, 131), (255, 257), (257, 257)], ids=PC.shape_id)
def test_short_mass_runs_off_the_cdf(oracle, hw):
    b = PC.belief_of(*hw, "short_mass")
    end = PC.running_sum_end(b)
    assert 0.74 < end < 0.76
    rs = oracle.RandState(1)
    draws = [np.float32(rs.next()) / np.float32(2.0 ** 31) for _ in range(50)]
    assert sum(r > end for r in draws) >= 1
    # the clamp's target -- the first cell of the cdf's last run of equal
    # running sums -- lies more than two 16-cell blocks before the end
    cdf = np.cumsum(b, dtype=np.float32)
    target = int(np.nonzero(cdf < end)[0][-1]) + 1
    assert b.size - PC.SHORT_MASS_TAIL - 16 <= target < b.size - PC.SHORT_MASS_TAIL
    assert b[target] > 0


def test_switch_table_is_complete():
    """SWITCHES against the sources: the same names, every row held
    somewhere that exists, every new case off its row's default."""
    read = {}  # name -> [(file, text after the getenv)]
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith((".cpp", ".hip", ".h")):
            continue
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for m in re.finditer(r'getenv\(\s*"(PP2_\w+)"\s*\)', text):
            read.setdefault(m.group(1), []).append((fname, text[m.end():m.end() + 900]))
    assert set(read) == set(PC.SWITCHES), (
        f"read but not in SWITCHES: {sorted(set(read) - set(PC.SWITCHES))}; "
        f"in SWITCHES but not read: {sorted(set(PC.SWITCHES) - set(read))}")
    assert len(PC.SWITCHES) == 25
    ids = {PC.ref_case_id(c): c for c in PC.SWITCH_CASES}
    assert len(ids) == len(PC.SWITCH_CASES)
    for name, row in PC.SWITCHES.items():
        assert row["cached"] in ("process", "planner", "call"), name
        # the characters the row says flip it are compared in the source,
        # after one of the variable's reads
        after = [t for _, t in read[name]]
        if row["flips"] == "int":
            assert any(re.search(r"ato(i|ll)\(", t[:200]) for t in after), name
            int(row["default"])
        else:
            for ch in row["flips"]:
                assert any(f"== '{ch}'" in t for t in after), f"{name}: no == '{ch}'"
        if "exempt" in row:
            assert name in PC.EXEMPT_ALLOWED and row["exempt"], name
            assert "case" not in row and "tests" not in row, name
            continue
        assert row.get("case") or row.get("tests"), f"{name} is held nowhere"
        if "case" in row:
            assert row["case"] in ids, f"{name}: no case {row['case']}"
            sw = ids[row["case"]][5]
            assert name in sw and PC.differs_from_default(name, sw[name]), name
        for t in row.get("tests", []):
            fname, test = t.split("::")
            with open(os.path.join(ROOT, "tests", fname)) as f:
                text = f.read()
            assert re.search(rf"^def {test}\(", text, re.M), f"{name}: no {t}"
            if "PC.REF_CASES" in text and name not in text:
                # set through the case list (PP2_FC_WALK: through
                # pp2_debug_fc_walk, which writes the cached value)
                key = "fc_walk" if name == "PP2_FC_WALK" else name
                assert any(key in c[5] and (key == "fc_walk" or
                                            PC.differs_from_default(name, c[5][key]))
                           for c in PC.REF_CASES), f"{name}: no REF_CASES entry sets it"
            else:
                assert name in text, f"{name} does not appear in {fname}"
    # every variable a new case sets is set off its default, in the
    # character (or integer) the source compares
    for cid, c in ids.items():
        assert c[5], cid
        for name, value in c[5].items():
            if name.startswith("PP2_"):
                assert PC.differs_from_default(name, value), f"{cid}: {name}={value}"
            else:
                assert name == "pbvi_ties" and c[3] == 1, cid


def test_switch_cases_cover_the_issue():
    sw_cases = PC.SWITCH_CASES
    assert all(c[2] == "uniform" and c[4] == (1 if (c[0], c[1]) == (1, 7) else 2)
               for c in sw_cases)

    def process_cached(sw):
        return {k for k in sw if k in PC.SWITCHES and PC.SWITCHES[k]["cached"] == "process"}
    # the test's own process can set every switch of an in-process case ...
    assert all(not process_cached(c[5]) for c in PC.INPROCESS_SWITCH_CASES)
    # ... and every child set holds one that it cannot
    assert len(PC.CHILD_SETS) == 8 and all(process_cached(sw) for sw in PC.CHILD_SETS)
    assert len(sw_cases) == len(PC.INPROCESS_SWITCH_CASES) + 3 * len(PC.CHILD_SETS)
    for sw in PC.CHILD_SETS:
        cs = PC.child_cases(sw)
        assert [(c[0], c[1], c[3], c[4]) for c in cs] == [(1, 7, 0, 1), (33, 65, 1, 2),
                                                          (63, 131, 0, 2)]
        assert all(c in sw_cases and sw.items() <= c[5].items() for c in cs)
    for H, W, _, lb, _, sw in sw_cases:
        n = H * W
        on_chain_sets = n > PC.K["kSeqChainMax"] or sw.get("PP2_SEQ_CHAIN_MAX") == "0"
        if set(sw) == {"pbvi_ties"}:  # the near-tied alphas on the default leaf dots
            assert lb == 1
        elif "PP2_CHAIN_WALK" in sw:
            assert n <= PC.K["kWalkMax"] and not on_chain_sets
        elif "PP2_PAIR_SEQ" in sw:
            assert lb == 1 and n >= 1024
        elif "PP2_PBVI_FCHAIN" in sw:
            assert lb == 1 and sw.get("PP2_PBVI_STATS") == "1"
        else:  # every other switch acts on the chain sets' expansion only
            assert on_chain_sets and PC.branches(n, W)["fc_walk"]
            assert PC.fc_chunks(n) == {7: 1, 2145: 9, 8253: 33}[n]
    # sumtab stays where its whole grid (segments x 144 workgroups of 256
    # threads) is resident at once: at most 9 segments here
    assert max(PC.fc_chunks(c[0] * c[1]) for c in sw_cases if "PP2_FC_SUMTAB" in c[5]) == 33
    gys = sorted(int(sw["PP2_FC_KEPT_GY"]) for sw in PC.CHILD_SETS if "PP2_FC_KEPT_GY" in sw)
    assert gys == [1, 6]


@pytest.mark.parametrize("hw", sorted(PC.KEPT_CHILDREN), ids=PC.shape_id)
def test_switch_shapes_keep_enough_children(oracle, hw):
    """The kept children of the root expansion under the uniform belief: what
    PP2_FC_KEPT_GY's loop and the 64-group dispatch cap of a device group
    list (kFcDevGroups) run over."""
    with open(os.path.join(CSRC, "pp2_fchain.hip")) as f:
        found = re.findall(r"constexpr int kFcDevGroups = (\d+);", f.read())
    assert [int(v) for v in found] == [PC.FC_DEV_GROUPS]
    pl = oracle_planner(oracle, *hw, 0, False, PC.MAX_ITER)
    pl.step(0, 0, PC.belief_of(*hw, "uniform"))
    kept = int(sum(pl.info()["q_nchildren"][:9]))
    pl.close()
    assert kept == PC.KEPT_CHILDREN[hw]
    gy_max = max(int(sw["PP2_FC_KEPT_GY"]) for sw in PC.CHILD_SETS if "PP2_FC_KEPT_GY" in sw)
    assert kept > gy_max  # several children per workgroup row, several passes
    if hw != (1, 7):
        assert kept > PC.FC_DEV_GROUPS  # the device-list loop wraps
        assert kept % gy_max != 0  # a ragged last pass


@pytest.mark.parametrize("hw", sorted({(c[0], c[1]) for c in PC.SWITCH_CASES
                                      if c[5].get("pbvi_ties")}), ids=PC.shape_id)
def test_near_tied_alphas(hw):
    """pbvi_ties_of: a best group that no fp32 evaluation resolves, still a
    lower bound, the other rows untouched."""
    n = hw[0] * hw[1]
    al, act = PC.pbvi_ties_of(*hw)
    al0, act0 = PC.pbvi_of(*hw)
    ties = list(PC.TIES_ROWS)
    rest = [i for i in range(PC.PBVI_S) if i not in ties]
    assert np.array_equal(al[rest], al0[rest]) and np.array_equal(act, act0)
    assert 5 in rest  # the mixed-sign row stays
    _, _, _, alphas = host_model(*hw)
    assert al[ties].max() < -38.0 < -34.9 < alphas.min() and al[ties].min() >= -40.0
    # above every other row in every cell but the mixed-sign row's positive
    # ones: the group holds the maximum for beliefs that are not concentrated
    # on those cells (every 97th)
    mixed = np.arange(n) % 97 == 3
    others = [i for i in rest if i != 5]
    assert (al[ties].min(0) > al[others].max(0)).all()
    assert (al[ties].min(0)[~mixed] > al[5, ~mixed]).all()
    # whole ulps apart, at most 2 * TIES_STEPS, exactly; no row of the group
    # lies above another in every cell (fp32 sums are monotone: such a pair
    # every evaluation would order alike)
    steps = (al[ties] - al[ties[0]]) / PC.TIES_ULP
    assert (steps == np.round(steps)).all() and np.abs(steps).max() <= 2 * PC.TIES_STEPS
    if n >= 64:
        for i in ties:
            for j in ties:
                assert i == j or ((al[i] < al[j]).any() and (al[i] > al[j]).any())
    # under the uniform belief the group holds the maximum, and the true
    # dots of its two best rows lie closer than the rounding error an fp32
    # sum of n same-sign terms may carry ((n - 1) 2^-24 relative, each add
    # rounding once): inside every rigorous bound on an fp32 evaluation
    b = PC.belief_of(*hw, "uniform").astype(np.float64)
    d = al.astype(np.float64) @ b
    assert sorted(np.argsort(d)[::-1][:len(ties)]) == ties
    best = np.sort(d)[::-1]
    gap = (best[0] - best[1]) / abs(best[0])
    assert 0 <= gap < (n - 1) * 2.0 ** -24


SMALL_REF_CASES = [c for c in PC.REF_CASES
                   if (c[0], c[1]) not in (PC.LARGEST, PC.SECOND_LARGEST)]
# the oracle reads no environment switch: of SWITCH_CASES (all small), each
# schedule (shape, belief, bound, steps) that REF_CASES does not already run
def _schedule(c):
    return (*c[:5], bool(c[5].get("pbvi_ties")))


_ran = {_schedule(c) for c in SMALL_REF_CASES if not c[5].get("off_support")}
for _c in PC.SWITCH_CASES:
    if _schedule(_c) not in _ran:
        _ran.add(_schedule(_c))
        SMALL_REF_CASES.append((*_c[:5], {k: v for k, v in _c[5].items() if k == "pbvi_ties"}))


@pytest.mark.parametrize("case", SMALL_REF_CASES, ids=PC.ref_case_id)
def test_reference_oracle_runs_the_schedule(oracle, case):
    """The reference-arithmetic oracle runs step 0 and the following steps of
    every reference-order case without error (an expandable node at every
    expansion, finite bounds) and keeps a tree."""
    H, W, kind, lb, steps, sw = case
    T, L, R, alphas = host_model(H, W)
    grid = PC.grid_of(H, W)
    if sw.get("off_support"):
        T, cell = PC.off_support_model(grid, T)
        assert T[cell, 4].sum() == 1.0
    pl = oracle.Planner(grid, T, L, R, alphas, max_depth=PC.MAX_DEPTH, max_iter=PC.MAX_ITER)
    if lb:
        pl.set_pbvi(*PC.pbvi_alphas(H, W, sw))
    a, v = pl.step(0, 0, PC.belief_of(H, W, kind))
    zs = PC.zs_of(H, W, steps)
    for k in range(steps + 1):
        info = pl.info()
        assert info["total_vnodes"] > 0 and info["expansions"] > 0
        assert np.isfinite(v) and 0 <= a <= 8
        n = info["n_root_children"]
        for key in ("q_upper_bound", "q_lower_bound", "q_reward"):
            assert np.all(np.isfinite(info[key][:n])), key
        if k < steps:
            a, v = pl.step(a, zs[k])
    pl.close()
