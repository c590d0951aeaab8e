"""GPU: episodes whose world differs from the believed map, and resumed
segments (pp2_episodes_set_world, pp2_episodes_resume; the EXT instances of
k_episodes in csrc/pp2_episodes.hip) against the free-running NumPy reference
tests/episodes_world_reference.py.  Everything is compared as bit patterns: the
reference is fed the device's own Q planes, action plane, alpha sets, reward
planes and models, as the other episode tests' references are.

Shapes (``WR.world_case``): 9 x 13 (row stride 16, three pad columns, a wall in
the room), 7 x 10 (stride 12), 8 x 12 (no pad column, the world's obstacle on
the border, another goal in the world).  16 episodes, horizon 40, traces on.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import episodes_reference as R
import episodes_world_reference as WR
from conftest import GAMMA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESTATE, EINVAL = 5, 1
CASES = ("9x13", "7x10", "8x12")
POLICIES = ("mode", "qmdp", "fib", "pbvi", "fib-lookahead", "pbvi-lookahead")
PLACEMENTS = ("lds", "global")
PBVI_S = 12


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model_of(ctx, grid, goal):
    T, L, Rw, Cc = ctx.model_download()
    return R.Model(grid, goal, GAMMA, T=T, L=L, C=Cc), Rw


def solved_ctx(pp2, grid, goal, b0):
    """A believed context with everything the six policies read."""
    ctx = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    ctx.model_generate()
    ctx.mdp_solve()
    ctx.fib_solve()
    ctx.pbvi_belief_set(b0, PBVI_S)
    ctx.pbvi_backup(2)
    return ctx


def world_ctx(pp2, grid, goal):
    ctx = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    ctx.model_generate()
    return ctx


class Setup:
    def __init__(self, pp2, name):
        from path_planning_2d_amd import synthetic as S
        self.case = c = WR.world_case(name)
        self.b0 = S.uniform_belief(c["believed"])
        self.ctx = solved_ctx(pp2, c["believed"], c["goal"], self.b0)
        self.world = world_ctx(pp2, c["world"], c["world_goal"])
        self.mp, self.Rw = model_of(self.ctx, c["believed"], c["goal"])
        self.mw, _ = model_of(self.world, c["world"], c["world_goal"])
        self.refs = {}

    def close(self):
        self.world.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def setups(pp2):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Setup(pp2, name)
        return made[name]
    yield get
    for s in made.values():
        s.close()


def control_of(ep, ctx, mp, Rw, policy):
    """The reference's step 1 from what the last run of ``ep`` read on the device."""
    wp = ctx.row_stride
    if policy == "mode":
        return WR.mode_control(mp, ctx.mdp_get()[1])
    if policy == "qmdp":
        return WR.qmdp_control(mp, ep.qplanes(), wp)
    al, act = ep.alphas()
    if policy in ("fib", "pbvi"):
        return WR.alpha_control(mp, al, act, wp)
    return WR.look_control(mp, Rw, al, wp)


def snapshot(ep, policy):
    """Every output of the last run, floats as bit patterns."""
    out = dict(ep.results())
    if ep.record_trace:
        out.update(ep.trace())
        if policy in ("fib", "pbvi"):
            out.update(ep.trace_alpha())
        elif policy.endswith("lookahead"):
            out.update(ep.trace_lookahead())
    out["beliefs"] = np.stack([ep.belief(e) for e in range(ep.episodes)])
    return {k: bits(v) if v.dtype == np.float32 else v for k, v in out.items()}


def assert_snapshots_equal(got, want, what, keys=None):
    for k in keys or want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def ref_snapshot(ref, like):
    """The reference batch with the keys and representation of a device snapshot."""
    return {k: bits(ref[k]) if ref[k].dtype == np.float32 else ref[k] for k in like}


def run(ep, policy, b0, starts, seed):
    return ep.run(policy, b0, starts, seed, placed=True)


# ---------------------------------------------------------------- world parity
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", CASES)
def test_world_parity(pp2, setups, name, policy):
    """Every output of a run under a world == the reference, from LDS planes and
    from device-memory planes, and the two placements agree."""
    s = setups(name)
    c = s.case
    if name == "9x13":
        assert s.ctx.row_stride == 16
    if name == "8x12":
        assert s.ctx.row_stride == 12 and c["goal"] != c["world_goal"]
    snaps = {}
    for placement in PLACEMENTS:
        with pp2.EpisodeBatch(s.ctx, len(c["starts"]), c["horizon"], record_trace=True,
                              placement=placement) as ep:
            ep.set_world(s.world)
            run(ep, policy, s.b0, c["starts"], c["seed"])
            assert ep.placement()["last"] == PLACEMENTS.index(placement)
            if policy not in s.refs:
                s.refs[policy] = WR.run_batch(s.mp, s.mw, control_of(ep, s.ctx, s.mp, s.Rw, policy),
                                              s.b0, c["starts"], c["horizon"], c["seed"])
            snaps[placement] = snapshot(ep, policy)
        ref = s.refs[policy]
        assert_snapshots_equal(snaps[placement], ref_snapshot(ref, snaps[placement]),
                               f"{name} {policy} {placement}")
    assert_snapshots_equal(snaps["lds"], snaps["global"], f"{name} {policy} LDS == global")
    ref = s.refs[policy]
    # the start on the world's goal takes no step; the one on a cell that only
    # the believed map holds occupied runs
    assert ref["steps"][14] == 0 and ref["status"][14] == 1 and ref["steps"][15] > 0
    assert (ref["status"] == 0).any()


def test_world_differs_from_the_plain_run(pp2, setups):
    """The world is read: under it the 9 x 13 QMDP run is another run."""
    s = setups("9x13")
    c = s.case
    with pp2.EpisodeBatch(s.ctx, 16, c["horizon"], record_trace=True) as ep:
        run(ep, "qmdp", s.b0, c["starts"], c["seed"])
        plain = snapshot(ep, "qmdp")
        ep.set_world(s.world)
        run(ep, "qmdp", s.b0, c["starts"], c["seed"])
        under = snapshot(ep, "qmdp")
    assert not np.array_equal(plain["cells"], under["cells"])
    wall = {y * 13 + 6 for y in range(2, 7)}
    assert wall & set(plain["cells"].reshape(-1).tolist())      # the stale map drives through
    assert not wall & set(under["cells"].reshape(-1).tolist())  # the world does not let it


# ---------------------------------------------------------------- world == own context
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("policy", POLICIES)
def test_own_context_as_world_is_the_plain_run(pp2, setups, policy, placement):
    s = setups("9x13")
    c = s.case
    with pp2.EpisodeBatch(s.ctx, 16, c["horizon"], record_trace=True, placement=placement) as ep:
        run(ep, policy, s.b0, c["starts"], c["seed"])
        plain = snapshot(ep, policy)
        info = ep.info()
        ep.set_world(s.ctx)
        run(ep, policy, s.b0, c["starts"], c["seed"])
        assert_snapshots_equal(snapshot(ep, policy), plain, f"{policy} world = own context")
        assert ep.info() == info  # no LDS layout grows, the launch is sized alike
        ep.set_world(s.world)
        run(ep, policy, s.b0, c["starts"], c["seed"])
        ep.set_world(None)  # detaching restores the plain run
        run(ep, policy, s.b0, c["starts"], c["seed"])
        assert_snapshots_equal(snapshot(ep, policy), plain, f"{policy} detached")


def test_second_context_with_the_same_map_is_the_plain_run(pp2, setups):
    s = setups("7x10")
    c = s.case
    with world_ctx(pp2, c["believed"], c["goal"]) as twin:
        for policy in ("mode", "qmdp", "fib-lookahead"):
            with pp2.EpisodeBatch(s.ctx, 16, c["horizon"], record_trace=True) as ep:
                run(ep, policy, s.b0, c["starts"], c["seed"])
                plain = snapshot(ep, policy)
                ep.set_world(twin)
                run(ep, policy, s.b0, c["starts"], c["seed"])
                assert_snapshots_equal(snapshot(ep, policy), plain, f"{policy} twin world")


# ---------------------------------------------------------------- resume
RESUME_CASES = [("mode", "lds"), ("mode", "global"), ("qmdp", "lds"), ("qmdp", "global"),
                ("fib-lookahead", "lds")]
TRACE_KEYS = {"mode": ("mode_cells",), "qmdp": ("qsums",),
              "fib-lookahead": ("qsums", "q", "rewards", "leaf_max", "leaf_index")}


@pytest.fixture(scope="module")
def resume_setup(pp2, setups):
    """9 x 13 with cell (0, 0) of the world walled in and b0 = 2^-125 on every
    believed-free cell: the robots that start in the pocket observe z = 15,
    which the believed map makes unlikely everywhere, so their first update
    underflows to zero -- status 2 in segment 1 -- while the others carry on."""
    s = setups("9x13")
    c = s.case
    W = 13
    pocket = WR.pocket_world(c)
    starts = np.array(list(c["starts"][:10]) + [0, 0, 4 * W + 9, 4 * W + 10, 3 * W + 10, 4 * W + 11],
                      np.int32)
    world = world_ctx(pp2, pocket, c["world_goal"])
    mw, _ = model_of(world, pocket, c["world_goal"])
    yield s, world, mw, WR.tiny_b0(c["believed"]), starts
    world.close()


@pytest.mark.parametrize("policy,placement", RESUME_CASES)
@pytest.mark.parametrize("with_world", [True, False])
def test_resume_equals_the_long_run(pp2, resume_setup, policy, placement, with_world):
    """run + resume + resume on a horizon-12 batch == one run of a horizon-36
    batch: results, beliefs and the concatenated traces.  Without a world the
    first segment is a plain launch, which stores no discounts: the resume makes
    them up from the steps (the costs are compared bit for bit)."""
    s, world, mw, b0, starts = resume_setup
    c = s.case
    seed = c["seed"]
    E = len(starts)
    res_keys = ("steps", "status", "cost", "final_cell", "beliefs")
    tr_keys = ("actions", "observations", "cells") + TRACE_KEYS[policy]
    with pp2.EpisodeBatch(s.ctx, E, 36, record_trace=True, placement=placement) as long_ep:
        long_ep.set_world(world if with_world else None)
        run(long_ep, policy, b0, starts, seed)
        whole = snapshot(long_ep, policy)
        if policy != "fib-lookahead":  # (its reference: 144 belief updates a step)
            ref = WR.run_batch(s.mp, mw if with_world else s.mp,
                               control_of(long_ep, s.ctx, s.mp, s.Rw, policy), b0, starts, 36, seed)
            assert_snapshots_equal(whole, ref_snapshot(ref, whole), f"{policy} long run")
    with pp2.EpisodeBatch(s.ctx, E, 12, record_trace=True, placement=placement) as ep:
        ep.set_world(world if with_world else None)
        with pytest.raises(pp2.Pp2Error) as err:
            ep.resume(policy, seed)
        assert err.value.status == ESTATE  # nothing has run yet
        run(ep, policy, b0, starts, seed)
        segs = [snapshot(ep, policy)]
        for _ in range(2):
            ep.resume(policy, seed)
            segs.append(snapshot(ep, policy))
        assert ep.placement()["last"] == PLACEMENTS.index(placement)
    assert_snapshots_equal(segs[2], whole, f"{policy} 12 + 12 + 12", res_keys)
    for k in tr_keys:
        np.testing.assert_array_equal(np.concatenate([g[k] for g in segs]), whole[k],
                                      err_msg=f"{policy} concatenated {k}")
    # episodes that finished in segment 1 are untouched by the later segments,
    # a lost episode's raw belief included
    done = segs[0]["status"] != 0
    for k in res_keys:
        np.testing.assert_array_equal(segs[1][k][done], segs[0][k][done], err_msg=k)
        np.testing.assert_array_equal(segs[2][k][done], segs[0][k][done], err_msg=k)
    assert (segs[1]["actions"][:, done] == 255).all() and (segs[1]["cells"][:, done] == -1).all()
    if with_world:
        lost = segs[0]["status"] == 2
        assert lost[10] and lost[11] and (segs[0]["steps"][lost] == 1).all()
        assert not segs[0]["beliefs"][10].any()  # the raw update: all +0
        assert (segs[0]["status"] == 1).any() and (segs[0]["status"] == 0).any()
        assert (segs[2]["steps"] > 12).any()


# ---------------------------------------------------------------- sense, update, re-plan
def test_sense_update_replan(pp2):
    """Stale believed map, true world, QMDP: 12 steps (three segments of 4),
    pp2_map_update with the wall on the believed context and pp2_mdp_resolve,
    28 more steps (seven segments) == the reference driven the same way, the
    second part on the re-solved device Q and the updated believed model."""
    from path_planning_2d_amd import synthetic as S
    c = WR.world_case("9x13")
    b0 = S.uniform_belief(c["believed"])
    seed, starts = c["seed"], c["starts"]
    with solved_ctx(pp2, c["believed"], c["goal"], b0) as ctx, \
            world_ctx(pp2, c["world"], c["world_goal"]) as world:
        mw, _ = model_of(world, c["world"], c["world_goal"])
        mp1, _ = model_of(ctx, c["believed"], c["goal"])
        with pp2.EpisodeBatch(ctx, 16, 4, record_trace=True) as ep:
            ep.set_world(world)
            run(ep, "qmdp", b0, starts, seed)
            Q1 = ep.qplanes()
            ep.resume("qmdp", seed).resume("qmdp", seed)
            np.testing.assert_array_equal(bits(ep.qplanes()), bits(Q1))
            part1 = snapshot(ep, "qmdp")
            ctx.map_update(np.ones((5, 1), np.uint8), x0=6, y0=2)
            ctx.mdp_resolve()
            sensed = c["believed"].copy()
            sensed[2:7, 6] = 1
            mp2, _ = model_of(ctx, sensed, c["goal"])
            for _ in range(7):
                ep.resume("qmdp", seed)
            Q2 = ep.qplanes()
            part2 = snapshot(ep, "qmdp")
    assert not np.array_equal(bits(Q1), bits(Q2))
    wp = R.row_stride(13)
    ref1 = WR.run_batch(mp1, mw, WR.qmdp_control(mp1, Q1, wp), b0, starts, 12, seed)
    ref2 = WR.run_batch_segment(mp2, mw, WR.qmdp_control(mp2, Q2, wp), ref1["states"], 28, seed)
    res_keys = ("steps", "status", "cost", "final_cell", "beliefs")
    assert_snapshots_equal(part1, ref_snapshot(ref1, part1), "before the update", res_keys)
    assert_snapshots_equal(part2, ref_snapshot(ref2, part2), "after the update", res_keys)
    for k in ("actions", "observations", "cells", "qsums"):
        want = ref_snapshot(ref2, part2)[k][24:28]
        np.testing.assert_array_equal(part2[k], want, err_msg=f"the last segment's {k}")
    assert (ref2["status"] == 1).sum() > (ref1["status"] == 1).sum()


# ---------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(pp2, setups):
    from path_planning_2d_amd import _lib
    s = setups("7x10")
    c = s.case
    with pp2.EpisodeBatch(s.ctx, 16, 8) as ep:
        run(ep, "qmdp", s.b0, c["starts"], 1)
        before = (ep.info(), ep.results())

        def unchanged():
            assert ep.info() == before[0]
            after = ep.results()
            for k, v in before[1].items():
                np.testing.assert_array_equal(after[k], v, err_msg=k)

        def refused(status, fn):
            with pytest.raises(pp2.Pp2Error) as e:
                fn()
            assert e.value.status == status, e.value
            unchanged()
            return str(e.value)

        # a world of another size
        other = WR.world_case("8x12")
        with world_ctx(pp2, other["world"], other["world_goal"]) as w:
            refused(EINVAL, lambda: ep.set_world(w))
        assert ep.world is None
        # a world without a model: attached, refused at the run
        with pp2.GridContext(c["world"], c["world_goal"], gamma=float(GAMMA)) as w:
            ep.set_world(w)
            for fn in (lambda: run(ep, "qmdp", s.b0, c["starts"], 1),
                       lambda: run(ep, "fib-lookahead", s.b0, c["starts"], 1),
                       lambda: ep.resume("mode", 1)):
                assert "world" in refused(ESTATE, fn)
            ep.set_world(None)
        # a world on the dense path
        with world_ctx(pp2, c["world"], c["world_goal"]) as w:
            w.set_tuning(w.TUNE_CODED_MODEL, 0)
            ep.set_world(w)
            assert "world" in refused(ESTATE, lambda: run(ep, "mode", s.b0, c["starts"], 1))
            assert "world" in refused(ESTATE, lambda: ep.resume("qmdp", 1))
            w.set_tuning(w.TUNE_CODED_MODEL, 1)
            run(ep, "qmdp", s.b0, c["starts"], 1)  # and the batch runs again
            ep.set_world(None)
        # an unknown policy
        for bad in (-1, 6):
            with pytest.raises(pp2.Pp2Error) as e:
                _lib.call("pp2_episodes_resume", ep._h, bad, C.c_uint64(1))
            assert e.value.status == EINVAL
    with pp2.EpisodeBatch(s.ctx, 4, 4) as fresh:  # resume before any run
        info = fresh.info()
        with pytest.raises(pp2.Pp2Error) as e:
            fresh.resume("qmdp", 1)
        assert e.value.status == ESTATE and fresh.info() == info


# ---------------------------------------------------------------- streams
def test_world_on_its_own_stream(pp2, setups):
    """The run reads the world as it stands when it is enqueued: an update of the
    world enqueued right after the run does not reach it, one enqueued right
    before it does."""
    from path_planning_2d_amd import _lib
    hip = _lib.load()  # the HIP runtime's symbols, through the library that links it
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    s = setups("9x13")
    c = s.case
    E = 1024  # long enough a launch that an unordered update would land inside it
    starts = np.resize(c["starts"], E).astype(np.int32)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    opening = np.zeros((5, 1), np.uint8)  # the wall taken away again
    wall = np.ones((5, 1), np.uint8)
    with world_ctx(pp2, c["world"], c["world_goal"]) as w, \
            pp2.EpisodeBatch(s.ctx, E, c["horizon"]) as ep:
        ep.set_world(w)
        run(ep, "qmdp", s.b0, starts, c["seed"])
        walled = snapshot(ep, "qmdp")
        w.map_update(opening, x0=6, y0=2)
        w.synchronize()
        run(ep, "qmdp", s.b0, starts, c["seed"])
        opened = snapshot(ep, "qmdp")
        assert not np.array_equal(walled["final_cell"], opened["final_cell"])
        w.map_update(wall, x0=6, y0=2)
        w.synchronize()
        try:
            w.set_stream(stream.value)
            # run, then update: the run still sees the wall
            run(ep, "qmdp", s.b0, starts, c["seed"])
            w.map_update(opening, x0=6, y0=2)
            assert_snapshots_equal(snapshot(ep, "qmdp"), walled, "update after the run")
            # update, then run (no synchronise in between): the run sees the wall again
            run(ep, "qmdp", s.b0, starts, c["seed"])
            assert_snapshots_equal(snapshot(ep, "qmdp"), opened, "the opened world")
            w.map_update(wall, x0=6, y0=2)
            run(ep, "qmdp", s.b0, starts, c["seed"])
            assert_snapshots_equal(snapshot(ep, "qmdp"), walled, "update before the run")
        finally:
            w.synchronize()
            w.set_stream(None)
            ep.set_world(None)
            assert hip.hipStreamDestroy(stream) == 0


# ---------------------------------------------------------------- the example
def test_sense_demo_runs(pp2):
    exe = os.path.join(ROOT, "examples", "pp2_episodes_sense_demo")
    assert os.path.exists(exe), f"{exe} not built (the csrc Makefile builds it)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pp2_episodes_sense_demo ok" in out.stdout
    for case in ("never updated", "updated at k=", "known from start"):
        assert case in out.stdout
