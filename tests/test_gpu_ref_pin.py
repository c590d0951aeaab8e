"""The streaming device kernels against the reference's own kernels built for
the host (oracle/ref.py, the contracted-fma build), at the geometry where
their indexing can go wrong: one row, one column, and widths one below, at
and one above the 256-lane block span and the padded row width, at every
cells-per-lane setting and on the coded and dense model paths.

The expected values come from the reference library alone, not from the CPU
oracle.  Model tensors, the unnormalised belief, Bellman values and actions and
FIB alphas are compared bit for bit; the loop's normalised belief is held to
the project's bar (rel 1e-5 with the FLT_MIN floor).  The module reads only
oracle/_ref/ and skips only where those libraries were not built.
"""
import numpy as np
import pytest

from conftest import GAMMA, assert_rel_close
from oracle import ref as REF
from ref_pin_cases import GPU_SHAPES, belief, bits, goals, grid, shape_id

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not REF.available(),
                                 reason="oracle/_ref libraries are not built")]

SWEEPS = 7
LOOP_STEPS = 5


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


class Case:
    """One shape's inputs and reference results, each computed on first use
    and then shared read-only by every test of the module."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.grid = grid(H, W)
        self.goal = goals(H, W)[1]
        self._memo = {}

    def _once(self, key, make):
        if key not in self._memo:
            out = make()
            for a in (out if isinstance(out, tuple) else (out,)):
                a.setflags(write=False)
            self._memo[key] = out
        return self._memo[key]

    @property
    def pomdp(self):
        return self._once("pomdp", lambda: REF.model_pomdp(self.grid, self.goal))

    @property
    def mdp(self):
        return self._once("mdp", lambda: REF.model_mdp(self.grid, self.goal))

    @property
    def b0(self):
        return self._once("b0", lambda: belief(self.grid))

    def sweeps(self, n):
        """(J, A) after n reference Bellman sweeps from J = 0."""
        def make():
            Tm, C = self.mdp
            J = np.zeros(self.H * self.W, np.float32)
            A = np.zeros(self.H * self.W, np.uint8)
            for _ in range(n):
                J, A = REF.mdp_sweep(self.H, self.W, GAMMA, Tm, C, J)
            return J, A
        return self._once(("sweeps", n), make)

    @property
    def fib3(self):
        def make():
            T, L, R = self.pomdp
            a = np.zeros((self.H * self.W, 9), np.float32)
            for _ in range(3):
                a = REF.fib_sweep(self.H, self.W, GAMMA, T, L, R, a)
            return a
        return self._once("fib3", make)

    @property
    def trajectory(self):
        def make():
            rng = np.random.default_rng(5 + 3 * self.H + self.W)
            return (rng.integers(0, 9, LOOP_STEPS).astype(np.uint8),
                    rng.integers(0, 16, LOOP_STEPS).astype(np.uint8))
        return self._once("traj", make)

    @property
    def loop_belief(self):
        """LOOP_STEPS steps of reference kernel + fp64 normalisation."""
        def make():
            T, L, _ = self.pomdp
            us, zs = self.trajectory
            b = self.b0
            for u, z in zip(us, zs):
                raw = REF.belief_update(self.H, self.W, T, L, b, u, z).astype(np.float64)
                b = (raw / raw.sum()).astype(np.float32)
            return b
        return self._once("loop_belief", make)


_cases = {}


@pytest.fixture(params=GPU_SHAPES, ids=shape_id)
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(*request.param)
    return _cases[request.param]


def make_ctx(pp2, case, cpt=4, coded=1):
    ctx = pp2.GridContext(case.grid, case.goal, gamma=float(GAMMA))
    ctx.set_cells_per_lane(cpt)
    ctx.model_generate()
    ctx.set_tuning(ctx.TUNE_CODED_MODEL, coded)
    return ctx


def test_model_generation(pp2, case):
    T, L, R = case.pomdp
    Tm, C = case.mdp
    with make_ctx(pp2, case) as ctx:
        Td, Ld, Rd, Cd = ctx.model_download()
    np.testing.assert_array_equal(Td, T)
    np.testing.assert_array_equal(Td, Tm)  # the device keeps one T for both models
    np.testing.assert_array_equal(Ld, L)
    np.testing.assert_array_equal(Rd, R)
    np.testing.assert_array_equal(Cd, C)


@pytest.mark.parametrize("coded", [1, 0], ids=["coded", "dense"])
@pytest.mark.parametrize("cpt", [1, 2, 4])
def test_belief_update_raw(pp2, case, cpt, coded):
    T, L, _ = case.pomdp
    with make_ctx(pp2, case, cpt, coded) as ctx:
        for u in range(9):
            for z in (0, 5, 10, 15):
                ctx.belief_set(case.b0)
                ctx.belief_update(u, z)
                raw, _ = ctx.belief_get_raw()
                want = REF.belief_update(case.H, case.W, T, L, case.b0, u, z)
                np.testing.assert_array_equal(bits(raw), bits(want), err_msg=f"u={u} z={z}")


@pytest.mark.parametrize("coded", [1, 0], ids=["coded", "dense"])
@pytest.mark.parametrize("cpt", [1, 2, 4])
def test_mdp_sweeps(pp2, case, cpt, coded):
    J, A = case.sweeps(SWEEPS)
    with make_ctx(pp2, case, cpt, coded) as ctx:
        ctx.mdp_reset()
        for _ in range(SWEEPS):
            ctx.mdp_sweep(1)
        J1, A1 = ctx.mdp_get()
        ctx.mdp_reset()
        ctx.mdp_sweep(SWEEPS)  # one call: may run as one resident launch
        Jn, An = ctx.mdp_get()
    for got_j, got_a, how in ((J1, A1, "single sweeps"), (Jn, An, "one call")):
        np.testing.assert_array_equal(bits(got_j), bits(J), err_msg=how)
        np.testing.assert_array_equal(got_a, A, err_msg=how)


@pytest.mark.parametrize("kernel", ["dense", "sparse", "lds"])
def test_fib_sweeps(pp2, monkeypatch, case, kernel):
    """k_fib_sweep (dense model), k_fib_sweep_sparse and k_fib_sweep_lds
    (coded model; PP2_FIB_LDS picks between the two)."""
    monkeypatch.setenv("PP2_FIB_LDS", "1" if kernel == "lds" else "0")
    with make_ctx(pp2, case, 4, 0 if kernel == "dense" else 1) as ctx:
        if kernel != "dense":
            assert ctx.model_dict_info()[1], "support-only FIB path not selected"
        ctx.fib_reset()
        ctx.fib_sweep(3)
        got = ctx.fib_get()
    np.testing.assert_array_equal(bits(got), bits(case.fib3))


@pytest.mark.parametrize("coded", [1, 0], ids=["coded", "dense"])
def test_loop_run(pp2, case, coded):
    us, zs = case.trajectory
    J, A = case.sweeps(LOOP_STEPS)
    with make_ctx(pp2, case, 4, coded) as ctx:
        ctx.set_tuning(ctx.TUNE_NORM_BLOCK, 1)
        ctx.belief_set(case.b0)
        ctx.mdp_reset()
        ctx.loop_run(us, zs)
        b = ctx.belief_get()
        Jd, Ad = ctx.mdp_get()
    np.testing.assert_array_equal(bits(Jd), bits(J))
    np.testing.assert_array_equal(Ad, A)
    assert_rel_close(b, case.loop_belief, rel=1e-5, msg="loop belief")
