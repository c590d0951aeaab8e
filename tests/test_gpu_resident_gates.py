"""GPU: the sign and finiteness gates of the tile-resident kernels on uploaded
models and carried-over state (path_planning_2d_amd/csrc/pp2_dict_props.h;
the truth table itself: test_resident_gates_cpu.py).

The resident kernels hand a tile's edge rows to the neighbouring CU with the
slot's tag bit in bit 31 of every belief and value word, so they are correct
only while every handed-over word is finite and >= +0.  Here models and states
that break this are put on the two smallest two-tile resident shapes of the
suite -- 8 x 256 (2 CUs, 4 rows per tile: rows 3 | 4 are handed over) and
6 x 510 (2 CUs, 3 rows per tile: rows 2 | 3; the row is no multiple of the
padded width) -- on three contexts with the same inputs:
  r  the defaults (resident allowed, TUNE_RESIDENT_CUS 2),
  s  launch-per-step coded (TUNE_RESIDENT 0, TUNE_STEP_PAIRS 0),
  d  dense (TUNE_CODED_MODEL 0).
Per case: from a fresh belief_set + mdp_reset the first 7 steps of the covering
segment in launches of 2 and 5; from mdp_reset, mdp_sweep(8); mdp_solve(40).
After every call the raw belief bits, the mass bits, J bits and A of r and of
s equal d's (-0 != +0, NaN payloads included), and where all inputs are finite
J and A equal the oracle's sweeps iterated on the uploaded arrays bit for bit.
The path is read from resident_launches() / resident_masked(): both counters
advance on the generated model (uploaded untouched, norm blocks 1 and 8) and
must not move where the gates say no; where the header left a choice only the
bits are asserted.  resident_status()[0] == 0 throughout: no launch timed out
and was replayed (a replay would hide a wrong admission behind a right result).

Every case that can break the invariant is first run on the CPU (the oracle's
sweep and belief update on the same arrays, the device's per-step
normalisation) and must put a negative, -0 or non-finite word into one of the
two handed-over rows after a sweep or step strictly before the last one of a
launch; otherwise the test fails before any device call.  Found (8 x 256 |
6 x 510, words in the two rows):
  main weight of action 1 negated       J after sweeps 3..5: 17, 25, 3 | 62, 74, 8;
                                         belief from step 2 on: 115.. | 209..
  one cell's T[0][0] = +inf / NaN        belief from step 1 on: 2, then all 512 | 1020
  L column zs[2] = 1 negated             belief after step 2: all 512 | 1020
  L column 1 = -0 at every 7th free cell belief after step 2: 59 | 118 words -0
  cost -2.5 at free[::37], all actions   J after every sweep: 11 .. 286 | 22 .. 433
  belief -0 / <0 / inf / NaN             the initial belief itself, one word per row
  carried J (cost -2.5, 8 sweeps)        286 | 433 words at the upload, > 300 | > 450
                                         through the next 6 sweeps
  carried belief (L negated at every     303 | 419 words at the upload, >= 188 | >= 408
  2nd free cell, 5 steps)                through the next 7 steps
These cannot break it, on any cell (asserted on the CPU as well -- the gates
refuse them all the same, which the counters check): a -0 side weight or a -0
cost (a sum that starts at +0 stays +0), and costs of +inf, NaN or 3e38 (the
backup's minimum starts at FLT_MAX and takes `<`, so J stays finite).  The
cost cases set all nine actions of the cells of test_gpu_coded.py's
test_cost_precondition (with its two actions no J changes at all).  gamma = 1.0
or <= 0 never reaches a kernel: pp2_create refuses it.

The belief cases end with a valid belief_set and the resident loop again.  On
6 x 510 that found a third carrier of bad words: the planes' pad columns
(x = 510, 511), which pp2_belief_set did not write and which every kernel
recomputes from their own stale word -- after the +inf belief they held NaN,
and the resident loop's second launch on the valid belief timed out and was
replayed (resident_status()[0] == 1).  pp2_belief_set now zeroes them.
"""
import numpy as np
import pytest

import covering_trajectory as ct
from conftest import GAMMA

pytestmark = pytest.mark.gpu

SHAPES = [(8, 256, 2, (2, 4, 1)), (6, 510, 2, (2, 3, 1))]
IDS = [f"{s[0]}x{s[1]}" for s in SHAPES]
STEPS = 7
LAUNCHES = ((0, 2), (2, 7))
YES, NO, CHOICE = "yes", "no", "choice"


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


# ---------------------------------------------------------------- CPU side
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _viol(x):
    """Words that are negative, -0 or not finite."""
    return int((_bits(x) >= 0x7f800000).sum())


def _sweeps(oracle, H, W, T, Cc, J, n):
    """n oracle sweeps from J: [(J, A)] after each."""
    out = []
    with np.errstate(all="ignore"):
        for _ in range(n):
            J, A = oracle.mdp_sweep(H, W, GAMMA, T, Cc, J)
            out.append((J, A))
    return out


def _steps(oracle, H, W, T, L, b, us, zs):
    """The launch-per-step loop's raw beliefs on the CPU, norm block 1 (every
    step divides by the mass of its input)."""
    tiny = np.finfo(np.float32).tiny
    out = []
    b = b.astype(np.float32)
    with np.errstate(all="ignore"):
        for t in range(len(us)):
            p = oracle.belief_update(H, W, T, L, b, us[t], zs[t])
            p = (p * (np.float32(1.0) / np.float32(b.sum(dtype=np.float64)))).astype(np.float32)
            b = np.where(np.abs(p) < tiny, np.float32(0) * p, p).astype(np.float32)  # FTZ
            out.append(b)
    return out


def _seeded_grid(pp2, H, W):
    """test_gpu_resident_masked.py's grid: the first seed whose model is coded."""
    from path_planning_2d_amd import synthetic as S
    for seed in range(H * 7 + W, H * 7 + W + 8):
        grid = S.synth_grid(H, W, seed)
        goal = S.synth_goal(grid)
        with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as c:
            c.model_generate()
            if c.model_dict_info()[1]:
                return grid, goal
    pytest.fail(f"no coded model for {H} x {W}")


class Geo:
    def __init__(self, pp2, H, W, cus, tiling, block=1):
        from path_planning_2d_amd import synthetic as S
        self.H, self.W, self.cus, self.tiling = H, W, cus, tiling
        self.grid, self.goal = _seeded_grid(pp2, H, W)
        self.rt = tiling[1]
        self.edge = slice((self.rt - 1) * W, (self.rt + 1) * W)  # rows rt - 1 and rt
        self.free = np.flatnonzero(self.grid.reshape(-1) == 0)
        self.b0 = S.uniform_belief(self.grid)
        us, zs = ct.segments(block)[0]
        self.us, self.zs = us[:STEPS].copy(), zs[:STEPS].copy()

    def edge_free(self, row):
        c = self.free[(self.free >= row * self.W) & (self.free < (row + 1) * self.W)]
        return int(c[len(c) // 2])


def _reaches_J(oracle, g, T, Cc, J0, n, want, what):
    """want: some J of sweeps 1 .. n - 1 has a bad word in the edge rows (or,
    want False: no sweep's J has one anywhere).  Returns the counts."""
    js = _sweeps(oracle, g.H, g.W, T, Cc, J0, n)
    cnt = [_viol(J[g.edge]) for J, _ in js]
    print(f"{what}: bad J words in rows {g.rt - 1} | {g.rt} after each sweep: {cnt}")
    if want:
        assert max(cnt[:-1]) > 0, f"{what}: no bad value reaches the handed-over rows of J"
    else:
        assert sum(_viol(J) for J, _ in js) == 0, f"{what}: J does break the invariant"
    return cnt


def _reaches_b(oracle, g, T, L, b, want, what):
    """The 7 steps from b: a bad word in the edge rows of the belief a launch
    starts from or of a step's result before the launch's last."""
    bs = _steps(oracle, g.H, g.W, T, L, b, g.us, g.zs)
    cnt = [_viol(b[g.edge])] + [_viol(x[g.edge]) for x in bs]
    print(f"{what}: bad belief words in rows {g.rt - 1} | {g.rt} at the start and after each "
          f"step: {cnt}")
    if want:
        for lo, hi in LAUNCHES[1:]:
            assert max(cnt[lo:hi]) > 0, f"{what}: launch [{lo}, {hi}) hands no bad belief over"
    else:
        assert _viol(b) + sum(_viol(x) for x in bs) == 0, f"{what}: the belief does break it"
    return cnt


# ---------------------------------------------------------------- device side
def _contexts(pp2, g, block):
    cs = [pp2.GridContext(g.grid, g.goal, gamma=float(GAMMA)) for _ in range(3)]
    r, s, d = cs
    for c in cs:
        c.model_generate()
        assert c.model_dict_info()[1]
        c.set_tuning(c.TUNE_NORM_BLOCK, block)
    r.set_tuning(r.TUNE_RESIDENT_CUS, g.cus)
    s.set_tuning(s.TUNE_RESIDENT, 0)
    s.set_tuning(s.TUNE_STEP_PAIRS, 0)
    d.set_tuning(d.TUNE_CODED_MODEL, 0)
    assert r.resident_tiling() == g.tiling
    assert not d.model_dict_info()[1]
    return cs


def _compare(cs, what, JA=None):
    r, s, d = cs
    for c in cs:
        c.synchronize()
    rd, md = d.belief_get_raw()
    Jd, Ad = d.mdp_get()
    for name, c in (("r", r), ("s", s)):
        rc, mc = c.belief_get_raw()
        Jc, Ac = c.mdp_get()
        np.testing.assert_array_equal(_bits(rc), _bits(rd), err_msg=f"raw belief, {name} vs d, {what}")
        assert _bits(np.float32(mc)) == _bits(np.float32(md)), (what, name, mc, md)
        np.testing.assert_array_equal(_bits(Jc), _bits(Jd), err_msg=f"J, {name} vs d, {what}")
        np.testing.assert_array_equal(Ac, Ad, err_msg=f"A, {name} vs d, {what}")
    if JA is not None:
        np.testing.assert_array_equal(_bits(Jd), _bits(JA[0]), err_msg=f"J vs the oracle, {what}")
        np.testing.assert_array_equal(Ad, JA[1], err_msg=f"A vs the oracle, {what}")
    for c in cs:
        assert c.resident_status()[0] == 0, f"a resident launch timed out and was replayed: {what}"
    assert s.resident_launches() == (0, 0) and d.resident_launches() == (0, 0), what
    return rd, Jd


def _moved(r, before, kind, expect, what):
    """kind 0: the loop's launches (and the masked form's), 1: the sweeps'."""
    now = r.resident_launches() + (r.resident_masked()[1],)
    if expect == YES:
        assert now[kind] > before[kind], f"not resident: {what}"
        if kind == 0:
            assert now[2] - before[2] == now[0] - before[0], f"not the masked form: {what}"
    elif expect == NO:
        assert now[kind] == before[kind], f"resident on a refused model or state: {what}"
    assert now[1 - kind] == before[1 - kind], what


def _snap(r):
    return r.resident_launches() + (r.resident_masked()[1],)


def _loop_part(cs, g, expect, what, oracle_J=None):
    """The 7 steps in launches of 2 and 5.  oracle_J: [(J, A)] after 1 .. 7
    sweeps, or None."""
    r = cs[0]
    for lo, hi in LAUNCHES:
        before = _snap(r)
        for c in cs:
            c.loop_run(g.us[lo:hi], g.zs[lo:hi])
        w = f"{what}, loop steps [{lo}, {hi})"
        _compare(cs, w, oracle_J[hi - 1] if oracle_J else None)
        _moved(r, before, 0, expect, w)


def _sweep_part(cs, n, expect, what, oracle_J=None):
    r = cs[0]
    before = _snap(r)
    for c in cs:
        c.mdp_sweep(n)
    _compare(cs, f"{what}, mdp_sweep({n})", oracle_J[n - 1] if oracle_J else None)
    _moved(r, before, 1, expect, f"{what}, mdp_sweep({n})")


def _solve_part(cs, g, oracle, model, expect, what):
    r = cs[0]
    before = _snap(r)
    res = [c.mdp_solve(40) for c in cs]
    assert res[0][0] == res[2][0] == res[1][0], (what, res)
    assert np.array_equal(np.float64([x[1] for x in res]).view(np.uint64)[:2],
                          np.float64([res[2][1]] * 2).view(np.uint64)), (what, res)
    JA = None
    if model is not None:
        JA = _sweeps(oracle, g.H, g.W, model[0], model[2], np.zeros(g.H * g.W, np.float32),
                     res[2][0])[-1]
    _compare(cs, f"{what}, mdp_solve(40) = {res[2]}", JA)
    _moved(r, before, 1, expect, f"{what}, mdp_solve")


def _fresh(cs, g, b0=None):
    for c in cs:
        c.belief_set(g.b0 if b0 is None else b0)
        c.mdp_reset()


def _upload(cs, model, R0):
    T, L, Cc = model
    for c in cs:
        c.model_upload(T, L, R0, Cc)


def _finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


# ---------------------------------------------------------------- model cases
def _model_cases(g, T0, L0, C0):
    """name -> (T, L, C, loop, sweep, what must reach the edge rows)."""
    W, rt = g.W, g.rt
    out = {}
    T = T0.copy()
    m = T[:, 1, 1]
    m[m > 0] *= np.float32(-1)
    out["main_weight_negated"] = (T, L0, C0, NO, NO, "Jb")
    T = T0.copy()
    side = T[:, 5, :]
    side[(side == np.float32(0.1)) & (np.arange(9) != 4)[None, :]] = np.float32(-0.0)
    assert _viol(T) > 0
    out["side_weight_neg_zero"] = (T, L0, C0, NO, CHOICE, "none")
    cell = next(int(c) for c in g.free if (rt - 1) * W <= c < (rt + 1) * W and T0[c, 0, 0] > 0)
    for name, v in (("weight_inf", np.inf), ("weight_nan", np.nan)):
        T = T0.copy()
        T[cell, 0, 0] = np.float32(v)
        out[name] = (T, L0, C0, NO, NO, "b")
    z = int(g.zs[2])
    L = L0.copy()
    col = L[:, z]
    col[col > 0] *= np.float32(-1)
    out["L_column_negated"] = (T0, L, C0, NO, CHOICE, "b")
    L = L0.copy()
    L[g.free[::7], z] = np.float32(-0.0)
    out["L_column_neg_zero"] = (T0, L, C0, NO, CHOICE, "b")
    for name, v in (("neg_zero", -0.0), ("negative", -2.5), ("inf", np.inf), ("nan", np.nan),
                    ("huge", 3.0e38)):
        Cc = C0.copy()
        Cc[g.free[::37], :] = np.float32(v)
        out["cost_" + name] = (T0, L0, Cc, NO, NO, "J" if name == "negative" else "none")
    return out


MODEL_CASES = ["main_weight_negated", "side_weight_neg_zero", "weight_inf", "weight_nan",
               "L_column_negated", "L_column_neg_zero", "cost_neg_zero", "cost_negative",
               "cost_inf", "cost_nan", "cost_huge"]


@pytest.mark.parametrize("block", [1, 8])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_generated_model_uploaded_runs_resident(pp2, oracle, H, W, cus, tiling, block):
    """The control: the downloaded model uploaded untouched stays on the masked
    resident loop and the resident sweeps, and equals dense and the oracle."""
    g = Geo(pp2, H, W, cus, tiling, block)
    cs = _contexts(pp2, g, block)
    r, s, d = cs
    with r, s, d:
        T0, L0, R0, C0 = r.model_download()
        assert _viol(T0) + _viol(L0) + _viol(C0) == 0
        _upload(cs, (T0, L0, C0), R0)
        for c in (r, s):
            assert c.model_dict_info()[1]
        assert r.resident_masked() == (True, 0) and r.loop_steps_per_launch() == 2048
        oj = _sweeps(oracle, H, W, T0, C0, np.zeros(H * W, np.float32), 8)
        _fresh(cs, g)
        _loop_part(cs, g, YES, f"control, block {block}", oj)
        for c in cs:
            c.mdp_reset()
        _sweep_part(cs, 8, YES, f"control, block {block}", oj)
        _solve_part(cs, g, oracle, (T0, L0, C0), YES, f"control, block {block}")
        lo, so = r.resident_launches()
        assert lo == len(LAUNCHES) and so >= 2 and r.resident_masked() == (True, lo)


@pytest.mark.parametrize("case", MODEL_CASES)
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_model_that_breaks_the_invariant(pp2, oracle, H, W, cus, tiling, case):
    g = Geo(pp2, H, W, cus, tiling)
    cs = _contexts(pp2, g, 1)
    r, s, d = cs
    with r, s, d:
        T0, L0, R0, C0 = r.model_download()
        T, L, Cc, loop, sweep, reach = _model_cases(g, T0, L0, C0)[case]
        what = f"{case} {H} x {W}"
        # the CPU conditions, before any device call on the changed model
        zero = np.zeros(H * W, np.float32)
        if "J" in reach:
            _reaches_J(oracle, g, T, Cc, zero, 8, True, what)
            _reaches_J(oracle, g, T, Cc, zero, STEPS, True, what + " (the loop's sweeps)")
        if "b" in reach:
            _reaches_b(oracle, g, T, L, g.b0, True, what)
        if reach == "none":
            _reaches_J(oracle, g, T, Cc, zero, 8, False, what)
            _reaches_b(oracle, g, T, L, g.b0, False, what)
        finite = _finite(T, L, Cc)
        oj = _sweeps(oracle, H, W, T, Cc, zero, 8) if finite else None
        if oj is not None and not _finite(*[J for J, _ in oj]):
            oj = None
        _upload(cs, (T, L, Cc), R0)
        _fresh(cs, g)
        for c in (r, s):
            assert c.model_dict_info()[1], "the coded path stays active"
        assert r.loop_steps_per_launch() == 1, "the loop's gate refuses the model"
        assert r.resident_tiling() == (0, 0, 0)
        _loop_part(cs, g, loop, what, oj)
        for c in cs:
            c.mdp_reset()
        _sweep_part(cs, 8, sweep, what, oj)
        _solve_part(cs, g, oracle, (T, L, Cc) if oj is not None else None, sweep, what)
        if loop == NO and sweep == NO:
            assert r.resident_launches() == (0, 0) and r.resident_masked()[1] == 0


def test_discount_outside_the_unit_interval_is_refused(pp2):
    """gamma = 1.0, 0 and negative never reach a gate: pp2_create refuses."""
    g = Geo(pp2, *SHAPES[0])
    for gamma in (1.0, -0.5, 0.0, float("nan")):
        with pytest.raises(Exception, match="discount"):
            pp2.GridContext(g.grid, g.goal, gamma=gamma)


# ---------------------------------------------------------------- belief cases
@pytest.mark.parametrize("bad", ["neg_zero", "negative", "inf", "nan"])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_belief_that_breaks_the_invariant(pp2, oracle, H, W, cus, tiling, bad):
    g = Geo(pp2, H, W, cus, tiling)
    val = {"neg_zero": -0.0, "negative": -1e-3, "inf": np.inf, "nan": np.nan}[bad]
    bb = g.b0.copy()
    cells = [g.edge_free(g.rt - 1), g.edge_free(g.rt)]
    bb[cells] = np.float32(val)
    assert _viol(bb[g.edge]) == 2, "one bad word in each handed-over row"
    cs = _contexts(pp2, g, 1)
    r, s, d = cs
    with r, s, d:
        T0, L0, R0, C0 = r.model_download()
        oj = _sweeps(oracle, H, W, T0, C0, np.zeros(H * W, np.float32), STEPS)
        _fresh(cs, g, bb)
        assert r.loop_steps_per_launch() == 1 and not r.model_dict_info()[1]
        _loop_part(cs, g, NO, f"belief {bad} {H} x {W}", oj)
        assert r.resident_launches() == (0, 0)
        # a valid belief again: the resident loop again
        _fresh(cs, g)
        _loop_part(cs, g, YES, f"belief {bad} {H} x {W}, set again", oj)


# ---------------------------------------------------------------- carry-over
def _carry_models(g, T0, L0, C0):
    Cc = C0.copy()
    Cc[g.free[::37], :] = np.float32(-2.5)
    L = L0.copy()
    L[g.free[::2], :] *= np.float32(-1)
    return (T0, L0, Cc), (T0, L, C0)


def _clean_again(cs, how, model, R0):
    if how == "upload":
        _upload(cs, model, R0)
    else:
        for c in cs:
            c.model_generate()


@pytest.mark.parametrize("how", ["upload", "generate"])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_values_carried_over_a_model_change(pp2, oracle, H, W, cus, tiling, how):
    """J swept negative under a negative-cost model, then the clean model with
    no mdp_reset: mdp_sweep(6) and the loop start from that J."""
    g = Geo(pp2, H, W, cus, tiling)
    cs = _contexts(pp2, g, 1)
    r, s, d = cs
    with r, s, d:
        T0, L0, R0, C0 = r.model_download()
        negc, _ = _carry_models(g, T0, L0, C0)
        what = f"carried J ({how}) {H} x {W}"
        zero = np.zeros(H * W, np.float32)
        o8 = _sweeps(oracle, H, W, T0, negc[2], zero, 8)
        J8 = o8[-1][0]
        assert _viol(J8[g.edge]) > 0, "the carried J is bad in the handed-over rows"
        _reaches_J(oracle, g, T0, C0, J8, 6, True, what)
        o6 = _sweeps(oracle, H, W, T0, C0, J8, 6)
        _reaches_J(oracle, g, T0, C0, o6[-1][0], STEPS, True, what + " (the loop's sweeps)")
        o7 = _sweeps(oracle, H, W, T0, C0, o6[-1][0], STEPS)
        assert _finite(*[J for J, _ in o8 + o6 + o7])
        _upload(cs, negc, R0)
        _fresh(cs, g)
        _sweep_part(cs, 8, NO, what + ", the negative-cost model", o8)
        _clean_again(cs, how, (T0, L0, C0), R0)
        assert not r.model_dict_info()[1] and not s.model_dict_info()[1], \
            "a sparse dictionary over a J that may be negative"
        assert r.resident_masked()[0] is True, "(the model itself is admitted)"
        _sweep_part(cs, 6, NO, what + ", clean model, no reset", o6)
        _loop_part(cs, g, NO, what + ", clean model, no reset", o7)
        assert r.resident_launches() == (0, 0)
        # reset: resident again
        for c in cs:
            c.mdp_reset()
        assert r.model_dict_info()[1] and r.loop_steps_per_launch() == 2048
        oj = _sweeps(oracle, H, W, T0, C0, zero, 8)
        _sweep_part(cs, 8, YES, what + ", after mdp_reset", oj)
        for c in cs:
            c.mdp_reset()
        _loop_part(cs, g, YES, what + ", after mdp_reset", oj)


@pytest.mark.parametrize("how", ["upload", "generate"])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_belief_carried_over_a_model_change(pp2, oracle, H, W, cus, tiling, how):
    """A belief stepped negative under a negated-L model, then the clean model
    with no belief_set: the loop starts from that belief."""
    g = Geo(pp2, H, W, cus, tiling)
    cs = _contexts(pp2, g, 1)
    r, s, d = cs
    with r, s, d:
        T0, L0, R0, C0 = r.model_download()
        _, negl = _carry_models(g, T0, L0, C0)
        what = f"carried belief ({how}) {H} x {W}"
        b5 = _steps(oracle, H, W, T0, negl[1], g.b0, g.us[:5], g.zs[:5])
        assert _viol(b5[-1][g.edge]) > 0, "the carried belief is bad in the handed-over rows"
        after = _reaches_b(oracle, g, T0, L0, b5[-1], True, what)
        assert min(after[:-1]) > 0 and _finite(*b5)
        oj = _sweeps(oracle, H, W, T0, C0, np.zeros(H * W, np.float32), 5 + STEPS)
        _upload(cs, negl, R0)
        _fresh(cs, g)
        assert r.model_dict_info()[1] and r.loop_steps_per_launch() == 1
        before = _snap(r)
        for c in cs:
            c.loop_run(g.us[:5], g.zs[:5])
        raw, _ = _compare(cs, what + ", the negated-L model", oj[4])
        _moved(r, before, 0, NO, what + ", the negated-L model")
        assert _viol(raw[g.edge]) > 0, "the device's belief is bad in the handed-over rows"
        _clean_again(cs, how, (T0, L0, C0), R0)
        assert not r.model_dict_info()[1] and not s.model_dict_info()[1], \
            "a sparse dictionary over a belief that may be negative"
        assert r.loop_steps_per_launch() == 1
        _loop_part(cs, g, NO, what + ", clean model, no belief_set", oj[5:])
        assert r.resident_launches() == (0, 0)
        # a belief set again: resident again
        for c in cs:
            c.belief_set(g.b0)
        assert r.model_dict_info()[1] and r.loop_steps_per_launch() == 2048
        _loop_part(cs, g, YES, what + ", after belief_set")
        _sweep_part(cs, 2, YES, what + ", after belief_set")
