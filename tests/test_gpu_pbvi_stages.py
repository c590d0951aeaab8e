"""The PBVI backup stage by stage: every intermediate of one warm-started
pp2_pbvi_backup iteration against a plain reference of that stage alone
(pbvi_stage_cases.py), bit for bit, at the tile and padding edges of the five
kernels.

    k_pbvi_gamma_ao   G      against the reference's own cudaComputeGammaOA
                             built for the host (oracle/_ref) where it is
                             built, else the oracle's restatement -- the test
                             id says which
    k_gemm_nt         Cm     against orc_fma_chain_nt of the device's G
    k_argmax_rows     kstar  against the first row maximum of the device's Cm
    k_pbvi_gamma_a    Ga     against R + the gathered rows of the device's G
    k_rows_chain      V      against the sequential fp32 chain of the device's Ga
    k_pbvi_select            against the first strict maximum of the device's V

Each reference is computed from the device's own previous stage, so one fault
shows in one stage.  The stages are read through pp2_debug_pbvi_stage (with
their padding); pp2_debug_pbvi_group forces the action groups that only a
Gamma_ao set above the 48 GiB budget would otherwise take.  Further: state
reuse on one context (stale rows beyond a smaller S, reallocation), and
pp2_pbvi_evaluate at the large pair shape and over a second argmax pass.
Expected values never come from the kernels under test.

What these tests found when they were written: G and Cm each came out as +0
where the reference keeps -0 (the +-1e-36 alpha row; the 2^-125 belief row
against it) -- Gamma_ao's off-grid neighbours and the GEMM's pad cells entered
as (+0) * (+0) terms, and -0 + +0 = +0.  Both now enter as (-0) * (+0) = -0.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ref as REF
from pbvi_stage_cases import (CASES, GAMMA, alphas, beliefs, bits, case, case_id, ref_cm,
                              ref_gamma_a, ref_gamma_ao, ref_kstar, ref_select, ref_values,
                              slices)

pytestmark = pytest.mark.gpu

G_SOURCE = "ref" if REF.available() else "oracle"
ST_G, ST_CM, ST_KSTAR, ST_GA, ST_V = range(5)
PP2_EINVAL, PP2_ESTATE = 1, 5
TILE, CHUNK = 128, 64  # kGemmTile, kPbviChunk


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@pytest.fixture(scope="module")
def dbg():
    """The two test-only entries of pp2_pbvi.cpp (not in include/pp2.h)."""
    from path_planning_2d_amd import _lib
    lib = _lib.load()
    lib.pp2_debug_pbvi_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_ulonglong, C.POINTER(C.c_int)]
    lib.pp2_debug_pbvi_stage.restype = C.c_int
    lib.pp2_debug_pbvi_group.argtypes = [C.c_int]
    lib.pp2_debug_pbvi_group.restype = C.c_int
    return lib


def round_up(v, m):
    return (v + m - 1) // m * m


def make_ctx(pp2, cs):
    ctx = pp2.GridContext(cs.grid, cs.goal, gamma=float(GAMMA))
    ctx.model_generate()
    return ctx


def read_stage(dbg, ctx, which, index, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    dims = (C.c_int * 5)()
    st = dbg.pp2_debug_pbvi_stage(ctx.handle, which, index, out.ctypes.data_as(C.c_void_p),
                                  out.nbytes, dims)
    assert st == 0, f"pp2_debug_pbvi_stage({which}, {index}) -> {st}"
    return out, list(dims)


def diff(got, want, what, bad):
    """Record where two arrays differ bit for bit (float32 by bits)."""
    if got.dtype == np.float32:
        got, want = bits(got), bits(np.ascontiguousarray(want, np.float32))
    ne = np.asarray(got != want)
    if ne.any():
        fmt = (lambda v: hex(int(v))) if got.dtype == np.uint32 else int
        first = "; ".join(f"{tuple(int(v) for v in i)}: got {fmt(got[tuple(i)])} want "
                          f"{fmt(want[tuple(i)])}" for i in np.argwhere(ne)[:4])
        bad.append(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {first}")
    return ne


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"{case_id(c)}-G_{G_SOURCE}")
def test_stage_parity(pp2, dbg, oracle, c):
    cs = case(*c)
    H, W, S, hw = cs.H, cs.W, cs.S, cs.hw
    T, L, R = cs.model(oracle)
    B, A0 = cs.B, cs.A0
    Sp, ld = round_up(S, TILE), round_up(hw, CHUNK)
    pairs = slices(S)
    G = np.empty((144, Sp, ld), np.float32)
    ks = np.empty((144, Sp), np.int32)
    Cm = {}
    Ga = np.empty((9, Sp, ld), np.float32)
    with make_ctx(pp2, cs) as ctx:
        ctx.pbvi_set_beliefs(B)
        ctx.pbvi_set(A0, cs.acts0)  # S unchanged: the belief set stays
        ctx.pbvi_backup(1)
        for z in range(144):
            G[z], dims = read_stage(dbg, ctx, ST_G, z, (Sp, ld))
            ks[z], _ = read_stage(dbg, ctx, ST_KSTAR, z, (Sp,), np.int32)
        for a, o in pairs:
            Cm[a, o], _ = read_stage(dbg, ctx, ST_CM, 16 * a + o, (Sp, Sp))
        for a in range(9):
            Ga[a], _ = read_stage(dbg, ctx, ST_GA, a, (Sp, ld))
        V, _ = read_stage(dbg, ctx, ST_V, 0, (9, Sp))
        al, act = ctx.pbvi_get()
    assert dims == [S, Sp, ld, hw, 9]
    bad = []

    # G: the reference's kernel on the same alphas; pad columns +0
    neg_zero_lost = 0
    for a, o in pairs:
        z = 16 * a + o
        want = ref_gamma_ao(oracle, REF if G_SOURCE == "ref" else None, H, W, T, L, a, o, A0)
        ne = diff(G[z, :S, :hw], want, f"G[{a},{o}]", bad)
        neg_zero_lost += int((ne & (bits(want) == 0x80000000) & (bits(G[z, :S, :hw]) == 0)).sum())
    if neg_zero_lost:
        bad.append(f"G: {neg_zero_lost} results are +0 where the reference keeps -0")
    if ld > hw:
        diff(bits(G[:, :, hw:]), np.zeros((144, Sp, ld - hw), np.uint32), "G pad columns", bad)
        diff(bits(Ga[:, :, hw:]), np.zeros((9, Sp, ld - hw), np.uint32), "Ga pad columns", bad)

    # Cm, kstar: from the device's own G and Cm
    for a, o in pairs:
        z = 16 * a + o
        diff(Cm[a, o][:S, :S], ref_cm(oracle, B, G[z, :S, :hw]), f"Cm[{a},{o}]", bad)
        diff(ks[z, :S], ref_kstar(Cm[a, o][:S, :S]), f"kstar[{a},{o}]", bad)

    # Ga: from the device's G and kstar, all 16 observations of every action
    if ((ks[:, :S] < 0) | (ks[:, :S] >= S)).any():
        bad.append("kstar out of [0, S)")
    else:
        for a in range(9):
            want = ref_gamma_a(R, a, G[16 * a:16 * a + 16, :S, :hw], ks[16 * a:16 * a + 16, :S])
            diff(Ga[a, :S, :hw], want, f"Ga[{a}]", bad)

    # V and the selection: from the device's Ga and V
    Gad = np.ascontiguousarray(Ga[:, :S, :hw])
    diff(V[:, :S], ref_values(B, Gad), "V", bad)
    want_al, want_act = ref_select(np.ascontiguousarray(V[:, :S]), Gad)
    diff(act, want_act, "selected actions", bad)
    diff(al, want_al, "selected alphas", bad)

    # end to end: the oracle's backup from the same alphas (all 144 slices)
    al_o, act_o = cs.backup(oracle)
    diff(act, act_o, "actions against the oracle's backup", bad)
    diff(al, al_o, "alphas against the oracle's backup", bad)
    assert not bad, "\n".join(bad)


def test_stage_entry_rejects(pp2, dbg, oracle):
    """pp2_debug_pbvi_stage: PP2_ESTATE before any backup of the state,
    PP2_EINVAL for a bad stage, a bad index and a short buffer; read-only."""
    cs = case(1, 7, 16)
    buf = np.empty(128 * 128, np.float32)
    dims = (C.c_int * 5)()

    def call(ctx, which, index, nbytes=buf.nbytes):
        return dbg.pp2_debug_pbvi_stage(ctx.handle, which, index, buf.ctypes.data_as(C.c_void_p),
                                        nbytes, dims)

    with make_ctx(pp2, cs) as ctx:
        assert call(ctx, ST_V, 0) == PP2_ESTATE  # no PBVI state at all
        ctx.pbvi_set_beliefs(cs.B)
        ctx.pbvi_set(cs.A0, cs.acts0)
        assert call(ctx, ST_V, 0) == PP2_ESTATE  # no backup yet
        ctx.pbvi_backup(1)
        before = ctx.pbvi_get()
        assert call(ctx, ST_G, 143) == 0 and list(dims) == [16, 128, 64, 7, 9]
        for which, index in ((5, 0), (-1, 0), (ST_G, 144), (ST_CM, -1), (ST_KSTAR, 144),
                             (ST_GA, 9), (ST_V, 1)):
            assert call(ctx, which, index) == PP2_EINVAL, (which, index)
        assert call(ctx, ST_G, 0, 128 * 64 * 4 - 1) == PP2_EINVAL
        assert call(ctx, ST_CM, 0, 128 * 128 * 4 - 1) == PP2_EINVAL
        assert call(ctx, ST_CM, 0) == 0
        after = ctx.pbvi_get()
        np.testing.assert_array_equal(bits(before[0]), bits(after[0]))
        ctx.pbvi_set(cs.A0, cs.acts0)            # a new state: its stages are not there yet
        assert call(ctx, ST_V, 0) == PP2_ESTATE


def test_state_reuse_on_one_context(pp2, oracle):
    """ensure_state keeps the belief set, G, Cm and kstar while Sp and ld stay:
    after S = 200, a set of 129 (the same Sp = 256) leaves rows 129..199 of
    all four stale; S = 5 reallocates; pbvi_solve then builds its own set.
    Each result equals the oracle's, bit for bit."""
    cs = case(3, 3, 129)
    H, W = cs.H, cs.W
    T, L, R = cs.model(oracle)
    with make_ctx(pp2, cs) as ctx:
        for S in (200, 129, 5):
            Bs, (As, acts) = beliefs(H, W, S), alphas(H, W, S)
            ctx.pbvi_set_beliefs(Bs)
            ctx.pbvi_set(As, acts)
            ctx.pbvi_backup(2)
            al, act = ctx.pbvi_get()
            al_o, act_o, _ = oracle.pbvi_backup(H, W, GAMMA, T, L, R, Bs, alphas=As, iterations=2)
            np.testing.assert_array_equal(act, act_o, err_msg=f"S={S}")
            np.testing.assert_array_equal(bits(al), bits(al_o), err_msg=f"S={S}")
        # from zero alphas too: set_beliefs alone resets them
        Bs = beliefs(H, W, 129)
        ctx.pbvi_set_beliefs(Bs)
        ctx.pbvi_backup(2)
        al, act = ctx.pbvi_get()
        al_o, act_o, _ = oracle.pbvi_backup(H, W, GAMMA, T, L, R, Bs, iterations=2)
        np.testing.assert_array_equal(act, act_o, err_msg="zero start")
        np.testing.assert_array_equal(bits(al), bits(al_o), err_msg="zero start")
        b0 = Bs[4]
        ctx.pbvi_solve(b0, 40)
        al, act = ctx.pbvi_get()
        Bd = ctx.pbvi_get_beliefs()
    Bo, _ = oracle.pbvi_belief_set(H, W, T, L, b0, 40)
    al_o, act_o, _ = oracle.pbvi_backup(H, W, GAMMA, T, L, R, Bo)
    np.testing.assert_array_equal(bits(Bd), bits(Bo))
    np.testing.assert_array_equal(act, act_o, err_msg="solve")
    np.testing.assert_array_equal(bits(al), bits(al_o), err_msg="solve")


@pytest.mark.parametrize("c", [(1, 7, 16), (3, 3, 129)], ids=case_id)
def test_action_groups(pp2, dbg, oracle, c):
    """Groups of 1, 2 and 4 actions (2 and 4 leave a ragged last group) offset
    G, kstar and Ga by the group's first action: two warm-started iterations
    give the alphas and actions of the single group of 9, and the oracle's."""
    cs = case(*c)
    al_o, act_o = cs.backup(oracle, 2)
    buf = np.empty(256 * 256, np.float32)
    dims = (C.c_int * 5)()
    prev = dbg.pp2_debug_pbvi_group(0)
    try:
        got = {}
        for group in (0, 1, 2, 4):
            assert dbg.pp2_debug_pbvi_group(group) in (0, 1, 2, 4)
            with make_ctx(pp2, cs) as ctx:
                ctx.pbvi_set_beliefs(cs.B)
                ctx.pbvi_set(cs.A0, cs.acts0)
                ctx.pbvi_backup(2)
                got[group] = ctx.pbvi_get()
                # the slices of a grouped run are gone; Ga and V are whole
                st = [dbg.pp2_debug_pbvi_stage(ctx.handle, w, 0, buf.ctypes.data_as(C.c_void_p),
                                               buf.nbytes, dims) for w in (ST_G, ST_GA, ST_V)]
                assert st == ([0, 0, 0] if group == 0 else [PP2_ESTATE, 0, 0])
                assert dims[4] == (group or 9)
        for group, (al, act) in got.items():
            np.testing.assert_array_equal(act, act_o, err_msg=f"group {group}")
            np.testing.assert_array_equal(bits(al), bits(al_o), err_msg=f"group {group}")
    finally:
        dbg.pp2_debug_pbvi_group(prev)


def eval_reference(oracle, beliefs_, al, act):
    v = np.empty(len(beliefs_), np.float32)
    a = np.empty(len(beliefs_), np.uint8)
    for i, b in enumerate(beliefs_):
        v[i], a[i] = oracle.pbvi_eval(b, al, act)
    return v, a


def test_evaluate_large_pair_shape(pp2, oracle):
    """1100 beliefs against 1000 alphas: 18 x 16 tiles of 64 x 64 pairs, the
    large shape of the pair kernel (k_pair_chain<PAIR_DOT, 64, 16, 32>), with
    ragged last tiles both ways, then two argmax passes over each row."""
    cs = case(3, 3, 129)
    rng = np.random.default_rng(77)
    n, S, hw = 1100, 1000, cs.hw
    al = rng.uniform(-20.0, 20.0, (S, hw)).astype(np.float32)
    for k, k2 in ((3, 67), (100, 612), (511, 512), (40, 999)):
        al[k] = np.clip(al[k] + 12.0, -20.0, 20.0)
        al[k2] = al[k]
    act = rng.integers(0, 9, S).astype(np.uint8)
    act[[67, 612, 512, 999]] = (act[[3, 100, 511, 40]] + 1) % 9  # a wrong winner shows
    Bs = rng.random((n, hw)) * (rng.random((n, hw)) < 0.7)
    Bs[:, 0] += 1e-3
    Bs = (Bs / Bs.sum(1, keepdims=True)).astype(np.float32)
    Bs[5, 1::2] = np.float32(1e-42)
    Bs[6] = np.ldexp(Bs[6], -125)
    vo, ao = eval_reference(oracle, Bs, al, act)
    with make_ctx(pp2, cs) as ctx:
        ctx.pbvi_set(al, act)
        v, a = ctx.pbvi_evaluate(Bs)
    np.testing.assert_array_equal(a, ao)
    np.testing.assert_array_equal(bits(v), bits(vo))


def test_evaluate_second_argmax_pass(pp2, oracle):
    """7 beliefs against 600 alphas; alphas 70 and 582 are equal and above
    every other: the same lane of k_argmax_rows a pass apart, and the first
    has to win (the two carry different actions)."""
    cs = case(3, 3, 600)
    rng = np.random.default_rng(78)
    S, hw = 600, cs.hw
    al = rng.uniform(-20.0, 10.0, (S, hw)).astype(np.float32)
    al[70] = rng.uniform(15.0, 20.0, hw).astype(np.float32)
    al[582] = al[70]
    act = rng.integers(0, 9, S).astype(np.uint8)
    act[70], act[582] = 3, 5
    Bs = beliefs(cs.H, cs.W, 7)
    vo, ao = eval_reference(oracle, Bs, al, act)
    assert (ao == 3).all()
    with make_ctx(pp2, cs) as ctx:
        ctx.pbvi_set(al, act)
        v, a = ctx.pbvi_evaluate(Bs)
    np.testing.assert_array_equal(a, ao)
    np.testing.assert_array_equal(bits(v), bits(vo))
