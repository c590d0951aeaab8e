"""Seeded inputs and one plain reference per stage of the PBVI backup, shared
by test_pbvi_stage_cpu.py and test_gpu_pbvi_stages.py.  Everything here is a
pure function of (H, W, S); grids, goals and bit views are those of
ref_pin_cases.py.

The backup (pp2_pbvi.cpp) is five chained stages:

  G      Gamma_ao, cudaComputeGammaOA of every alpha        [144][S][hw]
  Cm     <b_i, G[a,o][k]>, the pinned x-ordered fmaf chain   [144][S][S]
  kstar  first argmax_k of each row of Cm                    [144][S]
  Ga     R[:, a] + G[a,0][k*] + ... + G[a,15][k*], fp32       [9][S][hw]
  V      inner_product(b_i, Ga[a][i]): product rounded, then
         the sequential fp32 sum                             [9][S]
  and the selection: first strict maximum over a from -FLT_MAX, that row of
  Ga copied.

Each reference below takes the previous stage as an argument, so a test can
feed it the device's own previous stage: one fault then shows in one stage.
"""
import functools

import numpy as np

from ref_pin_cases import bits, goals, grid  # noqa: F401  (bits: re-exported)

GAMMA = np.float32(0.95)

# (H, W, S).  The device pads hw to ld = a multiple of 64 (the GEMM's x chunk
# is 32) and S to Sp = a multiple of the 128-row GEMM tile; k_pbvi_gamma_ao
# takes 16 alpha rows per thread and 256 cells per block; k_argmax_rows takes
# 512 columns per pass.
CASES = [
    (3, 3, 1),       # one belief
    (1, 7, 16),      # one grid row; S at the 16-row block of Gamma_ao
    (5, 1, 17),      # one grid column; one row past it
    (1, 64, 15),     # hw = ld = 64: no pad column; one row below
    (2, 255, 17),    # hw 510: the second 256-cell block two cells short of full
    (2, 256, 16),    # hw 512: two full 256-cell blocks, no pad column
    (3, 257, 15),    # hw 771: a fourth block of three cells
    (33, 65, 33),    # ld 2176: 68 GEMM chunks, three row blocks of Gamma_ao
    (3, 3, 127),     # one below the GEMM tile
    (3, 3, 128),     # the tile
    (3, 3, 129),     # one above: 2 x 2 tiles, 127 pad rows
    (5, 13, 385),    # Sp 512: 4 x 4 tiles; hw 65 -> ld 128, the last three chunks padding
    (3, 3, 600),     # Sp 640: 5 x 5 tiles, second argmax pass
]
# stage parity reads all 144 (a, o) slices up to this S, 18 above it
ALL_SLICES_MAX_S = 129


def case_id(c):
    return f"{c[0]}x{c[1]}-S{c[2]}"


def slices(S):
    """The (a, o) slices whose G, Cm and kstar a stage test compares."""
    if S <= ALL_SLICES_MAX_S:
        return [(a, o) for a in range(9) for o in range(16)]
    return sorted({(a, o) for a in range(9) for o in (a, 15 - a)})


def beliefs(H, W, S):
    """[S, hw] float32.  Rows 0..7, as far as S reaches: uniform; sparse; one-hot
    at x = 0; one-hot at x = hw - 1; a random row; its exact copy; a row with
    every third entry 1e-42 (subnormal operands); a row scaled by 2^-125
    (subnormal operands, and partial sums in the subnormal range).  The rest
    are random rows normalised in float64."""
    hw = H * W
    rng = np.random.default_rng(101 + 7 * H + 13 * W + 1009 * S)
    B = rng.random((S, hw))
    B /= B.sum(1, keepdims=True)
    B = B.astype(np.float32)
    special = []
    special.append(np.full(hw, 1.0 / hw))
    sp = rng.random(hw) * (rng.random(hw) < 0.25)
    sp[rng.integers(0, hw)] += 0.5
    special.append(sp / sp.sum())
    e0 = np.zeros(hw)
    e0[0] = 1.0
    special.append(e0)
    e1 = np.zeros(hw)
    e1[hw - 1] = 1.0
    special.append(e1)
    dup = rng.random(hw)
    dup /= dup.sum()
    special.append(dup)
    special.append(dup)
    tiny = rng.random(hw)
    tiny /= tiny.sum()
    tiny = tiny.astype(np.float32)
    tiny[::3] = np.float32(1e-42)
    special.append(tiny)
    sc = rng.random(hw)
    sc /= sc.sum()
    special.append(np.ldexp(sc.astype(np.float32), -125))
    for i, row in enumerate(special[:S]):
        B[i] = np.asarray(row, np.float32)
    return B


# exact duplicates: alpha row `second` is a copy of row `first`, and the first
# must win every tie.  64 apart: the same lane of k_argmax_rows, the next load
# of one pass; 512 apart (70 / 582): the same lane, the next pass; 1 and 37
# apart: different lanes (the shuffle reduction's index rule); 127 / 128 and
# 120 / 140: across the GEMM tile edge.
DUPLICATES = [(4, 68), (70, 582), (6, 7), (9, 46), (127, 128), (120, 140), (300, 364),
              (513, 530)]
ROW_TINY, ROW_ZERO, ROW_CONST = 1, 2, 3


def alphas(H, W, S):
    """(A0 [S, hw] float32, actions [S] uint8).  Mixed sign in +-20; row 1 is
    +-U(0,1) * 1e-36 (products that underflow and flush to -0 in Gamma_ao),
    row 2 zero, row 3 constant, as far as S reaches; DUPLICATES as far as S
    reaches, and lifted a little so that they win often."""
    hw = H * W
    rng = np.random.default_rng(211 + 5 * H + 11 * W + 2003 * S)
    A = rng.uniform(-20.0, 20.0, (S, hw)).astype(np.float32)
    if S > ROW_TINY:
        A[ROW_TINY] = (rng.uniform(-1.0, 1.0, hw) * 1e-36).astype(np.float32)
    if S > ROW_ZERO:
        A[ROW_ZERO] = 0.0
    if S > ROW_CONST:
        A[ROW_CONST] = np.float32(-7.25)
    # a duplicated row is lifted by about 1.5 standard deviations of a row's
    # mean, so that it is the maximum for a fair share of the beliefs, not all
    lift = np.float32(1.5 * 20.0 / np.sqrt(3.0 * hw))
    for k, k2 in DUPLICATES:
        if k2 < S:
            A[k] = np.clip(A[k] + lift, -20.0, 20.0)
            A[k2] = A[k]
    return A, rng.integers(0, 9, S).astype(np.uint8)


# ------------------------------------------------------------------ references
def ref_gamma_ao(O, REF, H, W, T, L, a, o, A):
    """Stage G.  REF: oracle.ref where oracle/_ref is built (the reference's
    own kernel), else None (the oracle's restatement)."""
    if REF is not None:
        return REF.pbvi_gamma_ao(H, W, GAMMA, T, L, a, o, A)
    return O.pbvi_gamma_ao(H, W, GAMMA, T, L, a, o, A)


def ref_cm(O, B, G):
    """Stage Cm of one slice: B [S, hw], G [S, hw] -> [S, S]."""
    return O.fma_chain_nt(B, G)


def ref_kstar(Cm):
    """Stage kstar of one slice: the first index of each row's maximum."""
    return np.argmax(Cm, axis=1).astype(np.int32)


def ref_gamma_a(R, a, G16, k16):
    """Stage Ga of action a: G16 [16, S, hw], k16 [16, S] -> [S, hw]."""
    S = G16.shape[1]
    v = np.repeat(np.ascontiguousarray(R[:, a], np.float32)[None, :], S, axis=0)
    for o in range(16):
        v = v + G16[o][k16[o]]
    assert v.dtype == np.float32
    return v


def ref_values(B, Ga):
    """Stage V: B [S, hw], Ga [9, S, hw] -> [9, S]; fl(b * g), then the
    sequential fp32 chain from +0."""
    t = B[None, :, :] * Ga
    assert t.dtype == np.float32
    z = np.zeros(t.shape[:2] + (1,), np.float32)
    return np.add.accumulate(np.concatenate([z, t], axis=2), axis=2, dtype=np.float32)[:, :, -1]


def ref_select(V, Ga):
    """Selection: V [9, S], Ga [9, S, hw] -> (alphas [S, hw], actions [S])."""
    S = V.shape[1]
    opt = np.full(S, -np.finfo(np.float32).max, np.float32)
    oa = np.zeros(S, np.int64)
    for a in range(9):
        better = V[a] > opt
        opt = np.where(better, V[a], opt)
        oa = np.where(better, a, oa)
    return Ga[oa, np.arange(S)].copy(), oa.astype(np.uint8)


def ref_backup_stages(O, H, W, T, L, R, B, A, visit=None):
    """One backup from A by the stage references chained: dict Ga [9, S, hw],
    V [9, S], alphas [S, hw], actions [S].  visit(a, o, G, Cm, kstar) sees
    every slice's first three stages on the way."""
    S, hw = B.shape
    Ga = np.empty((9, S, hw), np.float32)
    for a in range(9):
        G16 = np.empty((16, S, hw), np.float32)
        k16 = np.empty((16, S), np.int32)
        for o in range(16):
            G16[o] = ref_gamma_ao(O, None, H, W, T, L, a, o, A)
            Cm = ref_cm(O, B, G16[o])
            k16[o] = ref_kstar(Cm)
            if visit is not None:
                visit(a, o, G16[o], Cm, k16[o])
        Ga[a] = ref_gamma_a(R, a, G16, k16)
    V = ref_values(B, Ga)
    al, act = ref_select(V, Ga)
    return {"Ga": Ga, "V": V, "alphas": al, "actions": act}


# ------------------------------------------------------------------ cases
class Case:
    """One (H, W, S): inputs and the oracle's warm-started backups, computed on
    first use and then shared read-only."""

    def __init__(self, H, W, S):
        self.H, self.W, self.S = H, W, S
        self.hw = H * W
        self.grid = grid(H, W)
        self.goal = goals(H, W)[1]
        self._memo = {}

    def _once(self, key, make):
        if key not in self._memo:
            out = make()
            for a in (out if isinstance(out, tuple) else (out,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[key] = out
        return self._memo[key]

    def model(self, O):
        return self._once("model", lambda: O.model_pomdp(self.grid, self.goal))

    @property
    def B(self):
        return self._once("B", lambda: beliefs(self.H, self.W, self.S))

    @property
    def A0(self):
        return self._once("A0", lambda: alphas(self.H, self.W, self.S))[0]

    @property
    def acts0(self):
        return self._once("A0", lambda: alphas(self.H, self.W, self.S))[1]

    def backup(self, O, iterations=1):
        """(alphas, actions) of oracle.pbvi_backup warm-started from A0."""
        def make():
            T, L, R = self.model(O)
            al, act, _ = O.pbvi_backup(self.H, self.W, GAMMA, T, L, R, self.B, alphas=self.A0,
                                       iterations=iterations)
            return al, act
        return self._once(("backup", iterations), make)


@functools.lru_cache(maxsize=None)
def case(H, W, S):
    return Case(H, W, S)
