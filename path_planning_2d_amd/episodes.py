"""Batched closed-loop policy episodes (include/pp2.h "episodes").

``EpisodeBatch`` runs E simulated robots under a control policy -- the
belief-mode policy of the reference MDP node, the QMDP policy, the greedy
policy of the FIB alphas or of the PBVI alpha vectors, or the one-step
lookahead over either set -- each with its own belief, for up to ``horizon``
steps in one kernel launch, and returns how the policy did: steps to the goal,
status and discounted cost per episode.
Everything runs in libpp2_hip.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import call
from .core import GridContext, _f32, _u8

MAX_EPISODES = 131072
MAX_HORIZON = 4096

STATUS_HORIZON = 0   # still running after the last step
STATUS_GOAL = 1      # the true robot reached the goal
STATUS_LOST = 2      # the belief update left no finite positive value

ALPHA_FIB = 0        # the context's current FIB alphas (K = 9, action of vector k = k)
ALPHA_PBVI = 1       # the context's PBVI alpha vectors and their actions (K = S)
_ALPHA_SETS = {"fib": ALPHA_FIB, "pbvi": ALPHA_PBVI}

# where an episode's two belief planes live (include/pp2.h "Placement")
EPISODES_LDS = 0     # in the workgroup's LDS; a grid that does not fit is refused
EPISODES_GLOBAL = 1  # in device memory: any grid the context supports
EPISODES_AUTO = 2    # per launch: LDS if that launch's layout fits, else device memory
_PLACEMENTS = {"lds": EPISODES_LDS, "global": EPISODES_GLOBAL, "auto": EPISODES_AUTO}
# ``run``'s names of the one-step lookahead over a set
_LOOKAHEAD = {"fib-lookahead": "fib", "pbvi-lookahead": "pbvi"}
# ``set_action_table``'s names (PP2_TABLE_*)
_TABLES = {"mdp": 0, "path": 1}
# ``resume``'s policies (PP2_EPISODE_*)
_RESUME = {"mode": 0, "qmdp": 1, "fib": 2, "pbvi": 3, "fib-lookahead": 4, "pbvi-lookahead": 5}


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _check_placed(placed) -> bool:
    if not isinstance(placed, bool):
        raise ValueError(f"placed must be a bool, not {placed!r}")
    return placed


def check_placement(placement) -> int:
    """The constant of a placement ("lds" | "global" | "auto" or one of the three
    EPISODES_* constants); raises ValueError on anything else (and never calls
    the library)."""
    if isinstance(placement, str):
        if placement not in _PLACEMENTS:
            raise ValueError(f"unknown placement {placement!r}")
        return _PLACEMENTS[placement]
    if (isinstance(placement, bool) or not isinstance(placement, (int, np.integer))
            or placement not in (EPISODES_LDS, EPISODES_GLOBAL, EPISODES_AUTO)):
        raise ValueError(f"unknown placement {placement!r}")
    return int(placement)


class EpisodeBatch:
    """E closed-loop episodes over an unsharded ``GridContext`` with a model,
    solved (or at least current) MDP values and an active coded model.
    ``placement``: "lds" (the default: the belief planes in the workgroup's
    LDS, a grid that does not fit is refused), "global" (the planes in device
    memory, any grid) or "auto" (per launch, LDS where it fits); the results
    are the same bits from either.  Every policy follows the placement; the
    lookahead does so with ``placed=True`` (``run_lookahead`` / ``run``), which
    calls ``pp2_episodes_run_lookahead_placed``.  Without it the lookahead keeps
    the older entry's contract: it runs from LDS planes, and a "global" batch
    or an "auto" batch whose lookahead layout does not fit LDS refuses it."""

    def __init__(self, ctx: GridContext, episodes: int, horizon: int,
                 record_trace: bool = False, placement="lds"):
        episodes, horizon = int(episodes), int(horizon)
        if not 1 <= episodes <= MAX_EPISODES:
            raise ValueError(f"episodes {episodes} outside 1..{MAX_EPISODES}")
        if not 1 <= horizon <= MAX_HORIZON:
            raise ValueError(f"horizon {horizon} outside 1..{MAX_HORIZON}")
        placement = check_placement(placement)
        self._h = None
        self.ctx = ctx
        self.episodes = episodes
        self.horizon = horizon
        self.record_trace = bool(record_trace)
        self.cells = ctx.cells
        self.policy = None
        self.alpha_set = None    # of the last run, if that was an alpha or a lookahead run
        self.lookahead = False   # the last run was a lookahead run
        self.world = None        # the attached world context (set_world)
        h = C.c_void_p()
        if placement == EPISODES_LDS:
            call("pp2_episodes_create", C.byref(h), ctx.handle, episodes, horizon,
                 int(self.record_trace))
        else:
            call("pp2_episodes_create_placed", C.byref(h), ctx.handle, episodes, horizon,
                 int(self.record_trace), placement)
        self._h = h

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            call("pp2_episodes_destroy", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ running
    @staticmethod
    def check_run_args(cells: int, episodes: int, policy, b0, start_cells, seed):
        """Validated (policy, b0, start_cells, seed) of a run; raises ValueError
        on anything the library would reject (and never calls it)."""
        if isinstance(policy, str):
            if policy not in GridContext._POLICIES:
                raise ValueError(f"unknown control policy {policy!r}")
            policy = GridContext._POLICIES[policy]
        if policy not in (GridContext.CONTROL_MODE, GridContext.CONTROL_QMDP):
            raise ValueError(f"unknown control policy {policy!r}")
        b0 = np.ascontiguousarray(b0, np.float32).reshape(-1)
        if b0.size != cells:
            raise ValueError(f"b0 has {b0.size} cells, the grid {cells}")
        if not (np.isfinite(b0).all() and (b0 >= 0).all() and not np.signbit(b0).any()):
            raise ValueError("b0 must be finite and >= +0 everywhere")
        start = np.asarray(start_cells)
        if start.ndim != 1 or start.size != episodes:
            raise ValueError(f"start_cells must hold {episodes} cells")
        if not np.issubdtype(start.dtype, np.integer):
            raise ValueError("start_cells must be integers")
        if start.size and (start.min() < 0 or start.max() >= cells):
            raise ValueError(f"start_cells outside [0, {cells})")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        return int(policy), b0, np.ascontiguousarray(start, np.int32), seed

    def run(self, policy, b0, start_cells, seed: int = 0, placed: bool = False):
        """Enqueue one batch: every episode starts from belief ``b0`` with its
        true robot at ``start_cells[e]`` (``y * W + x``).  ``policy``: "mode",
        "qmdp" (or CONTROL_MODE / CONTROL_QMDP), "fib" / "pbvi", which are
        ``run_alpha``, or "fib-lookahead" / "pbvi-lookahead", which are
        ``run_lookahead`` (``placed`` as there; the other policies follow the
        placement anyway, so it changes nothing for them).  Asynchronous."""
        placed = _check_placed(placed)
        if isinstance(policy, str) and policy in _ALPHA_SETS:
            return self.run_alpha(policy, b0, start_cells, seed)
        if isinstance(policy, str) and policy in _LOOKAHEAD:
            return self.run_lookahead(_LOOKAHEAD[policy], b0, start_cells, seed, placed)
        policy, b0, start, seed = self.check_run_args(self.cells, self.episodes, policy, b0,
                                                      start_cells, seed)
        call("pp2_episodes_run", self._h, policy, C.c_uint64(seed), _f32(b0), _i32(start))
        self.policy = policy
        self.alpha_set = None
        self.lookahead = False
        return self

    def _check_alpha_args(self, alpha_set, b0, start_cells, seed):
        if isinstance(alpha_set, str):
            if alpha_set not in _ALPHA_SETS:
                raise ValueError(f"unknown alpha set {alpha_set!r}")
            alpha_set = _ALPHA_SETS[alpha_set]
        if (isinstance(alpha_set, bool) or not isinstance(alpha_set, (int, np.integer))
                or alpha_set not in (ALPHA_FIB, ALPHA_PBVI)):
            raise ValueError(f"unknown alpha set {alpha_set!r}")
        # (b0, the starts and the seed are checked as for any run; the policy
        # argument only has to be a valid one)
        _, b0, start, seed = self.check_run_args(self.cells, self.episodes,
                                                 GridContext.CONTROL_QMDP, b0, start_cells, seed)
        return int(alpha_set), b0, start, seed

    def run_alpha(self, alpha_set, b0, start_cells, seed: int = 0):
        """``run`` under the greedy policy of an alpha-vector set: "fib" (or
        ALPHA_FIB), the context's current FIB alphas, or "pbvi" (ALPHA_PBVI),
        its PBVI alpha vectors.  The cost stays the MDP cost, so all
        policies are compared on one scale.  Asynchronous."""
        alpha_set, b0, start, seed = self._check_alpha_args(alpha_set, b0, start_cells, seed)
        call("pp2_episodes_run_alpha", self._h, alpha_set, C.c_uint64(seed), _f32(b0),
             _i32(start))
        self.policy = None
        self.alpha_set = alpha_set
        self.lookahead = False
        return self

    def run_lookahead(self, alpha_set, b0, start_cells, seed: int = 0, placed: bool = False):
        """``run`` under the one-step lookahead policy over an alpha-vector set
        ("fib" / "pbvi", as ``run_alpha``): the action with the largest
        Q(b, u) = <b, R_u> + gamma * sum_z max_k <L_z . T_u^T b, alpha_k>, the
        reference POMDP node's tree at depth 1 with exact observation
        weights.  ``placed=True`` follows the batch's placement as every other
        run does (``pp2_episodes_run_lookahead_placed``: device-memory planes
        on a "global" batch and on an "auto" batch whose lookahead layout does
        not fit LDS, the same bits); the default runs from LDS planes or raises
        ``Pp2Error`` (PP2_EINVAL).  Asynchronous."""
        placed = _check_placed(placed)
        alpha_set, b0, start, seed = self._check_alpha_args(alpha_set, b0, start_cells, seed)
        call("pp2_episodes_run_lookahead_placed" if placed else "pp2_episodes_run_lookahead",
             self._h, alpha_set, C.c_uint64(seed), _f32(b0), _i32(start))
        self.policy = None
        self.alpha_set = alpha_set
        self.lookahead = True
        return self

    def set_world(self, world: GridContext | None):
        """Attach the context that holds the true map (include/pp2.h "The
        world"): motion, observation, cost and goal of every later ``run`` and
        ``resume`` come from it, control and the belief update stay on the
        batch's own context.  ``None`` detaches.  The batch keeps a reference,
        so the world outlives it unless closed by hand."""
        call("pp2_episodes_set_world", self._h, None if world is None else world.handle)
        self.world = world
        return self

    def set_action_table(self, table):
        """The table a "mode" run or resumed "mode" segment reads at the belief's
        mode: "mdp" (the default: the MDP's action plane) or "path" (the
        context's shortest-path table, ``GridContext.path_solve``; a run
        without a valid field raises PP2_ESTATE).  Every other policy ignores
        it.  Belongs to the batch, as ``set_world``."""
        if not isinstance(table, str) or table not in _TABLES:
            raise ValueError(f"unknown action table {table!r}")
        call("pp2_episodes_set_action_table", self._h, _TABLES[table])
        self.action_table = table
        return self

    def resume(self, policy, seed: int = 0):
        """Continue every episode for another ``horizon`` steps from where the
        last ``run`` or ``resume`` left it (include/pp2.h "Resumed segments"),
        under ``policy``: one of the names ``run`` takes ("mode", "qmdp", "fib",
        "pbvi", "fib-lookahead", "pbvi-lookahead").  Reads the values, alpha
        sets, models and world current now.  Follows the placement.
        Asynchronous."""
        if not isinstance(policy, str) or policy not in _RESUME:
            raise ValueError(f"unknown episode policy {policy!r}")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        call("pp2_episodes_resume", self._h, _RESUME[policy], C.c_uint64(seed))
        self.lookahead = policy in _LOOKAHEAD
        self.alpha_set = _ALPHA_SETS.get(_LOOKAHEAD.get(policy, policy))
        self.policy = GridContext._POLICIES[policy] if self.alpha_set is None else None
        return self

    def results(self) -> dict:
        """steps, status, cost, final_cell of every episode (synchronises)."""
        E = self.episodes
        steps = np.empty(E, np.int32)
        status = np.empty(E, np.uint8)
        cost = np.empty(E, np.float32)
        final = np.empty(E, np.int32)
        call("pp2_episodes_results", self._h, _i32(steps), _u8(status), _f32(cost), _i32(final))
        return {"steps": steps, "status": status, "cost": cost, "final_cell": final}

    def trace(self) -> dict:
        """The last run's per-step record, [horizon, E] arrays (qsums
        [horizon, E, 9]: QMDP's S_u, a FIB run's V_k or a lookahead run's Q_u,
        else 0; mode_cells only
        for mode runs).  Steps not taken hold 255, 255, -1, 0, -1."""
        sh = (self.horizon, self.episodes)
        a = np.empty(sh, np.uint8)
        z = np.empty(sh, np.uint8)
        cells = np.empty(sh, np.int32)
        q = np.empty(sh + (9,), np.float32)
        mode = np.empty(sh, np.int32)
        call("pp2_episodes_trace", self._h, _u8(a), _u8(z), _i32(cells), _f32(q), _i32(mode))
        return {"actions": a, "observations": z, "cells": cells, "qsums": q, "mode_cells": mode}

    def trace_alpha(self) -> dict:
        """The last alpha run's winners, [horizon, E]: the index of the winning
        vector and its sum (steps not taken: -1, 0)."""
        sh = (self.horizon, self.episodes)
        best = np.empty(sh, np.int32)
        vsum = np.empty(sh, np.float32)
        call("pp2_episodes_trace_alpha", self._h, _i32(best), _f32(vsum))
        return {"best_index": best, "best_sum": vsum}

    def trace_lookahead(self) -> dict:
        """The last lookahead run's record: ``q`` and ``rewards`` [horizon, E,
        9] (Q_u, <b, R_u>), ``leaf_max`` and ``leaf_index`` [horizon, E, 9, 16]
        (per (u, z) the largest <raw_uz, alpha_k> and its k).  Steps not taken
        hold 0, 0, 0, -1."""
        sh = (self.horizon, self.episodes)
        q = np.empty(sh + (9,), np.float32)
        rew = np.empty(sh + (9,), np.float32)
        lmax = np.empty(sh + (9, 16), np.float32)
        lidx = np.empty(sh + (9, 16), np.int32)
        call("pp2_episodes_trace_lookahead", self._h, _f32(q), _f32(rew), _f32(lmax), _i32(lidx))
        return {"q": q, "rewards": rew, "leaf_max": lmax, "leaf_index": lidx}

    def alphas(self):
        """(alphas[K, hw], actions[K]): the alpha set the last alpha or
        lookahead run read."""
        k = C.c_int(0)
        call("pp2_episodes_get_alpha", self._h, C.byref(k), None, None)
        al = np.empty((k.value, self.cells), np.float32)
        act = np.empty(k.value, np.uint8)
        call("pp2_episodes_get_alpha", self._h, C.byref(k), _f32(al), _u8(act))
        return al, act

    def belief(self, e: int) -> np.ndarray:
        """The stored (power-of-two scaled) belief of episode ``e`` after the run."""
        b = np.empty(self.cells, np.float32)
        call("pp2_episodes_get_belief", self._h, int(e), _f32(b))
        return b

    def qplanes(self) -> np.ndarray:
        """Q[hw, 9] of the last run: the sweep's cost of every action from the J
        the run read."""
        q = np.empty((self.cells, 9), np.float32)
        call("pp2_episodes_get_q", self._h, _f32(q))
        return q

    def info(self) -> dict:
        lds, wgs, th = C.c_int(0), C.c_int(0), C.c_int(0)
        call("pp2_episodes_info", self._h, C.byref(lds), C.byref(wgs), C.byref(th))
        return {"lds_bytes": lds.value, "workgroups": wgs.value, "threads": th.value}

    def placement(self) -> dict:
        """``requested``: the placement the batch was created with; ``last``:
        that of the last launch (-1 before any run); ``scratch_bytes``: the
        device memory held for the global planes (0 until first needed)."""
        req, last, nbytes = C.c_int(0), C.c_int(0), C.c_longlong(0)
        call("pp2_episodes_placement", self._h, C.byref(req), C.byref(last), C.byref(nbytes))
        return {"requested": req.value, "last": last.value, "scratch_bytes": nbytes.value}

    def summary(self) -> dict:
        """Success rate, mean steps of the successful episodes (nan if none)
        and mean discounted cost of the last run."""
        r = self.results()
        ok = r["status"] == STATUS_GOAL
        return {"episodes": self.episodes,
                "success_rate": float(ok.mean()),
                "mean_steps": float(r["steps"][ok].mean()) if ok.any() else float("nan"),
                "mean_cost": float(r["cost"].astype(np.float64).mean()),
                "lost": int((r["status"] == STATUS_LOST).sum())}
