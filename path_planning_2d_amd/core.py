"""Host-side handle over one ``pp2_ctx`` (a grid, or a row shard of one, on one
MI355X).  Thin numpy-facing layer over the C ABI in include/pp2.h; every call
goes to the gfx950 kernels in libpp2_hip.so -- there is no CPU path.

Arrays use the reference layouts (path_planning_2d/src/pomdp/
model_generation_cuda.cu:27-38): ``T[hw, 9, 9]``, ``L[hw, 16]``,
``R/C[hw, 9]``, beliefs and values ``[hw]`` with ``idx = y * W + x``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import call


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


_NULLF = C.POINTER(C.c_float)()


class GridContext:
    """One device-resident grid: model tensors, belief, MDP values, FIB alphas.

    Mirrors the state the reference keeps in its ``dev_*``/``host_*`` globals
    (src/mdp/path_planning_2d_cuda.cu:26-38, src/pomdp/model_generation_cuda.cu:
    27-38, src/pomdp/fast_informed_bound_cuda.cu:43-51).
    """

    def __init__(self, grid: np.ndarray, goal, gamma: float = 0.95,
                 device: int = 0, rows: tuple[int, int] | None = None):
        grid = np.ascontiguousarray(grid, dtype=np.uint8)
        if grid.ndim != 2:
            raise ValueError("grid must be 2-D (H, W)")
        self.global_height, self.width = grid.shape
        self.goal = (int(goal[0]), int(goal[1]))
        self.gamma = float(gamma)
        self.device = int(device)
        h = C.c_void_p()
        if rows is None:
            call("pp2_create", C.byref(h), self.device, self.global_height,
                 self.width, _u8(grid), self.goal[0], self.goal[1],
                 C.c_float(self.gamma))
            self.row_begin, self.row_end = 0, self.global_height
        else:
            r0, r1 = int(rows[0]), int(rows[1])
            call("pp2_create_shard", C.byref(h), self.device,
                 self.global_height, self.width, r0, r1, _u8(grid),
                 self.goal[0], self.goal[1], C.c_float(self.gamma))
            self.row_begin, self.row_end = r0, r1
        self._h = h
        self.rows = self.row_end - self.row_begin
        self.cells = self.rows * self.width
        rs = C.c_uint32()
        call("pp2_get_geometry", self._h, None, None, C.byref(rs), None)
        self.row_stride = rs.value

    # ------------------------------------------------------------ lifetime
    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().pp2_destroy(self._h)
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

    def set_stream(self, stream_handle: int | None):
        call("pp2_set_stream", self._h, C.c_void_p(stream_handle or 0))

    def synchronize(self):
        call("pp2_synchronize", self._h)

    def set_cells_per_lane(self, cpt: int):
        call("pp2_set_cells_per_lane", self._h, int(cpt))

    TUNE_CELLS_PER_LANE = 1
    TUNE_NT_STREAMS = 2
    TUNE_CODED_MODEL = 3
    TUNE_HALO_DEPTH = 4
    TUNE_COMM_STREAM = 5
    TUNE_NORM_BLOCK = 6
    TUNE_STEP_PAIRS = 7
    TUNE_RESIDENT = 8
    TUNE_RESIDENT_HALO = 9
    TUNE_RESIDENT_CUS = 10
    TUNE_RESIDENT_STALL = 11
    TUNE_RESIDENT_TILE_COLS = 12
    TUNE_SHARD_LAG = 13
    TUNE_COMM_TIMING = 14
    TUNE_RESIDENT_MASKED = 15
    TUNE_MAP_INCREMENTAL = 16

    def set_tuning(self, key: int, value: int):
        call("pp2_set_tuning", self._h, int(key), int(value))

    def comm_rounds(self, max_rounds: int = 256):
        """The RCCL rounds timed since TUNE_COMM_TIMING was set or the last
        call (pp2_comm_rounds): (durations in us as a float32 array, rounds
        beyond the 256 timed ones).  Synchronises; clears the record."""
        n = C.c_int(0)
        dropped = C.c_longlong(0)
        buf = np.zeros(max(1, max_rounds), np.float32)
        call("pp2_comm_rounds", self._h, C.byref(n), C.byref(dropped), _f32(buf),
             int(max_rounds))
        return buf[:min(n.value, max_rounds)].copy(), dropped.value

    # ------------------------------------------------------------ model
    def model_generate(self):
        call("pp2_model_generate", self._h)

    def model_dict_info(self):
        """(entries, active) of the dictionary-coded model (pp2_model_dict_info)."""
        e, a = C.c_int(0), C.c_int(0)
        call("pp2_model_dict_info", self._h, C.byref(e), C.byref(a))
        return e.value, bool(a.value)

    # ------------------------------------------------------------ live updates
    def map_update(self, patch, x0: int = 0, y0: int = 0):
        """Rows [y0, y0 + h) x columns [x0, x0 + w) of the map take ``patch``
        ((h, w) uint8, 1 = occupied); under a generated model the changed
        cells are regenerated in place (pp2_map_update).  State is kept: the
        caller re-solves (``mdp_resolve``)."""
        patch = np.ascontiguousarray(patch, dtype=np.uint8)
        if patch.ndim != 2:
            raise ValueError("patch must be 2-D (h, w)")
        call("pp2_map_update", self._h, int(x0), int(y0), patch.shape[1],
             patch.shape[0], _u8(patch))

    def goal_set(self, goal):
        """Move the goal (pp2_goal_set); ``self.goal`` follows."""
        gx, gy = int(goal[0]), int(goal[1])
        call("pp2_goal_set", self._h, gx, gy)
        self.goal = (gx, gy)

    def map_get(self):
        """(map (H, W) uint8, goal (gx, gy)) in force (pp2_map_get)."""
        m = np.empty((self.global_height, self.width), np.uint8)
        gx, gy = C.c_int32(), C.c_int32()
        call("pp2_map_get", self._h, _u8(m), C.byref(gx), C.byref(gy))
        return m, (gx.value, gy.value)

    def map_update_info(self):
        """(updates that changed the model, served by the patch path, served
        by the full build, dictionary rows the last one appended)."""
        u, i, r = C.c_longlong(), C.c_longlong(), C.c_longlong()
        a = C.c_int()
        call("pp2_map_update_info", self._h, C.byref(u), C.byref(i), C.byref(r),
             C.byref(a))
        return u.value, i.value, r.value, a.value

    def resident_launches(self):
        """(tile-resident loop launches, resident MDP-solve launches) so far."""
        lo = C.c_int()
        so = C.c_int()
        call("pp2_resident_launches", self._h, C.byref(lo), C.byref(so))
        return lo.value, so.value

    def resident_masked(self):
        """(the model is admitted to the resident loop's masked-support form,
        resident loop launches that ran it)."""
        ad = C.c_int()
        n = C.c_int()
        call("pp2_resident_masked", self._h, C.byref(ad), C.byref(n))
        return bool(ad.value), n.value

    def resident_status(self):
        """(resident launches re-run after a timeout, resident kernels enabled)."""
        f = C.c_int()
        e = C.c_int()
        call("pp2_resident_status", self._h, C.byref(f), C.byref(e))
        return f.value, bool(e.value)

    def loop_steps_per_launch(self) -> int:
        """Loop steps one kernel launch of pp2_loop_run covers (2048 resident,
        the resident halo depth on a shard, 2 for step pairs, else 1)."""
        n = C.c_int(0)
        call("pp2_loop_steps_per_launch", self._h, C.byref(n))
        return n.value

    def resident_tiling(self):
        """(tiles, rows per tile, tile columns) of the resident loop on this
        context, (0, 0, 0) when it does not run resident."""
        t, r, c = C.c_int(0), C.c_int(0), C.c_int(0)
        call("pp2_resident_tiling", self._h, C.byref(t), C.byref(r), C.byref(c))
        return t.value, r.value, c.value

    def model_download(self):
        n = self.cells
        T = np.empty((n, 9, 9), np.float32)
        L = np.empty((n, 16), np.float32)
        R = np.empty((n, 9), np.float32)
        Cc = np.empty((n, 9), np.float32)
        call("pp2_model_download", self._h, _f32(T), _f32(L), _f32(R), _f32(Cc))
        return T, L, R, Cc

    def model_upload(self, T=None, L=None, R=None, Cc=None):
        keep = []

        def p(a, shape):
            if a is None:
                return _NULLF
            a = np.ascontiguousarray(a, np.float32).reshape(shape)
            keep.append(a)
            return _f32(a)
        n = self.cells
        call("pp2_model_upload", self._h, p(T, (n, 9, 9)), p(L, (n, 16)),
             p(R, (n, 9)), p(Cc, (n, 9)))

    def model_save(self, directory: str):
        call("pp2_model_save", self._h, directory.encode())

    def model_load(self, directory: str):
        call("pp2_model_load", self._h, directory.encode())

    # ------------------------------------------------------------ belief
    def belief_set(self, b):
        b = np.ascontiguousarray(b, np.float32).reshape(self.cells)
        call("pp2_belief_set", self._h, _f32(b))

    def belief_get(self) -> np.ndarray:
        out = np.empty(self.cells, np.float32)
        call("pp2_belief_get", self._h, _f32(out))
        return out

    def belief_update(self, u: int, z: int):
        call("pp2_belief_update", self._h, int(u), int(z))

    def belief_get_raw(self):
        out = np.empty(self.cells, np.float32)
        m = C.c_float()
        call("pp2_belief_get_raw", self._h, _f32(out), C.byref(m))
        return out, m.value

    def belief_mass(self) -> float:
        m = C.c_float()
        call("pp2_belief_mass", self._h, C.byref(m))
        return m.value

    # ------------------------------------------------------------ MDP
    def mdp_reset(self):
        call("pp2_mdp_reset", self._h)

    def mdp_sweep(self, n: int = 1):
        call("pp2_mdp_sweep", self._h, int(n))

    def mdp_solve(self, max_sweeps: int = 0):
        s = C.c_int()
        nrm = C.c_double()
        call("pp2_mdp_solve", self._h, int(max_sweeps), C.byref(s), C.byref(nrm))
        return s.value, nrm.value

    def mdp_resolve(self, max_sweeps: int = 0):
        """``mdp_solve`` from the current J instead of J = 0 (pp2_mdp_resolve)."""
        s = C.c_int()
        nrm = C.c_double()
        call("pp2_mdp_resolve", self._h, int(max_sweeps), C.byref(s), C.byref(nrm))
        return s.value, nrm.value

    def mdp_get(self):
        J = np.empty(self.cells, np.float32)
        A = np.empty(self.cells, np.uint8)
        call("pp2_mdp_get", self._h, _f32(J), _u8(A))
        return J, A

    # ------------------------------------------------------------ north star
    def loop_step(self, u: int, z: int):
        call("pp2_loop_step", self._h, int(u), int(z))

    def loop_run(self, us, zs):
        us = np.ascontiguousarray(us, np.uint8)
        zs = np.ascontiguousarray(zs, np.uint8)
        if us.shape != zs.shape:
            raise ValueError("us and zs must have the same length")
        call("pp2_loop_run", self._h, int(us.size), us.tobytes(), zs.tobytes())

    def loop_launcher(self, us, zs):
        """A zero-argument callable that runs pp2_loop_run on this trajectory:
        the arguments are converted once, here, so a timed call pays only the
        C-ABI call itself (what a compiled client pays)."""
        us = np.ascontiguousarray(us, np.uint8)
        zs = np.ascontiguousarray(zs, np.uint8)
        if us.shape != zs.shape:
            raise ValueError("us and zs must have the same length")
        lib = _lib.load()
        fn, h, n, ub, zb = lib.pp2_loop_run, self._h, int(us.size), us.tobytes(), zs.tobytes()

        def run():
            st = fn(h, n, ub, zb)
            if st != _lib.PP2_OK:
                msg = lib.pp2_last_error()
                raise _lib.Pp2Error(st, "pp2_loop_run", msg.decode() if msg else "")
        return run

    # ------------------------------------------------------------ control
    CONTROL_MODE = 0   # action of the belief's mode (the reference MDP node)
    CONTROL_QMDP = 1   # argmin_u of the belief-expected Q over the current J
    _POLICIES = {"mode": CONTROL_MODE, "qmdp": CONTROL_QMDP}

    def belief_mode(self):
        """(cell, prob): the first strict maximum > 0 of the normalised belief
        (cell = y * W + x; (0, 0.0) when no cell is > 0), found on the device."""
        cell = C.c_int32(0)
        prob = C.c_float(0.0)
        call("pp2_belief_mode", self._h, C.byref(cell), C.byref(prob))
        return cell.value, np.float32(prob.value)

    def mdp_qvalues(self) -> np.ndarray:
        """q[u] = E_b[C(x, u) + gamma * sum_i T(x, u, i) J(x + off_i)] over the
        current belief and values (float32[9]), reduced on the device."""
        q = np.empty(9, np.float32)
        call("pp2_mdp_qvalues", self._h, _f32(q))
        return q

    def mdp_control(self, policy="qmdp"):
        """(action, value, cell) of a control policy: "mode" (or CONTROL_MODE)
        looks the belief's mode up in the action plane, "qmdp" (CONTROL_QMDP)
        takes the first minimum of mdp_qvalues() (cell = -1)."""
        if isinstance(policy, str):
            if policy not in self._POLICIES:
                raise ValueError(f"unknown control policy {policy!r}")
            policy = self._POLICIES[policy]
        a = C.c_uint8(0)
        v = C.c_float(0.0)
        cell = C.c_int32(0)
        call("pp2_mdp_control", self._h, int(policy), C.byref(a), C.byref(v), C.byref(cell))
        return a.value, np.float32(v.value), cell.value

    # ------------------------------------------------------------ shortest-path field
    def path_solve(self, max_rounds: int | None = None):
        """(rounds, converged, reached): the goal-rooted shortest-path field of
        the map and goal in force, cold (pp2_path_solve).  ``max_rounds``
        defaults to H * W.  Not converged: the field stays invalid."""
        if max_rounds is None:
            max_rounds = self.rows * self.width
        r, cv, n = C.c_int(), C.c_int(), C.c_int()
        call("pp2_path_solve", self._h, int(max_rounds), C.byref(r), C.byref(cv), C.byref(n))
        return r.value, bool(cv.value), n.value

    def path_resolve(self, max_rounds: int | None = None):
        """(rounds, converged, reached, warm): the same field as ``path_solve``,
        repaired from the one the planes hold after ``map_update`` calls
        (pp2_path_resolve): raise what no longer stands, then relax.  ``warm``
        is False when the call fell back to a cold solve (no converged field,
        the goal or its cell changed, more than 16 updates pending).  With a
        valid field: (0, True, reached, True) without a launch."""
        if max_rounds is None:
            max_rounds = self.rows * self.width
        r, cv, n, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        call("pp2_path_resolve", self._h, int(max_rounds), C.byref(r), C.byref(cv), C.byref(n),
             C.byref(w))
        return r.value, bool(cv.value), n.value, bool(w.value)

    def path_resolve_info(self):
        """dict, of the last ``path_resolve``: warm, raised (cells that were
        finite, are still free and were raised), raise_rounds, relax_rounds,
        seed_cells (cells of the pending rectangles the seed pass visited)."""
        v = [C.c_int() for _ in range(5)]
        call("pp2_path_resolve_info", self._h, *[C.byref(x) for x in v])
        keys = ("warm", "raised", "raise_rounds", "relax_rounds", "seed_cells")
        out = {k: x.value for k, x in zip(keys, v)}
        out["warm"] = bool(out["warm"])
        return out

    def path_get(self):
        """(D[H, W] float32, A_path[H, W] uint8) of the valid field."""
        D = np.empty((self.rows, self.width), np.float32)
        A = np.empty((self.rows, self.width), np.uint8)
        call("pp2_path_get", self._h, _f32(D), _u8(A))
        return D, A

    def path_control(self):
        """(action, dist, cell): A_path and D at the belief's mode -- the A*
        node's control, chosen on the device."""
        a = C.c_uint8(0)
        d = C.c_float(0.0)
        cell = C.c_int32(0)
        call("pp2_path_control", self._h, C.byref(a), C.byref(d), C.byref(cell))
        return a.value, np.float32(d.value), cell.value

    def path_trace(self, start):
        """(cells int32[n], length): the path A_path walks from ``start`` (a
        cell index y * W + x, or an (x, y) pair) to the goal, both inclusive;
        n = 0 from an occupied or unreachable start."""
        if isinstance(start, (tuple, list)):
            if len(start) != 2:
                raise ValueError("start is a cell index or an (x, y) pair")
            x, y = int(start[0]), int(start[1])
            if not (0 <= x < self.width and 0 <= y < self.rows):
                raise ValueError(f"start {start!r} is off the grid")
            cell = y * self.width + x
        else:
            cell = int(start)
            if not 0 <= cell < self.rows * self.width:
                raise ValueError(f"start cell {cell} outside [0, {self.rows * self.width})")
        n = C.c_int(0)
        length = C.c_float(0.0)
        lib = _lib.load()
        # the count first (a too-small buffer reports it), then the cells
        st = lib.pp2_path_trace(self._h, cell, None, 0, C.byref(n), C.byref(length))
        if st != _lib.PP2_OK and n.value == 0:
            msg = lib.pp2_last_error()
            raise _lib.Pp2Error(st, "pp2_path_trace", msg.decode() if msg else "")
        cells = np.empty(n.value, np.int32)
        if n.value:
            call("pp2_path_trace", self._h, cell, cells.ctypes.data_as(C.POINTER(C.c_int32)),
                 int(cells.size), C.byref(n), C.byref(length))
        return cells, np.float32(length.value)

    def path_info(self):
        """dict: valid, and the last solve's or resolve's rounds / launches / polls, and the
        relaxation's tile (tile_rows, tile_cols)."""
        v = [C.c_int() for _ in range(6)]
        call("pp2_path_info", self._h, *[C.byref(x) for x in v])
        keys = ("valid", "rounds", "launches", "polls", "tile_rows", "tile_cols")
        out = {k: x.value for k, x in zip(keys, v)}
        out["valid"] = bool(out["valid"])
        return out

    # ------------------------------------------------------------ policy evaluation
    _POLICY_TABLES = {"mdp": 0, "path": 1, "user": 2}
    _POLICY_ROUTES = {"auto": 0, "planes": 1, "tiles": 2}

    def policy_set_table(self, table):
        """The ``"user"`` table of ``policy_evaluate``: H x W actions, every
        entry <= 8 (pp2_policy_set_table); ``None`` drops it."""
        if table is None:
            call("pp2_policy_set_table", self._h, None)
            return
        t = np.ascontiguousarray(table, dtype=np.uint8)
        if t.size != self.rows * self.width:
            raise ValueError(f"table has {t.size} entries, the grid {self.rows * self.width}")
        call("pp2_policy_set_table", self._h, _u8(t))

    def policy_evaluate(self, horizon: int, table="mdp", world=None, route="auto", block: int = 0):
        """Enqueue the exact outcome fields of an action table over ``horizon``
        steps (pp2_policy_evaluate): ``table`` is ``"mdp"`` (A), ``"path"``
        (A_path) or ``"user"``; ``world`` the context whose model the robot
        moves in (None: this one); ``route`` ``"auto"``, ``"planes"`` or
        ``"tiles"``; ``block`` the steps per launch of the tiles route (0: the
        default).  ``policy_get`` returns the result."""
        if isinstance(table, str):
            if table not in self._POLICY_TABLES:
                raise ValueError(f"unknown action table {table!r}")
            table = self._POLICY_TABLES[table]
        if isinstance(route, str):
            if route not in self._POLICY_ROUTES:
                raise ValueError(f"unknown route {route!r}")
            route = self._POLICY_ROUTES[route]
        call("pp2_policy_evaluate", self._h, world._h if world is not None else None,
             int(table), int(horizon), int(route), int(block))

    def policy_get(self):
        """(G, P, N) as H x W float32 arrays: expected discounted cost, goal
        probability within the horizon and expected steps per start cell, of
        the last ``policy_evaluate``.  Synchronises."""
        out = [np.empty((self.rows, self.width), np.float32) for _ in range(3)]
        call("pp2_policy_get", self._h, *[_f32(a) for a in out])
        return tuple(out)

    def policy_info(self):
        """dict: valid, table, horizon, route_taken, block and launches of the
        last evaluation; tile_rows, tile_cols, default_block, max_block of the
        tiles route."""
        v = [C.c_int() for _ in range(10)]
        call("pp2_policy_info", self._h, *[C.byref(x) for x in v])
        keys = ("valid", "table", "horizon", "route_taken", "block", "launches", "tile_rows",
                "tile_cols", "default_block", "max_block")
        out = {k: x.value for k, x in zip(keys, v)}
        out["valid"] = bool(out["valid"])
        return out

    # ------------------------------------------------------------ occupancy
    def occupancy_evaluate(self, horizon: int, b0=None, table="mdp", world=None, route="auto",
                           block: int = 0):
        """Enqueue the forward occupancy of an action table over ``horizon``
        steps from the start distribution ``b0`` (pp2_occupancy_evaluate): H x W
        entries in [0, 1], ``None`` for the context's belief (``belief_get``).
        ``table``, ``world``, ``route`` and ``block`` as in ``policy_evaluate``.
        ``occupancy_get`` returns the result."""
        if isinstance(table, str):
            if table not in self._POLICY_TABLES:
                raise ValueError(f"unknown action table {table!r}")
            table = self._POLICY_TABLES[table]
        if isinstance(route, str):
            if route not in self._POLICY_ROUTES:
                raise ValueError(f"unknown route {route!r}")
            route = self._POLICY_ROUTES[route]
        if b0 is None:
            b0 = self.belief_get()
        b = np.ascontiguousarray(b0, dtype=np.float32)
        if b.size != self.rows * self.width:
            raise ValueError(f"b0 has {b.size} entries, the grid {self.rows * self.width}")
        call("pp2_occupancy_evaluate", self._h, world._h if world is not None else None,
             int(table), _f32(b), int(horizon), int(route), int(block))

    def occupancy_get(self):
        """(D, V, curve) of the last ``occupancy_evaluate``: the distribution
        after the horizon and the expected visits before arrival as H x W
        float32 arrays, and the mass at the goal after step 0 .. horizon.
        Synchronises."""
        horizon = self.occupancy_info()["horizon"]
        D = np.empty((self.rows, self.width), np.float32)
        V = np.empty((self.rows, self.width), np.float32)
        curve = np.empty(horizon + 1, np.float32)
        call("pp2_occupancy_get", self._h, _f32(D), _f32(V), _f32(curve))
        return D, V, curve

    def occupancy_info(self):
        """dict: valid, table, horizon, route_taken, block and launches of the
        last occupancy evaluation; tile_rows, tile_cols, default_block,
        max_block of the tiles route."""
        v = [C.c_int() for _ in range(10)]
        call("pp2_occupancy_info", self._h, *[C.byref(x) for x in v])
        keys = ("valid", "table", "horizon", "route_taken", "block", "launches", "tile_rows",
                "tile_cols", "default_block", "max_block")
        out = {k: x.value for k, x in zip(keys, v)}
        out["valid"] = bool(out["valid"])
        return out

    # ------------------------------------------------------------ FIB
    def fib_reset(self):
        call("pp2_fib_reset", self._h)

    def fib_sweep(self, n: int = 1):
        call("pp2_fib_sweep", self._h, int(n))

    def fib_solve(self, max_sweeps: int = 0):
        s = C.c_int()
        nrm = C.c_float()
        call("pp2_fib_solve", self._h, int(max_sweeps), C.byref(s), C.byref(nrm))
        return s.value, nrm.value

    def fib_resolve(self, max_sweeps: int = 0):
        """``fib_solve`` from the current alphas instead of 0 (pp2_fib_resolve)."""
        s = C.c_int()
        nrm = C.c_float()
        call("pp2_fib_resolve", self._h, int(max_sweeps), C.byref(s), C.byref(nrm))
        return s.value, nrm.value

    def fib_get(self) -> np.ndarray:
        out = np.empty((self.cells, 9), np.float32)
        call("pp2_fib_get", self._h, _f32(out))
        return out

    def fib_set(self, alphas):
        a = np.ascontiguousarray(alphas, np.float32).reshape(self.cells, 9)
        call("pp2_fib_set", self._h, _f32(a))

    def fib_save(self, directory: str):
        call("pp2_fib_save", self._h, directory.encode())

    def fib_load(self, directory: str):
        call("pp2_fib_load", self._h, directory.encode())

    # ------------------------------------------------------------ PBVI
    def pbvi_belief_set(self, b0, set_size: int = 500, rand_seed: int = 1) -> int:
        """generateBeliefSet; returns the number of rand() draws it made."""
        b0 = np.ascontiguousarray(b0, np.float32).reshape(self.cells)
        n = C.c_uint64()
        call("pp2_pbvi_belief_set", self._h, _f32(b0), int(set_size), int(rand_seed),
             C.byref(n))
        return n.value

    def pbvi_set_beliefs(self, beliefs):
        B = np.ascontiguousarray(beliefs, np.float32).reshape(-1, self.cells)
        call("pp2_pbvi_set_beliefs", self._h, B.shape[0], _f32(B))

    def pbvi_info(self):
        s = C.c_uint32()
        h = C.c_int()
        call("pp2_pbvi_info", self._h, C.byref(s), C.byref(h))
        return s.value, bool(h.value)

    def pbvi_get_beliefs(self) -> np.ndarray:
        S, _ = self.pbvi_info()
        out = np.empty((S, self.cells), np.float32)
        call("pp2_pbvi_get_beliefs", self._h, _f32(out))
        return out

    def pbvi_backup(self, iterations: int = 0):
        call("pp2_pbvi_backup", self._h, int(iterations))

    def pbvi_solve(self, b0, set_size: int = 500, rand_seed: int = 1) -> int:
        """pointBasedValueIteration; returns the number of rand() draws."""
        b0 = np.ascontiguousarray(b0, np.float32).reshape(self.cells)
        n = C.c_uint64()
        call("pp2_pbvi_solve", self._h, _f32(b0), int(set_size), int(rand_seed), C.byref(n))
        return n.value

    def pbvi_get(self):
        S, _ = self.pbvi_info()
        al = np.empty((S, self.cells), np.float32)
        act = np.empty(S, np.uint8)
        call("pp2_pbvi_get", self._h, _f32(al), _u8(act))
        return al, act

    def pbvi_set(self, alphas, actions):
        al = np.ascontiguousarray(alphas, np.float32).reshape(-1, self.cells)
        act = np.ascontiguousarray(actions, np.uint8).reshape(al.shape[0])
        call("pp2_pbvi_set", self._h, al.shape[0], _f32(al), _u8(act))

    def pbvi_evaluate(self, beliefs):
        """evaluatePbviCpu over a batch: (values[n], actions[n])."""
        B = np.ascontiguousarray(beliefs, np.float32).reshape(-1, self.cells)
        v = np.empty(B.shape[0], np.float32)
        a = np.empty(B.shape[0], np.uint8)
        call("pp2_pbvi_evaluate", self._h, B.shape[0], _f32(B), _f32(v), _u8(a))
        return v, a

    def pbvi_save(self, directory: str):
        call("pp2_pbvi_save", self._h, directory.encode())

    def pbvi_load(self, directory: str, set_size: int = 500):
        call("pp2_pbvi_load", self._h, directory.encode(), int(set_size))

    # ------------------------------------------------------------ shards
    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = (C.c_uint8 * _lib.RCCL_ID_BYTES)()
        call("pp2_rccl_unique_id", buf)
        return bytes(buf)

    def shard_comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * _lib.RCCL_ID_BYTES).from_buffer_copy(uid)
        call("pp2_shard_comm_init", self._h, buf, int(nranks), int(rank))


def device_count() -> int:
    n = C.c_int()
    call("pp2_device_count", C.byref(n))
    return n.value


class ShardGroup:
    """Row shards of one grid driven from one process (pp2_shard_group_*):
    halo rows and the belief mass move by device copies between the shard
    contexts, which may live on one or several devices.

    ``bounds`` are the row boundaries, e.g. (0, 256, 512, ..., H)."""

    def __init__(self, grid: np.ndarray, goal, bounds, gamma: float = 0.95,
                 devices=None):
        bounds = [int(b) for b in bounds]
        n = len(bounds) - 1
        devices = list(devices) if devices is not None else [0] * n
        self.shards = [GridContext(grid, goal, gamma=gamma, device=devices[i],
                                   rows=(bounds[i], bounds[i + 1]))
                       for i in range(n)]
        arr = (C.c_void_p * n)(*[s.handle.value for s in self.shards])
        h = C.c_void_p()
        call("pp2_shard_group_create", C.byref(h), arr, n)
        self._h = h
        self.bounds = bounds

    def model_generate(self):
        for s in self.shards:
            s.model_generate()

    def belief_set(self, b):
        b = np.ascontiguousarray(b, np.float32).reshape(-1)
        for s in self.shards:
            s.belief_set(b[s.row_begin * s.width:s.row_end * s.width])

    def belief_get(self):
        return np.concatenate([s.belief_get() for s in self.shards])

    def mdp_reset(self):
        for s in self.shards:
            s.mdp_reset()
        self.synchronize()

    def mdp_get(self):
        parts = [s.mdp_get() for s in self.shards]
        return (np.concatenate([p[0] for p in parts]),
                np.concatenate([p[1] for p in parts]))

    def fib_get(self):
        return np.concatenate([s.fib_get() for s in self.shards])

    def fib_reset(self):
        for s in self.shards:
            s.fib_reset()
        self.synchronize()

    def set_halo_depth(self, k: int):
        """Loop steps per halo exchange (= halo rows exchanged), on every shard."""
        for s in self.shards:
            s.set_tuning(GridContext.TUNE_HALO_DEPTH, int(k))

    def loop_step(self, u, z):
        call("pp2_shard_group_loop_step", self._h, int(u), int(z))

    def loop_run(self, us, zs):
        us = np.ascontiguousarray(us, np.uint8)
        zs = np.ascontiguousarray(zs, np.uint8)
        if us.shape != zs.shape:
            raise ValueError("us and zs must have the same length")
        call("pp2_shard_group_loop_run", self._h, int(us.size), us.tobytes(), zs.tobytes())

    def set_tuning(self, key: int, value: int):
        for s in self.shards:
            s.set_tuning(key, value)

    def loop_steps_per_launch(self):
        return [s.loop_steps_per_launch() for s in self.shards]

    def belief_update(self, u, z):
        call("pp2_shard_group_belief_update", self._h, int(u), int(z))

    def mdp_sweep(self, n=1):
        call("pp2_shard_group_mdp_sweep", self._h, int(n))

    def mdp_solve(self, max_sweeps=0):
        s = C.c_int()
        nrm = C.c_double()
        call("pp2_shard_group_mdp_solve", self._h, int(max_sweeps), C.byref(s),
             C.byref(nrm))
        return s.value, nrm.value

    def fib_sweep(self, n=1):
        call("pp2_shard_group_fib_sweep", self._h, int(n))

    def synchronize(self):
        call("pp2_shard_group_synchronize", self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().pp2_shard_group_destroy(self._h)
            self._h = None
        for s in getattr(self, "shards", []):
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
