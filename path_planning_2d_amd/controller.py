"""Belief + MDP controllers: the plan step after the belief update / Bellman
sweep, chosen on the device (pp2_mdp_control).

``BeliefMdpController`` has ``QVTreePlanner.step``'s shape, so it plugs into
``synthetic.closed_loop``: every message updates the context's belief and asks
the policy for the next action -- "mode" is the reference MDP node's
beliefCallback (the action plane at the belief's mode), "qmdp" the argmin of
the belief-expected Q values of the current J.
"""
from __future__ import annotations

import numpy as np

from .core import GridContext


class BeliefMdpController:
    """Control selection over a ``GridContext`` that holds a model and MDP
    values (``mdp_solve`` / ``mdp_sweep``).

    ``sweeps_per_step`` = 0 keeps J as it is and only propagates the belief;
    1 runs the fused loop step (belief update + one Bellman sweep) per message,
    the benchmarked loop with its plan step attached."""

    def __init__(self, ctx: GridContext, policy="qmdp", sweeps_per_step: int = 0):
        if sweeps_per_step not in (0, 1):
            raise ValueError("sweeps_per_step must be 0 or 1")
        if isinstance(policy, str) and policy not in GridContext._POLICIES:
            raise ValueError(f"unknown control policy {policy!r}")
        self.ctx = ctx
        self.policy = policy
        self.sweeps_per_step = int(sweeps_per_step)
        self.last_cell = -1

    def step(self, action: int, observation: int, belief=None):
        """One message: (last action, observation, root belief or None) ->
        (action, value).  ``value`` is J at the mode ("mode") or the expected
        Q of the chosen action ("qmdp")."""
        if belief is not None:
            self.ctx.belief_set(belief)
        elif self.sweeps_per_step == 1:
            self.ctx.loop_step(action, observation)
        else:
            self.ctx.belief_update(action, observation)
        a, v, cell = self.ctx.mdp_control(self.policy)
        self.last_cell = cell
        return int(a), np.float32(v)


class AStarController:
    """The A* node's control over a ``GridContext`` that holds a model (for the
    belief updates) and a valid shortest-path field (``path_solve``): every
    message updates the belief and takes the first step of the shortest path
    from the belief's mode (``path_control``).  ``step`` has
    ``BeliefMdpController.step``'s shape; ``value`` is the path length from the
    mode."""

    def __init__(self, ctx: GridContext):
        self.ctx = ctx
        self.last_cell = -1

    def step(self, action: int, observation: int, belief=None):
        if belief is not None:
            self.ctx.belief_set(belief)
        else:
            self.ctx.belief_update(action, observation)
        a, d, cell = self.ctx.path_control()
        self.last_cell = cell
        return int(a), np.float32(d)
