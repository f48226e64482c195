"""Inputs of test_gpu_neighbour_shortcuts.py (GPU) and test_neighbour_shortcut_inputs.py (CPU): one
swarm of 63 agents on dyadic coordinates (exact squared distances, as exact_geometry_cases.py) whose
within-radius candidate counts sit on both sides of every branch of the 16-lane query's ranking
(grid_neighbors_finish, kernels/impc_common.hpp): no more than knn_k candidates (all kept, no
ranking), more than knn_k (ranked), no more than 16 (one candidate per lane) and more than 16 (two).

The pieces, each at least 16 away from the others (beyond every radius used here):
  line    33 agents along x at spacing 0.25: with radius 4.0 the ends see 16 others, the next 17, ...
          the middle one all 32; with radius 3.75 the ends see 15, then 16, 17, ... 30
  single  one agent alone (0)
  pair    two agents 0.5 apart (1 each)
  c8      2 x 4 patch, spacing 0.5 (7 each)
  c9      3 x 3 patch, spacing 0.5 (8 each)
  c10     2 x 5 patch, spacing 0.5 (9 each): with knn_k = 8 the cut drops one candidate, at the
          middle column out of a shell of two at equal distance
The agents are indexed round-robin over the pieces, so that the four agents of a wave of the 16-lane
kernels (agents 4 w .. 4 w + 3) come from different pieces. Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

from mpccbf import swarm

LINE_N, LINE_STEP = 33, 0.25
# (knn_k, knn_radius) -> candidate counts some agent must have under it
QUERIES = {
    (8, 4.0): {0, 1, 7, 8, 9, 16, 17, 32},      # 0, 1, k - 1, k, k + 1, 16, 17, 32
    (1, 4.0): {0, 1, 7, 16, 17, 32},            # k = 1: k - 1, k, and ranked beyond
    (16, 4.0): {0, 1, 9, 16, 17, 32},           # the largest k: k and k + 1 on the line
    (16, 3.75): {0, 15, 16, 17, 30},            # ... and k - 1
}
K_MAX = 16  # NB_MAX of kernels/impc.hpp: the largest knn_k of the grid query


def _pieces():
    line = [(-4.0 + LINE_STEP * i, 0.0) for i in range(LINE_N)]
    single = [(32.0, 32.0)]
    pair = [(-32.0, 32.0), (-31.5, 32.0)]

    def patch(x0, y0, nx, ny):
        return [(x0 + 0.5 * i, y0 + 0.5 * j) for j in range(ny) for i in range(nx)]

    return [line, single, pair, patch(32.0, -32.0, 4, 2), patch(-32.0, -32.0, 3, 3), patch(0.0, 48.0, 5, 2)]


def shortcut_swarm():
    """(states 63 x 6, targets 63 x 3): the pieces above, indexed round-robin over the pieces (an
    exhausted piece drops out of the rotation); at rest, each agent its own target."""
    pieces = [list(p) for p in _pieces()]
    pos = []
    while any(pieces):
        for p in pieces:
            if p:
                pos.append(p.pop(0))
    states = np.zeros((len(pos), 6))
    states[:, :2] = np.asarray(pos)
    return states, states[:, :3].copy()


def counts(states, radius):
    """Candidates within the radius (inclusive) per agent, self excluded."""
    p = states[:, :2]
    d2 = np.sum((p[:, None, :] - p[None, :, :]) ** 2, axis=-1)
    return (d2 <= radius * radius).sum(axis=1) - 1


_REF = {}


def reference_lists(query):
    """swarm.knn_csr of shortcut_swarm() under (knn_k, knn_radius), computed once."""
    if query not in _REF:
        _REF[query] = swarm.knn_csr(shortcut_swarm()[0], *query)
    return _REF[query]


# ---------------------------------------------------------------------------------------------
# the solve compared with the oracle: a 6 x 6 lattice at spacing 2.5 (d_min = 2.0), radius 5.0, k = 8
# ---------------------------------------------------------------------------------------------
SOLVE_QUERY = (8, 5.0)


def solve_lattice():
    """36 agents, x and y from -6.25 to +6.25 at spacing 2.5, velocities -0.25 * sign(position) per axis,
    targets -0.5 * position: corners see 5 candidates, edges 7 or 8, the interior 10 to 12 — a wave
    without a ranked group, waves that mix kept-unranked and ranked groups, none beyond 16. Returns (states, targets)."""
    g = np.arange(36)
    states = np.zeros((36, 6))
    states[:, 0] = -6.25 + 2.5 * (g % 6)
    states[:, 1] = -6.25 + 2.5 * (g // 6)
    states[:, 3] = -0.25 * np.sign(states[:, 0])
    states[:, 4] = -0.25 * np.sign(states[:, 1])
    targets = np.zeros((36, 3))
    targets[:, :2] = -0.5 * states[:, :2]
    return states, targets
