"""Inputs and the decision check of the formation-rollout tests (mpccbf_formation_rollout,
mpccbf.FormationRollouts): the instances of the parity batch, the seeded team batches of the shape
edges, the hand-built teams of the summary test, and the teacher-forced reference — the unchanged
oracle (oracle_lib.connectivity_control, oracle_lib.normal_sample) applied to the table every
decision of a recorded run planned from.

Shared by tests/test_formation_rollout_inputs.py (CPU), tests/test_formation_rollout_api.py (CPU) and
tests/test_gpu_formation_rollout.py (GPU).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from mpccbf import formation, swarm

# the parity batch: 2, 3, 3, 3, 5, 6, 8 ("3r/line3" holds 8 robots) and 8 robots
PARITY_NAMES = ("2r/line", "3r/bend", "3r/line2", "3r/triangle", "5r/circle", "6r/upward", "3r/line3", "8r/circle2")
PARITY_STEPS = 30
PARITY_SEED = 20240611
SPRING = 0.5
L2_SWITCH = 0.1  # ConnectivityControl.cpp:69


def desired_control(state, target, k=SPRING):
    """criticallyDampedSpringControl (Controls.h:18-27)."""
    return k * (np.asarray(target) - state[:3]) - 2.0 * np.sqrt(k) * state[3:6]


def noise_draw(seed, step, robot, pos_std, vel_std):
    """The six noise terms of robot `robot` (index in its team) at absolute step `step`."""
    return np.array([(pos_std if c < 3 else vel_std) * O.normal_sample(seed, step, robot, c)
                     if (pos_std if c < 3 else vel_std) > 0.0 else 0.0 for c in range(6)])


@functools.lru_cache(maxsize=None)
def parity_groups(slack: bool):
    """The parity batch under preprocess="own" with the slack mode overridden, grouped by parameters
    (formation.instance_groups, which FormationRollouts.from_instances builds its objects from): a
    tuple of dicts(cfg, names, teams, pos_std, vel_std, shape_half), teams = [(name, states, targets)].
    Built without a GPU; what the groups must be is pinned in test_formation_rollout_inputs.py."""
    return tuple(formation.instance_groups(PARITY_NAMES, "own", slack))


def oracle_free_run(cfg, states, targets, seed, steps, Ts, pos_std, vel_std, step_first=0):
    """The example's loop on the CPU with the oracle (free-running): dict(trace [steps][n][6],
    status, lambda2 [steps][n], cbf_u, desired_u [steps][n][3], tables [steps][n] = the table each
    decision planned from)."""
    cur = np.array(states, dtype=np.float64)
    n = len(cur)
    out = dict(trace=np.zeros((steps, n, 6)), status=np.zeros((steps, n), dtype=np.int32), lambda2=np.zeros((steps, n)),
               cbf_u=np.zeros((steps, n, 3)), desired_u=np.zeros((steps, n, 3)), tables=[])
    for s in range(steps):
        row = []
        for i in range(n):
            row.append(cur.copy())
            ud = desired_control(cur[i], targets[i])
            st, u, _, l2 = O.connectivity_control(cfg, cur, i, ud)
            if st != O.OPTIMAL:
                u = np.zeros(3)
            cur[i] = O.apply_input(Ts, cur[i], u) + noise_draw(seed, step_first + s, i, pos_std, vel_std)
            out["status"][s, i], out["lambda2"][s, i], out["cbf_u"][s, i], out["desired_u"][s, i] = st, l2, u, ud
        out["tables"].append(row)
        out["trace"][s] = cur
    return out


def check_decisions(cfg, states0, targets, seed, rec, Ts, pos_std, vel_std, step_first=0, order="gauss_seidel"):
    """Every decision of one team's recorded run against the oracle on the table that decision planned
    from, rebuilt from the run's own trace: robots < i from sample s, the others from sample s - 1
    (or the initial states). order="jacobi": the whole table from sample s - 1 (the wrong order: the
    witness that the check tells the two apart). rec: the team's slices trace [steps][n][6], cbf_u,
    desired_u [steps][n][3], status, lambda2 [steps][n].
    Returns the list of mismatches as strings (empty: every decision agrees)."""
    states0 = np.asarray(states0, dtype=np.float64)
    n, steps = len(states0), len(rec["trace"])
    bad = []

    def near(a, b, rel):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return bool(np.all(np.abs(a - b) <= rel * np.maximum(1.0, np.abs(b))))

    for s in range(steps):
        prev = states0 if s == 0 else rec["trace"][s - 1]
        for i in range(n):
            tab = np.array(prev) if order == "jacobi" else np.concatenate([rec["trace"][s][:i], prev[i:]])
            ud = desired_control(tab[i], targets[i])
            st, u, _, l2 = O.connectivity_control(cfg, tab, i, ud)
            g_st, g_l2, g_u = int(rec["status"][s, i]), float(rec["lambda2"][s, i]), rec["cbf_u"][s, i]
            tag = f"step {s} robot {i}"
            if g_st != st:
                bad.append(f"{tag}: status {g_st} != oracle {st}")
            if (g_l2 > L2_SWITCH) != (l2 > L2_SWITCH):
                bad.append(f"{tag}: branch lambda2 {g_l2!r} vs oracle {l2!r}")
            if not abs(g_l2 - l2) <= 1e-10 * max(1.0, abs(l2)):
                bad.append(f"{tag}: lambda2 {g_l2!r} vs oracle {l2!r}")
            if st == O.OPTIMAL and g_st == O.OPTIMAL:
                if not np.allclose(g_u, u, atol=1e-5, rtol=1e-5):
                    bad.append(f"{tag}: u {g_u} vs oracle {u}")
            elif g_st != O.OPTIMAL and np.any(g_u != 0.0):
                bad.append(f"{tag}: not OPTIMAL but cbf_u {g_u} is not the zero fallback")
            if not near(rec["desired_u"][s, i], ud, 1e-12):
                bad.append(f"{tag}: desired_u {rec['desired_u'][s, i]} vs {ud}")
            nxt = O.apply_input(Ts, tab[i], g_u) + noise_draw(seed, step_first + s, i, pos_std, vel_std)
            if not near(rec["trace"][s][i], nxt, 1e-12):
                bad.append(f"{tag}: next state {rec['trace'][s][i]} vs {nxt}")
    return bad


# ---- seeded teams of the shape edges ----------------------------------------------------------
def edge_cfg(slack=False):
    c = dict(d_min=0.8, d_max=3.0, v_min=[-1.0, -1.0, -2.6179938779914944], v_max=[1.0, 1.0, 2.6179938779914944],
             Ts=0.01, control_slack_mode=0, slack_cost=1e5, slack_decay_rate=0.1)
    if slack:
        c["control_slack_mode"] = 1
    return c


EDGE_NOISE = dict(pos_std=0.001, vel_std=0.01)


def edge_batch(sizes, seed=11, spacing=1.6, shape="ring"):
    """(states, targets, team_ptr, seeds) of seeded teams (swarm.team_swarm: rings whose neighbours
    are `spacing` apart, or square lattices with that spacing; slower than the velocity bounds), one
    noise key per team."""
    states, targets, team_ptr = swarm.team_swarm(sizes, spacing=spacing, seed=seed, shape=shape, speed=(0.1, 0.6),
                                                 vel_noise=0.1)
    seeds = [1000003 * (t + 1) + seed for t in range(len(sizes))]
    return states, targets, team_ptr, seeds


# teams at the row capacity on the connectivity row: 15 and 16 robots on a lattice 1.0 apart (above d_min
# 0.8 with the 0.05 position noise, well inside d_max 3.0: lambda2 1.6), where the rings of edge_batch's
# default spacing are on the CLF rows (lambda2 0.07)
DENSE_SIZES = (15, 16)


def dense_batch():
    return edge_batch(list(DENSE_SIZES), seed=11, spacing=1.0, shape="grid")


# ---- hand-built teams of the summary test -----------------------------------------------------
def summary_teams():
    """(cfg, shape_half, goal_radius, teams) without noise; teams = list of (name, states, targets):
    head_on   two robots 0.3 apart (inside d_min 0.8, boxes of half extent 0.2 overlap: offsets below
              0.4) closing at 0.5 each: the safety rows cannot be met, control is zero, the first
              sample collides as (0, 0, 1) and the instance fails;
    arrive_then_collide   both robots are inside their goal areas from sample 0 on, 0.45 apart and
              closing by 0.018 a step under zero control: the boxes overlap from sample 2 (0.396) on,
              after the walk has stopped at the arrival, so the instance succeeds;
    same_sample   as head_on but each robot's target under it: the last arrival and the first
              collision are both sample 0, which fails."""
    cfg = edge_cfg(False)
    shape_half, goal_radius = (0.2, 0.2), 0.5
    z = np.zeros
    S = z((2, 6))
    S[:, :2] = [(0.0, 0.0), (0.3, 0.05)]
    S[:, 3] = (0.5, -0.5)
    head_on = ("head_on", S.copy(), np.array([[5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]]))
    same_sample = ("same_sample", S.copy(), np.array([[0.0, 0.0, 0.0], [0.3, 0.05, 0.0]]))
    S = z((2, 6))
    S[:, :2] = [(0.0, 0.0), (0.45, 0.0)]
    S[:, 3] = (0.9, -0.9)
    arrive = ("arrive_then_collide", S.copy(), np.array([[0.1, 0.0, 0.0], [0.3, 0.0, 0.0]]))
    return cfg, shape_half, goal_radius, [head_on, arrive, same_sample]
