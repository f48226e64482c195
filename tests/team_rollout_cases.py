"""Inputs and the decision checks of the team-rollout tests (mpccbf_team_rollout,
mpccbf.TeamRollouts): the instances compared bit for bit with the per-robot-launch simulator, the
parity batch and its teacher-forced rule against the unchanged oracle
(oracle_lib.closed_loop_gauss_seidel(..., inputs=)), the order witness, the seeded team batches of
the shape edges and the hand-built teams of the summary test.

Shared by tests/test_team_rollout_inputs.py (CPU), tests/test_team_rollout_api.py (CPU) and
tests/test_gpu_team_rollout.py (GPU).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from mpccbf import instances, swarm

# 1. bit for bit the simulator: (instance, steps). 2r/circle crosses OPTIMAL -> INFEASIBLE near step 11,
# 5r/circle at step 2; 8r/circle starts inside d_min (every QP INFEASIBLE, the robots hold position)
BITS_CASES = (("2r/circle", 24), ("5r/circle", 16), ("8r/circle", 10), ("3r/line", 20))
BITS_SEED = 20251015
INSIDE_DMIN = ("8r/circle",)  # of BITS_CASES: started inside d_min

# 2. the parity batch: 2, 3, 3, 3, 5, 6, 8 ("3r/line3" holds 8 robots) and 8 robots, on the base config
PARITY_NAMES = ("2r/line", "3r/bend", "3r/line2", "3r/triangle", "5r/circle", "6r/upward", "3r/line3", "8r/circle2")
PARITY_ROBOTS = (2, 3, 3, 3, 5, 6, 8, 8)
PARITY_STEPS = 30
PARITY_SEED = 20240611
WITNESS = "5r/circle"  # the order witness' team of the parity batch


@functools.lru_cache(maxsize=None)
def instance(name):
    """(cfg, states, targets, shape, kind, noise) of a baseline instance on the base config."""
    return instances.instance(name, preprocess="base")


def min_start_distance(states):
    st = np.asarray(states)
    d = np.sqrt(((st[:, None, :2] - st[None, :, :2]) ** 2).sum(-1)) + np.diag(np.full(len(st), np.inf))
    return float(d.min())


# ---- the teacher-forced rule of test_gpu_reference_instances.py --------------------------------
def check_oracle_parity(cfg, states, targets, trace, status, objs, seed, pos_std, vel_std, label=""):
    """One team's recorded run against the oracle fed with the run's own tables. trace: steps + 1 x n
    x 6 (the initial states, then the table after every step); status, objs: steps x n x impc_iter.
    Statuses equal; every next state within 1e-8, else within 1e-6 with the device objective not
    worse than the oracle's beyond 1e-8 relative; at most max(2, 2 %) such updates. Returns
    (updates beyond 1e-8, updates)."""
    states, targets = np.asarray(states, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    steps, n = len(status), len(states)
    one, one_status = O.closed_loop_gauss_seidel(cfg, states, targets, steps, pos_std=pos_std, vel_std=vel_std,
                                                 seed=seed, neighbours="all", inputs=trace)
    np.testing.assert_array_equal(np.asarray(status), one_status, err_msg=label)
    err = np.max(np.abs(trace - one), axis=2)
    p = O.make_params(cfg)
    refs = np.tile(targets, (1, cfg["k_hor"]))
    for s1, i in zip(*np.nonzero(err > 1e-8)):
        assert err[s1, i] <= 1e-6, (label, s1, i, err[s1, i])
        st = s1 - 1
        cur = np.concatenate([trace[st + 1][:i], trace[st][i:]])
        nb = np.array([j for j in range(n) if j != i], dtype=np.int32)
        r = O.impc_optimize(p, cur, i, nb, refs[i])
        ok = r["status"] == O.OPTIMAL
        assert np.all(objs[st][i][ok] <= r["obj"][ok] + 1e-8 * np.maximum(1.0, np.abs(r["obj"][ok]))), \
            (label, st, i, objs[st][i], r["obj"])
    loose = int((err > 1e-8).sum())
    assert loose <= max(2, 0.02 * err.size), (label, np.argwhere(err > 1e-8))
    return loose, int(err.size)


# ---- the order witness --------------------------------------------------------------------------
def order_mismatches(cfg, states, targets, trace, seed, pos_std, vel_std, order="jacobi", tol=1e-6):
    """Every update of one team's recorded run repeated by the oracle from the table of the given
    order: "jacobi" = the whole table of the previous sample (the wrong order for this kernel),
    "gauss_seidel" = robots < i from the new sample. The loop is oracle_lib.closed_loop_gauss_seidel's
    (kept curve, traj_t, hold position, the noise draws), with the table chosen here.
    Returns [(step, robot, |difference|)] of the next states further than tol from the trace's."""
    p = O.make_params(cfg)
    states, targets = np.asarray(states, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    n, steps = len(states), len(trace) - 1
    refs = np.tile(targets, (1, cfg["k_hor"]))
    nsub = int(cfg["h"] / cfg["Ts"])
    eval_step, tmax = cfg["Ts"] * nsub, cfg["num_pieces"] * cfg["piece_max_parameter"]
    xs, traj_t, bad = [None] * n, np.full(n, -1.0), []
    for s in range(steps):
        for i in range(n):
            tab = np.array(trace[s]) if order == "jacobi" else np.concatenate([trace[s + 1][:i], trace[s][i:]])
            nb = np.array([j for j in range(n) if j != i], dtype=np.int32)
            r = O.impc_optimize(p, tab, i, nb, refs[i])
            ok = np.nonzero(r["status"] == O.OPTIMAL)[0]
            if len(ok):
                xs[i], traj_t[i] = r["x"][ok[-1]].copy(), 0.0
            nxt = np.zeros(6)
            for c in range(6):
                sd = pos_std if c < 3 else vel_std
                if xs[i] is not None:
                    t_new = min(traj_t[i] + eval_step, tmax)
                    v = O.eval_curve(p, xs[i], t_new, 0 if c < 3 else 1)[c % 3]
                    nxt[c] = v + sd * O.normal_sample(seed, s, i, c) if sd > 0.0 else v
                else:
                    v = tab[i, c] if c < 3 else 0.0
                    for kk in range(1, nsub + 1):
                        dn = sd * O.normal_sample(seed, s, i, c, nsub - kk) if sd > 0.0 else 0.0
                        v = v + dn if c < 3 else dn
                    nxt[c] = v
            if xs[i] is not None:
                traj_t[i] = min(traj_t[i] + eval_step, tmax)
            d = float(np.max(np.abs(nxt - trace[s + 1][i])))
            if not d <= tol:
                bad.append((s, i, d))
    return bad


# ---- seeded teams of the shape edges ----------------------------------------------------------
EDGE_NOISE = dict(pos_std=0.001, vel_std=0.01)
EDGE_SPACING = 2.6  # above the base config's d_min = 2 with the 0.05 position noise of team_swarm


def base_cfg(**over):
    cfg = dict(instance("2r/line")[0])
    cfg.update(over)
    return cfg


def edge_batch(sizes, seed=11, spacing=EDGE_SPACING):
    """(states, targets, team_ptr, seeds) of seeded teams on square lattices of the given spacing
    (swarm.team_swarm; slower than the velocity bounds), one noise key per team. Sizes 0 and above 16
    are laid out like the others (the kernel must not step them)."""
    states, targets, team_ptr = swarm.team_swarm(sizes, spacing=spacing, seed=seed, shape="grid", speed=(0.1, 0.6),
                                                 vel_noise=0.1)
    seeds = [1000003 * (t + 1) + seed for t in range(len(sizes))]
    return states, targets, team_ptr, seeds


SHAPE_SIZES = (1, 2, 15, 16)
KHOR10_SIZES = (4,)  # the seeded team run at k_hor = 10
BATCH_COUNTS = (1, 33, 300)


def small_batch(teams, seed=5):
    """`teams` teams of 2 and 3 robots in turn."""
    return edge_batch([2 + (t % 2) for t in range(teams)], seed=seed)


# ---- hand-built teams of the summary test -----------------------------------------------------
def summary_teams():
    """(shape_half, goal_radius, steps, teams) on the base config without noise; teams = list of
    (name, states, targets, expected), expected = (instance_success, first_collision, arrived):
    on_targets   two robots 0.3 apart: inside d_min = 2, every QP INFEASIBLE, both hold position; the
                 boxes (half extent 0.2: offsets below 0.4 overlap) collide from sample 0 on; each
                 target under its robot: the last arrival and the first collision are both sample 0,
                 which fails;
    far_targets  the same pair with targets 50 m away: never arrives, collides in sample 0, fails;
    clean_arrive two robots 10 m apart, each 0.5 m from its target (inside the goal radius 1 from
                 sample 0 on, and staying: the curve leads to the target): succeeds;
    clean_far    the same pair with targets 50 m away: no collision, no arrival within the run."""
    z = np.zeros
    S = z((2, 6))
    S[:, :2] = [(0.0, 0.0), (0.3, 0.05)]
    on = ("on_targets", S.copy(), np.array([[0.0, 0.0, 0.0], [0.3, 0.05, 0.0]]), (False, (0, 0, 1), True))
    far = ("far_targets", S.copy(), np.array([[50.0, 0.0, 0.0], [-50.0, 0.0, 0.0]]), (False, (0, 0, 1), False))
    S = z((2, 6))
    S[:, :2] = [(0.0, 0.0), (10.0, 0.0)]
    arrive = ("clean_arrive", S.copy(), np.array([[0.0, 0.5, 0.0], [10.0, 0.5, 0.0]]), (True, None, True))
    clean_far = ("clean_far", S.copy(), np.array([[0.0, 50.0, 0.0], [10.0, 50.0, 0.0]]), (True, None, False))
    return (0.2, 0.2), 1.0, 3, [on, far, arrive, clean_far]
