"""CPU: the inputs of the team-rollout tests are what tests/test_gpu_team_rollout.py takes them for
(team sizes, which instances start inside d_min, distinct noise keys, lattices above d_min, one
parameter set), and the hand-built summary teams give their stated answers under mpccbf.metrics on
hand-written traces. No GPU, no library."""
import numpy as np

import team_rollout_cases as T
from mpccbf import metrics, team_rollout


def test_bit_identity_instances_are_what_they_claim():
    sizes = {"2r/circle": 2, "5r/circle": 5, "8r/circle": 8, "3r/line": 3}
    assert [n for n, _ in T.BITS_CASES] == list(sizes)
    for name, steps in T.BITS_CASES:
        cfg, states, targets, shape, kind, noise = T.instance(name)
        team_rollout.check_config(cfg)  # the collision controller without slack variables
        assert len(states) == sizes[name] <= team_rollout.TEAM_MAX and kind == "box"
        assert np.all(states[:, 3:] == 0.0) and noise == dict(pos_std=0.001, vel_std=0.01)
        assert (T.min_start_distance(states) < cfg["d_min"]) == (name in T.INSIDE_DMIN), name
        assert 1 <= steps <= 24
    # the dense 64 x 4 layout's configuration: two box-row slots per lane at k_hor = 16
    assert T.instance("2r/circle")[0]["k_hor"] == 16 and T.instance("2r/circle")[0]["impc_iter"] == 2


def test_parity_batch_is_one_parameter_set():
    """TeamRollouts.from_instances takes one parameter set per object: the base config gives one."""
    first = T.instance(T.PARITY_NAMES[0])
    for name, robots in zip(T.PARITY_NAMES, T.PARITY_ROBOTS):
        cfg, states, targets, shape, kind, noise = T.instance(name)
        assert len(states) == len(targets) == robots <= team_rollout.TEAM_MAX
        assert (cfg, shape, kind, noise) == (first[0], first[3], first[4], first[5])
    assert sum(T.PARITY_ROBOTS) == 38 and T.WITNESS in T.PARITY_NAMES
    assert T.PARITY_ROBOTS[T.PARITY_NAMES.index(T.WITNESS)] == 5
    # 15 * cbf_horizon CBF rows of a full team fit the layout's 256 row slots beside the shared rows
    assert first[0]["cbf_horizon"] == 2


def test_edge_batches():
    cfg = T.base_cfg()
    team_rollout.check_config(cfg)
    for sizes in (list(T.SHAPE_SIZES), list(T.KHOR10_SIZES), [3, 17, 0, 2]):
        states, targets, team_ptr, seeds = T.edge_batch(sizes)
        assert np.diff(team_ptr).tolist() == sizes and len(states) == sum(sizes) == len(targets)
        assert len(set(seeds)) == len(seeds)
        for t, n in enumerate(sizes):
            if n > 1:  # every team starts outside d_min: its first QPs are solvable
                assert T.min_start_distance(states[team_ptr[t]:team_ptr[t + 1]]) > cfg["d_min"], (sizes, t)
    assert max(T.SHAPE_SIZES) == team_rollout.TEAM_MAX and min(T.SHAPE_SIZES) == 1
    for teams in T.BATCH_COUNTS:
        states, targets, team_ptr, seeds = T.small_batch(teams)
        assert len(team_ptr) == teams + 1 and set(np.diff(team_ptr).tolist()) <= {2, 3}
        assert len(set(seeds)) == teams
    # a team's data does not depend on the batch it is built in (the place-in-batch tests rely on it)
    s1, t1, p1, k1 = T.small_batch(1)
    s33, t33, p33, k33 = T.small_batch(33)
    assert np.array_equal(s1, s33[:p33[1]]) and np.array_equal(t1, t33[:p33[1]]) and k1[0] == k33[0]
    assert T.base_cfg(k_hor=10)["k_hor"] == 10 and cfg["k_hor"] == 16


def test_summary_teams_give_their_stated_answers():
    """Each hand-built pair held at its start (the overlapping pairs hold by construction: inside
    d_min with no noise; for the clean pairs the stated answers only need them to stay apart and, for
    clean_arrive, inside their goal areas) scored by metrics.instance_success over the run's samples."""
    shape_half, goal_radius, steps, teams = T.summary_teams()
    cfg = T.base_cfg()
    samples = steps * int(cfg["h"] / cfg["Ts"])
    assert [t[0] for t in teams] == ["on_targets", "far_targets", "clean_arrive", "clean_far"]
    for name, states, targets, (ok, first, arrived) in teams:
        inside = T.min_start_distance(states) < cfg["d_min"]
        assert inside == (first is not None), name
        traj = np.repeat(states[:, None, :], samples, axis=1)
        got_ok, span, got_first = metrics.instance_success(traj, targets, goal_radius, list(shape_half), "box")
        assert (got_ok, got_first) == (ok, first), name
        reached = bool(np.all(metrics.reach_goal_area(states[:, :2], targets[:, :2], goal_radius)))
        assert reached == arrived, name
        if ok:
            assert span == (0 if arrived else samples), name
