"""CPU: the inputs of the formation-rollout parity test (tests/formation_rollout_cases.py) pinned
with the oracle alone. The GPU test compares every decision of a run with the oracle on the table
that decision planned from; that is only a fair test where the oracle's own answer does not hang on
the last digits of the table. Here the example's loop runs on the CPU for the test's instances,
both slack modes and the test's noise, and every decision is repeated on 8 perturbed copies of its
table (1e-7, far above the 1e-12 the GPU's next state may differ by): no status and no branch
(lambda2 > 0.1) may change. The run must also hold what the GPU test is there to see: OPTIMAL and
INFEASIBLE decisions, both branches and the zero-control fallback."""
import numpy as np

import formation_rollout_cases as F
import oracle_lib as O

PERTURB = 1e-7
DRAWS = 8


def test_parity_batch_is_what_the_issue_names():
    sizes = {g_name: len(st) for slack in (False, True) for g in F.parity_groups(slack) for g_name, st, _ in g["teams"]}
    assert sizes == {"2r/line": 2, "3r/bend": 3, "3r/line2": 3, "3r/triangle": 3, "5r/circle": 5, "6r/upward": 6,
                     "3r/line3": 8, "8r/circle2": 8}
    for slack in (False, True):
        groups = F.parity_groups(slack)
        assert sorted(n for g in groups for n in g["names"]) == sorted(F.PARITY_NAMES)
        for g in groups:
            assert g["cfg"]["control_slack_mode"] == int(slack)
            assert (g["pos_std"], g["vel_std"], g["cfg"]["Ts"]) == (0.001, 0.01, 0.01)
            assert g["shape_half"] == (0.2, 0.2)
    # one launch takes one parameter set: the instances' own parameters fall into three
    for slack in (False, True):
        groups = F.parity_groups(slack)
        assert [g["names"] for g in groups] == [["2r/line", "3r/bend", "3r/line2", "3r/triangle", "5r/circle", "6r/upward"],
                                                ["3r/line3"], ["8r/circle2"]]
        assert [(g["cfg"]["d_min"], g["cfg"]["d_max"], g["cfg"]["slack_cost"], g["cfg"]["v_max"][0]) for g in groups] == \
            [(0.8, 3.0, 1e5, 1.0), (2.0, 8.0, 1e6, 1.0), (2.0, 8.0, 1e5, 2.0)]


def test_oracle_decisions_do_not_hang_on_the_last_digits():
    rng = np.random.default_rng(5)
    seen = {}
    decisions = flips = 0
    for slack in (False, True):
        for g in F.parity_groups(slack):
            for name, states, targets in g["teams"]:
                run = F.oracle_free_run(g["cfg"], states, targets, F.PARITY_SEED, F.PARITY_STEPS, g["cfg"]["Ts"],
                                        g["pos_std"], g["vel_std"])
                n = len(states)
                for s in range(F.PARITY_STEPS):
                    for i in range(n):
                        tab = run["tables"][s][i]
                        st, l2 = int(run["status"][s, i]), float(run["lambda2"][s, i])
                        decisions += 1
                        for _ in range(DRAWS):
                            pt = tab + PERTURB * rng.standard_normal(tab.shape)
                            pst, _, _, pl2 = O.connectivity_control(g["cfg"], pt, i, F.desired_control(pt[i], targets[i]))
                            flips += int(pst != st) + int((pl2 > F.L2_SWITCH) != (l2 > F.L2_SWITCH))
                stat = run["status"]
                seen[(name, slack)] = dict(
                    optimal=bool(np.any(stat == O.OPTIMAL)), infeasible=bool(np.any(stat == O.INFEASIBLE)),
                    conn=bool(np.any(run["lambda2"] > F.L2_SWITCH)), clf=bool(np.any(run["lambda2"] <= F.L2_SWITCH)),
                    fallback=bool(np.any((stat != O.OPTIMAL) & np.all(run["cbf_u"] == 0.0, axis=-1))))
    assert decisions == 2 * 38 * F.PARITY_STEPS
    assert flips == 0, f"{flips} status / branch changes under {PERTURB} perturbations of {decisions} decisions"
    for key in ("optimal", "infeasible", "conn", "clf", "fallback"):
        assert any(v[key] for v in seen.values()), key
    # where it is: 6r/upward solves on the connectivity row; 3r/triangle (its robots beyond d_max of each
    # other: lambda2 = 0, CLF rows) is INFEASIBLE at every decision without slack, so the example falls
    # back to zero control there, and OPTIMAL on the same rows with slack
    a, b, c = seen[("6r/upward", False)], seen[("3r/triangle", True)], seen[("3r/triangle", False)]
    assert a["optimal"] and a["conn"] and not a["clf"]
    assert b["optimal"] and b["clf"] and not b["conn"]
    assert c["infeasible"] and c["fallback"] and c["clf"] and not c["optimal"]


def test_edge_teams_do_not_hang_on_the_last_digits_either():
    """The seeded teams of the shape-edge tests (sizes 1, 2, 15, 16 and the batch sizes' 3, 4, 5, 8),
    two steps, both modes: the same count, and what they add to the parity batch — teams at the row
    capacity on the CLF rows, INFEASIBLE without slack and OPTIMAL with it."""
    rng = np.random.default_rng(6)
    sizes = [1, 2, 15, 16, 3, 4, 5, 8]
    flips = 0
    for slack in (False, True):
        cfg = F.edge_cfg(slack)
        states, targets, team_ptr, seeds = F.edge_batch(sizes)
        for t, n in enumerate(sizes):
            r = slice(int(team_ptr[t]), int(team_ptr[t + 1]))
            run = F.oracle_free_run(cfg, states[r], targets[r], seeds[t], 2, cfg["Ts"], **F.EDGE_NOISE)
            for s in range(2):
                for i in range(n):
                    tab = run["tables"][s][i]
                    for _ in range(DRAWS):
                        pt = tab + PERTURB * rng.standard_normal(tab.shape)
                        pst, _, _, pl2 = O.connectivity_control(cfg, pt, i, F.desired_control(pt[i], targets[r][i]))
                        flips += int(pst != run["status"][s, i])
                        flips += int((pl2 > F.L2_SWITCH) != (run["lambda2"][s, i] > F.L2_SWITCH))
            if n >= 15:
                assert np.all(run["lambda2"] <= F.L2_SWITCH)
                assert np.all(run["status"] == (O.OPTIMAL if slack else O.INFEASIBLE))
    assert flips == 0


def test_dense_teams_are_at_capacity_on_the_connectivity_row():
    """The lattice teams of 15 and 16 robots: every decision OPTIMAL on the lambda2 row (the sum over a
    full 16-lane group), in both modes, and none hangs on the last digits."""
    rng = np.random.default_rng(7)
    flips = 0
    for slack in (False, True):
        cfg = F.edge_cfg(slack)
        states, targets, team_ptr, seeds = F.dense_batch()
        for t, n in enumerate(F.DENSE_SIZES):
            r = slice(int(team_ptr[t]), int(team_ptr[t + 1]))
            run = F.oracle_free_run(cfg, states[r], targets[r], seeds[t], 2, cfg["Ts"], **F.EDGE_NOISE)
            assert np.all(run["lambda2"] > 1.0) and np.all(run["status"] == O.OPTIMAL)
            for s in range(2):
                for i in range(n):
                    tab = run["tables"][s][i]
                    for _ in range(DRAWS):
                        pt = tab + PERTURB * rng.standard_normal(tab.shape)
                        pst, _, _, pl2 = O.connectivity_control(cfg, pt, i, F.desired_control(pt[i], targets[r][i]))
                        flips += int(pst != run["status"][s, i]) + int(pl2 <= F.L2_SWITCH)
    assert flips == 0
