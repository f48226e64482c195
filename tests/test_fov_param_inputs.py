"""CPU: the inputs of the FoV IMPC tests off the base field of view (tests/fov_param_cases.py), no GPU.

Every case the GPU tests solve is held here on the oracle alone: statuses, how many agents' optima
the FoV rows shape (liveness), the row counts at the capacity edges, the decision margins of the
feasibility edge and which slack-in-use curves are stable enough to compare. The committed numbers
(fov_param_cases.PINS and the constants next to the cases) are asserted to be what the code
computes, so a changed input cannot silently empty a case."""
import math

import numpy as np
import pytest

import fov_param_cases as P
import oracle_lib as O
from mpccbf import swarm


def test_effective_cone():
    d = P.DEG
    for beta, half in ((40 * d, 20 * d), (math.pi, math.pi / 2), (181 * d, 89.5 * d), (240 * d, 60 * d),
                       (300 * d, 30 * d), (2 * math.pi, math.pi)):
        assert abs(P.effective_half_angle(beta) - half) < 1e-12
    # up to pi the lists are swarm.fov_csr's; above, a neighbour in the field of view but outside
    # the effective cone is not listed
    states, _ = P.swarm_states()
    for beta in (60 * d, 120 * d, math.pi):
        a, b = P.visible_csr(states, 8, 6.0, beta), swarm.fov_csr(states, 8, 6.0, beta)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = P.visible_csr(states, 8, 6.0, 240 * d), swarm.fov_csr(states, 8, 6.0, 240 * d)
    assert a[0][-1] < b[0][-1]


def test_a_neighbour_in_view_but_outside_the_effective_cone_is_infeasible(oracle):
    """The reason for visible_csr: above pi, a neighbour at bearing fov_beta / 2 - 0.15 is inside the
    field of view and INFEASIBLE in plain mode."""
    for beta in (240 * P.DEG, 300 * P.DEG):
        b = 0.5 * beta - 0.15
        nb = np.zeros((1, 6))
        nb[0, :2] = [3.0 * math.cos(b), 3.0 * math.sin(b)]
        c = P.batch([(np.zeros(6), np.array([2.0, 0.0, 0.0]), nb)])
        st, _, _ = P.oracle_case(P.config("plain", fov_beta=beta), c)
        assert st[0, 0] == O.INFEASIBLE, (beta, st)


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.SWARM_CONFIGS))
def test_swarm_cases_are_optimal_and_live(oracle, name, setting):
    cfg = P.config(setting, **P.SWARM_CONFIGS[name])
    c = P.swarm_case(name)
    st, ob, _ = P.oracle_case(cfg, c)
    assert np.all(st == O.OPTIMAL), np.argwhere(st != O.OPTIMAL)
    assert np.nanmax(np.abs(ob)) < 1e4  # (the suite's rule applies to every agent)
    live = P.liveness(cfg, c, ob)
    print(name, setting, "live", live, "neighbours", np.diff(c["rp"]).max())
    assert live == P.PINS["swarm_live"][name]
    if name not in ("b360", "bbox"):
        assert len(live) >= 4
    assert int(np.diff(c["rp"]).max()) == P.PINS["swarm_max_nb"][name]
    if "fov_beta" in P.SWARM_CONFIGS[name] and cfg["fov_beta"] <= math.pi:
        ang, rad = P.cone_margin(c, cfg["fov_beta"], cfg["fov_Rs"])
        assert ang >= 1e-9 and rad >= 1e-9


def test_some_swarm_agents_see_five_or_more():
    assert sum(P.PINS["swarm_max_nb"][n] >= 5 for n in P.SWARM_CONFIGS) >= 6
    assert max(P.PINS["swarm_max_nb"].values()) == 8


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.FAN_BETAS))
def test_fans_are_optimal(oracle, name, setting):
    cfg = P.config(setting, fov_beta=P.FAN_BETAS[name])
    c = P.fan_batch(name, setting)
    assert c["agent_first"] > 0 and c["num_agents"] == 2 * len(P.FAN_KS[setting])
    assert np.diff(c["rp"]).tolist() == [k for k in P.FAN_KS[setting] for _ in P.TURNS]
    st, ob, _ = P.oracle_case(cfg, c)
    assert np.all(st == O.OPTIMAL), st
    assert np.nanmax(np.abs(ob)) < 1e4
    live = P.liveness(cfg, c, ob)
    print(name, setting, live)
    assert live == P.PINS["fan_live"][f"{name}/{setting}"]
    # a border row binds on some fan of every field of view with borders; at 2 pi none does (the
    # ring fans below cover it)
    assert (len(live) > 0) == (name != "b360")
    over = P.fan_batch(name, setting, over_cap=True)
    assert int(np.diff(over["rp"])[-1]) == P.NB_CAP[setting] + 1 == P.FAN_OVER_CAP[setting]


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.RING_CONFIGS))
def test_full_circle_fans_are_optimal(oracle, name, setting):
    cfg = P.ring_config(name, setting)
    c = P.ring_batch(name)
    st, ob, _ = P.oracle_case(cfg, c)
    assert np.all(st == O.OPTIMAL), st
    live = P.liveness(cfg, c, ob)
    assert live == P.PINS["ring_live"][name]


def test_range_and_safety_rows_bind_at_the_full_circle(oracle):
    """Directly: the range row (kind 3) resp. the safety row (kind 0) of neighbour 0 holds with
    equality at the oracle's iteration-1 solution of every 2 pi fan, at sample 1. (At Ds 0.5 the
    liveness count is empty although the row binds: at rest the safety row of the FoV-free
    comparison, Ds 1e-3, stops the observer just the same.)"""
    for name in P.RING_CONFIGS:
        cfg, c = P.ring_config(name, "plain"), P.ring_batch(name)
        for i in range(c["num_agents"]):
            assert P.binding_fov_rows(cfg, c, i) == P.PINS["ring_binding"][name], (name, i)
        assert P.PINS["ring_binding"][name] == [(3 if name == "range" else 0, 1)]
    assert P.PINS["ring_live"]["range"] == [0, 1, 2]
    assert sum(len(P.PINS["ring_live"][n]) > 0 for n in P.RING_CONFIGS if n.startswith("safety")) >= 2


@pytest.mark.parametrize("name", list(P.ROW_CAP))
def test_row_capacity_edges(oracle, mpclib, name):
    """m + 4 n Voronoi rows + every FoV row (4 kinds, 2 at 2 pi, times the samples): the committed
    neighbour counts are the two sides of 192 in iteration 1, and the oracle solves both."""
    over, opts, (fits, too_many) = P.ROW_CAP[name]
    assert opts == dict(no_cbf_filter=True) and too_many == fits + 1
    cfg = P.config("plain", **over)
    m = P.shared_rows(cfg)
    kinds = 2 if P.is_full_circle(cfg["fov_beta"]) else 4
    for n in (fits, too_many):
        c = P.cap_fan(n, cfg["fov_beta"])
        st, _, xs = P.oracle_case(cfg, c)
        assert np.all(st == O.OPTIMAL)
        rows = P.image_rows(cfg, c, 0, xs[0, 0], cbf_filter=False)
        assert rows == [m + 4 * n + kinds * n, m + 4 * n + kinds * cfg["cbf_horizon"] * n]
        assert rows == P.PINS["cap_rows"][name][str(n)]
        assert rows[0] <= P.WROWS and (rows[1] <= P.WROWS) == (n == fits)
    if name == "h2":
        assert m + 12 * fits == P.WROWS  # (the exact edge)


def test_row_capacity_with_the_filter(oracle, mpclib):
    over, n = P.FILTERED_CAP
    cfg = P.config("plain", **over)
    c = P.cap_fan(n, cfg["fov_beta"])
    st, _, xs = P.oracle_case(cfg, c)
    assert np.all(st == O.OPTIMAL)
    rows = P.image_rows(cfg, c, 0, xs[0, 0])
    assert rows == list(P.FILTERED_ROWS) and P.WROWS - 8 <= rows[1] <= P.WROWS
    # the filter decides: without it the same fan is far over the capacity
    assert P.image_rows(cfg, c, 0, xs[0, 0], cbf_filter=False)[1] > P.WROWS


def test_slack_capacity_figures(mpclib):
    """round16(m + 4 n) + 80 against 192: at m = 72 eight neighbours (the cap) land on it exactly;
    with keep_redundant m is so large that no neighbour count fits, not even none."""
    cfg = P.config("slack")
    assert P.shared_rows(cfg) == P.PINS["shared_rows"]["reduced"]
    assert P.shared_rows(cfg, keep_redundant=True) == P.PINS["shared_rows"]["kept"]
    assert P.slack_image_rows(cfg, 8) == P.WROWS
    # (the neighbour cap of 8 comes first: the rows would run out at 11 neighbours)
    assert min(n for n in range(32) if P.slack_image_rows(cfg, n) > P.WROWS) == 11 > P.NB_CAP["slack"]
    assert all(P.slack_image_rows(cfg, n, keep_redundant=True) > P.WROWS for n in range(0, 9))


def test_feasibility_edge(oracle):
    """Plain mode: OPTIMAL up to SWEEP_LAST_OPTIMAL degrees, INFEASIBLE from the next x on, and
    neither status at the edge changes when every inequality bound moves by +-SHIFT relative. Slack
    mode: OPTIMAL at every x, the plain objective while plain mode is feasible."""
    plain, slack = P.config("plain"), P.config("slack")
    for x in P.SWEEP_X:
        c = P.sweep_case(x)
        st, ob, _ = P.oracle_case(plain, c)
        want = [O.OPTIMAL, O.OPTIMAL] if x <= P.SWEEP_LAST_OPTIMAL else [O.INFEASIBLE, O.UNKNOWN]
        assert st[0].tolist() == want, (x, st)
        ss, so, _ = P.oracle_case(slack, c)
        assert ss[0].tolist() == [O.OPTIMAL, O.OPTIMAL], (x, ss)
        if x <= P.SWEEP_LAST_OPTIMAL:
            assert np.all(np.abs(so - ob) <= 1e-8 * np.abs(ob))
        else:
            assert so[0, 1] >= 1e4
    edge = [x for x in P.SWEEP_X if x > P.SWEEP_LAST_OPTIMAL][0]
    for x in (P.SWEEP_LAST_OPTIMAL, edge):
        c = P.sweep_case(x)
        base = P.python_impc(plain, c)["status"].tolist()
        assert base == P.oracle_case(plain, c)[0][0].tolist()  # (the Python loop is the oracle's)
        for sh in (P.SHIFT, -P.SHIFT):
            assert P.python_impc(plain, c, shift=sh)["status"].tolist() == base, (x, sh)


def _curve_move(cfg, c):
    base, up, dn = (P.python_impc(cfg, c, shift=sh) for sh in (0.0, P.SHIFT, -P.SHIFT))
    assert all(r["status"].tolist() == [O.OPTIMAL, O.OPTIMAL] for r in (base, up, dn))
    nc = cfg["num_pieces"] * 3 * cfg["num_control_points"]
    return max(float(np.max(np.abs(r["x"][it][:nc] - base["x"][it][:nc]))) for r in (up, dn) for it in range(2))


def test_slack_in_use_curves_are_compared_where_stable(oracle):
    """Slack in use at large objectives (the sweep from 20 degrees on at decay 0.9, 45 degrees at both
    decay rates): the curve is compared where the oracle's own curve moves less than 1e-6 under
    +-SHIFT, SWEEP_CURVES pins which; at most a quarter of these cases may fall out of the curve
    comparison. (The criterion passes and fails by a few per cent, see SWEEP_CURVES.)"""
    in_use = [(x, "slack") for x in P.SWEEP_X if x > P.SWEEP_LAST_OPTIMAL] + [(P.SWEEP_FAR, "slack"), (P.SWEEP_FAR, "slack01")]
    assert in_use == list(P.SWEEP_CURVES)
    for x, setting in in_use:
        cfg, c = P.config(setting), P.sweep_case(x)
        assert P.oracle_case(cfg, c)[1][0, 1] >= 1e4
        mv = _curve_move(cfg, c)
        print(x, setting, mv)
        assert (mv < 1e-6) == P.SWEEP_CURVES[(x, setting)], (x, setting, mv)
    out = sum(not v for v in P.SWEEP_CURVES.values())
    assert out == 1 and out <= len(in_use) // 4


def test_penalty_objective_is_the_oracles_objective(oracle):
    """At the oracle's own optimum the penalty objective (slacks at their least feasible values) is
    its objective, and the hard rows hold."""
    cfg = P.config("slack")
    for x in (20, 30):
        c = P.sweep_case(x)
        r = P.python_impc(cfg, c)
        _, ob, xs = P.oracle_case(cfg, c)
        for it in range(2):
            pen, viol = P.penalty_objective(r["qp"][it], xs[0, it], 3)
            assert abs(pen - ob[0, it]) <= 1e-9 * abs(ob[0, it]) and viol <= 1e-9, (x, it, pen, ob, viol)
    # a curve that breaks a hard row shows in the violation
    bad = xs[0, 1].copy()
    bad[0] += 1e-3
    assert P.penalty_objective(r["qp"][1], bad, 3)[1] > 1e-4


def test_slack_order_case(oracle):
    c, covs, (p, q) = P.order_case()
    cfg = P.config("slack01", fov_beta=60.0 * P.DEG)
    me = c["states"][c["agent_first"]]
    d = {k: [O.distance_to_ellipse(me[:2], c["states"][j, :2], covs[k][j]) for j in c["col"]] for k in covs}
    ip, iq = list(c["col"]).index(p), list(c["col"]).index(q)
    assert d["A"][ip] < d["A"][iq] < min(v for j, v in enumerate(d["A"]) if j not in (ip, iq))
    assert d["B"][iq] < d["B"][ip] < min(v for j, v in enumerate(d["B"]) if j not in (ip, iq))
    ob = {}
    for k, cov in (("A", covs["A"]), ("B", covs["B"]), ("none", None)):
        st, o, _ = P.oracle_cov(cfg, c, cov)
        assert st.tolist() == [O.OPTIMAL, O.OPTIMAL]
        ob[k] = o
        assert np.allclose(o, P.PINS["order_obj"][k], rtol=1e-9, atol=0.0)
    assert abs(ob["A"][1] - ob["B"][1]) > 0.01 * abs(ob["A"][1])
    # no covariances: the list order, whose nearest two are in B's order here
    assert ip > iq and np.array_equal(ob["none"], ob["B"])


def test_all_others_lists_are_feasible_and_beyond_the_oracle(oracle):
    """The example's all-others lists on heading_swarm(8) in slack mode: the oracle reports
    INFEASIBLE or UNKNOWN for every robot, yet the same QPs without the FoV rows (box and Voronoi
    rows kept) are OPTIMAL, and a slack QP is feasible whenever those rows are: the oracle's statuses
    are wrong here, and these inputs are outside its reach."""
    c = P.all_others_case()
    assert np.diff(c["rp"]).tolist() == [7] * 8
    for setting in ("slack", "slack01"):
        st, _, _ = P.oracle_case(P.config(setting), c)
        assert st.tolist() == P.PINS["all_others_status"]
        assert not np.any(st == O.OPTIMAL)
    st, _, _ = P.oracle_case(P.config("plain", **P.FREE), c)
    assert np.all(st == O.OPTIMAL)


def test_recorded_all_others_cases_are_the_swarms(oracle):
    """The fixtures of tests/golden/regress_cases.json held by the penalty objective are robots of
    all_others_case (row 0 the ego, then its list), feasible and beyond the oracle as above."""
    c = P.all_others_case()
    recs = P.recorded_cases()
    assert [r["name"] for r, _ in recs] == [f"heading8_all_others_robot{i}" for i in (0, 2, 3, 4, 5, 7)]
    for rec, case in recs:
        i = int(rec["name"][-1])
        rows = [i] + list(c["col"][c["rp"][i]:c["rp"][i + 1]])
        assert np.array_equal(case["states"], c["states"][rows]) and np.array_equal(case["targets"][0], c["targets"][i])
        assert rec["controller"] == "fov_slack" and rec["cov"] is None and rec["device_status"][0] == O.OPTIMAL
        assert all((s == O.OPTIMAL) == (o is not None and o > 1e4) for s, o in zip(rec["device_status"], rec["device_obj"]))
        cfg = P.config("slack", slack_cost=rec["slack_cost"], slack_decay_rate=rec["slack_decay_rate"])
        assert P.oracle_case(cfg, case)[0].tolist() == [P.PINS["all_others_status"][i]]
        assert np.all(P.oracle_case(P.config("plain", **P.FREE), case)[0] == O.OPTIMAL)
