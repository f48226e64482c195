"""GPU: the FoV IMPC kernel (impc_fov_kernel<SLACK>) off the base field of view, on the inputs of
tests/fov_param_cases.py: every fov_border branch, Ds / Rs that bind, the Voronoi shift, the row
capacity (WROWS = 192) from both sides, the neighbour caps, the feasibility edge and the slack order.

The reference is the oracle on the same inputs (statuses equal, objectives within OBJ_TOL relative,
control points within X_TOL: the suite's rule). Where slacks are in use at objectives of 1e4 and
more the objective is judged by the penalty objective (fov_param_cases.penalty_objective): the
device's curve must keep the hard rows to 1e-6, cost no more than OBJ_TOL relative above the
oracle's curve evaluated the same way, and its reported objective must be its own penalty objective
to 1e-6 relative. "Bit for bit" is parity_rule.same_bits. One launch per swarm or fan batch, every
agent compared."""
import functools
import math

import numpy as np
import pytest

import fov_param_cases as P
import oracle_lib as O
from gpu_harness import Solver as _Solver, same_bits, same_values, to_device, to_host
from parity_rule import OBJ_TOL, ROUTE_REL, X_TOL, check_parity

pytestmark = pytest.mark.gpu

OUTS = ("x", "status", "obj", "iters", "next_states", "nb_out")
EST_NAME = {"plain": "impc_fov_kernel<false,true>", "slack": "impc_fov_kernel<true,true>"}
BIG = 1e4           # objectives from here on: the penalty rule
HARD_TOL = 1e-6     # scaled violation of the hard rows (test_gpu_certify.py)
FILTER_TOL = ROUTE_REL  # no_cbf_filter against the filtered solve (the dual-active-set / PDIP bound)


# every solve asserts impc_fov_kernel<SLACK> of the setting
Solver = functools.partial(_Solver, kernel_names=P.KERNEL)


@functools.lru_cache(maxsize=None)
def _oracle(kind, name, setting):
    """The oracle's (status, obj, x) of a named case, computed once per session."""
    if kind == "swarm":
        return P.oracle_case(P.config(setting, **P.SWARM_CONFIGS[name]), P.swarm_case(name))
    if kind == "fans":
        return P.oracle_case(P.config(setting, fov_beta=P.FAN_BETAS[name]), P.fan_batch(name, setting))
    if kind == "ring":
        return P.oracle_case(P.ring_config(name, setting), P.ring_batch(name))
    raise KeyError(kind)


def _assert_matches_oracle(out, ref, what):
    """The suite's rule on every agent: statuses, objectives of OPTIMAL iterations, the curve of
    the last OPTIMAL iteration."""
    g = to_host(out)
    check_parity(g, ref, label=what)
    return g


# ---- swarm cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.SWARM_CONFIGS))
def test_swarm_matches_oracle(mpclib, oracle, name, setting):
    """33 agents at every field of view, Ds / Rs and box of SWARM_CONFIGS, lists by the reference's
    cone. For fov_beta <= pi the grid query (knn_k 8, radius Rs) finds the same lists and gives the
    CSR solve bit for bit."""
    cfg = P.config(setting, **P.SWARM_CONFIGS[name])
    c = P.swarm_case(name)
    s = Solver(mpclib, cfg, c)
    out = s.solve()
    assert s.ctx.kernel_name == P.KERNEL[setting]
    _assert_matches_oracle(out, _oracle("swarm", name, setting), f"swarm/{name}/{setting}")
    nb = out["nb_out"].cpu().numpy()
    for a in range(33):
        lst = c["col"][c["rp"][a]:c["rp"][a + 1]]
        assert list(nb[a, :len(lst)]) == list(lst) and np.all(nb[a, len(lst):] == -1)
    if cfg["fov_beta"] <= math.pi:
        ang, rad = P.cone_margin(c, cfg["fov_beta"], cfg["fov_Rs"])
        assert ang >= 1e-9 and rad >= 1e-9  # (test_gpu_exact_geometry: no pair on a decision boundary)
        same_bits(s.solve(grid=True), out, keys=OUTS, what=f"grid/{name}/{setting}")


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", [n for n, o in P.SWARM_CONFIGS.items() if "fov_beta" in o])
def test_no_cbf_filter_changes_no_result(mpclib, name, setting):
    """Metamorphic, at every fov_beta: every FoV row staged (8 neighbours x 4 kinds x 2 samples fit
    the image next to 72 box and 32 Voronoi rows) against the filtered solve — statuses equal,
    objectives within FILTER_TOL relative."""
    cfg = P.config(setting, **P.SWARM_CONFIGS[name])
    c = P.swarm_case(name)
    a = to_host(Solver(mpclib, cfg, c).solve())
    b = to_host(Solver(mpclib, cfg, c, no_cbf_filter=True).solve())
    assert np.array_equal(a["status"], b["status"]), (a["status"], b["status"])
    assert int((a["status"] == O.OPTIMAL).sum()) == 66
    err = np.abs(a["obj"] - b["obj"]) / np.maximum(1.0, np.abs(a["obj"]))
    print(f"no_cbf_filter/{name}/{setting}: largest objective difference {err.max():.3e} (relative), "
          f"largest |dx| {np.abs(a['x'] - b['x']).max():.3e}")
    assert err.max() <= FILTER_TOL, (name, setting, err.max())


# ---- fan cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.FAN_BETAS))
def test_fans_match_oracle_and_one_over_the_cap_is_error(mpclib, oracle, name, setting):
    """Fans of 1 .. 16 (slack mode: 1 .. 8) neighbours placed by the effective cone, two targets
    each, one batch with agent_first > 0; a fan of one neighbour more than the cap in the same
    batch reports ERROR, then UNKNOWN for the stopped IMPC, and leaves every other observer's
    outputs as they are without it."""
    cfg = P.config(setting, fov_beta=P.FAN_BETAS[name])
    c = P.fan_batch(name, setting)
    s = Solver(mpclib, cfg, c)
    out = s.solve()
    assert s.ctx.kernel_name == P.KERNEL[setting] and c["agent_first"] > 0
    _assert_matches_oracle(out, _oracle("fans", name, setting), f"fans/{name}/{setting}")
    over = Solver(mpclib, cfg, P.fan_batch(name, setting, over_cap=True)).solve()
    n = c["num_agents"]
    print("over the cap:", over["status"][n].tolist())
    assert over["status"][n].tolist() == [O.ERROR, O.UNKNOWN]
    assert bool(s.torch.isnan(over["x"][n]).all()) and bool(s.torch.isnan(over["obj"][n]).all())
    for k in ("x", "status", "obj", "iters", "next_states"):
        same_values(over[k][:n], out[k], what=k)


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", ["b60", "b360"])
def test_fans_in_the_estimate_form(mpclib, name, setting):
    """True positions attached through set_fov_estimates: the estimate form of the kernel gives the
    unattached solve bit for bit at the narrow and at the full-circle field of view."""
    cfg = P.config(setting, fov_beta=P.FAN_BETAS[name])
    c = P.fan_batch(name, setting)
    s = Solver(mpclib, cfg, c)
    plain = s.solve()
    assert s.ctx.kernel_name == P.KERNEL[setting]
    nb_xy = to_device(c["states"][c["col"], :2])
    s.ctx.set_fov_estimates(nb_xy, None)
    est = s.solve(kernel=EST_NAME[setting])
    assert s.ctx.kernel_name == EST_NAME[setting]
    same_bits(est, plain, keys=OUTS, what=f"estimates/{name}/{setting}")
    assert int((plain["status"] == O.OPTIMAL).sum()) == 2 * c["num_agents"]


@pytest.mark.parametrize("setting", ["plain", "slack"])
@pytest.mark.parametrize("name", list(P.RING_CONFIGS))
def test_full_circle_fans_match_oracle(mpclib, oracle, name, setting):
    """fov_beta = 2 pi (no border rows): a neighbour at Rs - 0.1 with the target away from it (the
    range row binds), one at Ds + 0.3 with the target beyond it (the safety row; Ds 0.5, 1, 2)."""
    s = Solver(mpclib, P.ring_config(name, setting), P.ring_batch(name))
    out = s.solve()
    assert s.ctx.kernel_name == P.KERNEL[setting]
    _assert_matches_oracle(out, _oracle("ring", name, setting), f"ring/{name}/{setting}")


# ---- row caps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.ROW_CAP))
def test_row_capacity_edge_without_the_filter(mpclib, oracle, name):
    """no_cbf_filter: every FoV row enters the image. The largest fan whose iteration-1 image fits
    192 rows is OPTIMAL in both iterations, as on the oracle (which has no capacity); one neighbour
    more fits in iteration 0 (one sample) and reports ERROR in iteration 1."""
    over, opts, (fits, too_many) = P.ROW_CAP[name]
    cfg = P.config("plain", **over)
    c = P.cap_fan(fits, cfg["fov_beta"])
    ref = P.oracle_case(cfg, c)
    assert P.image_rows(cfg, c, 0, ref[2][0, 0], cbf_filter=False)[1] <= P.WROWS
    s = Solver(mpclib, cfg, c, **opts)
    _assert_matches_oracle(s.solve(), ref, f"rowcap/{name}/{fits}")
    assert s.ctx.kernel_name == P.KERNEL["plain"]
    c = P.cap_fan(too_many, cfg["fov_beta"])
    ref = P.oracle_case(cfg, c)
    rows = P.image_rows(cfg, c, 0, ref[2][0, 0], cbf_filter=False)
    assert rows[0] <= P.WROWS < rows[1] and np.all(ref[0] == O.OPTIMAL)
    out = to_host(Solver(mpclib, cfg, c, **opts).solve())
    print(f"rowcap/{name}/{too_many}: rows {rows}, status {out['status'][0]}")
    assert out["status"][0].tolist() == [O.OPTIMAL, O.ERROR]
    assert abs(out["obj"][0, 0] - ref[1][0, 0]) <= OBJ_TOL * max(1.0, abs(ref[1][0, 0])) and np.isnan(out["obj"][0, 1])
    # (the iteration-0 curve is kept)
    assert np.max(np.abs(out["x"][0] - ref[2][0, 0])) <= X_TOL
    if name == "h2":
        # a third iteration after the ERROR: the IMPC has stopped, UNKNOWN with no objective
        out = to_host(Solver(mpclib, dict(cfg, impc_iter=3), c, **opts).solve())
        assert out["status"][0].tolist() == [O.OPTIMAL, O.ERROR, O.UNKNOWN] and np.all(np.isnan(out["obj"][0, 1:]))
        assert np.max(np.abs(out["x"][0] - ref[2][0, 0])) <= X_TOL


def test_row_capacity_with_the_filter(mpclib, oracle):
    """The filter on: by the numpy restatement of the kernel's decision 16 neighbours at 60 degrees,
    cbf_horizon 4 keep FILTERED_ROWS rows, within 8 of the capacity. The kernel reports no row
    count, so the device side shows only that this image is solved as on the oracle — neither ERROR
    (rows kept that the restatement drops) nor another optimum (rows dropped that matter)."""
    over, fits = P.FILTERED_CAP
    cfg = P.config("plain", **over)
    c = P.cap_fan(fits, cfg["fov_beta"])
    ref = P.oracle_case(cfg, c)
    rows = P.image_rows(cfg, c, 0, ref[2][0, 0])
    assert rows == list(P.FILTERED_ROWS) and P.WROWS - 8 <= rows[1] <= P.WROWS
    _assert_matches_oracle(Solver(mpclib, cfg, c).solve(), ref, "rowcap/filtered")


def test_slack_mode_with_every_box_row_has_no_room(mpclib):
    """keep_redundant in slack mode: 117 box rows and one neighbour's 4 Voronoi rows round up to
    128, and 128 + 80 > 192: ERROR whatever the neighbour count (include/mpccbf.h). Without
    keep_redundant the same fan is solved."""
    cfg = P.config("slack")
    c = P.cap_fan(1)
    assert P.slack_image_rows(cfg, 1, keep_redundant=True) > P.WROWS >= P.slack_image_rows(cfg, 8)
    out = to_host(Solver(mpclib, cfg, c, keep_redundant=True).solve())
    assert out["status"][0].tolist() == [O.ERROR, O.UNKNOWN]
    out = to_host(Solver(mpclib, cfg, c).solve())
    assert out["status"][0].tolist() == [O.OPTIMAL, O.OPTIMAL]


# ---- feasibility edge, slack in use --------------------------------------------------------------
def _device_penalty(mpclib, cfg, case, cov=None):
    """Every observer of a slack-mode case on the device, with the penalty objective of its own
    curves: per observer and iteration (status, reported objective, penalty objective, hard-row
    violation, the QP), and the curves. The iteration-1 QP is assembled at the device's own
    iteration-0 curve, which a context with impc_iter 1 returns (its solve is iteration 0 of the
    two-iteration solve, bit for bit)."""
    one = to_host(Solver(mpclib, dict(cfg, impc_iter=1), case).solve(cov=cov))
    two = to_host(Solver(mpclib, cfg, case).solve(cov=cov))
    assert np.array_equal(one["status"][:, 0], two["status"][:, 0])
    assert np.array_equal(one["obj"][:, 0], two["obj"][:, 0], equal_nan=True)
    p = O.make_params(cfg)
    res = []
    for i in range(case["num_agents"]):
        lst = case["col"][case["rp"][i]:case["rp"][i + 1]]
        me, nbs = case["states"][case["agent_first"] + i], case["states"][lst]
        sw = P.slack_weights_cov(cfg, case, cov, i)
        per, pred = [], None
        for it, g in ((0, one), (1, two)):
            if two["status"][i, it] != O.OPTIMAL:
                per.append((int(two["status"][i, it]), np.nan, np.nan, np.nan, None))
                continue
            qp = O.assemble_qp(p, me, case["refs"][i], nbs, it, pred, slack_w=sw)
            pen, viol = P.penalty_objective(qp, g["x"][i], len(lst))
            per.append((O.OPTIMAL, float(two["obj"][i, it]), pen, viol, qp))
            pred = np.array([np.concatenate([O.eval_curve(p, g["x"][i], cfg["h"] * k, 0),
                                             O.eval_curve(p, g["x"][i], cfg["h"] * k, 1)]) for k in range(cfg["cbf_horizon"])])
        res.append(per)
    return res, one["x"], two["x"]


def _penalty_check(mpclib, cfg, case, cov, ref_x, what, compare_x):
    """One observer in slack mode by the penalty rule. ref_x: the oracle's curves per iteration."""
    nnb = int(case["rp"][1] - case["rp"][0])
    res, x0, x1 = _device_penalty(mpclib, cfg, case, cov)
    for it, xd in ((0, x0[0]), (1, x1[0])):
        st, od, pen_d, viol_d, qp = res[0][it]
        assert st == O.OPTIMAL, (what, it, st)
        pen_r, viol_r = P.penalty_objective(qp, ref_x[it], nnb)
        print(f"{what} it {it}: device obj {od:.10e} penalty {pen_d:.10e} hard {viol_d:.2e}; oracle curve penalty "
              f"{pen_r:.10e} hard {viol_r:.2e}; |dx| {np.max(np.abs(xd - ref_x[it])):.2e}")
        assert viol_d <= HARD_TOL, (what, it, viol_d)
        assert pen_d <= pen_r + OBJ_TOL * max(1.0, abs(pen_r)), (what, it, pen_d, pen_r)
        assert abs(od - pen_d) <= 1e-6 * max(1.0, abs(pen_d)), (what, it, od, pen_d)
    if compare_x:
        assert np.max(np.abs(x1[0] - ref_x[1])) <= X_TOL, what


@pytest.mark.parametrize("setting", ["plain", "slack"])
def test_neighbours_outside_the_cone(mpclib, oracle, setting):
    """The sweep: two neighbours x and x / 2 degrees outside the borders. Plain mode follows the
    oracle from OPTIMAL (up to 16 degrees) to INFEASIBLE (from 20); slack mode is OPTIMAL
    throughout, by the suite's rule below 1e4 and by the penalty rule above."""
    cfg = P.config(setting)
    for x in P.SWEEP_X:
        c = P.sweep_case(x)
        ref = P.oracle_case(cfg, c)
        if setting == "slack" and ref[1][0, 1] >= BIG:
            assert np.all(ref[0] == O.OPTIMAL)
            _penalty_check(mpclib, cfg, c, None, ref[2][0], f"sweep/{x}/{setting}", P.SWEEP_CURVES[(x, setting)])
        else:
            g = _assert_matches_oracle(Solver(mpclib, cfg, c).solve(), ref, f"sweep/{x}/{setting}")
            print(f"sweep/{x}/{setting}: status {g['status'][0]}")
        if setting == "plain":
            assert ref[0][0, 0] == (O.OPTIMAL if x <= P.SWEEP_LAST_OPTIMAL else O.INFEASIBLE)


def test_slack_order_follows_the_covariances(mpclib, oracle):
    """Decay 0.1: covariance tables A and B swap the two nearest neighbours in the slack order and
    the objectives differ by more than 1 % (pinned on the CPU); no covariances give the list order."""
    c, covs, _ = P.order_case()
    cfg = P.config("slack01", fov_beta=60.0 * P.DEG)
    res = {}
    for k, cov in (("A", covs["A"]), ("B", covs["B"]), ("none", None)):
        st, ob, xs = P.oracle_cov(cfg, c, cov)
        s = Solver(mpclib, cfg, c)
        g = _assert_matches_oracle(s.solve(cov=cov), (st[None], ob[None], xs[None]), f"order/{k}")
        assert s.ctx.kernel_name == P.KERNEL["slack01"]
        res[k] = g["obj"][0, 1]
    assert abs(res["A"] - res["B"]) > 0.01 * abs(res["A"])


# ---- the recorded discrepancy ----------------------------------------------
def test_sweep_at_45_degrees(mpclib, oracle):
    """Both neighbours far outside the cone (objectives of 5e12): the oracle is still OPTIMAL, and
    the device's curves cost no more by the penalty rule, at both decay rates; the curve is compared
    at decay 0.9, where the oracle's own is stable (SWEEP_CURVES)."""
    c = P.sweep_case(P.SWEEP_FAR)
    for setting in ("slack", "slack01"):
        cfg = P.config(setting)
        ref = P.oracle_case(cfg, c)
        assert np.all(ref[0] == O.OPTIMAL) and ref[1][0, 1] > 1e12
        _penalty_check(mpclib, cfg, c, None, ref[2][0], f"sweep/45/{setting}", P.SWEEP_CURVES[(P.SWEEP_FAR, setting)])


def test_all_others_lists_stay_at_their_recorded_solves(mpclib):
    """heading_swarm(8) with the example's all-others lists, slack mode: feasible QPs (OPTIMAL
    without the FoV rows, tests/test_fov_param_inputs.py) that the oracle reports INFEASIBLE or
    UNKNOWN, with objectives of 1e28 .. 1e51. Every iteration recorded as OPTIMAL in
    tests/golden/regress_cases.json stays OPTIMAL, keeps the hard rows to 1e-6, reports its own
    penalty objective to 1e-6 relative and stays at the recorded objective to 1e-6 relative; the
    device never reports such a QP INFEASIBLE."""
    cases = P.recorded_cases()
    assert len(cases) == 6
    for rec, c in cases:
        cfg = P.config("slack", slack_cost=rec["slack_cost"], slack_decay_rate=rec["slack_decay_rate"])
        res, _, _ = _device_penalty(mpclib, cfg, c)
        for it, (st, od, pen, viol, _) in enumerate(res[0]):
            print(f"{rec['name']} it {it}: status {st} obj {od!r} penalty {pen!r} hard {viol:.3e}")
            assert st != O.INFEASIBLE
            if rec["device_status"][it] != O.OPTIMAL:
                continue
            assert st == O.OPTIMAL and viol <= HARD_TOL, (rec["name"], it, st, viol)
            assert abs(od - pen) <= 1e-6 * abs(pen), (rec["name"], it, od, pen)
            assert abs(od - rec["device_obj"][it]) <= 1e-6 * abs(rec["device_obj"][it]), (rec["name"], it, od)
