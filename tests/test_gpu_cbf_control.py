"""GPU: the two CBF-only controller kernels (mpccbf_fov_control_solve: kernels/cbf_control.hip;
mpccbf_connectivity_control_solve: kernels/connectivity_control.hip) on the hand-built cases of
cbf_control_cases.py, against references that are not a PDIP: the exact projection (every active
set of 0 .. 3 rows) in plain mode, the penalty objective in slack mode; statuses against the
oracle's. Row capacity (13 / 14 neighbours, 16 / 17 in slack mode, teams of 16 / 17), batch tails
(1, 15, 17, 33 agents, an ERROR agent among solvable ones), the fov_border branches, the slack
weights' order, optional outputs, guard rows, empty / single / disconnected / symmetric teams."""
import numpy as np
import pytest

import cbf_control_cases as Cs
import oracle_lib as O
from gpu_harness import require_gpu, to_device

pytestmark = pytest.mark.gpu

POISON = -12345.678
LEGAL = (O.OPTIMAL, O.INFEASIBLE, O.UNKNOWN)


def _fov_solve(torch, mpclib, cfg, agents, outputs=True, use_cov=True):
    """One launch over `agents`; every output has a poisoned guard row past the end. Returns dict
    u / status / obj / iters (numpy, without the guard) after checking the guards."""
    dev = torch.device("cuda", 0)
    states, desired, rp, nb, cov = Cs.fov_batch(agents)
    n = len(agents)
    t = lambda v, dt=torch.float64: to_device(v, dt)  # noqa: E731
    u = torch.full((n + 1, 3), POISON, dtype=torch.float64, device=dev)
    status = torch.full((n + 1,), -77, dtype=torch.int32, device=dev)
    obj = torch.full((n + 1,), POISON, dtype=torch.float64, device=dev)
    iters = torch.full((n + 1,), -77, dtype=torch.int32, device=dev)
    kw = dict(status=status[:n], obj=obj[:n], iters=iters[:n]) if outputs else {}
    if use_cov and cfg.get("control_slack_mode"):
        kw["nb_cov"] = t(cov if len(cov) else np.zeros((1, 3)))
    mpclib.fov_control_solve(cfg, t(states), t(desired), t(rp, torch.int32), t(nb if len(nb) else np.zeros((1, 2))),
                             u[:n], **kw)
    torch.cuda.synchronize()
    out = dict(u=u.cpu().numpy(), status=status.cpu().numpy(), obj=obj.cpu().numpy(), iters=iters.cpu().numpy())
    assert np.all(out["u"][n] == POISON) and out["status"][n] == -77 and out["obj"][n] == POISON and out["iters"][n] == -77
    if not outputs:
        assert np.all(out["status"] == -77) and np.all(out["obj"] == POISON) and np.all(out["iters"] == -77)
    return {k: v[:n] for k, v in out.items()}


def _check_plain(name, ref, u, status, obj, iters, worst):
    assert status == ref["status"], (name, status, ref["status"])
    if ref["status"] == O.OPTIMAL:
        assert 1 <= iters <= 60, (name, iters)
        worst["u"] = max(worst["u"], float(np.max(np.abs(u - ref["u"]) / (1.0 + np.abs(ref["u"])))))
        worst["obj"] = max(worst["obj"], abs(obj - ref["obj"]) / max(1.0, abs(ref["obj"])))
        print(f"  {name}: |u - exact| {float(np.max(np.abs(u - ref['u']))):.3e}, objective {obj:.9g} (exact {ref['obj']:.9g}), "
              f"{iters} iterations, active {ref['active']}")
        np.testing.assert_allclose(u, ref["u"], atol=Cs.PLAIN_U_TOL, rtol=Cs.PLAIN_U_TOL, err_msg=name)
        assert abs(obj - ref["obj"]) <= Cs.PLAIN_OBJ_TOL * max(1.0, abs(ref["obj"])), (name, obj, ref["obj"])
    else:
        assert np.all(np.isnan(u)) and np.isnan(obj), (name, u, obj)
        if ref["status"] == O.ERROR:
            assert iters == 0, (name, iters)


def _check_slack(name, ref, u_des, u, status, obj, iters, worst):
    """Slack mode: obj = penalty_objective(u_dev); neither the device's nor the oracle's point is
    better than the other by more than the tolerance; u within the tolerance; hard rows hold."""
    assert status == ref["status"], (name, status, ref["status"])
    if ref["status"] != O.OPTIMAL:
        assert np.all(np.isnan(u)) and np.isnan(obj) and (ref["status"] != O.ERROR or iters == 0), (name, u, obj, iters)
        return
    assert 1 <= iters <= 60, (name, iters)
    pen_dev = Cs.penalty_objective(ref["rows"], ref["weights"], u_des, u)[0]
    pen_ref = ref["obj"]
    tol = Cs.SLACK_OBJ_TOL * max(1.0, abs(pen_ref))
    e_obj = abs(obj - pen_dev) / max(1.0, abs(pen_dev))
    e_u = float(np.max(np.abs(u - ref["u"]) / (1.0 + np.abs(ref["u"]))))
    hard = Cs.hard_excess(ref["rows"], u)
    worst["obj"] = max(worst["obj"], e_obj)
    worst["gap"] = max(worst["gap"], abs(pen_dev - pen_ref) / max(1.0, abs(pen_ref)))
    worst["u"] = max(worst["u"], e_u)
    worst["hard"] = max(worst["hard"], hard)
    print(f"  {name}: obj {obj:.9g}, penalty(u) {pen_dev:.9g}, penalty(u_oracle) {pen_ref:.9g}, |u - oracle| "
          f"{float(np.max(np.abs(u - ref['u']))):.3e}, hard-row excess {hard:.3e}, {iters} iterations")
    assert e_obj <= Cs.SLACK_OBJ_TOL, (name, obj, pen_dev)
    assert pen_dev <= pen_ref + tol and pen_ref <= pen_dev + tol, (name, pen_dev, pen_ref)
    np.testing.assert_allclose(u, ref["u"], atol=Cs.SLACK_U_TOL, rtol=Cs.SLACK_U_TOL, err_msg=name)
    assert hard <= 1e-8, (name, hard)


@pytest.fixture(scope="module")
def fov(oracle):
    return Cs.fov_cases()


def test_fov_plain_cases(mpclib, fov):
    """Every plain case alone in its launch (its own configuration): 0 .. 13 neighbours with the
    optimum fixed by rows of slot 0, slot 3 and the lone lane-0 rows of slots 1 .. 3, 14 neighbours
    (ERROR, NaN u and objective, 0 iterations), fov 60 / 180 / 240 / 360 degrees at headings +-pi
    and 7.0, a neighbour at the ego position, velocity at and beyond v_max (INFEASIBLE).
    Measured on the MI355X: max |u - exact| 1.7e-10 (scaled), objective 2.6e-10 (relative)."""
    torch = require_gpu()
    worst = dict(u=0.0, obj=0.0)
    names = [n for n, e in fov.items() if not e["case"]["cfg"].get("control_slack_mode")]
    seen = set()
    for name in names:
        c, r = fov[name]["case"], fov[name]["ref"]
        got = _fov_solve(torch, mpclib, c["cfg"], [c])
        _check_plain(name, r, got["u"][0], int(got["status"][0]), float(got["obj"][0]), int(got["iters"][0]), worst)
        seen.add(r["status"])
    print(f"FoV plain: {len(names)} cases, max |u - exact| {worst['u']:.3e} (scaled by 1 + |u|), "
          f"max objective error {worst['obj']:.3e} (relative)")
    assert seen == {O.OPTIMAL, O.INFEASIBLE, O.ERROR}


@pytest.mark.parametrize("n", Cs.BATCH_SIZES)
def test_fov_batch_tails(mpclib, fov, n):
    """1, 15, 17 and 33 agents (16 per block). The batch of 17 holds one agent with 14 neighbours:
    it alone reports ERROR, and the others equal, bit for bit, the same agents solved without it.
    A second launch without status / obj / iters writes the same u.
    Measured on the MI355X: max |u - exact| 9.4e-11 (scaled), objective 7.2e-11 (relative)."""
    torch = require_gpu()
    err = Cs.ERROR_SLOT if n == 17 else None
    pool = Cs.plain_pool(n, with_error=err)
    cfg = pool[0]["cfg"]
    got = _fov_solve(torch, mpclib, cfg, pool)
    worst = dict(u=0.0, obj=0.0)
    for k, a in enumerate(pool):
        _check_plain(a["name"], Cs.fov_reference(a), got["u"][k], int(got["status"][k]), float(got["obj"][k]),
                     int(got["iters"][k]), worst)
    print(f"FoV batch of {n}: max |u - exact| {worst['u']:.3e} (scaled), max objective error {worst['obj']:.3e} (relative)")
    bare = _fov_solve(torch, mpclib, cfg, pool, outputs=False)
    np.testing.assert_array_equal(bare["u"], got["u"])
    if err is not None:
        assert got["status"][err] == O.ERROR and np.sum(got["status"] == O.ERROR) == 1
        rest = _fov_solve(torch, mpclib, cfg, Cs.plain_pool(n - 1))
        keep = [k for k in range(n) if k != err]
        for key in ("u", "status", "obj", "iters"):
            np.testing.assert_array_equal(got[key][keep], rest[key])


def test_fov_slack_cases(mpclib, fov):
    """Slack mode: 0, 1, 16 and 17 (ERROR) neighbours, nb_cov = None at decay 0.5 (all keys tie:
    index order), an infinite covariance among finite ones, two equidistant neighbours at decay
    1.0, fov = 2 pi (two of a neighbour's four rows absent), a crowded agent with >= 3 positive
    slacks.
    Measured on the MI355X: |obj - penalty(u)| 5.6e-12, penalty gap to the oracle's point 8.0e-10
    (both relative), |u - oracle| 3.0e-8 (scaled)."""
    torch = require_gpu()
    worst = dict(u=0.0, obj=0.0, gap=0.0, hard=-np.inf)
    names = [n for n, e in fov.items() if e["case"]["cfg"].get("control_slack_mode")]
    for name in names:
        c, r = fov[name]["case"], fov[name]["ref"]
        got = _fov_solve(torch, mpclib, c["cfg"], [c], use_cov=c["nb_cov"] is not None)
        _check_slack(name, r, c["u_des"], got["u"][0], int(got["status"][0]), float(got["obj"][0]),
                     int(got["iters"][0]), worst)
    print(f"FoV slack: {len(names)} cases, max |obj - penalty(u)| {worst['obj']:.3e} (relative), "
          f"max penalty gap to the oracle's point {worst['gap']:.3e} (relative), max |u - oracle| {worst['u']:.3e} "
          f"(scaled), largest hard-row excess {worst['hard']:.3e}")


def _conn_solve(torch, mpclib, cfg, ptr, states, desired, outputs=True):
    dev = torch.device("cuda", 0)
    t = lambda v, dt=torch.float64: to_device(v, dt)  # noqa: E731
    R, T = len(states), len(ptr) - 1
    u = torch.full((R + 1, 3), POISON, dtype=torch.float64, device=dev)
    status = torch.full((R + 1,), -77, dtype=torch.int32, device=dev)
    obj = torch.full((R + 1,), POISON, dtype=torch.float64, device=dev)
    iters = torch.full((R + 1,), -77, dtype=torch.int32, device=dev)
    l2 = torch.full((T + 1,), POISON, dtype=torch.float64, device=dev)
    kw = dict(status=status[:R], obj=obj[:R], iters=iters[:R], lambda2=l2[:T]) if outputs else {}
    mpclib.connectivity_control_solve(cfg, t(ptr, torch.int32), t(states), t(desired), u[:R], **kw)
    torch.cuda.synchronize()
    out = dict(u=u.cpu().numpy(), status=status.cpu().numpy(), obj=obj.cpu().numpy(), iters=iters.cpu().numpy(),
               l2=l2.cpu().numpy())
    assert np.all(out["u"][R] == POISON) and out["status"][R] == -77 and out["obj"][R] == POISON
    assert out["iters"][R] == -77 and out["l2"][T] == POISON
    return out


@pytest.mark.parametrize("slack", [False, True], ids=["plain", "slack"])
def test_connectivity_cases(mpclib, oracle, slack):
    """Teams of 1, 0, 2, 3, 16, 17, all-pairs-beyond-d_max, two clusters, triangle, hexagon in one
    launch whose team_ptr starts at row 2: lambda2 against LAPACK, statuses against the oracle, u
    and objective against the exact projection (plain) or the penalty objective (slack); rows of
    no team keep their poison; degenerate teams (the regular polygons) only have to give a legal
    status and, where OPTIMAL, satisfy their safety and velocity rows.
    Measured on the MI355X: lambda2 2.0e-15; plain |u - exact| 5.6e-7 (scaled; 1.2e-6 absolute against
    the allowed 1e-6 + 1e-6 |u| = 2.2e-6) on robot 15 of the team of 16, where next to the active
    safety row a velocity row is 7.6e-4 from active: at the PDIP's exit it still holds a multiplier
    of about mu / 7.6e-4 ~ 1e-6, which moves u by that much; every other robot is within 1.5e-7;
    objective 4.5e-9; slack |obj - penalty(u)| 5.8e-9, penalty gap 5.8e-9, |u - oracle| 5.8e-7 (the
    same robot)."""
    torch = require_gpu()
    cs = Cs.conn_cases(slack)
    cfg, ptr, states, desired = cs["cfg"], cs["team_ptr"], cs["states"], cs["desired"]
    got = _conn_solve(torch, mpclib, cfg, ptr, states, desired)
    R = len(states)
    # rows before team_ptr[0] (and the empty team, which has none) are not written
    for key, val in (("u", POISON), ("status", -77), ("obj", POISON), ("iters", -77)):
        assert np.all(got[key][:Cs.ROW_OFFSET] == val), key
    worst = dict(u=0.0, obj=0.0, gap=0.0, hard=-np.inf, l2=0.0)
    for t, info in enumerate(cs["teams"]):
        n = len(info["S"])
        l2 = got["l2"][t]
        if n == 0 or n > Cs.TEAM_CAP:
            assert np.isnan(l2), (info["name"], l2)  # no spectrum: NaN (include/mpccbf.h)
        else:
            e = abs(l2 - info["lambda2"]) / max(1.0, abs(info["lambda2"]))
            worst["l2"] = max(worst["l2"], e)
            assert e <= Cs.L2_TOL, (info["name"], l2, info["lambda2"])
        for i in range(n):
            r = int(ptr[t]) + i
            u, st, ob, it = got["u"][r], int(got["status"][r]), float(got["obj"][r]), int(got["iters"][r])
            ref = cs["ref"][r]
            name = f"{info['name']}[{i}]"
            if ref is None:  # degenerate: the Fiedler vector is not unique
                assert st in LEGAL, (name, st)
                if st == O.OPTIMAL:
                    assert 1 <= it <= 60
                    rows, tag = Cs.conn_rows(cfg, info["S"], i, slack=False)
                    # (in slack mode the safety rows may use their slacks: the velocity rows are hard)
                    hard = [(g, h, -1) for (g, h, _), tg in zip(rows, tag)
                            if tg[0] == "v" or (tg.startswith("safety") and not slack)]
                    assert len(hard) == (6 if slack else n + 5)
                    assert Cs.hard_excess(hard, u) <= 1e-8, (name, Cs.hard_excess(hard, u))
                else:
                    assert np.all(np.isnan(u))
                continue
            if slack:
                _check_slack(name, ref, info["u_des"][i], u, st, ob, it, worst)
            else:
                _check_plain(name, ref, u, st, ob, it, worst)
    if slack:
        print(f"connectivity slack: max |obj - penalty(u)| {worst['obj']:.3e} (relative), max penalty gap to the "
              f"oracle's point {worst['gap']:.3e} (relative), max |u - oracle| {worst['u']:.3e} (scaled), largest "
              f"hard-row excess {worst['hard']:.3e}, max lambda2 error {worst['l2']:.3e}")
    else:
        print(f"connectivity plain: max |u - exact| {worst['u']:.3e} (scaled), max objective error "
              f"{worst['obj']:.3e} (relative), max lambda2 error {worst['l2']:.3e} (relative to max(1, |lambda2|))")
    # the team of 1: u_des clipped by the velocity rows, lambda2 = 0
    one = int(ptr[0])
    assert got["l2"][0] == 0.0 and got["status"][one] == O.OPTIMAL
    np.testing.assert_allclose(got["u"][one], [0.1, -0.8, 0.2], atol=1e-6)
    # the empty team changes nothing: the same call without it gives the other teams' rows bit for bit
    ptr2 = np.delete(ptr, 1)
    alt = _conn_solve(torch, mpclib, cfg, ptr2, states, desired)
    for key in ("u", "status", "obj", "iters"):
        np.testing.assert_array_equal(alt[key][:R], got[key][:R])
    np.testing.assert_array_equal(alt["l2"][:len(ptr2) - 1], np.delete(got["l2"][:len(ptr) - 1], 1))
    # without the optional outputs: the same u
    bare = _conn_solve(torch, mpclib, cfg, ptr, states, desired, outputs=False)
    np.testing.assert_array_equal(bare["u"], got["u"])
    assert np.all(bare["status"] == -77) and np.all(bare["l2"] == POISON)
