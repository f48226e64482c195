"""CPU: the inputs of test_gpu_cbf_control.py (cbf_control_cases.py) are what that test needs —
every case keeps its reference status when every bound moves by +-1e-6 relative, every "row X
binds" claim holds in the exact projection's active set, the exact projection and the oracle agree
on every plain OPTIMAL case (so the reference alone stays within the tolerances), the statuses
cover OPTIMAL, INFEASIBLE and ERROR, and the degenerate teams are exactly the regular polygons."""
import numpy as np
import pytest

import cbf_control_cases as Cs
import oracle_lib as O


@pytest.fixture(scope="module")
def fov(oracle):
    return Cs.fov_cases()


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "slack"])
def conn(oracle, request):
    return Cs.conn_cases(request.param)


def test_exact_projection_on_known_answers():
    """Box clipping, one oblique row, a vertex of three rows, duplicate rows, a zero row and an
    infeasible pair."""
    box = np.vstack([np.eye(3), -np.eye(3)])
    u, obj, act = Cs.exact_projection(box, np.array([1.0, 2.0, 3.0, 1.0, 2.0, 3.0]), [4.0, -5.0, 0.5])
    np.testing.assert_allclose(u, [1.0, -2.0, 0.5], atol=1e-15)
    assert abs(obj - 18.0) < 1e-14 and set(act) == {0, 4}
    g = np.array([[1.0, 1.0, 1.0]])
    u, obj, act = Cs.exact_projection(g, [0.0], [1.0, 2.0, 3.0])
    np.testing.assert_allclose(u, [-1.0, 0.0, 1.0], atol=1e-15)
    assert act == (0,) and abs(obj - 12.0) < 1e-14
    u, obj, act = Cs.exact_projection(np.eye(3), [0.0, 0.0, 0.0], [1.0, 2.0, 3.0])
    np.testing.assert_allclose(u, 0.0, atol=1e-15)
    assert set(act) == {0, 1, 2}
    u, _, act = Cs.exact_projection(np.vstack([g, g, np.zeros((1, 3))]), [0.0, 0.0, 1.0], [1.0, 2.0, 3.0])
    np.testing.assert_allclose(u, [-1.0, 0.0, 1.0], atol=1e-15)
    assert len(act) == 1
    assert Cs.exact_projection([[1.0, 0, 0], [-1.0, 0, 0]], [-1.0, -1.0], [0.0, 0.0, 0.0]) is None
    assert Cs.exact_projection(np.zeros((1, 3)), [-1e-30], [0.0, 0.0, 0.0]) is None
    # against a random brute force: the projection is the feasible point nearest to u_des
    rng = np.random.default_rng(0)
    for _ in range(20):
        G = rng.normal(size=(12, 3))
        h = rng.uniform(0.1, 1.0, 12)
        ud = rng.normal(size=3) * 3
        u, obj, act = Cs.exact_projection(G, h, ud)
        assert np.all(G @ u <= h + 1e-12)
        for k in act:
            assert abs(G[k] @ u - h[k]) < 1e-12
        pts = u + rng.normal(size=(2000, 3)) * 0.05
        pts = pts[np.all(pts @ G.T <= h, axis=1)]
        assert np.all(np.sum((pts - ud) ** 2, axis=1) >= obj - 1e-12)


def test_penalty_objective_by_hand():
    rows = [(np.array([1.0, 0, 0]), 0.5, 0), (np.array([0, 1.0, 0]), -1.0, 0), (np.array([0, 0, 1.0]), 0.0, 1),
            (np.array([1.0, 0, 0]), 5.0, -1)]
    val, v = Cs.penalty_objective(rows, [10.0, 100.0], [1.0, 1.0, 1.0], [1.0, 0.0, -2.0])
    np.testing.assert_allclose(v, [1.0, 0.0])
    assert abs(val - (1.0 + 9.0 + 10.0)) < 1e-14
    assert Cs.hard_excess(rows, np.array([1.0, 0.0, -2.0])) == pytest.approx(-4.0 / 6.0)


def test_slack_weights_follow_the_reference_sort():
    """w_i = cost * decay^idx[i], idx = the neighbours sorted by ellipse distance (the index of the
    i-th smallest, FovControl.cpp:44-46), ties in index order; the distance restatement agrees
    with the oracle's."""
    cfg = Cs.fov_slack_cfg(0.5)
    st = np.array([0.0, 0.0, 0.0, 0, 0, 0])
    nb = np.array([[3.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    cov = np.tile([0.01, 0.0, 0.01], (3, 1))
    # keys ascend with the distance: sorted order (1, 2, 0) -> w = cost * decay^(1, 2, 0)
    np.testing.assert_allclose(Cs.fov_slack_weights(cfg, st, nb, cov), [500.0, 250.0, 1000.0])
    np.testing.assert_allclose(Cs.fov_slack_weights(cfg, st, nb, None), [1000.0, 500.0, 250.0])
    rng = np.random.default_rng(2)
    for _ in range(50):
        L = rng.normal(size=(2, 2))
        c = L @ L.T + 0.01 * np.eye(2)
        cov3 = (c[0, 0], c[0, 1], c[1, 1])
        r, m = rng.uniform(-3, 3, 2), rng.uniform(-3, 3, 2)
        assert abs(Cs.ellipse_distance(r, m, cov3) - O.distance_to_ellipse(r, m, cov3)) <= 1e-12
    assert Cs.ellipse_distance([0, 0], [1, 1], (np.inf, 0.0, np.inf)) == -5.0


def test_fov_cases_cover_what_the_issue_lists(fov):
    plain, slack = Cs.fov_plain_cases(), Cs.fov_slack_cases()
    counts = sorted(len(c["nb_xy"]) for n, c in plain.items() if n.startswith("plain_n"))
    assert counts == [0, 1, 2, 6, 10, 13, 13, 13, 14]
    betas = sorted({round(c["cfg"]["fov_beta"], 12) for c in plain.values()})
    assert betas == sorted(round(b, 12) for b in (np.deg2rad(60), np.deg2rad(120), np.pi, np.deg2rad(240), 2 * np.pi))
    assert plain["fov180"]["cfg"]["fov_beta"] == np.pi  # the == branch needs the exact value
    yaws = {c["state"][2] for c in plain.values()}
    assert {np.pi, -np.pi, 7.0} <= yaws
    assert np.array_equal(plain["nb_at_ego"]["nb_xy"][0], plain["nb_at_ego"]["state"][:2])
    assert plain["at_vmax"]["state"][3] == plain["at_vmax"]["cfg"]["v_max"][0]
    assert sorted(len(c["nb_xy"]) for c in slack.values())[-2:] == [16, 17]
    assert {0, 1} <= {len(c["nb_xy"]) for c in slack.values()}
    assert slack["slack_nocov"]["nb_cov"] is None and slack["slack_nocov"]["cfg"]["slack_decay_rate"] == 0.5
    assert np.isinf(slack["slack_infcov"]["nb_cov"][2, 0]) and np.all(np.isfinite(slack["slack_infcov"]["nb_cov"][[0, 1, 3, 4]]))
    assert slack["slack_fov360"]["cfg"]["fov_beta"] == 2 * np.pi
    # every neighbour of the count cases is inside the cone and between Ds and Rs
    for n, c in plain.items():
        if n.startswith("plain_n"):
            d = c["nb_xy"] - c["state"][:2]
            r = np.hypot(d[:, 0], d[:, 1])
            b = np.arctan2(d[:, 1], d[:, 0]) - c["state"][2]
            assert np.all((r > c["cfg"]["fov_Ds"]) & (r < c["cfg"]["fov_Rs"])) and np.all(np.abs(b) < 0.5 * c["cfg"]["fov_beta"])


def test_fov_statuses_are_stable_and_as_expected(fov):
    seen = set()
    for name, e in fov.items():
        c, r = e["case"], e["ref"]
        assert r["status"] == c["expect"], (name, r["status"])
        seen.add(r["status"])
        for sh in (Cs.SHIFT, -Cs.SHIFT):
            assert Cs.fov_reference(c, sh)["status"] == r["status"], (name, sh)
        if r["status"] != O.ERROR:  # the oracle's own controller says the same
            assert O.fov_control(c["cfg"], c["state"], c["u_des"], c["nb_xy"], nb_cov=c["nb_cov"])[0] == r["status"], name
    assert {O.OPTIMAL, O.INFEASIBLE, O.ERROR} <= seen
    for name, e in fov.items():  # no desired control sits exactly on a control bound (a weakly active row)
        cfg, ud = e["case"]["cfg"], e["case"]["u_des"]
        assert not np.any(ud == cfg.get("u_max", cfg["a_max"])) and not np.any(ud == cfg.get("u_min", cfg["a_min"])), name
    slack = [e for e in fov.values() if e["case"]["cfg"].get("control_slack_mode")]
    assert all(e["ref"]["status"] == O.OPTIMAL or len(e["case"]["nb_xy"]) == 17 for e in slack)


def _drop(ref, u_des, name):
    """The exact projection without the named rows."""
    keep = [k for k, t in enumerate(ref["tag"]) if (t[0] if isinstance(t, tuple) else t) not in name]
    G = np.array([ref["rows"][k][0] for k in keep])
    h = np.array([ref["rows"][k][1] for k in keep])
    return Cs.exact_projection(G, h, u_des)


def test_fov_named_rows_bind(fov):
    """Each claim: the row is in the exact active set, it holds with equality at the optimum, and
    without it the objective drops by more than 1e-3 — it alone keeps the optimum where it is."""
    slots = {}
    for name, e in fov.items():
        c, r = e["case"], e["ref"]
        if not c["binds"]:
            continue
        assert c["binds"] in r["active"], (name, r["active"])
        k = [t[0] for t in r["tag"]].index(c["binds"])
        g, h, _ = r["rows"][k]
        assert abs(g @ r["u"] - h) <= 1e-9 * max(1.0, abs(h)), name
        drop = {c["binds"]}
        if c["cfg"]["fov_beta"] == np.pi:  # at pi the left and right border rows are one row twice
            drop.add(c["binds"].replace("left", "right"))
            k2 = [t[0] for t in r["tag"]].index("nb0.right")
            assert np.array_equal(r["rows"][k2][0], g) and r["rows"][k2][1] == h
        free = _drop(r, c["u_des"], drop)
        assert free is not None and free[1] < r["obj"] - 1e-3, (name, free[1], r["obj"])
        slots[name] = divmod(r["tag"][k][1], 16)
    # slot / lane of the binding rows in the plain kernel (row t: slot t // 16, lane t % 16)
    assert slots["plain_n2"] == (1, 0) and slots["plain_n6"] == (2, 0) and slots["plain_n10"] == (3, 0)
    assert slots["plain_n13_nb0"][0] == 0 and slots["plain_n13_nb12"][0] == 3 and slots["plain_n13_bound"][0] == 3
    # at 13 neighbours every velocity and control-bound row is in slot 3
    tags = fov["plain_n13_bound"]["ref"]["tag"]
    assert {t // 16 for n, t in tags if n[0] in "vu"} == {3} and max(t for _, t in tags) == 60


def test_exact_projection_agrees_with_the_oracle_on_plain_cases(fov):
    worst_u = worst_o = 0.0
    n = 0
    for name, e in fov.items():
        c, r = e["case"], e["ref"]
        if c["cfg"].get("control_slack_mode") or r["status"] != O.OPTIMAL:
            continue
        st, u, obj = O.fov_control(c["cfg"], c["state"], c["u_des"], c["nb_xy"])
        assert st == O.OPTIMAL and np.all(np.isfinite(r["u"])), name
        worst_u = max(worst_u, float(np.max(np.abs(u - r["u"]) / (1.0 + np.abs(r["u"])))))
        worst_o = max(worst_o, abs(obj - r["obj"]) / max(1.0, abs(r["obj"])))
        n += 1
    print(f"FoV plain: {n} cases, max |u_oracle - u_exact| {worst_u:.3e} (scaled), objective {worst_o:.3e} (relative)")
    assert n >= 14 and worst_u <= 1e-9 and worst_o <= 1e-9  # 1e-3 of the device tolerances


def test_fov_slack_cases_use_their_slacks(fov):
    """The crowded case has at least three positive slacks; where ties could reorder the weights
    (decay < 1) the keys are distinct, except with nb_cov = None; the oracle's objective is the
    penalty objective at its own u."""
    assert int(np.sum(fov["slack_crowded"]["ref"]["slacks"] > 1e-3)) >= 3
    assert np.any(fov["slack_fov360"]["ref"]["slacks"] > 1e-3)
    for name, e in fov.items():
        c, r = e["case"], e["ref"]
        if not c["cfg"].get("control_slack_mode") or r["status"] != O.OPTIMAL:
            continue
        keys = Cs.fov_slack_keys(c["state"], c["nb_xy"], c["nb_cov"])
        if c["cfg"]["slack_decay_rate"] < 1.0 and c["nb_cov"] is not None and len(keys) > 1:
            assert np.min(np.diff(np.sort(keys))) > 1e-6, name
        assert abs(r["oracle_obj"] - r["obj"]) <= 1e-6 * max(1.0, abs(r["obj"])), (name, r["oracle_obj"], r["obj"])
        assert Cs.hard_excess(r["rows"], r["u"]) <= 1e-7, name
    k = Cs.fov_slack_keys(*[fov["slack_equidistant"]["case"][f] for f in ("state", "nb_xy", "nb_cov")])
    assert abs(k[0] - k[1]) <= 1e-12 and fov["slack_equidistant"]["case"]["cfg"]["slack_decay_rate"] == 1.0
    # the weight order matters where it is tested: reversing the tie order of the all-ties case, or
    # swapping the connectivity-free weights of the infinite-covariance case, changes the objective
    for name in ("slack_nocov", "slack_infcov"):
        r, c = fov[name]["ref"], fov[name]["case"]
        other = Cs.penalty_objective(r["rows"], r["weights"][::-1], c["u_des"], r["u"])[0]
        assert abs(other - r["obj"]) > 1e-2 * abs(r["obj"]), name


def test_batches(fov):
    assert Cs.BATCH_SIZES == (1, 15, 17, 33)
    pool = Cs.plain_pool(17, with_error=Cs.ERROR_SLOT)
    assert len(pool[Cs.ERROR_SLOT]["nb_xy"]) == 14 and sum(len(a["nb_xy"]) == 14 for a in pool) == 1
    rest = Cs.plain_pool(16)
    for a, b in zip(pool[:Cs.ERROR_SLOT] + pool[Cs.ERROR_SLOT + 1:], rest):
        assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["nb_xy"], b["nb_xy"])
        assert np.array_equal(a["u_des"], b["u_des"])
    for a in Cs.plain_pool(33):
        r = Cs.fov_reference(a)
        assert r["status"] == O.OPTIMAL
        for sh in (Cs.SHIFT, -Cs.SHIFT):
            assert Cs.fov_reference(a, sh)["status"] == O.OPTIMAL
    states, desired, rp, nb, cov = Cs.fov_batch(pool)
    assert states.shape == (17, 6) and rp[-1] == len(nb) == len(cov) and rp.dtype == np.int32


def test_conn_layout_and_spectra(conn):
    ptr = conn["team_ptr"]
    assert ptr[0] == Cs.ROW_OFFSET > 0
    assert list(np.diff(ptr)) == [1, 0, 2, 3, 16, 17, 5, 6, 3, 6]
    by = {t["name"]: t for t in conn["teams"]}
    dmax = conn["cfg"]["d_max"]
    assert by["one"]["lambda2"] == 0.0 and np.isnan(by["empty"]["lambda2"])
    # all pairs beyond d_max: the Laplacian is zero; two clusters 2 d_max apart: lambda2 = 0, disconnected
    S = by["far5"]["S"]
    assert min(np.hypot(*(S[i, :2] - S[j, :2])) for i in range(5) for j in range(i)) > dmax
    assert not np.any(Cs.laplacian(S[:, :2], dmax))
    S = by["clusters6"]["S"]
    assert min(np.hypot(*(S[i, :2] - S[j, :2])) for i in range(3) for j in range(3, 6)) >= 2.0 * dmax
    w = Cs.spectrum(S, dmax)[2]
    assert abs(w[1]) < 1e-12 and w[2] > 1.0
    # degenerate teams are exactly the regular polygons; no other team is near the 0.1 threshold
    assert [t["name"] for t in conn["teams"] if t["degenerate"]] == ["triangle", "hexagon"]
    for t in conn["teams"]:
        if len(t["S"]) >= 3 and not t["degenerate"]:
            w = Cs.spectrum(t["S"], dmax)[2]
            assert w[2] - w[1] >= 1e-6 or t["lambda2"] < 0.1 - 1e-3, t["name"]
        if len(t["S"]) and not t["degenerate"]:
            assert abs(t["lambda2"] - 0.1) >= 1e-3, t["name"]
        if len(t["S"]) >= 2:  # the oracle's Jacobi agrees with LAPACK
            assert abs(O.lambda2(t["S"][:, :2], dmax)[0] - t["lambda2"]) <= Cs.L2_TOL * max(1.0, abs(t["lambda2"]))
    modes = {t["lambda2"] > 0.1 for t in conn["teams"] if len(t["S"]) >= 2 and not t["degenerate"]}
    assert modes == {True, False}


def test_conn_statuses_are_stable(conn):
    cfg, ptr = conn["cfg"], conn["team_ptr"]
    slack = bool(cfg.get("control_slack_mode"))
    seen = set()
    worst_u = worst_o = 0.0
    for t, info in enumerate(conn["teams"]):
        for i in range(len(info["S"])):
            r = conn["ref"][int(ptr[t]) + i]
            if r is None:
                continue
            seen.add(r["status"])
            if r["status"] == O.ERROR:
                continue
            for sh in (Cs.SHIFT, -Cs.SHIFT):
                assert Cs.conn_reference(cfg, info["S"], i, info["u_des"][i], sh)["status"] == r["status"], (info["name"], i)
            st, u, obj, _ = O.connectivity_control(cfg, info["S"], i, info["u_des"][i])
            assert st == r["status"], (info["name"], i, st, r["status"])
            if slack:
                assert r["status"] == O.OPTIMAL
                assert abs(obj - r["obj"]) <= 1e-6 * max(1.0, abs(r["obj"])), (info["name"], i, obj, r["obj"])
            elif st == O.OPTIMAL:
                worst_u = max(worst_u, float(np.max(np.abs(u - r["u"]) / (1.0 + np.abs(r["u"])))))
                worst_o = max(worst_o, abs(obj - r["obj"]) / max(1.0, abs(r["obj"])))
    if slack:
        assert seen == {O.OPTIMAL, O.ERROR}
        # the team of 2: the connectivity row's slack (the last one, n - 1 = 1) is in use
        for i in range(2):
            r = conn["ref"][int(ptr[2]) + i]
            assert r["tag"][-1] == "conn" and r["rows"][-1][2] == 1 and r["slacks"][1] > 1e-2 and r["slacks"][0] == 0.0
    else:
        assert seen == {O.OPTIMAL, O.INFEASIBLE, O.ERROR}
        print(f"connectivity plain: max |u_oracle - u_exact| {worst_u:.3e} (scaled), objective {worst_o:.3e} (relative)")
        assert worst_u <= 1e-9 and worst_o <= 1e-9
        one = conn["ref"][int(ptr[0])]
        np.testing.assert_allclose(one["u"], [0.1, -0.8, 0.2], atol=1e-15)
        # both kinds of added row fix some optimum
        act = {a for r in conn["ref"].values() if r for a in r["active"]}
        assert "conn" in act and any(a.startswith("safety") for a in act)
