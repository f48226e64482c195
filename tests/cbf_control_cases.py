"""Inputs of test_gpu_cbf_control.py (GPU) and test_cbf_control_inputs.py (CPU): hand-built agents
and teams at the edges of the two CBF-only controllers (mpccbf_fov_control_solve,
mpccbf_connectivity_control_solve) — row capacity, batch tails, the fov_border branches, the slack
weights' order, empty / single / disconnected / symmetric teams — and two references that are not
a PDIP. Nothing here touches a GPU.

References
  exact_projection(G, h, u_des): min ||u - u_des||^2 s.t. G u <= h over 3 variables by enumerating
    every active set of 0 .. 3 rows in long double (the projection on each set is closed form); the
    KKT point among them is the optimum. The rows come from O.fov_cbf / O.safety_cbf / O.clf_cbf /
    O.conn_cbf (pinned by the symbolic goldens and the reference's known answers) plus velocity and
    bound rows written here. The oracle's solver gives statuses only.
  penalty_objective(rows, weights, u_des, u): slack mode, with every slack eliminated:
    ||u - u_des||^2 + sum_j w_j max(0, max_r (g_jr u - h_jr)).

Slack weights (FovControl.cpp:25-46): idx = the neighbour indices sorted by distanceToEllipse, and
neighbour i gets slack_cost * decay^idx[i] — the index of the i-th smallest, not i's rank (kept).
The reference sorts with std::sort, which leaves the order of equal keys unspecified; libstdc++
sorts up to 16 elements by insertion, which keeps them in index order, and that is what the
restatement here (a stable argsort) and the device do. Exact ties with decay < 1 are therefore kept
out of the cases, with one exception the controller's interface forces: nb_cov = None makes every
key -5 (FovControl.cpp:157), so that case (decay 0.5) is all ties, in index order. The two
equidistant neighbours appear at decay 1.0 only, where the order cannot matter.
ConnectivityControl.cpp:31-38 has no sort: slack i weighs slack_cost * decay^i.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import oracle_lib as O
from mpccbf import swarm

SHIFT = 1e-6     # the stability check: every bound moved by +-SHIFT relative (conn_impc_cases.SHIFT)
LD = np.longdouble
DBL_MAX = np.finfo(np.float64).max

PLAIN_U_TOL, PLAIN_OBJ_TOL = 1e-6, 1e-6
SLACK_U_TOL, SLACK_OBJ_TOL = 1e-5, 1e-4
L2_TOL = 1e-10

FOV_PLAIN_CAP = 13   # 4 * 13 + 9 = 61 <= 64 rows
FOV_SLACK_CAP = 16   # one neighbour per lane
TEAM_CAP = 16


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def exact_projection(G, h, u_des):
    """min ||u - u_des||^2 s.t. G u <= h (3 variables): (u, objective, active set) or None when no
    active set of 0 .. 3 rows gives a feasible point with non-negative multipliers (infeasible rows).
    The active set is the smallest one: every multiplier of it is positive unless the optimum is
    degenerate."""
    G = np.asarray(G, dtype=LD).reshape(-1, 3)
    h = np.asarray(h, dtype=LD).reshape(-1)
    ud = np.asarray(u_des, dtype=LD)
    nrm = np.sqrt(np.sum(G * G, axis=1))
    zero = nrm == 0
    if np.any(h[zero] < 0):
        return None
    idx = np.nonzero(~zero)[0]
    Gn, hn = G[idx] / nrm[idx, None], h[idx] / nrm[idx]
    m = len(idx)
    ftol = LD(1e-13)

    def feasible(U):  # U: (k, 3) -> (k,) bool
        r = U @ Gn.T - hn[None, :]
        return np.all(r <= ftol * (1 + np.abs(hn))[None, :], axis=1)

    def result(u, act):
        u64 = np.asarray(u, dtype=np.float64)
        return u64, float(np.sum((u - ud) ** 2)), tuple(int(idx[a]) for a in act)

    if m == 0 or feasible(ud[None, :])[0]:
        return result(ud, ())
    viol = Gn @ ud - hn  # the multiplier of a row alone
    # one row
    U1 = ud[None, :] - viol[:, None] * Gn
    ok = (viol >= 0) & feasible(U1)
    if np.any(ok):
        k = int(np.nonzero(ok)[0][0])
        return result(U1[k], (k,))
    # two rows: Gram [[1, c], [c, 1]]
    if m >= 2:
        i, j = np.triu_indices(m, 1)
        c = np.sum(Gn[i] * Gn[j], axis=1)
        det = 1 - c * c
        good = det > LD(1e-20)
        dd = np.where(good, det, 1)
        mi = (viol[i] - c * viol[j]) / dd
        mj = (viol[j] - c * viol[i]) / dd
        U2 = ud[None, :] - mi[:, None] * Gn[i] - mj[:, None] * Gn[j]
        ok = good & (mi >= 0) & (mj >= 0)
        ok[ok] = feasible(U2[ok])
        if np.any(ok):
            k = int(np.nonzero(ok)[0][0])
            return result(U2[k], (i[k], j[k]))
    # three rows: the vertex G_A u = h_A (Cramer), multipliers mu = G_A^-T (u_des - u)
    if m >= 3:
        tri = np.array(list(itertools.combinations(range(m), 3)))
        a, b, cc = Gn[tri[:, 0]], Gn[tri[:, 1]], Gn[tri[:, 2]]
        bc, ca, ab = np.cross(b, cc), np.cross(cc, a), np.cross(a, b)
        det = np.sum(a * bc, axis=1)
        good = np.abs(det) > LD(1e-12)
        dd = np.where(good, det, 1)[:, None]
        ha, hb, hc = hn[tri[:, 0]], hn[tri[:, 1]], hn[tri[:, 2]]
        U3 = (ha[:, None] * bc + hb[:, None] * ca + hc[:, None] * ab) / dd
        e = ud[None, :] - U3
        # u_des - u = mu_a a + mu_b b + mu_c c  ->  mu_a = e . (b x c) / det, ...
        mu = np.stack([np.sum(e * bc, axis=1), np.sum(e * ca, axis=1), np.sum(e * ab, axis=1)], axis=1) / dd
        ok = good & np.all(mu >= 0, axis=1) & np.all(np.isfinite(U3), axis=1)
        ok[ok] = feasible(U3[ok])
        if np.any(ok):
            k = int(np.nonzero(ok)[0][0])
            return result(U3[k], tuple(tri[k]))
    return None


def penalty_objective(rows, weights, u_des, u):
    """||u - u_des||^2 + sum_j w_j max(0, max over the rows of slack j of g u - h): the slack-mode
    objective with every slack at its optimal value for this u. rows: (g, h, slack) triples; rows
    with slack < 0 are hard (they must hold at u; not part of the sum)."""
    u = np.asarray(u, dtype=LD)
    ud = np.asarray(u_des, dtype=LD)
    v = np.zeros(len(weights), dtype=LD)
    for g, hh, j in rows:
        if j >= 0:
            v[j] = max(v[j], np.dot(np.asarray(g, dtype=LD), u) - LD(hh))
    return float(np.sum((u - ud) ** 2) + np.dot(np.asarray(weights, dtype=LD), v)), np.asarray(v, dtype=np.float64)


def hard_excess(rows, u):
    """Largest g u - h over the hard rows, scaled by 1 + |h| (<= 0: all satisfied)."""
    worst = -np.inf
    for g, hh, j in rows:
        if j < 0:
            worst = max(worst, float((np.dot(g, u) - hh) / (1.0 + abs(hh))))
    return worst


def oracle_status(rows, u_des, nslack=0, weights=None, shift=0.0):
    """Status of the QP built from `rows` (hard rows, or slack rows with one variable >= 0 per slack)
    by the oracle's dense solver, every bound moved by shift * max(1, |bound|)."""
    n = 3 + nslack
    H = np.zeros((n, n))
    H[:3, :3] = np.eye(3)
    c = np.zeros(n)
    c[:3] = -2.0 * np.asarray(u_des)
    if nslack:
        c[3:] = weights
    A = np.zeros((len(rows), n))
    hi = np.zeros(len(rows))
    for k, (g, hh, j) in enumerate(rows):
        A[k, :3] = g
        if j >= 0:
            A[k, 3 + j] = -1.0
        hi[k] = hh + shift * max(1.0, abs(hh))
    vlo = np.concatenate([np.full(3, -np.inf), np.zeros(nslack)])
    qp = dict(n=n, H=H, c=c, c0=float(np.dot(u_des, u_des)), A=A, lo=np.full(len(rows), -DBL_MAX), hi=hi,
              vlo=vlo, vhi=np.full(n, np.inf))
    return O.solve_dense_qp(qp)["status"]


# ---------------------------------------------------------------------------------------------
# FoV controller: rows
# ---------------------------------------------------------------------------------------------
def fov_cfg(**over):
    return dict(swarm.fov_config(20), **over)


def fov_slack_cfg(decay=0.5, **over):
    return fov_cfg(control_slack_mode=1, slack_cost=1000.0, slack_decay_rate=decay, **over)


def fov_rows(cfg, state, nb_xy, slack=False):
    """The controller's rows as g u <= h: (rows, tag) with rows = (g, h, slack index or -1) and
    tag[k] = (name, kernel row t): t is the plain kernel's row number (4 j + kind for neighbour j,
    then 4 nnb + 0..2 min velocity, + 3..5 max velocity, + 6..8 control bounds; row t sits in slot
    t // 16, lane t % 16). The control bounds appear as two one-sided rows with the same t."""
    st = np.asarray(state, dtype=np.float64)
    nb = np.reshape(np.asarray(nb_xy, dtype=np.float64), (-1, 2))
    rows, tag = [], []
    kinds = ("safety", "left", "right", "range")
    for j, o in enumerate(nb):
        A, b, present = O.fov_cbf(st, o, cfg["fov_beta"], cfg["fov_Ds"], cfg["fov_Rs"])
        for r in range(4):
            if present[r]:
                rows.append((-A[r], float(b[r]), j if slack else -1))
                tag.append((f"nb{j}.{kinds[r]}", 4 * j + r))
    base = 4 * len(nb)
    umin = cfg.get("u_min", cfg["a_min"])
    umax = cfg.get("u_max", cfg["a_max"])
    for d in range(3):
        rows.append((-np.eye(3)[d], st[3 + d] - cfg["v_min"][d], -1))
        tag.append((f"vmin{d}", base + d))
    for d in range(3):
        rows.append((np.eye(3)[d], cfg["v_max"][d] - st[3 + d], -1))
        tag.append((f"vmax{d}", base + 3 + d))
    for d in range(3):
        rows.append((np.eye(3)[d], umax[d], -1))
        tag.append((f"umax{d}", base + 6 + d))
        rows.append((-np.eye(3)[d], -umin[d], -1))
        tag.append((f"umin{d}", base + 6 + d))
    return rows, tag


def ellipse_distance(robot_xy, mean_xy, cov3):
    """FovControl::distanceToEllipse (FovControl.cpp:92-158) restated with numpy's symmetric
    eigen-decomposition: signed distance to the 90 % ellipse (s = 4.605), -5 for an unknown
    (infinite) covariance, 5 where the distance is NaN."""
    cxx, cxy, cyy = (float(v) for v in cov3)
    if np.isinf(cxx):
        return -5.0
    w, V = np.linalg.eigh(np.array([[cxx, cxy], [cxy, cyy]]))
    a, b = np.sqrt(4.605 * w[1]), np.sqrt(4.605 * w[0])  # major, minor
    th = np.arctan2(V[1, 1], V[0, 1])
    if th < 0.0:
        th += np.pi
    rx, ry = robot_xy
    mx, my = mean_xy
    sl = np.arctan2(ry - my, rx - mx)
    xn = mx + a * np.cos(sl - th) * np.cos(th) - b * np.sin(sl - th) * np.sin(th)
    yn = my + a * np.cos(sl - th) * np.sin(th) + b * np.sin(sl - th) * np.cos(th)
    dist = np.hypot(xn - rx, yn - ry)
    if np.isnan(dist):
        return 5.0
    return -dist if np.hypot(mx - rx, my - ry) < np.hypot(mx - xn, my - yn) else dist


def fov_slack_keys(state, nb_xy, nb_cov):
    nb = np.reshape(np.asarray(nb_xy, dtype=np.float64), (-1, 2))
    if nb_cov is None:
        return np.full(len(nb), -5.0)
    return np.array([ellipse_distance(state[:2], nb[j], nb_cov[j]) for j in range(len(nb))])


def fov_slack_weights(cfg, state, nb_xy, nb_cov):
    """FovControl.cpp:25-46: w_i = slack_cost * decay^idx[i], idx the neighbours sorted by key."""
    keys = fov_slack_keys(state, nb_xy, nb_cov)
    idx = np.argsort(keys, kind="stable")
    return cfg["slack_cost"] * cfg["slack_decay_rate"] ** idx.astype(np.float64)


# ---------------------------------------------------------------------------------------------
# FoV controller: cases
# ---------------------------------------------------------------------------------------------
def _polar(state, dist, bearing):
    """Points at the given distances and bearings (relative to the heading) from the ego."""
    ang = state[2] + np.asarray(bearing, dtype=np.float64)
    return np.stack([state[0] + dist * np.cos(ang), state[1] + dist * np.sin(ang)], axis=1)


def _spread(n):
    """n neighbours well inside a 120-degree cone and between Ds and Rs: distances 3 .. 4.5,
    bearings within +-30 degrees — none of their rows comes near binding."""
    k = np.arange(n)
    dist = 3.0 + 1.5 * ((k * 5) % 13) / 12.0
    bearing = np.deg2rad(-30.0 + 60.0 * ((k * 7) % 13) / 12.0)
    return dist, bearing


def _agent(name, state, u_des, nb_xy, cfg=None, nb_cov=None, binds=None, expect=O.OPTIMAL):
    return dict(name=name, state=np.asarray(state, dtype=np.float64), u_des=np.asarray(u_des, dtype=np.float64),
                nb_xy=np.reshape(np.asarray(nb_xy, dtype=np.float64), (-1, 2)), cfg=cfg or fov_cfg(),
                nb_cov=None if nb_cov is None else np.reshape(np.asarray(nb_cov, dtype=np.float64), (-1, 3)),
                binds=binds, expect=expect)


EGO = np.array([0.4, -0.3, 0.35, 0.05, 0.02, -1.0])  # yaw rate -1: the yaw velocity row stays behind u_max


def _count_case(n, far=None, u_des=(1.0, 0.5, 0.3), binds=None, name=None, expect=O.OPTIMAL):
    """n neighbours inside the cone; `far` sits 5.9 out (Rs = 6): its range row stops any
    acceleration away from it."""
    dist, bearing = _spread(n)
    if far is not None:
        dist[far] = 5.9
    return _agent(name or f"plain_n{n}", EGO, u_des, _polar(EGO, dist, bearing), binds=binds, expect=expect)


def fov_plain_cases():
    """Plain mode: (name -> agent). binds: the name of the row that fixes the optimum."""
    away = (-2.0, 0.5, 0.3)   # against the heading: a neighbour at 5.9 forbids it (range row)
    yaw = (1.0, 0.5, 3.4)     # yaw beyond u_max = pi: the yaw control bound, row 4 nnb + 8
    cs = [
        _count_case(0),
        _count_case(1, far=0, u_des=away, binds="nb0.range"),
        _count_case(2, u_des=yaw, binds="umax2"),     # row 16: slot 1, lane 0
        _count_case(6, u_des=yaw, binds="umax2"),     # row 32: slot 2, lane 0
        _count_case(10, u_des=yaw, binds="umax2"),    # row 48: slot 3, lane 0
        _count_case(13, far=0, u_des=away, binds="nb0.range", name="plain_n13_nb0"),     # row 3: slot 0
        _count_case(13, far=12, u_des=away, binds="nb12.range", name="plain_n13_nb12"),  # row 51: slot 3
        _count_case(13, u_des=(9.0, 0.5, 0.3), binds="vmax0", name="plain_n13_bound"),   # row 55: slot 3
        _count_case(14, expect=O.ERROR),
    ]
    # fov_beta branches (fov_border: < pi, == pi, > pi, 2 pi), headings at +-pi and 7.0 rad: neighbour 0
    # sits 0.3 rad inside the left border (2 pi: 5.9 out, behind), the desired control turns away
    for label, beta, yaw0, binds in (("fov60", np.deg2rad(60.0), np.pi, "nb0.left"), ("fov180", np.pi, -np.pi, "nb0.left"),
                                     ("fov240", np.deg2rad(240.0), 7.0, "nb0.left"), ("fov360", 2.0 * np.pi, 7.0, "nb0.range")):
        st = np.array([-0.2, 0.6, yaw0, 0.25, -0.15, 0.2])
        half = 0.5 * beta
        # the border rows' cone: half-angle fov / 2 below pi, pi / 2 at pi, pi - fov / 2 above it
        lim = half if beta < np.pi else np.pi - half
        bearing, dist = np.array([lim - 0.3, 0.05, -0.2]), np.array([2.0, 3.5, 4.0])
        if binds == "nb0.range":
            bearing[0], dist[0] = 2.5, 5.9
        cs.append(_agent(label, st, (0.5, -0.4, -0.8), _polar(st, dist, bearing), cfg=fov_cfg(fov_beta=float(beta)),
                         binds=binds))
    # one neighbour exactly at the ego position (ego moving: the safety row is 0 <= 2 |v|^2)
    st = np.array([1.0, 2.0, 0.3, 0.4, 0.2, 0.1])
    cs.append(_agent("nb_at_ego", st, (0.5, -0.5, 0.2), np.vstack([st[:2], _polar(st, np.array([3.0]), np.array([0.1]))])))
    # velocity rows: exactly at v_max (bound 0), and beyond it by more than the control range
    for name, vx, binds, expect in (("at_vmax", 2.0, "vmax0", O.OPTIMAL), ("beyond_vmax", 8.0, None, O.INFEASIBLE)):
        st = np.array([0.0, 0.0, 0.2, vx, 0.5, 0.0])
        cs.append(_agent(name, st, (1.5, 0.3, 0.1), _polar(st, *_spread(3)), binds=binds, expect=expect))
    return {c["name"]: c for c in cs}


def _covs(n, seed):
    rng = np.random.default_rng(seed)
    cov = np.zeros((n, 3))
    for j in range(n):
        L = rng.normal(size=(2, 2)) * 0.4
        c = L @ L.T + 0.02 * np.eye(2)
        cov[j] = (c[0, 0], c[0, 1], c[1, 1])
    return cov


SEGO = np.array([0.4, -0.3, 0.35, 0.5, 0.02, 0.3])  # the slack cases' ego
# a control box too small to turn every row feasible (no component of a desired control sits exactly
# on it: a bound that is active with a zero multiplier leaves an interior-point solver sqrt(mu) away)
BOX = dict(u_min=[-0.3, -0.3, -0.25], u_max=[0.3, 0.3, 0.25])


def _crowd(n, seed, outside, ego=SEGO):
    """n neighbours around the ego, the first `outside` of them 4, 7, 10 ... degrees outside the
    120-degree cone on alternating sides (their border rows cannot all hold inside BOX, so their
    slacks are in use), the rest inside."""
    rng = np.random.default_rng(seed)
    dist, bearing = _spread(n)
    dist = dist + rng.uniform(-0.2, 0.2, n)
    bearing = bearing + rng.uniform(-0.05, 0.05, n)
    for k in range(outside):
        bearing[k] = np.deg2rad(64.0 + 3.0 * k) * (1 if k % 2 == 0 else -1)
        dist[k] = 2.0 + 0.35 * k
    return _polar(ego, dist, bearing)


def fov_slack_cases():
    ud = (1.0, 0.5, 0.3)
    cs = [
        _agent("slack_n0", SEGO, ud, np.zeros((0, 2)), cfg=fov_slack_cfg(**BOX), nb_cov=np.zeros((0, 3))),
        _agent("slack_n1", SEGO, ud, _crowd(1, 1, 1), cfg=fov_slack_cfg(**BOX), nb_cov=_covs(1, 1)),
        _agent("slack_n16", SEGO, ud, _crowd(16, 2, 4), cfg=fov_slack_cfg(0.9, **BOX), nb_cov=_covs(16, 2)),
        _agent("slack_n17", SEGO, ud, _crowd(17, 3, 4), cfg=fov_slack_cfg(0.9, **BOX), nb_cov=_covs(17, 3), expect=O.ERROR),
        _agent("slack_nocov", SEGO, ud, _crowd(5, 4, 3), cfg=fov_slack_cfg(0.5, **BOX)),
        # 2 pi: no border rows (two of a neighbour's four rows absent); neighbour 4 inside Ds,
        # neighbour 5 behind the ego and beyond Rs
        _agent("slack_fov360", SEGO, (-2.0, 0.5, 0.3),
               np.vstack([_crowd(4, 6, 2), _polar(SEGO, np.array([0.15, 6.05]), np.array([2.0, np.pi]))]),
               cfg=fov_slack_cfg(0.5, fov_beta=2.0 * np.pi, **BOX), nb_cov=_covs(6, 6)),
        _agent("slack_crowded", SEGO, ud, _crowd(9, 7, 4), cfg=fov_slack_cfg(0.7, **BOX), nb_cov=_covs(9, 7)),
        _agent("slack_free", SEGO, ud, _crowd(9, 7, 4), cfg=fov_slack_cfg(0.7), nb_cov=_covs(9, 7)),
    ]
    cov = _covs(5, 5)
    cov[2] = (np.inf, 0.0, np.inf)
    cs.append(_agent("slack_infcov", SEGO, ud, _crowd(5, 5, 3), cfg=fov_slack_cfg(0.5, **BOX), nb_cov=cov))
    # two neighbours mirrored about the heading of an ego at yaw 0 with the same axis-aligned
    # covariance: equal ellipse distances; decay 1.0
    st = np.array([0.0, 0.0, 0.0, 0.5, 0.0, 0.0])
    nb = np.array([[2.0 * np.cos(1.4), 2.0 * np.sin(1.4)], [2.0 * np.cos(1.4), -2.0 * np.sin(1.4)], [3.0, 0.4]])
    cs.append(_agent("slack_equidistant", st, ud, nb, cfg=fov_slack_cfg(1.0, **BOX),
                     nb_cov=np.array([[0.1, 0.0, 0.05], [0.1, 0.0, 0.05], [0.2, 0.01, 0.1]])))
    return {c["name"]: c for c in cs}


def fov_reference(c, shift=0.0):
    """The reference result of one agent: dict(status, u, obj, active (row names), rows, tag,
    weights). Plain: the exact projection (status by the oracle's solver on the same rows); slack:
    the oracle's u, with the objective re-evaluated by penalty_objective."""
    cfg = c["cfg"]
    slack = bool(cfg.get("control_slack_mode", 0))
    nnb = len(c["nb_xy"])
    if nnb > (FOV_SLACK_CAP if slack else FOV_PLAIN_CAP):
        return dict(status=O.ERROR, u=np.full(3, np.nan), obj=np.nan, active=(), rows=[], tag=[], weights=None)
    rows, tag = fov_rows(cfg, c["state"], c["nb_xy"], slack)
    if not slack:
        status = oracle_status(rows, c["u_des"], shift=shift)
        out = dict(status=status, u=np.full(3, np.nan), obj=np.nan, active=(), rows=rows, tag=tag, weights=None)
        if status == O.OPTIMAL:
            G = np.array([r[0] for r in rows])
            h = np.array([r[1] + shift * max(1.0, abs(r[1])) for r in rows])
            ex = exact_projection(G, h, c["u_des"])
            if ex is not None:
                out.update(u=ex[0], obj=ex[1], active=tuple(tag[k][0] for k in ex[2]))
        return out
    w = fov_slack_weights(cfg, c["state"], c["nb_xy"], c["nb_cov"])
    status = oracle_status(rows, c["u_des"], nslack=nnb, weights=w, shift=shift)
    st_o, u_o, obj_o = O.fov_control(cfg, c["state"], c["u_des"], c["nb_xy"], nb_cov=c["nb_cov"])
    out = dict(status=status, u=u_o, obj=np.nan, active=(), rows=rows, tag=tag, weights=w, oracle_status=st_o,
               oracle_obj=obj_o)
    if status == O.OPTIMAL:
        out["obj"], out["slacks"] = penalty_objective(rows, w, c["u_des"], u_o)
    return out


@functools.lru_cache(maxsize=None)
def fov_cases():
    """Every FoV agent with its reference, computed once per process: name -> dict(case, ref)."""
    out = {}
    for name, c in {**fov_plain_cases(), **fov_slack_cases()}.items():
        out[name] = dict(case=c, ref=fov_reference(c))
    return out


def fov_batch(agents):
    """The controller's batch arrays of a list of agents: states, desired, row_ptr, nb_xy, nb_cov
    (zeros where an agent has none)."""
    states = np.array([a["state"] for a in agents])
    desired = np.array([a["u_des"] for a in agents])
    rp = np.concatenate([[0], np.cumsum([len(a["nb_xy"]) for a in agents])]).astype(np.int32)
    nb = np.vstack([a["nb_xy"] for a in agents] + [np.zeros((0, 2))])
    cov = np.vstack([a["nb_cov"] if a["nb_cov"] is not None else np.zeros((len(a["nb_xy"]), 3)) for a in agents]
                    + [np.zeros((0, 3))])
    return states, desired, rp, nb, cov


BATCH_SIZES = (1, 15, 17, 33)
ERROR_SLOT = 5  # the batch of 17: agent 5 has 14 neighbours


def plain_pool(n, with_error=None):
    """n plain-mode agents of the default configuration, cycling through the neighbour-count cases
    with the desired control varied per agent; with_error: the index that gets the 14-neighbour
    agent."""
    base = fov_plain_cases()
    names = ["plain_n0", "plain_n1", "plain_n2", "plain_n6", "plain_n10", "plain_n13_nb0", "plain_n13_nb12",
             "plain_n13_bound", "at_vmax", "nb_at_ego"]
    out = []
    k = 0
    while len(out) < n:
        if with_error is not None and len(out) == with_error:
            out.append(dict(base["plain_n14"], name=f"pool{len(out)}_n14"))
            continue
        c = dict(base[names[k % len(names)]])
        turn = k // len(names)
        c["u_des"] = c["u_des"] * (1.0 + 0.07 * turn)
        c["name"] = f"pool{len(out)}_{c['name']}"
        c["binds"] = None
        out.append(c)
        k += 1
    return out


# ---------------------------------------------------------------------------------------------
# connectivity controller
# ---------------------------------------------------------------------------------------------
def conn_cfg(slack=False):
    c = dict(d_min=0.8, d_max=3.0, v_min=[-1.0, -1.0, -2.6179938779914944], v_max=[1.0, 1.0, 2.6179938779914944])
    if slack:
        c.update(control_slack_mode=1, slack_cost=1e5, slack_decay_rate=0.5)
    return c


def laplacian(pos, dmax):
    """ConnectivityCBF::getLambda2's weighted Laplacian (ConnectivityCBF.cpp:375-414):
    A_ij = exp((d_max^2 - d^2)^2 / sigma) - 1 within d_max, sigma = d_max^4 / ln 2."""
    n = len(pos)
    sigma = dmax ** 4 / np.log(2.0)
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i != j:
                d2 = np.sum((pos[i] - pos[j]) ** 2)
                if d2 <= dmax * dmax:
                    A[i, j] = np.exp((dmax * dmax - d2) ** 2 / sigma) - 1
    return np.diag(A.sum(axis=1)) - A


def spectrum(S, dmax):
    """(lambda2, Fiedler vector, eigenvalues) by LAPACK; a team of 1 has lambda2 = 0 (its only
    eigenvalue, as getLambda2's sort leaves it), an empty team has none (NaN)."""
    if len(S) == 0:
        return np.nan, np.zeros(0), np.zeros(0)
    w, V = np.linalg.eigh(laplacian(S[:, :2], dmax))
    if len(S) == 1:
        return float(w[0]), V[:, 0], w
    return float(w[1]), V[:, 1], w


def degenerate(S, dmax):
    """The Fiedler vector enters the rows (lambda2 > 0.1) and is not unique (lambda3 - lambda2 < 1e-6)."""
    l2, _, w = spectrum(S, dmax)
    return len(S) >= 3 and l2 > 0.1 and w[2] - w[1] < 1e-6


def _ring(n, radius, phase=0.0):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1)


def _team(pos, seed, speed=0.5, gain=0.5):
    """States (zero yaw rate noise aside) and desired controls of a team at the given positions."""
    rng = np.random.default_rng(seed)
    n = len(pos)
    S = np.zeros((n, 6))
    S[:, :2] = pos
    S[:, 2] = rng.uniform(-0.5, 0.5, n)
    S[:, 3:5] = rng.uniform(-speed, speed, (n, 2))
    S[:, 5] = rng.uniform(-0.2, 0.2, n)
    targets = rng.uniform(-3, 3, (n, 3))
    ud = gain * (targets - S[:, :3]) - 2 * np.sqrt(gain) * S[:, 3:6]
    return S, ud


def _scatter(n, seed, box, min_dist):
    """n seeded positions in [-box, box]^2, pairwise at least min_dist apart."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.uniform(-box, box, 2)
        if all(np.hypot(*(p - q)) >= min_dist for q in pts):
            pts.append(p)
    return np.array(pts)


TEAM_NAMES = ("one", "empty", "two", "three", "sixteen", "seventeen", "far5", "clusters6", "triangle", "hexagon")
ROW_OFFSET = 2  # team_ptr[0]: the first two rows of the tables belong to no team


def conn_teams():
    """(names, list of (S, u_des)) in batch order: teams of 1, 0, 2, 3, 16, 17, then 5 robots all
    beyond d_max of each other, two clusters of 3 that are 2 d_max apart, an equilateral triangle and
    a regular hexagon."""
    teams = []
    S, ud = _team(np.array([[0.3, -0.2]]), 1)
    S[0, 3:6] = (0.9, -0.2, 0.1)
    ud[0] = (0.5, -1.0, 0.2)  # clipped by u_x <= 0.1 and u_y >= -0.8
    teams.append((S, ud))
    teams.append((np.zeros((0, 6)), np.zeros((0, 3))))
    # two robots 2.5 apart (lambda2 0.134: connectivity row) moving apart at 0.9 each: the row asks
    # for more than the velocity rows leave, so in slack mode its slack (lane n - 1 = 1) is in use
    S, ud = _team(np.array([[0.0, 0.0], [2.5, 0.0]]), 2)
    S[:, 3:6] = [(-0.9, 0.1, 0.0), (0.9, -0.1, 0.05)]
    ud[:] = [(-0.4, 0.2, 0.1), (0.3, 0.1, -0.1)]
    teams.append((S, ud))
    teams.append(_team(np.array([[0.0, 0.0], [1.6, 0.3], [0.5, 1.9]]), 3, speed=0.3))
    teams.append(_team(_scatter(16, 4, 2.6, 1.0), 4, speed=0.2))
    teams.append(_team(_scatter(17, 5, 2.8, 1.0), 5, speed=0.2))
    teams.append(_team(_ring(5, 3.3) * np.array([1.0, 1.15]) + np.array([[0.1, 0.0], [0, 0.2], [0, 0], [0.15, 0], [0, 0]]), 6, speed=0.2))
    c = np.array([[0.0, 0.0], [1.5, 0.2], [0.6, 1.4]])
    teams.append(_team(np.vstack([c, c[:, ::-1] * 0.9 + np.array([6.0 + 1.5, 0.0])]), 7, speed=0.2))
    teams.append(_team(_ring(3, 2.0 / np.sqrt(3.0), 0.3), 8, speed=0.2))
    teams.append(_team(_ring(6, 1.2, 0.1), 9, speed=0.2))
    return list(TEAM_NAMES), teams


def conn_batch():
    """(team_ptr, states, desired): team_ptr starts at ROW_OFFSET; the rows before it hold values
    no team refers to."""
    _, teams = conn_teams()
    ptr = ROW_OFFSET + np.concatenate([[0], np.cumsum([len(S) for S, _ in teams])])
    states = np.vstack([np.full((ROW_OFFSET, 6), 7.5)] + [S for S, _ in teams])
    desired = np.vstack([np.full((ROW_OFFSET, 3), -7.5)] + [u for _, u in teams])
    return ptr.astype(np.int32), states, desired


def conn_rows(cfg, S, i, slack=False):
    """Robot i's rows as (g, h, slack index or -1) and their names: safety rows against the other
    robots in index order (slack l for the l-th other robot), the velocity rows, then the
    connectivity row (lambda2 > 0.1; the last slack, n - 1) or one CLF row per other robot."""
    n = len(S)
    st = S[i]
    rows, tag = [], []
    others = [j for j in range(n) if j != i]
    for l, j in enumerate(others):
        a, b = O.safety_cbf(st, S[j], cfg["d_min"])
        rows.append((-a, b, l if slack else -1))
        tag.append(f"safety{j}")
    for d in range(3):
        rows.append((-np.eye(3)[d], st[3 + d] - cfg["v_min"][d], -1))
        tag.append(f"vmin{d}")
    for d in range(3):
        rows.append((np.eye(3)[d], cfg["v_max"][d] - st[3 + d], -1))
        tag.append(f"vmax{d}")
    l2, ev, _ = spectrum(S, cfg["d_max"])
    if l2 > 0.1:
        a, b, _ = O.conn_cbf(S, i, ev, l2, cfg["d_max"])
        rows.append((-a, b, n - 1 if slack else -1))
        tag.append("conn")
    else:
        for l, j in enumerate(others):
            a, b = O.clf_cbf(st, S[j])
            rows.append((a, -b, l if slack else -1))
            tag.append(f"clf{j}")
    return rows, tag


def conn_weights(cfg, n):
    """ConnectivityControl.cpp:31-38: slack i weighs slack_cost * decay^i, num_robots slacks."""
    return cfg["slack_cost"] * cfg["slack_decay_rate"] ** np.arange(n, dtype=np.float64)


def conn_reference(cfg, S, i, u_des, shift=0.0):
    """Robot i's reference: plain — status by the oracle's solver on the rows, u / obj / active by
    the exact projection; slack — the oracle's u with the objective by penalty_objective."""
    slack = bool(cfg.get("control_slack_mode", 0))
    n = len(S)
    if n > TEAM_CAP:
        return dict(status=O.ERROR, u=np.full(3, np.nan), obj=np.nan, active=(), rows=[], tag=[], weights=None)
    rows, tag = conn_rows(cfg, S, i, slack)
    if not slack:
        status = oracle_status(rows, u_des, shift=shift)
        out = dict(status=status, u=np.full(3, np.nan), obj=np.nan, active=(), rows=rows, tag=tag, weights=None)
        if status == O.OPTIMAL:
            G = np.array([r[0] for r in rows])
            h = np.array([r[1] + shift * max(1.0, abs(r[1])) for r in rows])
            ex = exact_projection(G, h, u_des)
            if ex is not None:
                out.update(u=ex[0], obj=ex[1], active=tuple(tag[k] for k in ex[2]))
        return out
    w = conn_weights(cfg, n)
    status = oracle_status(rows, u_des, nslack=n, weights=w, shift=shift)
    st_o, u_o, obj_o, _ = O.connectivity_control(cfg, S, i, u_des)
    out = dict(status=status, u=u_o, obj=np.nan, active=(), rows=rows, tag=tag, weights=w, oracle_status=st_o,
               oracle_obj=obj_o)
    if status == O.OPTIMAL:
        out["obj"], out["slacks"] = penalty_objective(rows, w, u_des, u_o)
    return out


@functools.lru_cache(maxsize=None)
def conn_cases(slack):
    """The batch with its references, computed once per process: dict(cfg, names, team_ptr, states,
    desired, teams (per team: S, u_des, lambda2, degenerate), ref (per table row, None for rows of
    degenerate teams and rows outside every team))."""
    cfg = conn_cfg(slack)
    names, teams = conn_teams()
    ptr, states, desired = conn_batch()
    info, ref = [], {}
    for t, (S, ud) in enumerate(teams):
        l2 = spectrum(S, cfg["d_max"])[0]
        deg = bool(degenerate(S, cfg["d_max"]))
        info.append(dict(S=S, u_des=ud, lambda2=l2, degenerate=deg, name=names[t]))
        for i in range(len(S)):
            ref[int(ptr[t]) + i] = None if deg else conn_reference(cfg, S, i, ud[i])
    return dict(cfg=cfg, names=names, team_ptr=ptr, states=states, desired=desired, teams=info, ref=ref)
