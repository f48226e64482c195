"""CPU reference of the batched IMPC with connectivity rows (Context.set_connectivity), built from
oracle_lib alone: per agent the collision QP of assemble_qp with the connectivity CBF row
(lambda2, conn_cbf) or the CLF rows (clf_cbf) appended as rows on the control points, solved by
solve_dense_qp; the next iteration's predicted states from eval_curve. Test infrastructure only."""
from __future__ import annotations

import numpy as np

import oracle_lib as O

GAMMA = 5.0
_U = {}


def accel_ops(cfg):
    """U_k (3 x n) for k < cbf_horizon: the acceleration of the curve at h k as a linear map of the
    n control-point variables (eval_curve of the unit vectors, second derivative). Cached."""
    key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()))
    if key not in _U:
        p = O.make_params(cfg)
        n = cfg["num_pieces"] * 3 * cfg["num_control_points"]
        U = np.zeros((cfg["cbf_horizon"], 3, n))
        for k in range(cfg["cbf_horizon"]):
            for i in range(n):
                e = np.zeros(n)
                e[i] = 1.0
                U[k, :, i] = O.eval_curve(p, e, cfg["h"] * k, 2)
        _U[key] = U
    return _U[key]


def team_spectrum(states, r0, n, d_max):
    """(lambda2, Fiedler vector, all eigenvalues ascending) of the team rows r0 .. r0 + n - 1."""
    l2, ev = O.lambda2(states[r0:r0 + n, :2], d_max)
    pos = states[r0:r0 + n, :2]
    d2 = np.sum((pos[:, None, :] - pos[None, :, :]) ** 2, axis=2)
    sigma = d_max ** 4 / np.log(2.0)
    W = np.where(d2 <= d_max ** 2, np.exp((d_max ** 2 - d2) ** 2 / sigma) - 1.0, 0.0)
    np.fill_diagonal(W, 0.0)
    lam = np.linalg.eigvalsh(np.diag(W.sum(axis=1)) - W)
    return l2, ev, lam


def added_rows(cfg, states, r0, n, self_row, e, k, l2, ev, conn_mode, d_max, l2_min):
    """The connectivity rows of sample k with the ego state e: list of (coefficients (n vars), hi)."""
    Uk = accel_ops(cfg)[k]
    me = self_row - r0
    rows = []
    if conn_mode:
        ts = np.array(states[r0:r0 + n], dtype=np.float64)
        ts[me] = e
        a, b, _ = O.conn_cbf(ts, me, ev, l2, d_max)
        b += GAMMA * GAMMA * (0.1 - l2_min)  # (conn_cbf has h = lambda2 - 0.1)
        rows.append((-(a @ Uk), b))
    else:
        for j in range(n):
            if j == me:
                continue
            a, B = O.clf_cbf(np.asarray(e, dtype=np.float64), np.asarray(states[r0 + j], dtype=np.float64))
            rows.append((a @ Uk, -B))
    return rows


def impc_agent(cfg, states, self_row, nb_idx, ref, team=None, d_max=None, l2_min=0.1, l2_switch=0.1, shift=0.0):
    """One agent's IMPC loop. team: (r0, n) or None (no added rows). shift: every added bound moves
    by shift * max(1, |bound|). Returns status / obj (impc_iter), x (list per iteration), rows (per
    iteration the added rows), l2, conn_mode."""
    p = O.make_params(cfg)
    iters, cbf_h, h = cfg["impc_iter"], cfg["cbf_horizon"], cfg["h"]
    status = np.full(iters, O.UNKNOWN, dtype=np.int32)
    obj = np.full(iters, np.nan)
    xs, rows_all = [None] * iters, [[] for _ in range(iters)]
    st = np.asarray(states[self_row], dtype=np.float64)
    nbs = np.asarray(states[np.asarray(nb_idx, dtype=np.int64)], dtype=np.float64) if len(nb_idx) else None
    l2 = ev = None
    conn_mode = False
    use = team is not None and 2 <= team[1] <= 16
    if use:
        l2, ev, _ = team_spectrum(np.asarray(states), team[0], team[1], d_max)
        conn_mode = l2 > l2_switch
    pred = None
    for it in range(iters):
        qp = O.assemble_qp(p, st, ref, nbs, it, pred)
        if use:
            add = []
            for k in range(1 if it == 0 else cbf_h):
                e = st if it == 0 else pred[k]
                add += added_rows(cfg, states, team[0], team[1], self_row, e, k, l2, ev, conn_mode, d_max, l2_min)
            add = [(c, b + shift * max(1.0, abs(b))) for c, b in add]
            rows_all[it] = add
            nvar = qp["n"]
            A = np.zeros((len(add), nvar))
            for i, (c, _) in enumerate(add):
                A[i, :len(c)] = c
            qp["A"] = np.vstack([qp["A"], A])
            qp["lo"] = np.concatenate([qp["lo"], np.full(len(add), -np.finfo(np.float64).max)])
            qp["hi"] = np.concatenate([qp["hi"], np.array([b for _, b in add])])
        r = O.solve_dense_qp(qp)
        status[it] = r["status"]
        if r["status"] != O.OPTIMAL:
            break
        obj[it] = r["obj"]
        xs[it] = r["x"].copy()
        pred = np.zeros((max(1, cbf_h), 6))
        for k in range(cbf_h):
            pred[k, :3] = O.eval_curve(p, r["x"], h * k, 0)
            pred[k, 3:] = O.eval_curve(p, r["x"], h * k, 1)
    return dict(status=status, obj=obj, x=xs, rows=rows_all, l2=l2, conn_mode=conn_mode)


def row_excess(rows, x):
    """Largest scaled excess (c . x - hi) / (1 + |hi|) of the added rows at x (-inf: none)."""
    return max([(float(c @ x[:len(c)]) - b) / (1.0 + abs(b)) for c, b in rows], default=-np.inf)


def binding(rows, x, tol=1e-7):
    """Whether some added row holds with equality at x (scaled)."""
    return any(abs(float(c @ x[:len(c)]) - b) <= tol * (1.0 + abs(b)) for c, b in rows)


def next_state(cfg, x, h=None):
    """Position and velocity of the curve x at t = h (the Jacobi update of the closed loop)."""
    p = O.make_params(cfg)
    t = cfg["h"] if h is None else h
    return np.concatenate([O.eval_curve(p, x, t, 0), O.eval_curve(p, x, t, 1)])
